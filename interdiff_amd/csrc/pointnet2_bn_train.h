// PointNet++ object encoder under batch statistics (the reference's train() regime): layouts the kernels of csrc/pointnet2_bn_train.hip share, and the per-row device
// functions EVERY pass evaluates a layer with -- the statistic phases of the forward, the live-slot pass, and each recompute of the dense backward -- so that a
// pre-activation, its ReLU mask and a pool winner carry the same bits wherever they are computed.
//
// A "row" is one (centre, sample) pair of an SA1 grouping: B * 1024 * 16 rows at r = 0.05, B * 1024 * 32 at r = 0.1.  A tile is TR = 64 consecutive rows (4 or 2 whole
// centres); inside a tile lane l of every wave owns row l and the waves share the output channels (channel o belongs to wave o % NW), so every weight and every
// normalisation constant is wave-uniform (scalar loads) and the LDS reads of the activations (row stride odd) are conflict-free.  VALU fp32 fmaf chains, channels ascending.
#pragma once
#include "pointnet2_train.h"

namespace pnbt {

using namespace pn2;

constexpr int TR = 64;                       // rows of a tile
constexpr int G_MAX = 512;                   // persistent workgroups per scale of a dense phase
constexpr int MAXB = 256;                    // clips per call
constexpr int NCH = 736;                     // normalised channels of the twelve sites
constexpr int P_DW = 0, P_S = 2048, P_Q = 2112, P_N = 2176, P_STRIDE = 2304;      // one workgroup's partial record, doubles
constexpr float BN_EPS_F = 1e-5f;

__device__ __forceinline__ int wave_id() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

// sum_c w[c] x[c], c ascending, one fmaf chain from zero
__device__ __forceinline__ float dotrow(const float *__restrict__ w, const float *x, int cin) {
    float s = 0.f;
    for (int c = 0; c < cin; ++c) s = fmaf(w[c], x[c], s);
    return s;
}

// normalised value and post-ReLU activation of a pre-activation z
__device__ __forceinline__ float bn_hat(float z, float mu, float rs) {
#pragma clang fp contract(off)
    return (z - mu) * rs;
}
__device__ __forceinline__ float bn_act(float h, float g, float b) { return fmaxf(fmaf(g, h, b), 0.f); }

// the batch-statistic backward of one site at one element: (gamma / sigma) (d - mean(d) - x^ mean(d x^))
__device__ __forceinline__ float bn_back(float d, float h, float g, float rs, float m, float q) {
#pragma clang fp contract(off)
    const float gr = g * rs;
    return gr * ((d - m) - h * q);
}

// the grouped input of row (clip b, centre point pc, neighbour point pn): [p_n - p_c | ||p_n||]
__device__ __forceinline__ void row_input(const float *__restrict__ pts, int pc, int pn, float *x) {
#pragma clang fp contract(off)
    const float *c = pts + (size_t)pc * 3, *p = pts + (size_t)pn * 3;
    const float px = p[0], py = p[1], pz = p[2];
    x[0] = px - c[0]; x[1] = py - c[1]; x[2] = pz - c[2];
    x[3] = sqrtf((px * px + py * py) + pz * pz);
}

// z[l][o] = W[o] . in[l] for the tile's rows (raw pre-activation, layer under measurement)
template <int NW>
__device__ __forceinline__ void conv_rows(const float *in, int sin, const float *__restrict__ W, int cin, int cout, float *out, int sout) {
    const int lane = threadIdx.x & 63;
    for (int o = wave_id(); o < cout; o += NW) out[lane * sout + o] = dotrow(W + (size_t)o * cin, in + lane * sin, cin);
}

// a finished layer: H = x^ (normalised), A = relu(gamma x^ + beta) (A may be null)
template <int NW>
__device__ __forceinline__ void layer_rows(const float *in, int sin, const float *__restrict__ W, int cin, int cout, const float *__restrict__ mu,
                                           const float *__restrict__ rs, const float *__restrict__ g, const float *__restrict__ be, float *H, float *A, int s) {
    const int lane = threadIdx.x & 63;
    for (int o = wave_id(); o < cout; o += NW) {
        const float h = bn_hat(dotrow(W + (size_t)o * cin, in + lane * sin, cin), mu[o], rs[o]);
        H[lane * s + o] = h;
        if (A) A[lane * s + o] = bn_act(h, g[o], be[o]);
    }
}

}  // namespace pnbt
