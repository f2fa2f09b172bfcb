// PointNet++ object encoder, training side: what the forward (csrc/pointnet2.hip) and the backward (csrc/pointnet2_train.hip) share -- the shared-MLP
// layer both evaluate with the same expression (so the backward's recomputed activations carry the forward's bits), the per-clip record the forward keeps
// (``saves``) and the layouts of the raw parameters, the running statistics and the folded gradient.
//
// Per-clip record, PN_SV_WORDS 32-bit words (include/interdiff_hip.h, interdiff_pointnet2_encode_saved):
//   POS  [48] int   FPS position of the SA1 centre in each SA2 slot (16 slots of the r = 0.1 ball, then 32 of the r = 0.2 ball; padding slots repeat)
//   PID  [48] int   its point id
//   DUP  [48] int   the first slot that holds the same POINT (its own index for a distinct centre): padding slots, a centre in both balls, and for
//                   P < 1024 the FPS positions that repeat a point all map to one slot, whose gradient they add into
//   CNT  [98] int   hits of the two SA2 ball queries, then per slot the hits of the SA1 r = 0.05 and r = 0.1 queries (not clipped to nsample)
//   NB0  [48][16], NB1 [48][32] int   neighbour point ids of each centre (rows of slots that repeat an FPS position are not written and never read)
//   FEAT [48][96] float   SA1 output of each slot
#pragma once
#include "common.h"

namespace pn2 {

constexpr int PT = 1024, NWV = PT / 64;
constexpr int MAXP = 2048;                 // points per cloud (two per thread)
constexpr int NP1 = 1024;                  // SA1 npoint
constexpr int NS0 = 16, NS1 = 32, NSLOT = NS0 + NS1;
constexpr int F1 = 96;                     // SA1 output channels (32 + 64)
constexpr int CIN2 = F1 + 3;               // SA2 input channels

constexpr int SV_POS = 0, SV_PID = 48, SV_DUP = 96, SV_CNT = 144, SV_NB0 = 244, SV_NB1 = SV_NB0 + NSLOT * NS0, SV_FEAT = SV_NB1 + NSLOT * NS1,
              SV_WORDS = SV_FEAT + NSLOT * F1;                                                       // 7156

// out[n][o] = relu(b[o] + sum_c W[o][c] in[n][c]) for n < ns, o < cout
template <int NT = PT>
__device__ __forceinline__ void mlp_layer(const float *in, int in_stride, const float *__restrict__ W, const float *__restrict__ bias,
                                          int cin, int cout, int ns, float *out, int out_stride) {
    for (int i = threadIdx.x; i < ns * cout; i += NT) {
        const int n = i / cout, o = i - n * cout;
        const float *w = W + (size_t)o * cin, *x = in + n * in_stride;
        float s = bias[o];
        for (int c = 0; c < cin; ++c) s += w[c] * x[c];
        out[n * out_stride + o] = fmaxf(s, 0.f);
    }
}

// ---- sampling and grouping, shared by the eval encoder (csrc/pointnet2.hip) and the batch-statistic trainer (csrc/pointnet2_bn_train.hip)
__device__ __forceinline__ float d2_exact(float ax, float ay, float az, float bx, float by, float bz) {
#pragma clang fp contract(off)
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    return (dx * dx + dy * dy) + dz * dz;
}

// rank of this thread's hit among all hits of the block in thread order (exclusive), and the block total
__device__ __forceinline__ int block_rank(bool hit, unsigned *wcount, int &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long m = __ballot(hit);
    const int below = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wcount[wave] = (unsigned)__popcll(m);
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < NWV; ++w) {
        const int c = (int)wcount[w];
        if (w < wave) base += c;
        tot += c;
    }
    __syncthreads();                           // wcount is reused by the next call
    total = tot;
    return base + below;
}

// furthest point sampling MAXP -> NP1 by one PT-thread workgroup whose LDS holds the cloud (x, y, z, ||p||; rows >= P are zero): start at 0, skip |p|^2 <= 1e-3,
// arg-max = lowest index on ties; a clip with nothing left to sample repeats point 0.  The caller synchronises before it reads fps.
__device__ __forceinline__ void fps_sample(const float4 *pts, int P, unsigned short *fps, float (*redv)[NWV], int (*redi)[NWV]) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float px[2], py[2], pz[2], tmp[2];
    bool ok[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int i = tid + PT * k;
        const float4 p = pts[i];
        px[k] = p.x; py[k] = p.y; pz[k] = p.z;
        tmp[k] = 1e10f;
        ok[k] = i < P && d2_exact(p.x, p.y, p.z, 0.f, 0.f, 0.f) > 1e-3f;
    }
    if (tid == 0) fps[0] = 0;
    int old = 0;
    for (int j = 1; j < NP1; ++j) {
        const float4 o = pts[old];
        float bv = -1.0f;
        int bi = 0x7fffffff;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (ok[k]) {
                const float d2 = fminf(d2_exact(px[k], py[k], pz[k], o.x, o.y, o.z), tmp[k]);
                tmp[k] = d2;
                if (d2 > bv) { bv = d2; bi = tid + PT * k; }      // k = 0 first: lower index wins ties inside the thread
            }
        }
        const float wv = wave_max(bv);
        const float wi = -wave_max(bv == wv ? -(float)bi : -3e9f);                   // lowest index among the wave's maxima
        const int buf = j & 1;
        if (lane == 0) { redv[buf][wave] = wv; redi[buf][wave] = wv > -1.0f ? (int)wi : 0x7fffffff; }
        __syncthreads();
        float fv = -1.0f;
        int fi = 0x7fffffff;
#pragma unroll
        for (int w = 0; w < NWV; ++w) {
            const float v = redv[buf][w];
            const int ii = redi[buf][w];
            if (v > fv || (v == fv && ii < fi)) { fv = v; fi = ii; }
        }
        old = fv > -1.0f ? fi : 0;
        if (tid == 0) fps[j] = (unsigned short)old;
    }
}

// the SA1 centres (FPS positions) the key point -- the first sampled centre -- groups: r = 0.1 / 16 into list[0 .. 16), r = 0.2 / 32 into list[16 .. 48), FPS order,
// padding slots repeat the first hit; tot0 / tot1: the hits of the two queries (not clipped).  One PT-thread workgroup; ends on a barrier.
__device__ __forceinline__ void sa2_slots(const float4 *pts, const unsigned short *fps, int *list, unsigned *wcount, int &tot0, int &tot1) {
    const int tid = threadIdx.x;
    const float4 c0 = pts[fps[0]];
    const float4 q = pts[fps[tid]];
    const float d2 = d2_exact(q.x, q.y, q.z, c0.x, c0.y, c0.z);
    const float r0 = 0.1f, r1 = 0.2f;
    int tot;
    int rk = block_rank(d2 < r0 * r0, wcount, tot);
    if (d2 < r0 * r0 && rk < NS0) list[rk] = tid;
    __syncthreads();
    if (tid < NS0 && tid >= tot) list[tid] = tot > 0 ? list[0] : 0;
    tot0 = tot;
    __syncthreads();
    rk = block_rank(d2 < r1 * r1, wcount, tot);
    if (d2 < r1 * r1 && rk < NS1) list[NS0 + rk] = tid;
    __syncthreads();
    if (tid < NS1 && tid >= tot) list[NS0 + tid] = tot > 0 ? list[NS0] : 0;
    tot1 = tot;
    __syncthreads();
}

// The twelve conv + BatchNorm layers in the reference's order (SA_modules.0.mlps.0, .0.mlps.1, .1.mlps.0, .1.mlps.1; three layers each) and the Linear.
//   raw    (the flat master / gradient vector, 38 tensors): per layer conv weight [cout][cin], BatchNorm weight [cout], bias [cout]; Linear.weight, Linear.bias
//   stats  per layer running_mean [cout], running_var [cout]
//   folded gradient: SA1's 4224 floats first (per layer dW' [cout][cin], db' [cout]), then SA2's, then the Linear's
struct Layer { int cin, cout; int raw_w, raw_g, raw_b, stat, fold_w, fold_b; };
struct Plan {
    Layer ly[12];
    int raw_lin_w, raw_lin_b, fold_lin_w, fold_lin_b, n_raw, n_fold, n_fold_sa1, n_stat;
};
constexpr int N_TENSORS = 38;

inline Plan make_plan() {
    static const int ch[4][4] = {{4, 16, 16, 32}, {4, 32, 32, 64}, {CIN2, 64, 64, 128}, {CIN2, 64, 96, 128}};
    Plan p{};
    int raw = 0, fold = 0, stat = 0;
    for (int g = 0; g < 4; ++g)
        for (int l = 0; l < 3; ++l) {
            Layer &y = p.ly[g * 3 + l];
            y.cin = ch[g][l]; y.cout = ch[g][l + 1];
            y.raw_w = raw; raw += y.cin * y.cout;
            y.raw_g = raw; raw += y.cout;
            y.raw_b = raw; raw += y.cout;
            y.stat = stat; stat += 2 * y.cout;
            y.fold_w = fold; fold += y.cin * y.cout;
            y.fold_b = fold; fold += y.cout;
            if (g == 1 && l == 2) p.n_fold_sa1 = fold;
        }
    p.raw_lin_w = raw; raw += 253 * 256;
    p.raw_lin_b = raw; raw += 253;
    p.fold_lin_w = fold; fold += 253 * 256;
    p.fold_lin_b = fold; fold += 253;
    p.n_raw = raw; p.n_fold = fold; p.n_stat = stat;
    return p;
}

}  // namespace pn2
