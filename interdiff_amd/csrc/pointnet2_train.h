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
