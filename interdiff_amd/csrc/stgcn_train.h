// Fine-tuning of the two ST-GCN correction predictors with FROZEN normalisation statistics: what the skeleton trainer (csrc/skeleton_train.h, NP = 20
// coefficients, 22 nodes) and the SMPL contact-frame trainer (csrc/objproj_train.h, NP = 10, 68 nodes) share -- the flat parameter plan, the compensated
// sum, the forward and backward of one ST-GCN layer on the folded arena block of csrc/stgcn.h, and the kernels that do not depend on the geometry: the
// fold of the per-clip partials in ascending clip order, the conversion of the folded convolutions' gradients to the reference parameters, Adam
// (torch.optim.Adam's order of operations) on the fp32 master parameters, and the re-fold into the arena the inference kernels read.
// The layer functions are members of StgcnFt<NP, VP> so that each trainer instantiates them for its own geometry; the kernels sit in an unnamed
// namespace: every translation unit that includes this header launches its own copy.  Behind them, the host side both predictors' launchers share: the
// table export, the workspace layout, the loss constants, and the launch sequences around a clip kernel (ft_export_table .. stgcn_ft_launch_step).
#pragma once
#include <math.h>
#include "stgcn.h"

namespace idf_stgcn_train {

using namespace idf_stgcn;

// Offsets (floats) of a layer's tensors in the flat parameter / gradient vector = named_parameters() order of ObjProjector:
//   [gcn.A [NP][nodes][nodes] (joint stack only)] gcn.T [NP][NP] or [nodes][NP][NP], tcn.0.weight [cout][cin], tcn.0.bias, tcn.1.weight, tcn.1.bias,
//   residual.0.weight [cout][cin], residual.0.bias, residual.1.weight, residual.1.bias, prelu.weight [1]
// bn: offset in the flat BatchNorm-buffer vector: tcn.1.running_mean, tcn.1.running_var, residual.1.running_mean, residual.1.running_var, cout each.
// ws_*: offsets of the saved planes in a clip's workspace slice.
struct FtLayer {
    int32_t A, T, Wt, bt, gt, bet, Wr, br, gr, ber, pr;
    int32_t cin, cout, nodes, v2, bn;
    int32_t ws_x, ws_u, ws_g, ws_h;
};
struct FtPlan {
    FtLayer L[12];
    int32_t n_param, n_bn, ws_clip;          // ws_clip: saved planes + the scratch plane sets G, X (one layer buffer each) at its end
};
constexpr int FT_TABLE_COLS = 16;            // interdiff_*_finetune_param_table: the first 16 ints of an FtLayer

// the plan of the three stacks (relative: nodes_rel nodes, object: 1 node, joint: nodes_rel + 1 nodes and its own A), four layers each, over np coefficients;
// buf_floats: the layer buffer, the size of each of the scratch plane sets G, X
inline FtPlan ft_plan_for(const int32_t *cin, const int32_t *cout, int np, int nodes_rel, int buf_floats) {
    FtPlan P{};
    int o = 0, bn = 0, ws = 0;
    for (int li = 0; li < 12; ++li) {
        FtLayer &L = P.L[li];
        const int st = li / 4, nodes = st == 0 ? nodes_rel : st == 1 ? 1 : nodes_rel + 1, ci = cin[li], co = cout[li], npos = np * nodes;
        L.cin = ci; L.cout = co; L.nodes = nodes; L.v2 = st == 2;
        L.A = -1;
        if (L.v2) { L.A = o; o += np * nodes * nodes; }
        L.T = o; o += (L.v2 ? nodes : 1) * np * np;
        L.Wt = o; o += co * ci;
        L.bt = o; o += co;
        L.gt = o; o += co;
        L.bet = o; o += co;
        L.Wr = o; o += co * ci;
        L.br = o; o += co;
        L.gr = o; o += co;
        L.ber = o; o += co;
        L.pr = o; o += 1;
        L.bn = bn; bn += 4 * co;
        L.ws_x = ws; ws += ci * npos;
        L.ws_u = -1;
        if (L.v2) { L.ws_u = ws; ws += ci * npos; }
        L.ws_g = ws; ws += ci * npos;
        L.ws_h = ws; ws += co * npos;
    }
    P.n_param = o; P.n_bn = bn; P.ws_clip = ws + 2 * buf_floats;
    return P;
}

// Compensated fp32 accumulation (Ogita-Rump-Oishi Dot2: TwoProduct by fma, TwoSum, the errors summed aside): every sum of the backward runs through it, so
// a gradient carries the rounding of its operands and of one final addition, not of the summation order -- the reference's BLAS sums blockwise, a plain
// sequential fp32 chain over the 440 (skeleton) or 680 (SMPL) positions of a plane would be the larger error.  fp32 arithmetic only; contraction off so that p is the rounded product TwoSum assumes.
struct Acc2 {
    float s = 0.f, c = 0.f;
    __device__ __forceinline__ void mac(float a, float b) {
#pragma clang fp contract(off)
        const float p = a * b, ep = fmaf(a, b, -p);
        const float t = s + p, bb = t - s;
        const float es = (s - (t - bb)) + (p - bb);
        s = t;
        c += ep + es;
    }
    __device__ __forceinline__ void add(float p) {
#pragma clang fp contract(off)
        const float t = s + p, bb = t - s;
        const float es = (s - (t - bb)) + (p - bb);
        s = t;
        c += es;
    }
    __device__ __forceinline__ float value() const { return s + c; }
};

template <int NP, int VP>
struct StgcnFt {
    // ---- forward of one layer on buf (cin planes in, cout planes out), saving x, u, g, h.  The arithmetic of st_gcn_layer (csrc/skeleton.h, csrc/objproj.h) on
    // the same folded arena, but every sum compensated (Acc2) on the VALU instead of K-blocked on the MFMA: a saved plane is the correctly rounded fp32 value
    // of its exact sum, which is what keeps the gradient inside 4 e_ref of the fp64 one.  Every step reads planes the PREVIOUS step saved to the
    // workspace and writes buf, so nothing is updated in place.
    // ft_fwd_graph: the input planes to sx, the temporal mix and (joint stack) the adjacency product to su / sg -- everything of a layer before its two 1x1
    // convolutions; the train-mode layer (csrc/skeleton_bn_train.h) shares it.
    template <bool V2>
    __device__ static inline void ft_fwd_graph(const float *buf, const LayerP &p, int cin, int nodes, float *sx, float *su, float *sg) {
        const int tid = threadIdx.x, npos = NP * nodes;
        for (int i = tid; i < cin * npos; i += NTHR) sx[i] = buf[i];
        __syncthreads();
        // temporal mix: u[c][q][v] = sum_t x[c][t][v] Tm[(v)][t][q]
        float *su_or_sg = V2 ? su : sg;
        for (int i = tid; i < cin * npos; i += NTHR) {
            const int c = i / npos, r = i - c * npos, q = r / nodes, v = r - q * nodes;
            const float *xc = sx + c * npos + v, *tmv = p.Tm + (V2 ? v * NP * NP : 0) + q;
            Acc2 a;
#pragma unroll 4
            for (int t = 0; t < NP; ++t) a.mac(xc[t * nodes], tmv[t * NP]);
            su_or_sg[i] = a.value();
        }
        __syncthreads();
        // adjacency product: g[c][t][w] = sum_v u[c][t][v] A[t][v][w]  (AT[t][w][v])
        if (V2) {
            for (int i = tid; i < cin * npos; i += NTHR) {
                const int c = i / npos, r = i - c * npos, t = r / nodes, w = r - t * nodes;
                const float *u = su + (c * NP + t) * nodes, *At = p.AT + ((size_t)t * VP + w) * VP;
                Acc2 a;
                for (int v = 0; v < nodes; ++v) a.mac(u[v], At[v]);
                sg[i] = a.value();
            }
            __syncthreads();
        }
    }

    template <bool V2>
    __device__ static inline void ft_layer_fwd(float *buf, const LayerP &p, int cin, int cout, int nodes, float *sx, float *su, float *sg, float *sh) {
        const int tid = threadIdx.x, npos = NP * nodes, cinp = pad16(cin);
        ft_fwd_graph<V2>(buf, p, cin, nodes, sx, su, sg);
        // h = Wt' g + bt' + Wr' x + br' in one compensated sum; PReLU
        const float slope = p.prelu;
        for (int i = tid; i < cout * npos; i += NTHR) {
            const int o = i / npos, pos = i - o * npos;
            const float *wt = p.Wt + o * cinp, *wr = p.Wr + o * cinp;
            Acc2 a;
            a.add(p.bt[o]);
            a.add(p.br[o]);
            for (int c = 0; c < cin; ++c) {
                a.mac(wt[c], sg[c * npos + pos]);
                a.mac(wr[c], sx[c * npos + pos]);
            }
            const float h = a.value();
            sh[i] = h;
            buf[i] = h >= 0.f ? h : slope * h;
        }
        __syncthreads();
    }

    // ---- backward of one layer, in three pieces (the train-mode layer, csrc/skeleton_bn_train.h, shares the first and the last)
    // PReLU: dh = dy * (h > 0 ? 1 : slope) in place; d slope = sum over h <= 0 of dy * h (a strided walk per thread, then a tree: fixed order)
    __device__ static inline void ft_bwd_prelu(float *dy, float *red, float slope, const float *sh, const FtLayer &L, float *part) {
        const int tid = threadIdx.x, n = L.cout * NP * L.nodes;
        {
            Acc2 acc;
            for (int i = tid; i < n; i += NTHR) {
                const float h = sh[i], d = dy[i];
                if (h > 0.f) {
                    dy[i] = d;
                } else {
                    acc.mac(d, h);
                    dy[i] = slope * d;
                }
            }
            red[tid] = acc.value();
            __syncthreads();
            for (int s = NTHR / 2; s > 0; s >>= 1) {
                if (tid < s) red[tid] += red[tid + s];
                __syncthreads();
            }
            if (tid == 0) part[L.pr] = red[0];
        }
    }

    // the graph part: G = the gradient of the mixed planes g, X = the residual branch's share of dx (both [cin][npos], read only from here on); dy: scratch in
    // (its planes are dead), dx out.  dA and dT to part[].
    __device__ static inline void ft_bwd_graph(float *dy, const LayerP &p, const FtLayer &L, const float *ws, const float *G, const float *X, float *part) {
        const int tid = threadIdx.x, cin = L.cin, nodes = L.nodes, npos = NP * nodes;
        const float *sx = ws + L.ws_x;
        // 4. adjacency product: dA[t][v][w] = sum_c u[c][t][v] G[c][t][w]; du[c][t][v] = sum_w G[c][t][w] A[t][v][w] -> dy (dh is dead)
        if (L.v2) {
            const float *su = ws + L.ws_u;
            for (int idx = tid; idx < NP * nodes * nodes; idx += NTHR) {
                const int t = idx / (nodes * nodes), r = idx - t * nodes * nodes, v = r / nodes, w = r - v * nodes;
                Acc2 a;
                for (int c = 0; c < cin; ++c) a.mac(su[(c * NP + t) * nodes + v], G[(c * NP + t) * nodes + w]);
                part[L.A + idx] = a.value();
            }
            for (int i = tid; i < cin * npos; i += NTHR) {
                const int c = i / npos, r = i - c * npos, t = r / nodes, v = r - t * nodes;
                const float *g = G + (c * NP + t) * nodes, *At = p.AT + (size_t)t * VP * VP + v;       // AT[t][w][v]
                Acc2 a;
                for (int w = 0; w < nodes; ++w) a.mac(g[w], At[w * VP]);
                dy[i] = a.value();
            }
        } else {
            for (int i = tid; i < cin * npos; i += NTHR) dy[i] = G[i];
        }
        __syncthreads();
        // 5. temporal mix: dT[(v)][t][q] = sum_c (sum_v) x[c][t][v] du[c][q][v]
        if (L.v2) {
            for (int idx = tid; idx < nodes * NP * NP; idx += NTHR) {
                const int v = idx / (NP * NP), r = idx - v * NP * NP, t = r / NP, q = r - t * NP;
                Acc2 a;
                for (int c = 0; c < cin; ++c) a.mac(sx[(c * NP + t) * nodes + v], dy[(c * NP + q) * nodes + v]);
                part[L.T + idx] = a.value();
            }
        } else {
            for (int idx = tid; idx < NP * NP; idx += NTHR) {
                const int t = idx / NP, q = idx - t * NP;
                Acc2 a;
                for (int c = 0; c < cin; ++c) {
                    const float *xp = sx + (c * NP + t) * nodes, *dp = dy + (c * NP + q) * nodes;
                    for (int v = 0; v < nodes; ++v) a.mac(xp[v], dp[v]);
                }
                part[L.T + idx] = a.value();
            }
        }
        __syncthreads();
        // 6. dx[c][t][v] = X[c][t][v] + sum_q du[c][q][v] Tm[(v)][t][q], in place (a thread owns its column)
        for (int i = tid; i < cin * nodes; i += NTHR) {
            const int c = i / nodes, v = i - c * nodes;
            float *col = dy + c * npos + v;
            const float *xc = X + c * npos + v, *tmv = p.Tm + (L.v2 ? v * NP * NP : 0);
            float du[NP];
#pragma unroll
            for (int q = 0; q < NP; ++q) du[q] = col[q * nodes];
#pragma unroll 2
            for (int t = 0; t < NP; ++t) {
                Acc2 a;
                a.add(xc[t * nodes]);
#pragma unroll
                for (int q = 0; q < NP; ++q) a.mac(du[q], tmv[t * NP + q]);
                col[t * nodes] = a.value();
            }
        }
        __syncthreads();
    }

    // backward of one layer: dy = cout gradient planes in, cin gradient planes out (in place); parameter gradients to part[]
    __device__ static inline void ft_layer_bwd(float *dy, float *red, const LayerP &p, const FtLayer &L, const float *ws, float *G, float *X, float *part) {
        const int tid = threadIdx.x, cin = L.cin, cout = L.cout, nodes = L.nodes, npos = NP * nodes, cinp = pad16(cin);
        const float *sx = ws + L.ws_x, *sg = ws + L.ws_g;
        // 1. PReLU
        ft_bwd_prelu(dy, red, p.prelu, ws + L.ws_h, L, part);
        // 2. folded convolution weights and biases: dWt'[o][c] = sum_pos dh[o][pos] g[c][pos], dWr'[o][c] = sum_pos dh[o][pos] x[c][pos], db' = sum_pos dh[o][pos]
        for (int idx = tid; idx < cout * cin + cout; idx += NTHR) {
            if (idx < cout * cin) {
                const int o = idx / cin, c = idx - o * cin;
                const float *d = dy + o * npos, *gp = sg + c * npos, *xp = sx + c * npos;
                Acc2 a, b;
                for (int pos = 0; pos < npos; ++pos) {
                    const float dv = d[pos];
                    a.mac(dv, gp[pos]);
                    b.mac(dv, xp[pos]);
                }
                part[L.Wt + idx] = a.value();
                part[L.Wr + idx] = b.value();
            } else {
                const int o = idx - cout * cin;
                const float *d = dy + o * npos;
                Acc2 a;
                for (int pos = 0; pos < npos; ++pos) a.add(d[pos]);
                part[L.bt + o] = a.value();
                part[L.br + o] = a.value();
                // the BatchNorm gamma / beta slots carry nothing per clip (stgcn_ft_convert_kernel derives them from the folded gradients): written as zeros so
                // that every element of partials[b][.] is written, and what the fold sums there is defined
                part[L.gt + o] = 0.f; part[L.bet + o] = 0.f; part[L.gr + o] = 0.f; part[L.ber + o] = 0.f;
            }
        }
        // 3. G = Wt'^T dh (gradient of the mixed planes), X = Wr'^T dh (the residual branch's share of dx) -> workspace
        for (int i = tid; i < cin * npos; i += NTHR) {
            const int c = i / npos, pos = i - c * npos;
            Acc2 a, b;
            for (int o = 0; o < cout; ++o) {
                const float d = dy[o * npos + pos];
                a.mac(p.Wt[o * cinp + c], d);
                b.mac(p.Wr[o * cinp + c], d);
            }
            G[i] = a.value();
            X[i] = b.value();
        }
        __syncthreads();
        ft_bwd_graph(dy, p, L, ws, G, X, part);
    }
};

// ---- the kernels around a trainer's clip kernel
constexpr int FT_THR = 256;
constexpr float BN_EPS = 1e-5f;

struct LossK {
    float w[8], inv_n[8];      // the 8 weights, 1 / (frames * B * width) of each mean
};

// torch.optim.Adam (torch/optim/adam.py _single_tensor_adam): grad += wd * p; exp_avg.lerp_(grad, 1 - beta1); exp_avg_sq = beta2 exp_avg_sq + (1 - beta2) grad^2;
// denom = sqrt(exp_avg_sq) / sqrt(1 - beta2^step) + eps; p += -(lr / (1 - beta1^step)) * exp_avg / denom
struct AdamK {
    float w1, beta2, w2, step_size, bc2_sqrt, eps, wd;
    int use_wd;
};

// the step's constants from the doubles torch computes them from, each rounded to fp32 once
inline AdamK ft_adam_constants(int step, double lr, double beta1, double beta2, double eps, double weight_decay) {
    AdamK k;
    const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
    k.w1 = (float)(1.0 - beta1);
    k.beta2 = (float)beta2;
    k.w2 = (float)(1.0 - beta2);
    k.step_size = (float)(lr / bc1);
    k.bc2_sqrt = (float)sqrt(bc2);
    k.eps = (float)eps;
    k.wd = (float)weight_decay;
    k.use_wd = weight_decay != 0.0;
    return k;
}

// one arena layer block's folded convolution from the master parameters, in double exactly as stgcn_pack.fold_bn does on the host (no contraction: W * s
// and (b - mu) * s + beta round once per operation)
__device__ __forceinline__ double ft_scale(float gamma, float var) {
#pragma clang fp contract(off)
    return (double)gamma / sqrt((double)var + 1e-5);
}
__device__ __forceinline__ float ft_fold_w(float w, double s) {
#pragma clang fp contract(off)
    return (float)((double)w * s);
}
__device__ __forceinline__ float ft_fold_b(float b, float mu, double s, float beta) {
#pragma clang fp contract(off)
    const double t = ((double)b - (double)mu) * s;
    return (float)(t + (double)beta);
}

namespace {

// gsum[i] = sum_b partials[b][i], b ascending; block 0 also folds the loss: out9 = loss, the 8 terms
__global__ __launch_bounds__(FT_THR) void stgcn_ft_fold_kernel(const float *__restrict__ partials, const float *__restrict__ loss_part, int B, int n_param,
                                                              const LossK lk, float *__restrict__ gsum, float *__restrict__ out9) {
    const int i = blockIdx.x * FT_THR + threadIdx.x;
    if (i < n_param) {
        Acc2 a;
        for (int b = 0; b < B; ++b) a.add(partials[(size_t)b * n_param + i]);
        gsum[i] = a.value();
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        float loss = 0.f;
        for (int k = 0; k < 8; ++k) {
            float a = 0.f;
            for (int b = 0; b < B; ++b) a += loss_part[(size_t)b * 8 + k];
            a *= lk.inv_n[k];
            out9[1 + k] = a;
            loss += lk.w[k] * a;
        }
        out9[0] = loss;
    }
}

// one block per layer: gradients of the folded (W s, (b - mu) s + beta), s = gamma / sqrt(var + eps), back to conv weight / bias and BN gamma / beta;
// T, A and the PReLU slope pass through
template <int NP>
__global__ __launch_bounds__(FT_THR) void stgcn_ft_convert_kernel(const FtPlan plan, const float *__restrict__ gsum, const float *__restrict__ params,
                                                                 const float *__restrict__ bn, float *__restrict__ grads) {
    const FtLayer &L = plan.L[blockIdx.x];
    const int tid = threadIdx.x, cin = L.cin, cout = L.cout;
    const int nT = (L.v2 ? L.nodes : 1) * NP * NP;
    if (L.v2)
        for (int i = tid; i < NP * L.nodes * L.nodes; i += FT_THR) grads[L.A + i] = gsum[L.A + i];
    for (int i = tid; i < nT; i += FT_THR) grads[L.T + i] = gsum[L.T + i];
    if (tid == 0) grads[L.pr] = gsum[L.pr];
    for (int br = 0; br < 2; ++br) {
        const int W = br ? L.Wr : L.Wt, bb = br ? L.br : L.bt, ga = br ? L.gr : L.gt, be = br ? L.ber : L.bet;
        const float *mu = bn + L.bn + 2 * br * cout, *var = mu + cout;
        for (int i = tid; i < cout * cin; i += FT_THR) {
            const int o = i / cin;
            const float s = params[ga + o] / sqrtf(var[o] + BN_EPS);
            grads[W + i] = gsum[W + i] * s;
        }
        for (int o = tid; o < cout; o += FT_THR) {
            const float r = 1.0f / sqrtf(var[o] + BN_EPS), db = gsum[bb + o];
            Acc2 a;
            for (int c = 0; c < cin; ++c) a.mac(gsum[W + o * cin + c], params[W + o * cin + c]);
            a.mac(db, params[bb + o] - mu[o]);
            grads[bb + o] = db * (params[ga + o] * r);
            grads[be + o] = db;
            grads[ga + o] = r * a.value();
        }
    }
}

__global__ __launch_bounds__(FT_THR) void stgcn_ft_adam_kernel(float *__restrict__ p, const float *__restrict__ grad, float *__restrict__ m, float *__restrict__ v, int n,
                                                              const AdamK k) {
    const int i = blockIdx.x * FT_THR + threadIdx.x;
    if (i >= n) return;
    float g = grad[i];
    const float pi = p[i];
    if (k.use_wd) g = g + k.wd * pi;
    float mi = m[i], vi = v[i];
    mi = mi + k.w1 * (g - mi);
    vi = vi * k.beta2 + k.w2 * g * g;
    const float denom = sqrtf(vi) / k.bc2_sqrt + k.eps;
    m[i] = mi;
    v[i] = vi;
    p[i] = pi + (-k.step_size) * (mi / denom);
}

// one block per layer: the arena layer block (csrc/stgcn.h) from the master parameters; padding stays what the host packer wrote (zero).  OP: the
// predictor's descriptor (its layer[] offsets are all that is read)
template <int NP, int VP, class OP>
__global__ __launch_bounds__(FT_THR) void stgcn_ft_refold_kernel(const OP op, const FtPlan plan, const float *__restrict__ params,
                                                                const float *__restrict__ bn, float *__restrict__ arena) {
    const int li = blockIdx.x;
    const FtLayer &L = plan.L[li];
    const int tid = threadIdx.x, cin = L.cin, cout = L.cout, nodes = L.nodes, cinp = pad16(cin), coutp = pad16(cout);
    const int nT = (L.v2 ? nodes : 1) * NP * NP;
    float *blk = arena + op.layer[li];
    for (int i = tid; i < nT; i += FT_THR) blk[i] = params[L.T + i];
    blk += pad16(nT);
    if (L.v2) {
        for (int i = tid; i < NP * nodes * nodes; i += FT_THR) {
            const int t = i / (nodes * nodes), r = i - t * nodes * nodes, v = r / nodes, w = r - v * nodes;
            blk[(t * VP + w) * VP + v] = params[L.A + i];
        }
        blk += NP * VP * VP;
    }
    for (int br = 0; br < 2; ++br) {
        const int W = br ? L.Wr : L.Wt, bb = br ? L.br : L.bt, ga = br ? L.gr : L.gt, be = br ? L.ber : L.bet;
        const float *mu = bn + L.bn + 2 * br * cout, *var = mu + cout;
        for (int i = tid; i < cout * cin; i += FT_THR) {
            const int o = i / cin, c = i - o * cin;
            blk[o * cinp + c] = ft_fold_w(params[W + i], ft_scale(params[ga + o], var[o]));
        }
        blk += coutp * cinp;
        for (int o = tid; o < cout; o += FT_THR) blk[o] = ft_fold_b(params[bb + o], mu[o], ft_scale(params[ga + o], var[o]), params[be + o]);
        blk += coutp;
    }
    if (tid == 0) blk[0] = params[L.pr];
}

// ---- host: what the launchers of both predictors do around their clip kernel (argument checks stay with each entry point)
// the first FT_TABLE_COLS ints of every layer of the plan, and its two counts
inline void ft_export_table(const FtPlan &P, int32_t *table, int32_t *n_param, int32_t *n_bn) {
    for (int li = 0; li < 12; ++li) {
        const int32_t *src = reinterpret_cast<const int32_t *>(&P.L[li]);
        for (int k = 0; k < FT_TABLE_COLS; ++k) table[li * FT_TABLE_COLS + k] = src[k];
    }
    *n_param = P.n_param;
    *n_bn = P.n_bn;
}

// a workspace region of n floats at the running offset o, regions 64-float aligned
inline size_t ft_ws_take(size_t &o, size_t n) {
    const size_t at = o;
    o += (n + 63) / 64 * 64;
    return at;
}

// a fine-tuner's workspace (floats): partials [B][n_param] | loss_part [B][8] | gsum [n_param] | clips [B][ws_clip]
struct FtWs {
    size_t partials, loss_part, gsum, clips, total;
};
inline FtWs ft_ws(const FtPlan &P, int B) {
    FtWs w{};
    w.partials = ft_ws_take(w.total, (size_t)B * P.n_param);
    w.loss_part = ft_ws_take(w.total, (size_t)B * 8);
    w.gsum = ft_ws_take(w.total, (size_t)P.n_param);
    w.clips = ft_ws_take(w.total, (size_t)B * P.ws_clip);
    return w;
}

// the 8 MSE means (MSE_KEYS order) as constants: term k averages frames * B * width values -- the past frames for k = 0, 1, 4, 5 and the future ones
// otherwise, rot_width rotation channels for even k and the 3 translation channels for odd k.  -> the fold's LossK; coef[k] = 2 w_k / n_k for the clip kernel
inline LossK ft_loss_constants(const float *weights8, int past, int T, int B, int rot_width, float *coef) {
    LossK lk;
    for (int k = 0; k < 8; ++k) {
        const double frames = (k == 0 || k == 1 || k == 4 || k == 5) ? past : T - past, width = (k & 1) ? 3 : rot_width;
        const double n = frames * (double)B * width;
        lk.w[k] = weights8[k];
        lk.inv_n[k] = (float)(1.0 / n);
        coef[k] = (float)(2.0 * (double)weights8[k] / n);
    }
    return lk;
}

// a fine-tuner's gradient call: clip() launches the clip kernel on st; then the fold over the clips and the conversion to the reference parameters
template <int NP, class Clip>
inline int stgcn_ft_launch_grads(const FtPlan &P, const FtWs &W, float *base, int B, const LossK &lk, const float *params, const float *bn, float *out9,
                                 float *grads, hipStream_t st, Clip &&clip) {
    idf_prof_mark(IDF_K_OTHER, st);
    clip();
    hipLaunchKernelGGL(stgcn_ft_fold_kernel, dim3((P.n_param + FT_THR - 1) / FT_THR), dim3(FT_THR), 0, st, base + W.partials, base + W.loss_part, B, P.n_param,
                       lk, base + W.gsum, out9);
    hipLaunchKernelGGL(stgcn_ft_convert_kernel<NP>, dim3(12), dim3(FT_THR), 0, st, P, base + W.gsum, params, bn, grads);
    idf_prof_mark(-1, st);
    IDF_CHECK_LAUNCH();
    return IDF_OK;
}

// Adam on the master parameters and the re-fold into the arena
template <int NP, int VP, class OP>
inline int stgcn_ft_launch_step(const OP &op, const FtPlan &P, float *arena, float *params, const float *bn, const float *grads, float *exp_avg,
                                float *exp_avg_sq, const AdamK &k, hipStream_t st) {
    idf_prof_mark(IDF_K_OTHER, st);
    hipLaunchKernelGGL(stgcn_ft_adam_kernel, dim3((P.n_param + FT_THR - 1) / FT_THR), dim3(FT_THR), 0, st, params, grads, exp_avg, exp_avg_sq, P.n_param, k);
    hipLaunchKernelGGL((stgcn_ft_refold_kernel<NP, VP, OP>), dim3(12), dim3(FT_THR), 0, st, op, P, params, bn, arena);
    idf_prof_mark(-1, st);
    IDF_CHECK_LAUNCH();
    return IDF_OK;
}

}  // namespace

}  // namespace idf_stgcn_train
