// Training of the two ST-GCN correction predictors the way the reference trains them (the module in train()): what the skeleton trainer
// (csrc/skeleton_bn_train.h, NP = 20 coefficients, 22 nodes, 64 channels) and the SMPL contact-frame trainer (csrc/objproj_bn_train.h, NP = 10, 68 nodes,
// 32 channels) share -- the train-mode ST-GCN layer cut into the four pieces its two batch normalisations need, built around the fine-tuner's layer code
// (StgcnFt, csrc/stgcn_train.h):
//
//     res = BN_r(conv_r(x));  g = gcn(x);  y = dropout(BN_t(conv_t(g)));  h = y + res;  out = PReLU(h)
//
//   FRONT(l)  saves the layer's input planes x, the mixed planes u / g, and the two PRE-BatchNorm convolutions ct = Wt g + bt, cr = Wr x + br (unfolded
//             reference weights read from the flat parameter vector, compensated sums); writes the clip's per-channel (sum, M2) of ct and cr, M2 about the
//             clip's own mean (two passes, double; 8 lanes per channel, tr_sum8).
//   FIN(l)    folds the per-clip (sum, M2) over the clips IN ASCENDING ORDER with Chan's pairwise merge (double; every workgroup redoes it, B * cout values),
//             h = gamma_t xhat_t + beta_t (times mask * s) + gamma_r xhat_r + beta_r in double rounded once, saves h, out = PReLU(h).
//   A(l)      PReLU backward (dh, slope gradient), dh saved over h; the clip's per-channel sums of dy and dy * xhat for both BatchNorms (double): they are the
//             seam of the backward AND the clip's share of d gamma, d beta.
//   B(l)      folds those sums over the clips in ascending order; d ct = gamma rstd (dy - mean(dy) - xhat mean(dy xhat)), likewise d cr, written over ct / cr;
//             the convolution weight gradients, G = Wt^T d ct, X = Wr^T d cr, then the fine-tuner's graph backward (dA, dT, dx).
// A piece needs the whole batch's statistics of the piece before it, so a trainer runs them in separate launches (its phase table), one workgroup per clip.
// The convolution biases cancel inside a batch normalisation: their gradient is identically zero and is WRITTEN as 0.0f.
// Dropout keep masks: one byte per element, the 12 layers in named_parameters() order, each [B][cout][NP][nodes]; keep iff the byte is nonzero.  The
// generator's draw (tr_uniform): Philox4x32-10 keyed by the seed, counter = (element index / 4, layer, step); an element keeps iff its uniform draw in
// [0, 1) is >= p.  The pieces only ever read bytes, so the injected and the generated route are the same code.
// The geometry is a template parameter (StgcnTr<NP, VP, MAXC, BUF>); what does not depend on it is plain functions of this namespace.
#pragma once
#include "stgcn_train.h"
#include "philox.h"

namespace idf_stgcn_train {

constexpr int TR_PHASES = 17;

// what a clip's workspace slice holds beyond the fine-tuner's planes (FtPlan: x, u, g, h per layer, then G, X)
struct TrPlan {
    int32_t ct[12], cr[12];          // pre-BatchNorm convolution planes [cout][npos] (the backward writes their gradients over them)
    int32_t mask[12];                // elements per clip of the layers before this one: the layer's masks start at B * mask[l]
    int32_t mask_clip;               // mask elements per clip, all layers
    int32_t keepf, keepb;            // [keep_floats] the joint stack's input (forward), the gradient at its output (backward)
    int32_t ws_clip;                 // floats per clip
};

// keep_floats: the size of each of the two skip-connection saves (a trainer that keeps them in double passes twice their count and sets align2)
inline TrPlan tr_plan_for(const FtPlan &P, int np, int keep_floats, bool align2 = false) {
    TrPlan t{};
    int ws = P.ws_clip, m = 0;
    for (int li = 0; li < 12; ++li) {
        const int n = P.L[li].cout * np * P.L[li].nodes;
        t.ct[li] = ws; ws += n;
        t.cr[li] = ws; ws += n;
        t.mask[li] = m; m += n;
    }
    t.mask_clip = m;
    if (align2) ws = (ws + 1) & ~1;
    t.keepf = ws; ws += keep_floats;
    t.keepb = ws; ws += keep_floats;
    if (align2) ws = (ws + 1) & ~1;
    t.ws_clip = ws;
    return t;
}

struct TrArgs {
    const float *params;             // [n_param] the flat reference parameters
    const uint8_t *masks;            // keep masks (layout above) or null: no dropout
    double *statp, *dyp;             // [B][TR_SEAM] per-clip (sum, M2) of ct / cr; per-clip (sum dy, sum dy xhat)
    float scale;                     // fp32(1 / (1 - p))
};

// one clip's view of a phase launch.  sm: the layer buffer (the start of the LDS); red: NTHR floats; st: TR_STAT doubles; arena / layer: the folded arena
// the graph products read and its 12 layer-block offsets
struct TrCtx {
    float *sm, *red;
    double *st;
    const float *arena;
    const int64_t *layer;
    const FtPlan &plan;
    const TrPlan &tp;
    const TrArgs &t;
    int B, b;
    float *ws, *part;
};

// Per-channel sums over a clip's positions: 8 adjacent lanes per (BatchNorm, channel) pair, each summing every 8th position in double, then an xor
// butterfly over the 8 lanes: a fixed order, and all 8 lanes end with the same bits.  Every lane of the workgroup calls it.
__device__ __forceinline__ double tr_sum8(double v) {
    v += __shfl_xor(v, 4);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 1);
    return v;
}

// the uniform draw in [0, 1) of element idx of layer li at training step `step`
__device__ __forceinline__ float tr_uniform(uint64_t seed, uint64_t step, int li, uint32_t idx) {
    uint32_t c0 = idx >> 2, c1 = (uint32_t)li, c2 = (uint32_t)step, c3 = (uint32_t)(step >> 32);
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        philox_round(c0, c1, c2, c3, k0, k1);
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    const uint32_t e = idx & 3u, w = e == 0 ? c0 : e == 1 ? c1 : e == 2 ? c2 : c3;
    return (float)(w >> 8) * (1.0f / 16777216.0f);
}

// NP coefficients, nodes padded to VP in the arena's adjacency operand, MAXC the widest layer, BUF the layer buffer (floats; the scratch plane sets G, X at
// the end of the fine-tuner's workspace slice are BUF floats each)
template <int NP, int VP, int MAXC, int BUF>
struct StgcnTr {
    using Ft = StgcnFt<NP, VP>;
    static constexpr int STAT = 8 * MAXC;                 // doubles in LDS: mu, rstd, m1, m2, each [2][MAXC]
    static constexpr int SEAM = 12 * 2 * MAXC * 2;        // doubles per clip: [layer][tcn | residual][channel][2]
    static_assert(NTHR / 8 >= 2 * MAXC, "8 lanes per (BatchNorm, channel) pair");

    __device__ __forceinline__ static size_t tr_seam_at(int b, int li, int br, int o) { return ((((size_t)b * 12 + li) * 2 + br) * MAXC + o) * 2; }

    // mean and BIASED variance of channel o of BatchNorm br of layer li over the whole batch: Chan's merge of the per-clip (sum, M2), clips ascending
    __device__ static inline void tr_fold_stats(const double *statp, int B, int li, int br, int o, int npos, double &mean, double &var) {
#pragma clang fp contract(off)
        const double nb = (double)npos;
        double n = 0.0, m = 0.0, M2 = 0.0;
        for (int b = 0; b < B; ++b) {
            const double *q = statp + tr_seam_at(b, li, br, o);
            const double mb = q[0] / nb;
            if (b == 0) {
                n = nb; m = mb; M2 = q[1];
            } else {
                const double d = mb - m, nn = n + nb;
                m = m + d * (nb / nn);
                M2 = M2 + q[1] + d * d * (n * nb / nn);
                n = nn;
            }
        }
        mean = m;
        var = M2 / n;
    }

    // mu, rstd of both BatchNorms of layer li -> LDS
    __device__ static inline void tr_load_stats(const TrCtx &c, int li) {
        const FtLayer &L = c.plan.L[li];
        double *st = c.st;
        __syncthreads();                                                   // (the previous piece may still read the region)
        if ((int)threadIdx.x < 2 * L.cout) {
            const int br = threadIdx.x / L.cout, o = threadIdx.x - br * L.cout;
            double mean, var;
            tr_fold_stats(c.t.statp, c.B, li, br, o, NP * L.nodes, mean, var);
            st[br * MAXC + o] = mean;
            st[(2 + br) * MAXC + o] = 1.0 / sqrt(var + 1e-5);
        }
        __syncthreads();
    }

    // mask * s of element i of layer li in this clip (1 without masks)
    __device__ __forceinline__ static float tr_keep(const TrCtx &c, int li, int n_layer, int i) {
        if (!c.t.masks) return 1.0f;
        return c.t.masks[(size_t)c.B * c.tp.mask[li] + (size_t)c.b * n_layer + i] ? c.t.scale : 0.0f;
    }

    // FRONT: buf = the layer's input planes
    __device__ static inline void tr_front(const TrCtx &c, int li) {
        const FtLayer &L = c.plan.L[li];
        const int tid = threadIdx.x, cin = L.cin, cout = L.cout, npos = NP * L.nodes;
        const LayerP p = layer_params<NP, VP>(c.arena + c.layer[li], cin, cout, L.nodes, L.v2);
        float *sx = c.ws + L.ws_x, *sg = c.ws + L.ws_g, *ct = c.ws + c.tp.ct[li], *cr = c.ws + c.tp.cr[li];
        if (L.v2) Ft::template ft_fwd_graph<true>(c.sm, p, cin, L.nodes, sx, c.ws + L.ws_u, sg);
        else Ft::template ft_fwd_graph<false>(c.sm, p, cin, L.nodes, sx, nullptr, sg);
        const float *Wt = c.t.params + L.Wt, *Wr = c.t.params + L.Wr, *bt = c.t.params + L.bt, *br = c.t.params + L.br;
        for (int i = tid; i < cout * npos; i += NTHR) {
            const int o = i / npos, pos = i - o * npos;
            const float *wt = Wt + o * cin, *wr = Wr + o * cin;
            Acc2 a, r;
            a.add(bt[o]);
            r.add(br[o]);
            for (int k = 0; k < cin; ++k) {
                a.mac(wt[k], sg[k * npos + pos]);
                r.mac(wr[k], sx[k * npos + pos]);
            }
            ct[i] = a.value();
            cr[i] = r.value();
        }
        __syncthreads();
        {
            const int pair = tid >> 3, sub = tid & 7;
            const bool on = pair < 2 * cout;
            const int b2 = on ? pair / cout : 0, o = on ? pair - b2 * cout : 0;
            const float *src = (b2 ? cr : ct) + o * npos;
            double s = 0.0, m2 = 0.0;
            if (on)
                for (int pos = sub; pos < npos; pos += 8) s += (double)src[pos];
            s = tr_sum8(s);
            const double mean = s / (double)npos;
            if (on)
                for (int pos = sub; pos < npos; pos += 8) {
                    const double d = (double)src[pos] - mean;
                    m2 += d * d;
                }
            m2 = tr_sum8(m2);
            if (on && sub == 0) {
                double *q = c.t.statp + tr_seam_at(c.b, li, b2, o);
                q[0] = s;
                q[1] = m2;
            }
        }
        __syncthreads();
    }

    // FIN: the layer's output planes -> buf, h saved
    __device__ static inline void tr_fin(const TrCtx &c, int li) {
        const FtLayer &L = c.plan.L[li];
        const int tid = threadIdx.x, cout = L.cout, npos = NP * L.nodes, n = cout * npos;
        const float slope = c.t.params[L.pr];
        const float *ct = c.ws + c.tp.ct[li], *cr = c.ws + c.tp.cr[li];
        const float *gt = c.t.params + L.gt, *bet = c.t.params + L.bet, *gr = c.t.params + L.gr, *ber = c.t.params + L.ber;
        float *sh = c.ws + L.ws_h, *buf = c.sm;
        const double *st = c.st;
        tr_load_stats(c, li);
        for (int i = tid; i < n; i += NTHR) {
            const int o = i / npos;
            const double xt = ((double)ct[i] - st[o]) * st[2 * MAXC + o], xr = ((double)cr[i] - st[MAXC + o]) * st[3 * MAXC + o];
            const double y = ((double)gt[o] * xt + (double)bet[o]) * (double)tr_keep(c, li, n, i);
            const float h = (float)(y + ((double)gr[o] * xr + (double)ber[o]));
            sh[i] = h;
            buf[i] = h >= 0.f ? h : slope * h;
        }
        __syncthreads();
    }

    // A: buf = the gradient of the layer's output planes
    __device__ static inline void tr_bwd_a(const TrCtx &c, int li) {
        const FtLayer &L = c.plan.L[li];
        const int tid = threadIdx.x, cout = L.cout, npos = NP * L.nodes, n = cout * npos;
        float *sh = c.ws + L.ws_h, *buf = c.sm, *red = c.red;
        const float *ct = c.ws + c.tp.ct[li], *cr = c.ws + c.tp.cr[li];
        const double *st = c.st;
        Ft::ft_bwd_prelu(buf, red, c.t.params[L.pr], sh, L, c.part);
        tr_load_stats(c, li);
        for (int i = tid; i < n; i += NTHR) sh[i] = buf[i];
        {
            const int pair = tid >> 3, sub = tid & 7;
            const bool on = pair < 2 * cout;
            const int b2 = on ? pair / cout : 0, o = on ? pair - b2 * cout : 0;
            const float *src = (b2 ? cr : ct) + o * npos, *d = buf + o * npos;
            const double mu = st[b2 * MAXC + o], rstd = st[(2 + b2) * MAXC + o];
            double s1 = 0.0, s2 = 0.0;
            if (on)
                for (int pos = sub; pos < npos; pos += 8) {
                    const double dy = b2 ? (double)d[pos] : (double)d[pos] * (double)tr_keep(c, li, n, o * npos + pos);
                    s1 += dy;
                    s2 += dy * (((double)src[pos] - mu) * rstd);
                }
            s1 = tr_sum8(s1);
            s2 = tr_sum8(s2);
            if (on && sub == 0) {
                double *q = c.t.dyp + tr_seam_at(c.b, li, b2, o);
                q[0] = s1;
                q[1] = s2;
                // the clip's share of d gamma, d beta; the convolution biases cancel inside the batch normalisation: exactly 0
                c.part[(b2 ? L.gr : L.gt) + o] = (float)s2;
                c.part[(b2 ? L.ber : L.bet) + o] = (float)s1;
                c.part[(b2 ? L.br : L.bt) + o] = 0.f;
            }
        }
        __syncthreads();
    }

    // B: the gradient of the layer's input planes -> buf
    __device__ static inline void tr_bwd_b(const TrCtx &c, int li) {
        const FtLayer &L = c.plan.L[li];
        const int tid = threadIdx.x, cin = L.cin, cout = L.cout, npos = NP * L.nodes, n = cout * npos;
        const LayerP p = layer_params<NP, VP>(c.arena + c.layer[li], cin, cout, L.nodes, L.v2);
        const float *sx = c.ws + L.ws_x, *sg = c.ws + L.ws_g, *sh = c.ws + L.ws_h;
        float *ct = c.ws + c.tp.ct[li], *cr = c.ws + c.tp.cr[li];
        float *G = c.ws + c.plan.ws_clip - 2 * BUF, *X = G + BUF;
        const float *Wt = c.t.params + L.Wt, *Wr = c.t.params + L.Wr, *gt = c.t.params + L.gt, *gr = c.t.params + L.gr;
        double *st = c.st;
        tr_load_stats(c, li);
        if (tid < 2 * cout) {                                              // the seam: means of dy and dy xhat over the batch, clips ascending
            const int b2 = tid / cout, o = tid - b2 * cout;
            double s1 = 0.0, s2 = 0.0;
            for (int b = 0; b < c.B; ++b) {
                const double *q = c.t.dyp + tr_seam_at(b, li, b2, o);
                s1 += q[0];
                s2 += q[1];
            }
            const double nn = (double)c.B * (double)npos;
            st[(4 + b2) * MAXC + o] = s1 / nn;
            st[(6 + b2) * MAXC + o] = s2 / nn;
        }
        __syncthreads();
        for (int i = tid; i < n; i += NTHR) {
            const int o = i / npos;
            const double dh = (double)sh[i];
            const double rt = st[2 * MAXC + o], rr = st[3 * MAXC + o];
            const double xt = ((double)ct[i] - st[o]) * rt, xr = ((double)cr[i] - st[MAXC + o]) * rr;
            const double dyt = dh * (double)tr_keep(c, li, n, i);
            ct[i] = (float)((double)gt[o] * rt * (dyt - st[4 * MAXC + o] - xt * st[6 * MAXC + o]));
            cr[i] = (float)((double)gr[o] * rr * (dh - st[5 * MAXC + o] - xr * st[7 * MAXC + o]));
        }
        __syncthreads();
        // convolution weights: dWt[o][k] = sum_pos d ct[o][pos] g[k][pos], dWr[o][k] = sum_pos d cr[o][pos] x[k][pos]
        for (int idx = tid; idx < cout * cin; idx += NTHR) {
            const int o = idx / cin, k = idx - o * cin;
            const float *dt = ct + o * npos, *dr = cr + o * npos, *gp = sg + k * npos, *xp = sx + k * npos;
            Acc2 a, r;
            for (int pos = 0; pos < npos; ++pos) {
                a.mac(dt[pos], gp[pos]);
                r.mac(dr[pos], xp[pos]);
            }
            c.part[L.Wt + idx] = a.value();
            c.part[L.Wr + idx] = r.value();
        }
        // G = Wt^T d ct (gradient of the mixed planes), X = Wr^T d cr (the residual branch's share of dx)
        for (int i = tid; i < cin * npos; i += NTHR) {
            const int k = i / npos, pos = i - k * npos;
            Acc2 a, r;
            for (int o = 0; o < cout; ++o) {
                a.mac(Wt[o * cin + k], ct[o * npos + pos]);
                r.mac(Wr[o * cin + k], cr[o * npos + pos]);
            }
            G[i] = a.value();
            X[i] = r.value();
        }
        __syncthreads();
        Ft::ft_bwd_graph(c.sm, p, L, c.ws, G, X, c.part);
    }
};

// ---- the kernels around a trainer's phase kernel that do not read its geometry beyond NP and MAXC
namespace {

// grid (groups of FT_THR elements of the largest layer, 12 layers): out[B * mask[l] + i] = keep
template <int NP>
__global__ __launch_bounds__(FT_THR) void stgcn_tr_masks_kernel(const FtPlan plan, const TrPlan tp, int B, float p, uint64_t seed, uint64_t step,
                                                               uint8_t *__restrict__ out) {
    const int li = blockIdx.y;
    const size_t n = (size_t)B * plan.L[li].cout * NP * plan.L[li].nodes, i = (size_t)blockIdx.x * FT_THR + threadIdx.x;
    if (i < n) out[(size_t)B * tp.mask[li] + i] = tr_uniform(seed, step, li, (uint32_t)i) >= p ? 1 : 0;
}

// one block per layer: mean and biased variance of the batch -> batch_stats (when given), and the running buffers
// running <- (1 - momentum) running + momentum {mean, var n / (n - 1)} (torch.nn.BatchNorm2d in train()), in double, rounded once
template <class TR, int NP, int MAXC>
__global__ __launch_bounds__(2 * MAXC) void stgcn_tr_stats_kernel(const FtPlan plan, const double *__restrict__ statp, int B, double momentum, int update,
                                                                 float *__restrict__ bn, float *__restrict__ batch_stats) {
#pragma clang fp contract(off)
    const int li = blockIdx.x;
    const FtLayer &L = plan.L[li];
    if ((int)threadIdx.x >= 2 * L.cout) return;
    const int br = threadIdx.x / L.cout, o = threadIdx.x - br * L.cout, npos = NP * L.nodes;
    double mean, var;
    TR::tr_fold_stats(statp, B, li, br, o, npos, mean, var);
    const int at = L.bn + 2 * br * L.cout + o;
    if (batch_stats) {
        batch_stats[at] = (float)mean;
        batch_stats[at + L.cout] = (float)var;
    }
    if (update) {
        const double n = (double)B * (double)npos;
        bn[at] = (float)((1.0 - momentum) * (double)bn[at] + momentum * mean);
        bn[at + L.cout] = (float)((1.0 - momentum) * (double)bn[at + L.cout] + momentum * (var * (n / (n - 1.0))));
    }
}

template <int NP>
inline void stgcn_tr_launch_masks(const FtPlan &P, const TrPlan &T, int B, double p, uint64_t seed, uint64_t step, uint8_t *out, hipStream_t st) {
    size_t widest = 0;
    for (int li = 0; li < 12; ++li) widest = std::max(widest, (size_t)B * P.L[li].cout * NP * P.L[li].nodes);
    hipLaunchKernelGGL(stgcn_tr_masks_kernel<NP>, dim3((unsigned)((widest + FT_THR - 1) / FT_THR), 12), dim3(FT_THR), 0, st, P, T, B, (float)p, seed, step, out);
}

// a trainer's workspace (floats): partials [B][n_param] | loss_part [B][8] | clips [B][ws_clip] | statp, dyp [B][seam] doubles | masks [B][mask_clip] bytes
struct TrWs {
    size_t partials, loss_part, clips, statp, dyp, masks, total;
};
inline TrWs tr_ws(const FtPlan &P, const TrPlan &T, int B, int seam) {
    TrWs w{};
    w.partials = ft_ws_take(w.total, (size_t)B * P.n_param);
    w.loss_part = ft_ws_take(w.total, (size_t)B * 8);
    w.clips = ft_ws_take(w.total, (size_t)B * T.ws_clip);
    w.statp = ft_ws_take(w.total, (size_t)B * seam * 2);
    w.dyp = ft_ws_take(w.total, (size_t)B * seam * 2);
    w.masks = ft_ws_take(w.total, ((size_t)B * T.mask_clip + 3) / 4);
    return w;
}

// a trainer's gradient call: the generator's masks when none are injected, the TR_PHASES launches -- phase(t, k) launches phase k with the TrArgs t on st --
// the fold over the clips, and the batch statistics / running-buffer update when asked for
template <class TR, int NP, int MAXC, class Phase>
inline int stgcn_tr_launch_grads(const FtPlan &P, const TrPlan &TP, const TrWs &W, float *base, int B, const LossK &lk, const float *params, float *bn,
                                 double p_drop, const uint8_t *masks, uint64_t seed, uint64_t step, double momentum, int update_running, float *out9,
                                 float *grads, float *batch_stats, hipStream_t st, Phase &&phase) {
    TrArgs t{};
    t.params = params;
    t.statp = reinterpret_cast<double *>(base + W.statp);
    t.dyp = reinterpret_cast<double *>(base + W.dyp);
    t.scale = (float)(1.0 / (1.0 - p_drop));
    t.masks = masks;
    idf_prof_mark(IDF_K_OTHER, st);
    if (!masks && p_drop > 0.0) {                       // the generator's masks go through the same buffer layout as injected ones
        uint8_t *mb = reinterpret_cast<uint8_t *>(base + W.masks);
        stgcn_tr_launch_masks<NP>(P, TP, B, p_drop, seed, step, mb, st);
        t.masks = mb;
    }
    for (int k = 0; k < TR_PHASES; ++k) phase(t, k);
    hipLaunchKernelGGL(stgcn_ft_fold_kernel, dim3((P.n_param + FT_THR - 1) / FT_THR), dim3(FT_THR), 0, st, base + W.partials, base + W.loss_part, B, P.n_param,
                       lk, grads, out9);
    if (batch_stats || update_running)
        hipLaunchKernelGGL((stgcn_tr_stats_kernel<TR, NP, MAXC>), dim3(12), dim3(2 * MAXC), 0, st, P, t.statp, B, momentum, update_running, bn, batch_stats);
    idf_prof_mark(-1, st);
    IDF_CHECK_LAUNCH();
    return IDF_OK;
}

}  // namespace

}  // namespace idf_stgcn_train
