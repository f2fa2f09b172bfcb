// Fine-tuning of the HO-GCN skeleton correction predictor with FROZEN normalisation statistics (the module in eval() with autograd on):
// the loss of LitObjInteraction._common_step (train_correction_skeleton.py:128-154) on ObjProjector.forward (model/correction_skeleton.py:68-137),
// d loss / d theta for every entry of named_parameters(), and torch.optim.Adam (train_correction_skeleton.py:41-47).  Device code; launchers:
// csrc/skeleton_train.hip.  The ST-GCN layer's forward with saves and its backward, the compensated sum, the flat parameter plan and the fold / Adam / re-fold
// kernels are shared with the SMPL predictor's trainer: csrc/stgcn_train.h.  Train-mode BatchNorm (batch statistics) and dropout: csrc/skeleton_bn_train.h,
// built from the pieces of this file.
//
// ONE 16-wave workgroup per clip, like skel_body (csrc/skeleton.h), in three parts:
//   1. FORWARD on the folded layers of the arena the inference kernels read: st_gcn_layer's arithmetic with every sum compensated (Acc2) on the VALU.  Each
//      layer saves to the clip's workspace slice: its input planes x, (joint stack) the temporally mixed planes u, the mixed planes g the tcn convolution
//      reads, and the pre-activation h.
//   2. LOSS GRADIENT on the clip's [T][7] pose: the 8 MSE means are over the batch, so their normalisers are constants (coef[k] = 2 w_k / n_k); the
//      velocity terms couple adjacent frames of the same clip only.  The clip's 8 sums of squares go to loss_part[b][8].
//   3. BACKWARD: xyzw reorder, matrix_to_quaternion (the selected candidate only, zero through sqrt at non-positive arguments, no gradient through an
//      active 0.1 floor), rotation_6d_to_matrix, the IDCT of node 0, the three skip connections, the three stacks in reverse.  A layer's backward:
//      PReLU (+ slope gradient), both folded 1x1 convolutions (+ weight and bias gradients), the adjacency product (+ dA per coefficient), the temporal mix
//      (+ dT, one per node in the joint stack).
// LDS: the gradient planes live in the layer buffer [64][440] (in place: dy -> dh -> du -> dx); in the 64 <-> 32 layers input planes + gradient planes would
// be 168 960 B > 160 KiB, so the other operand of every product (x, u, g, h and two scratch plane sets G = W^T dh, X = Wr^T dh) comes from the clip's
// workspace slice, which only this workgroup touches (__syncthreads orders its global accesses at workgroup scope).
// Parameter gradients: partials[b][.] in the FLAT REFERENCE LAYOUT (FtPlan, csrc/stgcn_train.h), gradients of the FOLDED convolutions in the conv slots, plain stores,
// every element written by exactly one thread in a fixed summation order -- no atomics; two calls give the same bits.
#pragma once
#include "skeleton.h"
#include "stgcn_train.h"

namespace idf_skel_train {

using namespace idf_skel_dev;
using idf_stgcn_train::Acc2;
using idf_stgcn_train::FtLayer;
using idf_stgcn_train::FtPlan;
using idf_stgcn_train::FT_TABLE_COLS;

// the flat parameter plan (csrc/stgcn_train.h) of this predictor: 21 / 1 / 22 nodes over NP = 20 coefficients; ws_clip ends with the scratch plane sets G, X
// (BUF floats each)
inline FtPlan ft_plan(const int32_t *cin, const int32_t *cout) { return idf_stgcn_train::ft_plan_for(cin, cout, NP, J, BUF); }

constexpr int FT_SMALL = 1536, FT_RED = NTHR;
constexpr size_t FT_LDS = (size_t)(BUF + KEEP + FT_SMALL + FT_RED) * sizeof(float);

struct FtArgs {
    const float *pose_gt;      // [T][B][7] translation | quaternion xyzw
    float *partials;           // [B][n_param]
    float *loss_part;          // [B][8]
    float *ws_clips;           // [B][ws_clip]
    float coef[8];             // 2 w_k / n_k, MSE_KEYS order: rot_past, nonrot_past, rot_future, nonrot_future, then the four velocity terms
};

// ---- the ST-GCN layer's forward with saves and its backward (csrc/stgcn_train.h) at this predictor's geometry
using Ft = idf_stgcn_train::StgcnFt<NP, VP>;
template <bool V2>
__device__ inline void ft_fwd_graph(const float *buf, const LayerP &p, int cin, int nodes, float *sx, float *su, float *sg) {
    Ft::ft_fwd_graph<V2>(buf, p, cin, nodes, sx, su, sg);
}
template <bool V2>
__device__ inline void ft_layer_fwd(float *buf, const LayerP &p, int cin, int cout, int nodes, float *sx, float *su, float *sg, float *sh) {
    Ft::ft_layer_fwd<V2>(buf, p, cin, cout, nodes, sx, su, sg, sh);
}
__device__ inline void ft_bwd_prelu(float *dy, float *red, float slope, const float *sh, const FtLayer &L, float *part) { Ft::ft_bwd_prelu(dy, red, slope, sh, L, part); }
__device__ inline void ft_bwd_graph(float *dy, const LayerP &p, const FtLayer &L, const float *ws, const float *G, const float *X, float *part) {
    Ft::ft_bwd_graph(dy, p, L, ws, G, X, part);
}
__device__ inline void ft_layer_bwd(float *dy, float *red, const LayerP &p, const FtLayer &L, const float *ws, float *G, float *X, float *part) {
    Ft::ft_layer_bwd(dy, red, p, L, ws, G, X, part);
}

__device__ inline void ft_stack_fwd(float *buf, const idf_skel_objproj &op, const FtPlan &plan, int stack, int nodes, float *ws) {
#pragma unroll 1
    for (int l = 0; l < 4; ++l) {
        const int li = stack * 4 + l;
        const FtLayer &L = plan.L[li];
        const LayerP p = layer_params<NP, VP>(op.arena + op.layer[li], L.cin, L.cout, nodes, stack == 2);
        if (stack == 2) ft_layer_fwd<true>(buf, p, L.cin, L.cout, nodes, ws + L.ws_x, ws + L.ws_u, ws + L.ws_g, ws + L.ws_h);
        else ft_layer_fwd<false>(buf, p, L.cin, L.cout, nodes, ws + L.ws_x, nullptr, ws + L.ws_g, ws + L.ws_h);
    }
}

__device__ inline void ft_stack_bwd(float *dy, float *red, const idf_skel_objproj &op, const FtPlan &plan, int stack, int nodes, const float *ws, float *G,
                                    float *X, float *part) {
#pragma unroll 1
    for (int l = 3; l >= 0; --l) {
        const int li = stack * 4 + l;
        const FtLayer &L = plan.L[li];
        const LayerP p = layer_params<NP, VP>(op.arena + op.layer[li], L.cin, L.cout, nodes, stack == 2);
        ft_layer_bwd(dy, red, p, L, ws, G, X, part);
    }
}

// ---- rotation head: d6 (the 6D rotation of one frame) -> q (w,x,y,z) = matrix_to_quaternion(rotation_6d_to_matrix(d6)) of pytorch3d 0.7.2 and, when dq
// (the gradient of q) is given, dd6 = what autograd gives on it.  In DOUBLE, the one place besides the re-fold: 20 threads per clip, a few hundred operations
// each, and the worst-conditioned link of the chain -- every parameter gradient is linear in these 20 x 9 seeds, and the PReLU-slope gradients are cancelling
// sums of 10^4 terms, so an fp32 head (3e-6 relative on a seed) alone costs them half of their 4 e_ref gate.
__device__ inline void ft_rot_head(const double *d, const double *dq, double *q, double *dd) {
    const double n1r = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]), n1 = fmax(n1r, 1e-12);
    const double b1[3] = {d[0] / n1, d[1] / n1, d[2] / n1};
    const double dt = b1[0] * d[3] + b1[1] * d[4] + b1[2] * d[5];
    const double u2[3] = {d[3] - dt * b1[0], d[4] - dt * b1[1], d[5] - dt * b1[2]};
    const double n2r = sqrt(u2[0] * u2[0] + u2[1] * u2[1] + u2[2] * u2[2]), n2 = fmax(n2r, 1e-12);
    const double b2[3] = {u2[0] / n2, u2[1] / n2, u2[2] / n2};
    double m[9] = {b1[0], b1[1], b1[2], b2[0], b2[1], b2[2], b1[1] * b2[2] - b1[2] * b2[1], b1[2] * b2[0] - b1[0] * b2[2], b1[0] * b2[1] - b1[1] * b2[0]};
    const double tr[4] = {1.0 + m[0] + m[4] + m[8], 1.0 + m[0] - m[4] - m[8], 1.0 - m[0] + m[4] - m[8], 1.0 - m[0] - m[4] + m[8]};
    double a[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) a[i] = tr[i] > 0.0 ? sqrt(tr[i]) : 0.0;
    int pick = 0;
    double best = a[0];
    if (a[1] > best) { best = a[1]; pick = 1; }
    if (a[2] > best) { best = a[2]; pick = 2; }
    if (a[3] > best) { best = a[3]; pick = 3; }
    const double den = 2.0 * fmax(best, 0.1);
    double c[4];
    if (pick == 0)      { c[0] = best * best; c[1] = m[7] - m[5]; c[2] = m[2] - m[6]; c[3] = m[3] - m[1]; }
    else if (pick == 1) { c[0] = m[7] - m[5]; c[1] = best * best; c[2] = m[3] + m[1]; c[3] = m[2] + m[6]; }
    else if (pick == 2) { c[0] = m[2] - m[6]; c[1] = m[3] + m[1]; c[2] = best * best; c[3] = m[5] + m[7]; }
    else                { c[0] = m[3] - m[1]; c[1] = m[6] + m[2]; c[2] = m[7] + m[5]; c[3] = best * best; }
#pragma unroll
    for (int j = 0; j < 4; ++j) q[j] = c[j] / den;
    if (!dq) return;
    double dc[4], dden = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        dc[j] = dq[j] / den;
        dden -= dq[j] * c[j] / (den * den);
    }
    const double da = (best >= 0.1 ? 2.0 * dden : 0.0) + 2.0 * best * dc[pick];
    const double dtr = tr[pick] > 0.0 ? da * 0.5 / best : 0.0;
    double dm[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    dm[0] = (pick <= 1 ? dtr : -dtr);
    dm[4] = (pick == 0 || pick == 2 ? dtr : -dtr);
    dm[8] = (pick == 0 || pick == 3 ? dtr : -dtr);
    if (pick == 0)      { dm[7] += dc[1]; dm[5] -= dc[1]; dm[2] += dc[2]; dm[6] -= dc[2]; dm[3] += dc[3]; dm[1] -= dc[3]; }
    else if (pick == 1) { dm[7] += dc[0]; dm[5] -= dc[0]; dm[3] += dc[2]; dm[1] += dc[2]; dm[2] += dc[3]; dm[6] += dc[3]; }
    else if (pick == 2) { dm[2] += dc[0]; dm[6] -= dc[0]; dm[3] += dc[1]; dm[1] += dc[1]; dm[5] += dc[3]; dm[7] += dc[3]; }
    else                { dm[3] += dc[0]; dm[1] -= dc[0]; dm[6] += dc[1]; dm[2] += dc[1]; dm[7] += dc[2]; dm[5] += dc[2]; }
    // rotation_6d_to_matrix: b3 = b1 x b2, b2 = u2 / |u2|, u2 = a2 - (b1 . a2) b1, b1 = a1 / |a1|
    const double *db3 = dm + 6;
    double db1[3] = {dm[0] + (b2[1] * db3[2] - b2[2] * db3[1]), dm[1] + (b2[2] * db3[0] - b2[0] * db3[2]), dm[2] + (b2[0] * db3[1] - b2[1] * db3[0])};
    const double db2[3] = {dm[3] + (db3[1] * b1[2] - db3[2] * b1[1]), dm[4] + (db3[2] * b1[0] - db3[0] * b1[2]), dm[5] + (db3[0] * b1[1] - db3[1] * b1[0])};
    double du2[3];
    {
        const double s = n2r >= 1e-12 ? b2[0] * db2[0] + b2[1] * db2[1] + b2[2] * db2[2] : 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i) du2[i] = (db2[i] - b2[i] * s) / n2;
    }
    const double ddt = -(du2[0] * b1[0] + du2[1] * b1[1] + du2[2] * b1[2]);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        db1[i] += -dt * du2[i] + ddt * d[3 + i];
        dd[3 + i] = du2[i] + ddt * b1[i];
    }
    {
        const double s = n1r >= 1e-12 ? b1[0] * db1[0] + b1[1] * db1[1] + b1[2] * db1[2] : 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i) dd[i] = (db1[i] - b1[i] * s) / n1;
    }
}

// ---- the pieces of a clip around the three stacks; sm: FT_LDS bytes = buf [BUF] | keep [KEEP] | small [FT_SMALL] | red [FT_RED].  All NTHR threads call
// each of them together.  The train-mode kernels (csrc/skeleton_bn_train.h) run the same pieces with a kernel boundary wherever a BatchNorm needs the batch.
#define FT_LDS_POINTERS \
    float *buf = sm, *keep = sm + BUF, *small = keep + KEEP; \
    float *og6 = small, *og = small + 96, *res = small + 288, *err = small + 480, *dres = small + 624;     /* [past][9] [9][NP] [NP][9] [NP][7] [NP][9] */ \
    double *errd = reinterpret_cast<double *>(small + 808);      /* [NP][7] the pose error in double (8-byte aligned: BUF + KEEP + 808 is even) */ \
    const int tid = threadIdx.x, past = op.past_len; \
    const float *Dp = op.arena + op.dct_pad, *Df = op.arena + op.dct, *Di = op.arena + op.idct; \
    (void)buf; (void)og6; (void)og; (void)res; (void)err; (void)dres; (void)errd; (void)past; (void)Dp; (void)Df; (void)Di; (void)tid;

// past object pose as 6D | translation, its DCT og, the relative branch's input -> buf and keep[.][.][1 + p]  (the non-hook path of skel_body, csrc/skeleton.h)
__device__ inline void ft_inputs(float *sm, const idf_skel_objproj &op, const Src &s, int B, int b) {
    FT_LDS_POINTERS
    if (tid < past) {
        const int t = tid;
        float m[6];
        const float *an = s.angles + ((size_t)t * B + b) * 4, *tt = s.trans + ((size_t)t * B + b) * 3;
        {                                                      // quaternion_to_matrix rows 0, 1 in double, rounded once
            const double r = an[3], i = an[0], j = an[1], k = an[2], s2 = 2.0 / (r * r + i * i + j * j + k * k);
            m[0] = (float)(1.0 - s2 * (j * j + k * k)); m[1] = (float)(s2 * (i * j - k * r)); m[2] = (float)(s2 * (i * k + j * r));
            m[3] = (float)(s2 * (i * j + k * r)); m[4] = (float)(1.0 - s2 * (i * i + k * k)); m[5] = (float)(s2 * (j * k - i * r));
        }
#pragma unroll
        for (int c = 0; c < 6; ++c) og6[t * CH + c] = m[c];
#pragma unroll
        for (int c = 0; c < 3; ++c) og6[t * CH + 6 + c] = tt[c];
    }
    __syncthreads();
    for (int i = tid; i < CH * NP; i += NTHR) {
        const int c = i / NP, k = i - c * NP;
        Acc2 v;
        for (int t = 0; t < past; ++t) v.mac(Dp[k * past + t], og6[t * CH + c]);
        og[i] = v.value();
    }
    __syncthreads();
    for (int i = tid; i < CH * NP * J; i += NTHR) {
        const int c = i / (NP * J), r = i - c * NP * J, k = r / J, p = r - k * J;
        float v = og[c * NP + k];
        if (c >= 6) {
            Acc2 h;
            for (int t = 0; t < past; ++t) h.mac(Dp[k * past + t], human_at<false>(s, B, b, t, p, c - 6));
            v -= h.value();
        }
        buf[i] = v;
        keep[c * NP * NJ + k * NJ + 1 + p] = v;
    }
    __syncthreads();
}

// buf = the relative stack's output: keep[.][.][1 + p] = rel + stack(rel) (+ the DCT of the body over all frames in the translation channels)
__device__ inline void ft_join_relative(float *sm, const idf_skel_objproj &op, const Src &s, int B, int b) {
    FT_LDS_POINTERS
    for (int i = tid; i < CH * NP * J; i += NTHR) {
        const int c = i / (NP * J), r = i - c * NP * J, k = r / J, p = r - k * J;
        float *kp = keep + c * NP * NJ + k * NJ + 1 + p;
        float v = *kp + buf[i];
        if (c >= 6) {
            Acc2 h;
            for (int t = 0; t < NP; ++t) h.mac(Df[k * NP + t], human_at<false>(s, B, b, t, p, c - 6));
            v += h.value();
        }
        *kp = v;
    }
    __syncthreads();
}

// the object-only stack's input: buf = og
__device__ inline void ft_object_input(float *sm, const idf_skel_objproj &op) {
    FT_LDS_POINTERS
    for (int i = tid; i < CH * NP; i += NTHR) buf[i] = og[i];
    __syncthreads();
}

// buf = the object-only stack's output: keep[.][.][0] = og + stack(og); then buf = keep, the joint stack's input
__device__ inline void ft_join_object(float *sm, const idf_skel_objproj &op) {
    FT_LDS_POINTERS
    for (int i = tid; i < CH * NP; i += NTHR) {
        const int c = i / NP, k = i - c * NP;
        keep[c * NP * NJ + k * NJ] = og[i] + buf[i];
    }
    __syncthreads();
    for (int i = tid; i < KEEP; i += NTHR) buf[i] = keep[i];
    __syncthreads();
}

// buf = the joint stack's output: keep += buf; the IDCT of node 0, the pose error and the clip's 8 sums of squares, the loss gradient on the pose and the
// rotation head's backward -> dres [NP][9]
__device__ inline void ft_head(float *sm, const idf_skel_objproj &op, const FtArgs &a, int B, int b) {
    FT_LDS_POINTERS
    for (int i = tid; i < KEEP; i += NTHR) keep[i] += buf[i];
    __syncthreads();
    for (int i = tid; i < NP * CH; i += NTHR) {
        const int t = i / CH, c = i - t * CH;
        Acc2 v;
        for (int k = 0; k < NP; ++k) v.mac(Di[t * NP + k], keep[c * NP * NJ + k * NJ]);
        res[i] = v.value();
    }
    __syncthreads();
    // ================= pose error, the clip's 8 sums of squares =================
    if (tid < NP) {
        const int t = tid;
        double d6[6], q[4];
#pragma unroll
        for (int c = 0; c < 6; ++c) d6[c] = res[t * CH + c];
        ft_rot_head(d6, nullptr, q, nullptr);
        const float *g = a.pose_gt + ((size_t)t * B + b) * 7, *tr = res + t * CH + 6;
        double *e = errd + t * 7;
        e[0] = (double)tr[0] - g[0]; e[1] = (double)tr[1] - g[1]; e[2] = (double)tr[2] - g[2];
        e[3] = q[1] - g[3]; e[4] = q[2] - g[4]; e[5] = q[3] - g[5]; e[6] = q[0] - g[6];
#pragma unroll
        for (int c = 0; c < 7; ++c) err[t * 7 + c] = (float)e[c];
    }
    __syncthreads();
    if (tid < 8) {
        // term tid: rot (channels 0..3) when even, nonrot (4..6) when odd; 0,1 past  2,3 future  4,5 past velocity  6,7 future velocity
        const int c0 = (tid & 1) ? 4 : 0, c1 = (tid & 1) ? 7 : 4, kind = tid >> 1;
        float acc = 0.f;
        for (int t = 0; t < NP; ++t) {
            const bool in = kind == 0 ? t < past : kind == 1 ? t >= past : kind == 2 ? t < past : t >= past;
            if (!in) continue;
            for (int c = c0; c < c1; ++c) {
                float v = err[t * 7 + c];
                if (kind == 2) v = err[(t + 1) * 7 + c] - v;
                if (kind == 3) v = v - err[(t - 1) * 7 + c];
                acc += v * v;
            }
        }
        a.loss_part[(size_t)b * 8 + tid] = acc;
    }
    // ================= loss gradient on the pose, rotation head backward =================
    if (tid < NP) {
        const int t = tid;
        double dp[7];
#pragma unroll
        for (int c = 0; c < 7; ++c) {
            const int nr = c < 4 ? 0 : 1;
            const double e = errd[t * 7 + c];
            double g = (double)(t < past ? a.coef[nr] : a.coef[2 + nr]) * e;
            // past velocity d_s = e[s+1] - e[s], s = 0 .. past-1
            double vp = 0.0;
            if (t >= 1 && t - 1 < past) vp += e - errd[(t - 1) * 7 + c];
            if (t < past) vp -= errd[(t + 1) * 7 + c] - e;
            g += (double)a.coef[4 + nr] * vp;
            // future velocity d_s = e[s] - e[s-1], s = past .. T-1
            double vf = 0.0;
            if (t >= past) vf += e - errd[(t - 1) * 7 + c];
            if (t + 1 >= past && t + 1 < NP) vf -= errd[(t + 1) * 7 + c] - e;
            g += (double)a.coef[6 + nr] * vf;
            dp[c] = g;
        }
        const double dq[4] = {dp[6], dp[3], dp[4], dp[5]};       // pose = translation | (x, y, z, w)
        double d6[6], q[4], dd[6];
#pragma unroll
        for (int c = 0; c < 6; ++c) d6[c] = res[t * CH + c];
        ft_rot_head(d6, dq, q, dd);
#pragma unroll
        for (int c = 0; c < 6; ++c) dres[t * CH + c] = (float)dd[c];
#pragma unroll
        for (int c = 0; c < 3; ++c) dres[t * CH + 6 + c] = (float)dp[c];
    }
    __syncthreads();
}

// IDCT of node 0: d keep[c][k][0] = sum_t idct[t][k] dres[t][c]; the other nodes get exactly 0.  -> keep and buf (the joint stack's output gradient)
__device__ inline void ft_head_bwd(float *sm, const idf_skel_objproj &op) {
    FT_LDS_POINTERS
    for (int i = tid; i < KEEP; i += NTHR) {
        const int c = i / (NP * NJ), r = i - c * NP * NJ, k = r / NJ, n = r - k * NJ;
        Acc2 acc;
        if (n == 0)
            for (int t = 0; t < NP; ++t) acc.mac(Di[t * NP + k], dres[t * CH + c]);
        const float v = acc.value();
        keep[i] = v;
        buf[i] = v;
    }
    __syncthreads();
}

// buf = the joint stack's input gradient: keep += buf (its skip connection); then buf = node 0, the object-only stack's output gradient (its own skip
// connection ends at the input)
__device__ inline void ft_split_object(float *sm) {
    float *buf = sm, *keep = sm + BUF;
    const int tid = threadIdx.x;
    for (int i = tid; i < KEEP; i += NTHR) keep[i] += buf[i];
    __syncthreads();
    for (int i = tid; i < CH * NP; i += NTHR) {
        const int c = i / NP, k = i - c * NP;
        buf[i] = keep[c * NP * NJ + k * NJ];
    }
    __syncthreads();
}

// buf = nodes 1.., the relative stack's output gradient
__device__ inline void ft_split_relative(float *sm) {
    float *buf = sm, *keep = sm + BUF;
    const int tid = threadIdx.x;
    for (int i = tid; i < CH * NP * J; i += NTHR) {
        const int c = i / (NP * J), r = i - c * NP * J, k = r / J, p = r - k * J;
        buf[i] = keep[c * NP * NJ + k * NJ + 1 + p];
    }
    __syncthreads();
}

// the whole clip: forward with saves, loss sums, loss gradient, backward.  All NTHR threads call it together; sm: FT_LDS bytes.
__device__ __forceinline__ void ft_clip_body(float *sm, const idf_skel_objproj &op, const Src &s, const FtPlan &plan, const FtArgs &a, int B, int b) {
    float *buf = sm, *red = sm + BUF + KEEP + FT_SMALL;
    float *ws = a.ws_clips + (size_t)b * plan.ws_clip, *G = ws + plan.ws_clip - 2 * BUF, *X = G + BUF;
    float *part = a.partials + (size_t)b * plan.n_param;
    ft_inputs(sm, op, s, B, b);
    ft_stack_fwd(buf, op, plan, 0, J, ws);
    ft_join_relative(sm, op, s, B, b);
    ft_object_input(sm, op);
    ft_stack_fwd(buf, op, plan, 1, 1, ws);
    ft_join_object(sm, op);
    ft_stack_fwd(buf, op, plan, 2, NJ, ws);
    ft_head(sm, op, a, B, b);
    ft_head_bwd(sm, op);
    ft_stack_bwd(buf, red, op, plan, 2, NJ, ws, G, X, part);
    ft_split_object(sm);
    ft_stack_bwd(buf, red, op, plan, 1, 1, ws, G, X, part);
    ft_split_relative(sm);
    ft_stack_bwd(buf, red, op, plan, 0, J, ws, G, X, part);
}

}  // namespace idf_skel_train
