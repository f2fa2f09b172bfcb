// Fine-tuning of the SMPL contact-frame correction predictor with FROZEN normalisation statistics (the module in eval() with autograd on): the loss of
// LitInteraction.calc_loss (train_correction_smpl.py:60-101, the eight object-pose MSE terms -- what _common_step trains on while the annealed geometry
// weights are zero) on ObjProjector.forward(data, initialize) (model/correction_smpl.py:69-138), d loss / d theta for every entry of named_parameters(),
// and torch.optim.Adam (train_correction_smpl.py:51-58).  Device code; launchers: csrc/objproj_train.hip.  The ST-GCN layer's forward with saves and its
// backward, the compensated sum, the flat parameter plan and the fold / Adam / re-fold kernels are shared with the skeleton trainer: csrc/stgcn_train.h.
//
// ONE 16-wave workgroup per clip, like objproj_body (csrc/objproj.h), in three parts:
//   1. FORWARD on the folded layers of the arena the inference kernels read: st_gcn_layer's arithmetic with every sum compensated (Acc2) on the VALU.  Each
//      layer saves to the clip's workspace slice: its input planes x, (joint stack) the temporally mixed planes u, the mixed planes g the tcn convolution
//      reads, and the pre-activation h.  Node selection as the reference's eval branch: initialize -> the mean over the 68 nodes (taken in coefficient space,
//      it commutes with the IDCT), otherwise node 0 (no contact in the clip) or node 1 + argmax(contact + hand bonus); one IDCT of that column.  Everything
//      AROUND the stacks -- DCT, skip connections, selection, IDCT -- runs in double (see ot_dct .. ot_split_relative).
//   2. LOSS GRADIENT on the clip's [T][9] prediction, in double: the 8 MSE means are over the batch, so their normalisers are constants (coef[k] = 2 w_k / n_k);
//      the velocity terms couple adjacent frames of the same clip only.  d_obj_pred [T][B][9], when given, is ADDED to it: the gradient of whatever else the
//      caller's objective reads from the prediction (the seam of the contact / penetration terms, whose kernel is not part of this file).  The clip's 8 sums
//      of squares go to loss_part[b][8].
//   3. BACKWARD: the IDCT transposed; the selection (1/68 of the gradient to every node, or all of it to the selected node and EXACT zeros elsewhere); the
//      joint stack and its skip connection; node 0 -> the object-only stack, nodes 1.. -> the relative stack, each with its skip connection.  The inputs are
//      data: the input gradients of the stacks' first layers are not used.
// LDS (156 736 B): the layer buffer [32][680] fp32 (the gradient planes in the backward, in place: dy -> dh -> du -> dx), keep [9][10][68] in double (the skip
// connections, forward and backward), the head's vectors in double and a reduction buffer; the other operand of every product (x, u, g, h and the scratch
// plane sets G = Wt^T dh, X = Wr^T dh) comes from the clip's workspace slice, which only this workgroup touches (__syncthreads orders its global accesses
// at workgroup scope).
// Parameter gradients: partials[b][.] in the FLAT REFERENCE LAYOUT (FtPlan, csrc/stgcn_train.h), gradients of the FOLDED convolutions in the conv slots, plain
// stores, every element written by exactly one thread in a fixed summation order -- no atomics; two calls give the same bits.
#pragma once
#include "objproj.h"
#include "stgcn_train.h"

namespace idf_objproj_train {

using namespace idf_objproj_dev;
using idf_stgcn_train::FtLayer;
using idf_stgcn_train::FtPlan;
using Ft = idf_stgcn_train::StgcnFt<NP, VP>;

constexpr int NM = MAXN - 1;               // the 67 markers of the relative stack
constexpr int MAXC = 32;                   // widest layer (idf_objproj_check)
constexpr int MAXT = 64;                   // frames of a clip the head's LDS vectors are sized for
constexpr int BUF = MAXC * PLANE;          // the layer buffer (floats)
constexpr int KEEP = CH * PLANE;           // [9][n_pre][68]: node 0 = object, 1.. = markers (doubles)
// the head's vectors (doubles): dct [NP][MAXT] | og [9][NP] | col [9][NP] | dcol [9][NP] | err [MAXT][9] | dres [MAXT][9]
constexpr int OT_DCT = 0, OT_OG = OT_DCT + NP * MAXT, OT_COL = OT_OG + 96, OT_DCOL = OT_COL + 96, OT_ERR = OT_DCOL + 96, OT_DRES = OT_ERR + MAXT * CH;
constexpr int OT_HEAD = OT_DRES + MAXT * CH, OT_RED = NTHR;
constexpr size_t OT_LDS = (size_t)BUF * sizeof(float) + (size_t)(KEEP + OT_HEAD) * sizeof(double) + (size_t)OT_RED * sizeof(float);
static_assert(CH * NP <= 96 && BUF % 2 == 0, "the head's vectors; the doubles behind the layer buffer are 8-byte aligned");
static_assert(OT_LDS + 64 <= 160 * 1024, "one workgroup per CU");

// the flat parameter plan of this predictor: 67 / 1 / 68 nodes over NP = 10 coefficients
inline FtPlan ot_plan(const int32_t *cin, const int32_t *cout) { return idf_stgcn_train::ft_plan_for(cin, cout, NP, NM, BUF); }

// ---- host: what the launchers (csrc/objproj_train.hip, csrc/objproj_bn_train.hip) check before a launch
// the channel widths the kernels were built for (all the parameter table needs)
inline int ot_check_widths(const idf_objproj *op) {
    if (idf_objproj_check(op) != IDF_OK) return IDF_E_INVAL;
    for (int st = 0; st < 3; ++st) {
        if (op->cin[st * 4] != CH || op->cout[st * 4 + 3] != CH) return IDF_E_INVAL;
        for (int l = 0; l < 4; ++l) {
            const int li = st * 4 + l;
            if (op->cin[li] < 1 || op->cin[li] > MAXC || op->cout[li] < 1 || op->cout[li] > MAXC) return IDF_E_INVAL;
            if (l < 3 && op->cout[li] != op->cin[li + 1]) return IDF_E_INVAL;
        }
    }
    return IDF_OK;
}

inline int ot_check(const idf_objproj *op, int B) {
    if (ot_check_widths(op) != IDF_OK || !op->arena || B < 1 || op->T < 2 || op->T > MAXT || op->past_len >= op->T) return IDF_E_INVAL;
    for (int li = 0; li < 12; ++li)
        if (op->layer[li] < 0) return IDF_E_INVAL;
    return IDF_OK;
}

struct OtArgs {
    const float *obj_angles;   // [T][B][6] 6D rotation: input of the past frames and target of all
    const float *obj_trans;    // [T][B][3]
    const float *markers;      // [T][B][67][3]
    const int32_t *contact;    // [B][67] summed future contact labels (not read when initialize)
    const float *d_obj_pred;   // [T][B][9] added to the loss gradient at the prediction, or null
    float *partials;           // [B][n_param]
    float *loss_part;          // [B][8]
    float *ws_clips;           // [B][ws_clip]
    float coef[8];             // 2 w_k / n_k, MSE_KEYS order: rot_past, nonrot_past, rot_future, nonrot_future, then the four velocity terms
    int32_t initialize;
    float *obj_pred_out;       // [T][B][9] the prediction the loss reads, rounded once to fp32, or null (the predict entries set it)
};

__device__ __forceinline__ float ot_pose_at(const OtArgs &a, int B, int b, int t, int c) {
    return c < 6 ? a.obj_angles[((size_t)t * B + b) * 6 + c] : a.obj_trans[((size_t)t * B + b) * 3 + (c - 6)];
}
__device__ __forceinline__ float ot_marker_at(const OtArgs &a, int B, int b, int t, int p, int c) { return a.markers[(((size_t)t * B + b) * NM + p) * 3 + c]; }

__device__ inline void ot_stack_fwd(float *buf, const idf_objproj &op, const FtPlan &plan, int stack, int nodes, float *ws) {
#pragma unroll 1
    for (int l = 0; l < 4; ++l) {
        const int li = stack * 4 + l;
        const FtLayer &L = plan.L[li];
        const LayerP p = layer_params<NP, VP>(op.arena + op.layer[li], L.cin, L.cout, nodes, stack == 2);
        if (stack == 2) Ft::ft_layer_fwd<true>(buf, p, L.cin, L.cout, nodes, ws + L.ws_x, ws + L.ws_u, ws + L.ws_g, ws + L.ws_h);
        else Ft::ft_layer_fwd<false>(buf, p, L.cin, L.cout, nodes, ws + L.ws_x, nullptr, ws + L.ws_g, ws + L.ws_h);
    }
}

__device__ inline void ot_stack_bwd(float *dy, float *red, const idf_objproj &op, const FtPlan &plan, int stack, int nodes, const float *ws, float *G, float *X,
                                    float *part) {
#pragma unroll 1
    for (int l = 3; l >= 0; --l) {
        const int li = stack * 4 + l;
        const FtLayer &L = plan.L[li];
        const LayerP p = layer_params<NP, VP>(op.arena + op.layer[li], L.cin, L.cout, nodes, stack == 2);
        Ft::ft_layer_bwd(dy, red, p, L, ws, G, X, part);
    }
}

// ---- the clip's glue around the stacks, one function per section so that the train-mode phases (csrc/objproj_bn_train.h) can end a launch between any
// two of them.  sm: the LDS = buf [BUF] floats | keep [KEEP] doubles | the head's vectors [OT_HEAD] doubles | red [OT_RED] floats.
// The SKIP PATH and the HEAD run in DOUBLE: the DCT matrix (formed from its definition, get_dct_matrix of model/correction_smpl.py:55-67; its inverse is its
// transpose), the DCT of the inputs, the three skip connections, the selection, the IDCT, the prediction error and the loss gradient.  The prediction is
// the (padded) past pose put through DCT and IDCT plus a small correction, and the loss gradient is proportional to prediction - target, a difference ~1e-2
// of O(1) values: fp32 roundings of the DCT matrices and of the skip sums alone put the PReLU-slope gradient of st_gcnns.3 at 2e-5 of its fp64 value, twice
// its gate.  The stacks read the skip path rounded to fp32 once and run in compensated fp32.
#define OT_LDS_POINTERS \
    float *buf = sm; \
    double *keep = reinterpret_cast<double *>(sm + BUF), *head = keep + KEEP; \
    double *Dd = head + OT_DCT, *og = head + OT_OG, *col = head + OT_COL, *dcol = head + OT_DCOL, *err = head + OT_ERR, *dres = head + OT_DRES; \
    const int tid = threadIdx.x, T = op.T, past = op.past_len; \
    (void)buf; (void)keep; (void)Dd; (void)og; (void)col; (void)dcol; (void)err; (void)dres; (void)tid; (void)T; (void)past;

__device__ __forceinline__ float *ot_red(float *sm) { return reinterpret_cast<float *>(reinterpret_cast<double *>(sm + BUF) + KEEP + OT_HEAD); }

// the orthonormal DCT-II matrix Dd[k][t], k < NP (numpy's expression order); the IDCT is its transpose
__device__ inline void ot_dct(float *sm, const idf_objproj &op) {
    OT_LDS_POINTERS
    for (int i = tid; i < NP * T; i += NTHR) {
        const int k = i / T, t = i - k * T;
        Dd[i] = sqrt((k == 0 ? 1.0 : 2.0) / (double)T) * cos(M_PI * ((double)t + 0.5) * (double)k / (double)T);
    }
    __syncthreads();
}

// the DCT matrix, the object's DCT coefficients og, the relative stack's input -> buf and keep[.][.][1 + p]
__device__ inline void ot_inputs(float *sm, const idf_objproj &op, const OtArgs &a, int B, int b) {
    OT_LDS_POINTERS
    ot_dct(sm, op);
    // object DCT coefficients og[c][k] over the idx_pad frames (the future frames repeat the last past frame)
    for (int i = tid; i < CH * NP; i += NTHR) {
        const int c = i / NP, k = i - c * NP;
        double v = 0.0;
        for (int t = 0; t < T; ++t) v += Dd[k * T + t] * (double)ot_pose_at(a, B, b, min(t, past - 1), c);
        og[i] = v;
    }
    __syncthreads();
    // the relative stack's input rel[c][k][p] -> buf (67 nodes) and keep[.][.][1 + p]
    for (int i = tid; i < CH * NP * NM; i += NTHR) {
        const int c = i / (NP * NM), r = i - c * NP * NM, k = r / NM, p = r - k * NM;
        double v = og[c * NP + k];
        if (c >= 6) {
            double h = 0.0;
            for (int t = 0; t < T; ++t) h += Dd[k * T + t] * (double)ot_marker_at(a, B, b, min(t, past - 1), p, c - 6);
            v -= h;
        }
        buf[i] = (float)v;
        keep[c * PLANE + k * MAXN + 1 + p] = v;
    }
    __syncthreads();
}

// buf = the relative stack's output: keep[.][.][1 + p] = rel + stack(rel) (+ the DCT of the markers over ALL frames in the translation channels)
__device__ inline void ot_join_relative(float *sm, const idf_objproj &op, const OtArgs &a, int B, int b) {
    OT_LDS_POINTERS
    for (int i = tid; i < CH * NP * NM; i += NTHR) {
        const int c = i / (NP * NM), r = i - c * NP * NM, k = r / NM, p = r - k * NM;
        double *kp = keep + c * PLANE + k * MAXN + 1 + p;
        double v = *kp + (double)buf[i];
        if (c >= 6) {
            double h = 0.0;
            for (int t = 0; t < T; ++t) h += Dd[k * T + t] * (double)ot_marker_at(a, B, b, t, p, c - 6);
            v += h;
        }
        *kp = v;
    }
    __syncthreads();
}

// the object-only stack's input (1 node): buf = og
__device__ inline void ot_object_input(float *sm, const idf_objproj &op) {
    OT_LDS_POINTERS
    for (int i = tid; i < CH * NP; i += NTHR) buf[i] = (float)og[i];
    __syncthreads();
}

// buf = the object-only stack's output: keep[.][.][0] = og + stack(og); then buf = keep, the joint stack's input over the 68 nodes
__device__ inline void ot_join_object(float *sm, const idf_objproj &op) {
    OT_LDS_POINTERS
    for (int i = tid; i < CH * NP; i += NTHR) {
        const int c = i / NP, k = i - c * NP;
        keep[c * PLANE + k * MAXN] = og[i] + (double)buf[i];
    }
    __syncthreads();
    for (int i = tid; i < KEEP; i += NTHR) buf[i] = (float)keep[i];
    __syncthreads();
}

// buf = the joint stack's output: keep += buf (its skip connection); node selection, one IDCT, the prediction error, the clip's 8 sums of squares and the
// loss gradient on the prediction -> dres.  nodes: [B] the node of every clip, or null: the reference's eval branch.  -> the node (-1: the mean)
__device__ inline int ot_head(float *sm, const idf_objproj &op, const OtArgs &a, const int32_t *nodes, int B, int b) {
    OT_LDS_POINTERS
    __shared__ int pick_s;
    for (int i = tid; i < KEEP; i += NTHR) keep[i] += (double)buf[i];
    // node selection (correction_smpl.py:122-136): -1 = the mean over the nodes
    if (tid == 0) {
        int pick = -1;
        if (!a.initialize) {
            if (nodes) {
                pick = min(max(nodes[b], 0), MAXN - 1);
            } else {
                const float *bonus = op.arena + op.hand_bonus;
                long csum = 0;
                float best = -1.f;
                int bi = 0;
                for (int p = 0; p < NM; ++p) {
                    const int cv = a.contact[(size_t)b * NM + p];
                    csum += cv;
                    const float sc = (float)cv + bonus[p];
                    if (sc > best) { best = sc; bi = p; }
                }
                pick = csum > 0 ? 1 + bi : 0;
            }
        }
        pick_s = pick;
    }
    __syncthreads();
    const int pick = pick_s;
    for (int i = tid; i < CH * NP; i += NTHR) {
        const double *row = keep + (i / NP) * PLANE + (i % NP) * MAXN;
        double v;
        if (pick < 0) {
            v = 0.0;
            for (int n = 0; n < MAXN; ++n) v += row[n];
            v /= (double)MAXN;
        } else {
            v = row[pick];
        }
        col[i] = v;
    }
    __syncthreads();
    for (int i = tid; i < T * CH; i += NTHR) {
        const int t = i / CH, c = i - t * CH;
        double v = 0.0;
        for (int k = 0; k < NP; ++k) v += Dd[k * T + t] * col[c * NP + k];
        if (a.obj_pred_out) a.obj_pred_out[((size_t)t * B + b) * CH + c] = (float)v;
        err[i] = v - (double)ot_pose_at(a, B, b, t, c);
    }
    __syncthreads();
    // ================= the clip's 8 sums of squares =================
    if (tid < 8) {
        // term tid: rot (channels 0..5) when even, nonrot (6..8) when odd; 0,1 past  2,3 future  4,5 past velocity  6,7 future velocity
        const int c0 = (tid & 1) ? 6 : 0, c1 = (tid & 1) ? CH : 6, kind = tid >> 1;
        double acc = 0.0;
        for (int t = 0; t < T; ++t) {
            const bool in = (kind == 0 || kind == 2) ? t < past : t >= past;
            if (!in) continue;
            for (int c = c0; c < c1; ++c) {
                double v = err[t * CH + c];
                if (kind == 2) v = err[(t + 1) * CH + c] - v;
                if (kind == 3) v = v - err[(t - 1) * CH + c];
                acc += v * v;
            }
        }
        a.loss_part[(size_t)b * 8 + tid] = (float)acc;
    }
    // ================= loss gradient on the prediction =================
    for (int i = tid; i < T * CH; i += NTHR) {
        const int t = i / CH, c = i - t * CH, nr = c < 6 ? 0 : 1;
        const double e = err[i];
        double g = (double)(t < past ? a.coef[nr] : a.coef[2 + nr]) * e;
        // past velocity d_s = e[s+1] - e[s], s = 0 .. past-1
        double vp = 0.0;
        if (t >= 1 && t - 1 < past) vp += e - err[(t - 1) * CH + c];
        if (t < past) vp -= err[(t + 1) * CH + c] - e;
        g += (double)a.coef[4 + nr] * vp;
        // future velocity d_s = e[s] - e[s-1], s = past .. T-1
        double vf = 0.0;
        if (t >= past) vf += e - err[(t - 1) * CH + c];
        if (t + 1 >= past && t + 1 < T) vf -= err[(t + 1) * CH + c] - e;
        g += (double)a.coef[6 + nr] * vf;
        if (a.d_obj_pred) g += (double)a.d_obj_pred[((size_t)t * B + b) * CH + c];
        dres[i] = g;
    }
    __syncthreads();
    return pick;
}

// IDCT transposed: dcol[c][k] = sum_t Dd[k][t] dres[t][c]; the selection: the mean hands every node 1/68, a selected node takes all and the others
// EXACTLY 0.  -> keep and buf (the joint stack's output gradient)
__device__ inline void ot_head_bwd(float *sm, const idf_objproj &op, int pick) {
    OT_LDS_POINTERS
    for (int i = tid; i < CH * NP; i += NTHR) {
        const int c = i / NP, k = i - c * NP;
        double v = 0.0;
        for (int t = 0; t < T; ++t) v += Dd[k * T + t] * dres[t * CH + c];
        dcol[i] = v;
    }
    __syncthreads();
    for (int i = tid; i < KEEP; i += NTHR) {
        const int c = i / PLANE, r = i - c * PLANE, k = r / MAXN, n = r - k * MAXN;
        const double d = dcol[c * NP + k];
        const double v = pick < 0 ? d / (double)MAXN : n == pick ? d : 0.0;
        keep[i] = v;
        buf[i] = (float)v;
    }
    __syncthreads();
}

// buf = the joint stack's input gradient: keep += buf (its skip connection); then buf = node 0, the object-only stack's output gradient (that stack's own
// skip connection ends at the input)
__device__ inline void ot_split_object(float *sm) {
    float *buf = sm;
    double *keep = reinterpret_cast<double *>(sm + BUF);
    const int tid = threadIdx.x;
    for (int i = tid; i < KEEP; i += NTHR) keep[i] += (double)buf[i];
    __syncthreads();
    for (int i = tid; i < CH * NP; i += NTHR) {
        const int c = i / NP, k = i - c * NP;
        buf[i] = (float)keep[c * PLANE + k * MAXN];
    }
    __syncthreads();
}

// buf = nodes 1.., the relative stack's output gradient
__device__ inline void ot_split_relative(float *sm) {
    float *buf = sm;
    const double *keep = reinterpret_cast<const double *>(sm + BUF);
    const int tid = threadIdx.x;
    for (int i = tid; i < CH * NP * NM; i += NTHR) {
        const int c = i / (NP * NM), r = i - c * NP * NM, k = r / NM, p = r - k * NM;
        buf[i] = (float)keep[c * PLANE + k * MAXN + 1 + p];
    }
    __syncthreads();
}

// the whole clip: forward with saves, loss sums, loss gradient, backward.  All NTHR threads call it together; sm: OT_LDS bytes.  The node is the
// reference's eval branch (ot_head with nodes = nullptr).
__device__ __forceinline__ void ot_clip_body(float *sm, const idf_objproj &op, const FtPlan &plan, const OtArgs &a, int B, int b) {
    float *ws = a.ws_clips + (size_t)b * plan.ws_clip, *G = ws + plan.ws_clip - 2 * BUF, *X = G + BUF;
    float *part = a.partials + (size_t)b * plan.n_param, *red = ot_red(sm);
    ot_inputs(sm, op, a, B, b);
    ot_stack_fwd(sm, op, plan, 0, NM, ws);
    ot_join_relative(sm, op, a, B, b);
    ot_object_input(sm, op);
    ot_stack_fwd(sm, op, plan, 1, 1, ws);
    ot_join_object(sm, op);
    ot_stack_fwd(sm, op, plan, 2, MAXN, ws);
    const int pick = ot_head(sm, op, a, nullptr, B, b);
    ot_head_bwd(sm, op, pick);
    ot_stack_bwd(sm, red, op, plan, 2, MAXN, ws, G, X, part);
    ot_split_object(sm);
    ot_stack_bwd(sm, red, op, plan, 1, 1, ws, G, X, part);
    ot_split_relative(sm);
    ot_stack_bwd(sm, red, op, plan, 0, NM, ws, G, X, part);
}

// the forward half of ot_clip_body alone, up to the head: the prediction goes to a.obj_pred_out (interdiff_correction_finetune_predict).  The saves and the
// clip's loss sums land in the workspace as in the gradient call; no parameter gradient is written.
__device__ __forceinline__ void ot_clip_predict(float *sm, const idf_objproj &op, const FtPlan &plan, const OtArgs &a, int B, int b) {
    float *ws = a.ws_clips + (size_t)b * plan.ws_clip;
    ot_inputs(sm, op, a, B, b);
    ot_stack_fwd(sm, op, plan, 0, NM, ws);
    ot_join_relative(sm, op, a, B, b);
    ot_object_input(sm, op);
    ot_stack_fwd(sm, op, plan, 1, 1, ws);
    ot_join_object(sm, op);
    ot_stack_fwd(sm, op, plan, 2, MAXN, ws);
    ot_head(sm, op, a, nullptr, B, b);
}

}  // namespace idf_objproj_train
