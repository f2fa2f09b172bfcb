// Training of the SMPL contact-frame correction predictor the way the reference trains it (train_correction_smpl.py: the module in train()): every
// BatchNorm2d normalises with the statistics of the BATCH and nn.Dropout follows the tcn BatchNorm (model/layers.py:308-318, :339-345); from epoch 10 on the
// contact node is drawn (model/correction_smpl.py:131-132) and arrives here as nodes[b].  Device code; launchers: csrc/objproj_train.hip.  The train-mode
// ST-GCN layer (FRONT, FIN, A, B), the Chan fold of the statistics, the keep masks and their Philox generator are csrc/stgcn_bn_train.h's, shared with the
// skeleton trainer; the flat parameter plan, the compensated sum and the graph forward / backward are the fine-tuner's (csrc/stgcn_train.h).
//
// The batch statistics couple all clips, so the network is CUT AT KERNEL BOUNDARIES, one cut per layer depth and direction -- no grid barrier inside a kernel.
// One 1024-thread workgroup per clip in every phase (objproj_tr_phase_kernel, phase = 0 .. 16); the relative (67-node) and the object (1-node) stacks are
// independent of each other and share their phases -- the skeleton trainer's table (csrc/skeleton_bn_train.h):
//   forward   0        inputs; FRONT(0), FRONT(4)
//             1..3     FIN(l-1), FRONT(l) for the layers l = phase and 4 + phase
//             4        inputs again (the LDS does not outlive a launch); FIN(3), FIN(7), the skip connections and the joint stack's input; FRONT(8)
//             5..7     FIN(l-1), FRONT(l), l = 4 + phase
//             8        FIN(11); the head in double: selection, one IDCT, the 8 sums of squares, the loss gradient (+ d_obj_pred), IDCT transposed; A(11)
//   backward  9..11    B(l), A(l-1), l = 20 - phase
//             12       B(8), the skip connections; A(7), A(3)
//             13..15   B(l), A(l-1) for l = 20 - phase and 16 - phase
//             16       B(4), B(0)
// The pieces around the stacks below are ot_clip_body's (csrc/objproj_train.h) sections, statement for statement -- the DCT, the skip connections and the head
// in DOUBLE for the reason given there -- as separate functions, so that a launch can end between any two of them.  The fine-tuner's kernel
// keeps its one-piece body: it is not recompiled by this file.  keep (double) crosses the launches 4 -> 8 and 8 -> 12 through the clip's workspace slice.
// LDS: the fine-tuner's 156 736 B + mu / rstd / the two seam means of 2 x 32 channels in double (2 048 B) = 158 784 B.
// Parameter gradients: partials[b][.] by plain stores in the flat reference layout, folded over the clips in ascending order (stgcn_ft_fold_kernel): no
// atomics; two calls give the same bits at any B.
#pragma once
#include "objproj_train.h"
#include "stgcn_bn_train.h"

namespace idf_objproj_train {

using idf_stgcn_train::TR_PHASES;
using idf_stgcn_train::TrArgs;
using idf_stgcn_train::TrCtx;
using idf_stgcn_train::TrPlan;
using Tr = idf_stgcn_train::StgcnTr<NP, VP, MAXC, BUF>;

constexpr int TR_SEAM = Tr::SEAM;
constexpr size_t TR_LDS = OT_LDS + (size_t)Tr::STAT * sizeof(double);
static_assert(OT_LDS % 8 == 0, "the statistics region of the LDS is read as doubles");
static_assert(TR_LDS + 64 <= 160 * 1024, "one workgroup per CU");

// the skip-connection saves are this predictor's keep planes in double: 2 KEEP floats each, 8-byte aligned in the clip's slice
inline TrPlan tr_plan(const FtPlan &P) { return idf_stgcn_train::tr_plan_for(P, NP, 2 * KEEP, true); }

__device__ __forceinline__ double *tr_stat_lds(float *sm) { return reinterpret_cast<double *>(reinterpret_cast<char *>(sm) + OT_LDS); }

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

__device__ inline void tr_keep_copy(double *dst, const double *src) {
    for (int i = threadIdx.x; i < KEEP; i += NTHR) dst[i] = src[i];
    __syncthreads();
}

// one phase of one clip (table at the top).  All NTHR threads call it together; sm: TR_LDS bytes.  nodes: [B] or null (ot_head)
__device__ __forceinline__ void tr_phase_body(float *sm, const idf_objproj &op, const FtPlan &plan, const TrPlan &tp, const OtArgs &a, const TrArgs &t,
                                              const int32_t *nodes, int B, int b, int phase) {
    float *ws = a.ws_clips + (size_t)b * tp.ws_clip;
    double *keep = reinterpret_cast<double *>(sm + BUF), *keepf = reinterpret_cast<double *>(ws + tp.keepf), *keepb = reinterpret_cast<double *>(ws + tp.keepb);
    const TrCtx c{sm, ot_red(sm), tr_stat_lds(sm), op.arena, op.layer, plan, tp, t, B, b, ws, a.partials + (size_t)b * plan.n_param};
    if (phase == 0) {
        ot_inputs(sm, op, a, B, b);
        Tr::tr_front(c, 0);
        ot_object_input(sm, op);
        Tr::tr_front(c, 4);
    } else if (phase <= 3) {
        Tr::tr_fin(c, phase - 1);
        Tr::tr_front(c, phase);
        Tr::tr_fin(c, 3 + phase);
        Tr::tr_front(c, 4 + phase);
    } else if (phase == 4) {
        ot_inputs(sm, op, a, B, b);
        Tr::tr_fin(c, 3);
        ot_join_relative(sm, op, a, B, b);
        Tr::tr_fin(c, 7);
        ot_join_object(sm, op);
        tr_keep_copy(keepf, keep);
        Tr::tr_front(c, 8);
    } else if (phase <= 7) {
        Tr::tr_fin(c, 3 + phase);
        Tr::tr_front(c, 4 + phase);
    } else if (phase == 8) {
        tr_keep_copy(keep, keepf);
        ot_dct(sm, op);
        Tr::tr_fin(c, 11);
        const int pick = ot_head(sm, op, a, nodes, B, b);
        ot_head_bwd(sm, op, pick);
        tr_keep_copy(keepb, keep);
        Tr::tr_bwd_a(c, 11);
    } else if (phase <= 11) {
        Tr::tr_bwd_b(c, 20 - phase);
        Tr::tr_bwd_a(c, 19 - phase);
    } else if (phase == 12) {
        Tr::tr_bwd_b(c, 8);
        tr_keep_copy(keep, keepb);
        ot_split_object(sm);
        Tr::tr_bwd_a(c, 7);
        ot_split_relative(sm);
        Tr::tr_bwd_a(c, 3);
    } else if (phase <= 15) {
        Tr::tr_bwd_b(c, 20 - phase);
        Tr::tr_bwd_a(c, 19 - phase);
        Tr::tr_bwd_b(c, 16 - phase);
        Tr::tr_bwd_a(c, 15 - phase);
    } else {
        Tr::tr_bwd_b(c, 4);
        Tr::tr_bwd_b(c, 0);
    }
}

}  // namespace idf_objproj_train
