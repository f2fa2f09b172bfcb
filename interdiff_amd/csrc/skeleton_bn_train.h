// Training of the HO-GCN skeleton correction predictor the way the reference trains it (train_correction_skeleton.py: the module in train()): every
// BatchNorm2d normalises with the statistics of the BATCH and nn.Dropout follows the tcn BatchNorm (model/layers.py:308-318, :339-345).  Device code;
// launchers: csrc/skeleton_train.hip.  Built AROUND the fine-tuner's per-clip code (csrc/skeleton_train.h): the temporal mix, the adjacency product, the PReLU
// and graph backward, the rotation head, the loss gradient and the glue between the stacks are the same device functions.
//
//     res = BN_r(conv_r(x));  g = gcn(x);  y = dropout(BN_t(conv_t(g)));  h = y + res;  out = PReLU(h)
//
// The batch statistics couple all clips, so the network is CUT AT KERNEL BOUNDARIES, one cut per layer depth and direction -- no grid barrier inside a kernel.
// One 1024-thread workgroup per clip in every phase (skel_tr_phase_kernel, phase = 0 .. 16); the relative (21-node) and the object (1-node) stacks are
// independent of each other and share their phases:
//   forward   0        inputs; FRONT(0), FRONT(4)
//             1..3     FIN(l-1), FRONT(l) for the layers l = phase and 4 + phase
//             4        FIN(3), FIN(7), the skip connections and the joint stack's input; FRONT(8)
//             5..7     FIN(l-1), FRONT(l), l = 4 + phase
//             8        FIN(11); pose, loss sums, loss gradient, rotation head and IDCT backward; A(11)
//   backward  9..11    B(l), A(l-1), l = 20 - phase
//             12       B(8), the skip connections; A(7), A(3)
//             13..15   B(l), A(l-1) for l = 20 - phase and 16 - phase
//             16       B(4), B(0)
// FRONT, FIN, A and B are the four pieces of the train-mode ST-GCN layer both predictors' trainers share (csrc/stgcn_bn_train.h, StgcnTr; there too: the Chan
// fold of the statistics, the keep masks and their Philox generator, the exact-zero convolution-bias gradients -- DESIGN.md 8.10).
// Parameter gradients: partials[b][.] by plain stores in the flat reference layout, folded over the clips in ascending order (stgcn_ft_fold_kernel, csrc/stgcn_train.h): no atomics;
// two calls give the same bits at any B.
#pragma once
#include "skeleton_train.h"
#include "stgcn_bn_train.h"

namespace idf_skel_train {

using idf_stgcn_train::TR_PHASES;
using idf_stgcn_train::TrArgs;
using idf_stgcn_train::TrCtx;
using idf_stgcn_train::TrPlan;
using Tr = idf_stgcn_train::StgcnTr<NP, VP, MAXC, BUF>;

constexpr int TR_STAT = Tr::STAT, TR_SEAM = Tr::SEAM;
constexpr size_t TR_LDS = FT_LDS + (size_t)TR_STAT * sizeof(double);
static_assert((BUF + KEEP + FT_SMALL + FT_RED) % 2 == 0, "the statistics region of the LDS is read as doubles");

// the skip-connection saves are this predictor's fp32 keep planes
inline TrPlan tr_plan(const FtPlan &P) { return idf_stgcn_train::tr_plan_for(P, NP, KEEP); }

__device__ __forceinline__ double *tr_stat_lds(float *sm) { return reinterpret_cast<double *>(sm + BUF + KEEP + FT_SMALL + FT_RED); }

__device__ inline void tr_front(const TrCtx &c, int li) { Tr::tr_front(c, li); }
__device__ inline void tr_fin(const TrCtx &c, int li) { Tr::tr_fin(c, li); }
__device__ inline void tr_bwd_a(const TrCtx &c, int li) { Tr::tr_bwd_a(c, li); }
__device__ inline void tr_bwd_b(const TrCtx &c, int li) { Tr::tr_bwd_b(c, li); }

__device__ inline void tr_keep_copy(float *dst, const float *src) {
    for (int i = threadIdx.x; i < KEEP; i += NTHR) dst[i] = src[i];
    __syncthreads();
}

// one phase of one clip (table at the top).  All NTHR threads call it together; sm: TR_LDS bytes.
__device__ __forceinline__ void tr_phase_body(float *sm, const idf_skel_objproj &op, const Src &s, const FtPlan &plan, const TrPlan &tp, const FtArgs &a,
                                              const TrArgs &t, int B, int b, int phase) {
    float *ws = a.ws_clips + (size_t)b * tp.ws_clip, *keep = sm + BUF;
    const TrCtx c{sm, sm + BUF + KEEP + FT_SMALL, tr_stat_lds(sm), op.arena, op.layer, plan, tp, t, B, b, ws, a.partials + (size_t)b * plan.n_param};
    if (phase == 0) {
        ft_inputs(sm, op, s, B, b);
        tr_front(c, 0);
        ft_object_input(sm, op);
        tr_front(c, 4);
    } else if (phase <= 3) {
        tr_fin(c, phase - 1);
        tr_front(c, phase);
        tr_fin(c, 3 + phase);
        tr_front(c, 4 + phase);
    } else if (phase == 4) {
        ft_inputs(sm, op, s, B, b);
        tr_fin(c, 3);
        ft_join_relative(sm, op, s, B, b);
        tr_fin(c, 7);
        ft_join_object(sm, op);
        tr_keep_copy(ws + tp.keepf, keep);
        tr_front(c, 8);
    } else if (phase <= 7) {
        tr_fin(c, 3 + phase);
        tr_front(c, 4 + phase);
    } else if (phase == 8) {
        tr_keep_copy(keep, ws + tp.keepf);
        tr_fin(c, 11);
        ft_head(sm, op, a, B, b);
        ft_head_bwd(sm, op);
        tr_keep_copy(ws + tp.keepb, keep);
        tr_bwd_a(c, 11);
    } else if (phase <= 11) {
        tr_bwd_b(c, 20 - phase);
        tr_bwd_a(c, 19 - phase);
    } else if (phase == 12) {
        tr_bwd_b(c, 8);
        tr_keep_copy(keep, ws + tp.keepb);
        ft_split_object(sm);
        tr_bwd_a(c, 7);
        ft_split_relative(sm);
        tr_bwd_a(c, 3);
    } else if (phase <= 15) {
        tr_bwd_b(c, 20 - phase);
        tr_bwd_a(c, 19 - phase);
        tr_bwd_b(c, 16 - phase);
        tr_bwd_a(c, 15 - phase);
    } else {
        tr_bwd_b(c, 4);
        tr_bwd_b(c, 0);
    }
}

}  // namespace idf_skel_train
