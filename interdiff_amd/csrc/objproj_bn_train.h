// Training of the SMPL contact-frame correction predictor the way the reference trains it (train_correction_smpl.py: the module in train()): every
// BatchNorm2d normalises with the statistics of the BATCH and nn.Dropout follows the tcn BatchNorm (model/layers.py:308-318, :339-345); from epoch 10 on the
// contact node is drawn (model/correction_smpl.py:131-132) and arrives here as nodes[b].  Device code; launchers: csrc/objproj_bn_train.hip.  The train-mode
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
//   predict   17       after 0 .. 7 in place of 8: FIN(11) and the head up to the prediction, which goes out rounded once (a.obj_pred_out)
// The glue around the stacks -- the DCT, the skip connections and the head, in DOUBLE -- is the fine-tuner's (csrc/objproj_train.h ot_dct ..
// ot_split_relative): its clip body and the phases below call the same functions.  keep (double) crosses the launches 4 -> 8 and 8 -> 12 through the clip's
// workspace slice.
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
constexpr int TR_PHASE_PREDICT = TR_PHASES;            // after the forward phases 0 .. 7: the head without the backward (interdiff_correction_train_predict)
constexpr size_t TR_LDS = OT_LDS + (size_t)Tr::STAT * sizeof(double);
static_assert(OT_LDS % 8 == 0, "the statistics region of the LDS is read as doubles");
static_assert(TR_LDS + 64 <= 160 * 1024, "one workgroup per CU");

// the skip-connection saves are this predictor's keep planes in double: 2 KEEP floats each, 8-byte aligned in the clip's slice
inline TrPlan tr_plan(const FtPlan &P) { return idf_stgcn_train::tr_plan_for(P, NP, 2 * KEEP, true); }

__device__ __forceinline__ double *tr_stat_lds(float *sm) { return reinterpret_cast<double *>(reinterpret_cast<char *>(sm) + OT_LDS); }

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
    } else if (phase == TR_PHASE_PREDICT) {            // phase 8's forward half alone: the prediction -> a.obj_pred_out
        tr_keep_copy(keep, keepf);
        ot_dct(sm, op);
        Tr::tr_fin(c, 11);
        ot_head(sm, op, a, nodes, B, b);
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
