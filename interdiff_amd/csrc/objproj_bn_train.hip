// Training of the SMPL contact-frame correction predictor with batch statistics, dropout and given contact nodes: launchers of the phase kernel
// (csrc/objproj_bn_train.h) and of the kernels around it -- the mask generator and the batch statistics / running-buffer update (csrc/stgcn_bn_train.h), the
// fold of the per-clip partials in ascending clip order (csrc/stgcn_train.h).  Adam and the re-fold are the fine-tuner's interdiff_correction_finetune_step
// (csrc/objproj_train.hip).  A translation unit of its own, next to the fine-tuner's.
#include <math.h>
#include "objproj_bn_train.h"

namespace {
using namespace idf_objproj_train;
using namespace idf_stgcn_train;

__global__ __launch_bounds__(NTHR) void objproj_tr_phase_kernel(const idf_objproj op, const FtPlan plan, const TrPlan tp, const OtArgs a, const TrArgs t,
                                                                const int32_t *nodes, int B, int phase) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    tr_phase_body(sm, op, plan, tp, a, t, nodes, B, blockIdx.x, phase);
}

}  // namespace

extern "C" size_t interdiff_correction_train_workspace_bytes(const idf_objproj *op, int32_t B) {
    if (B < 1 || ot_check_widths(op) != IDF_OK) return 0;
    const FtPlan P = ot_plan(op->cin, op->cout);
    return tr_ws(P, tr_plan(P), B, TR_SEAM).total * sizeof(float);
}

extern "C" int interdiff_correction_train_masks(const idf_objproj *op, int32_t B, double p_drop, uint64_t seed, uint64_t step, uint8_t *masks_out,
                                                void *stream) {
    if (!masks_out || ot_check_widths(op) != IDF_OK || B < 1 || !(p_drop >= 0.0 && p_drop < 1.0)) return IDF_E_INVAL;
    const FtPlan P = ot_plan(op->cin, op->cout);
    stgcn_tr_launch_masks<NP>(P, tr_plan(P), B, p_drop, seed, step, masks_out, idf_stream(stream));
    IDF_CHECK_LAUNCH();
    return IDF_OK;
}

extern "C" int interdiff_correction_train_grads(const idf_objproj *op, const float *params, float *bn, const float *obj_angles, const float *obj_trans,
                                                const float *markers, const int32_t *contact, const int32_t *nodes, const float *d_obj_pred, int32_t B,
                                                int32_t T, int32_t initialize, const float *weights8, double p_drop, const uint8_t *masks, uint64_t seed,
                                                uint64_t step, double momentum, int32_t update_running, float *out9, float *grads, float *batch_stats,
                                                void *ws, size_t ws_bytes, void *stream) {
    if (!params || !bn || !obj_angles || !obj_trans || !markers || !weights8 || !out9 || !grads || !ws) return IDF_E_INVAL;
    if (!initialize && !contact && !nodes) return IDF_E_INVAL;
    if (ot_check(op, B) != IDF_OK || T != op->T) return IDF_E_INVAL;
    if (!(p_drop >= 0.0 && p_drop < 1.0) || !(momentum >= 0.0 && momentum <= 1.0) || (update_running != 0 && update_running != 1)) return IDF_E_INVAL;
    const FtPlan P = ot_plan(op->cin, op->cout);
    const TrPlan TP = tr_plan(P);
    const TrWs W = tr_ws(P, TP, B, TR_SEAM);
    if (ws_bytes < W.total * sizeof(float)) return IDF_E_INVAL;
    float *base = static_cast<float *>(ws);
    hipStream_t st = idf_stream(stream);
    OtArgs a{};
    const LossK lk = ft_loss_constants(weights8, op->past_len, T, B, 6, a.coef);
    a.obj_angles = obj_angles; a.obj_trans = obj_trans; a.markers = markers; a.contact = contact; a.d_obj_pred = d_obj_pred;
    a.partials = base + W.partials;
    a.loss_part = base + W.loss_part;
    a.ws_clips = base + W.clips;
    a.initialize = initialize != 0;
    static std::atomic<uint64_t> lds_ok{0};
    if (idf_opt_in_lds(reinterpret_cast<const void *>(objproj_tr_phase_kernel), (int)TR_LDS, lds_ok) != IDF_OK) return IDF_E_LAUNCH;
    return stgcn_tr_launch_grads<Tr, NP, MAXC>(P, TP, W, base, B, lk, params, bn, p_drop, masks, seed, step, momentum, update_running, out9, grads, batch_stats, st,
                                               [&](const TrArgs &t, int phase) {
                                                   hipLaunchKernelGGL(objproj_tr_phase_kernel, dim3(B), dim3(NTHR), TR_LDS, st, *op, P, TP, a, t, nodes, B, phase);
                                               });
}

extern "C" int interdiff_correction_train_predict(const idf_objproj *op, const float *params, const float *obj_angles, const float *obj_trans,
                                                  const float *markers, const int32_t *contact, const int32_t *nodes, int32_t B, int32_t T,
                                                  int32_t initialize, double p_drop, const uint8_t *masks, uint64_t seed, uint64_t step, float *obj_pred_out,
                                                  void *ws, size_t ws_bytes, void *stream) {
    if (!params || !obj_angles || !obj_trans || !markers || !obj_pred_out || !ws) return IDF_E_INVAL;
    if (!initialize && !contact && !nodes) return IDF_E_INVAL;
    if (ot_check(op, B) != IDF_OK || T != op->T) return IDF_E_INVAL;
    if (!(p_drop >= 0.0 && p_drop < 1.0)) return IDF_E_INVAL;
    const FtPlan P = ot_plan(op->cin, op->cout);
    const TrPlan TP = tr_plan(P);
    const TrWs W = tr_ws(P, TP, B, TR_SEAM);
    if (ws_bytes < W.total * sizeof(float)) return IDF_E_INVAL;
    float *base = static_cast<float *>(ws);
    hipStream_t st = idf_stream(stream);
    OtArgs a{};                                        // coef stays 0: the head's loss gradient is not read
    a.obj_angles = obj_angles; a.obj_trans = obj_trans; a.markers = markers; a.contact = contact;
    a.partials = base + W.partials;
    a.loss_part = base + W.loss_part;
    a.ws_clips = base + W.clips;
    a.initialize = initialize != 0;
    a.obj_pred_out = obj_pred_out;
    TrArgs t{};                                        // as stgcn_tr_launch_grads sets them: the same masks, the same scale
    t.params = params;
    t.statp = reinterpret_cast<double *>(base + W.statp);
    t.dyp = reinterpret_cast<double *>(base + W.dyp);
    t.scale = (float)(1.0 / (1.0 - p_drop));
    t.masks = masks;
    static std::atomic<uint64_t> lds_ok{0};
    if (idf_opt_in_lds(reinterpret_cast<const void *>(objproj_tr_phase_kernel), (int)TR_LDS, lds_ok) != IDF_OK) return IDF_E_LAUNCH;
    idf_prof_mark(IDF_K_OTHER, st);
    if (!masks && p_drop > 0.0) {
        uint8_t *mb = reinterpret_cast<uint8_t *>(base + W.masks);
        stgcn_tr_launch_masks<NP>(P, TP, B, p_drop, seed, step, mb, st);
        t.masks = mb;
    }
    for (int k = 0; k <= 8; ++k)                       // the forward phases 0 .. 7, then the head alone
        hipLaunchKernelGGL(objproj_tr_phase_kernel, dim3(B), dim3(NTHR), TR_LDS, st, *op, P, TP, a, t, nodes, B, k < 8 ? k : TR_PHASE_PREDICT);
    idf_prof_mark(-1, st);
    IDF_CHECK_LAUNCH();
    return IDF_OK;
}
