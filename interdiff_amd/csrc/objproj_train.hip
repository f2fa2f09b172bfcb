// Fine-tuning of the SMPL contact-frame correction predictor with frozen normalisation statistics: launchers of the clip kernel (csrc/objproj_train.h) and
// of the kernels around it (csrc/stgcn_train.h) -- the fold of the per-clip partials in ascending clip order, the conversion of the folded convolutions'
// gradients to the reference parameters, Adam on the fp32 master parameters, and the re-fold into the arena that interdiff_objprojector_sample / _forward
// and the correction hook read.
// Training with batch statistics and dropout: csrc/objproj_bn_train.hip, which shares Adam and the re-fold below.
#include <math.h>
#include "objproj_train.h"

namespace {
using namespace idf_objproj_train;
using namespace idf_stgcn_train;

__global__ __launch_bounds__(NTHR) void objproj_ft_clip_kernel(const idf_objproj op, const FtPlan plan, const OtArgs a, int B) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    ot_clip_body(sm, op, plan, a, B, blockIdx.x);
}

__global__ __launch_bounds__(NTHR) void objproj_ft_predict_kernel(const idf_objproj op, const FtPlan plan, const OtArgs a, int B) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    ot_clip_predict(sm, op, plan, a, B, blockIdx.x);
}

}  // namespace

extern "C" int interdiff_correction_finetune_predict(const idf_objproj *op, const float *params, const float *bn, const float *obj_angles,
                                                     const float *obj_trans, const float *markers, const int32_t *contact, int32_t B, int32_t T,
                                                     int32_t initialize, float *obj_pred_out, void *ws, size_t ws_bytes, void *stream) {
    if (!params || !bn || !obj_angles || !obj_trans || !markers || !obj_pred_out || !ws) return IDF_E_INVAL;
    if (!initialize && !contact) return IDF_E_INVAL;
    if (ot_check(op, B) != IDF_OK || T != op->T) return IDF_E_INVAL;
    const FtPlan P = ot_plan(op->cin, op->cout);
    const FtWs W = ft_ws(P, B);
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
    static std::atomic<uint64_t> lds_ok{0};
    if (idf_opt_in_lds(reinterpret_cast<const void *>(objproj_ft_predict_kernel), (int)OT_LDS, lds_ok) != IDF_OK) return IDF_E_LAUNCH;
    idf_prof_mark(IDF_K_OTHER, st);
    hipLaunchKernelGGL(objproj_ft_predict_kernel, dim3(B), dim3(NTHR), OT_LDS, st, *op, P, a, B);
    idf_prof_mark(-1, st);
    IDF_CHECK_LAUNCH();
    return IDF_OK;
}

extern "C" int interdiff_correction_finetune_param_table(const idf_objproj *op, int32_t *table, int32_t *n_param, int32_t *n_bn) {
    if (!table || !n_param || !n_bn || ot_check_widths(op) != IDF_OK) return IDF_E_INVAL;
    ft_export_table(ot_plan(op->cin, op->cout), table, n_param, n_bn);
    return IDF_OK;
}

extern "C" size_t interdiff_correction_finetune_workspace_bytes(const idf_objproj *op, int32_t B) {
    if (B < 1 || ot_check_widths(op) != IDF_OK) return 0;
    return ft_ws(ot_plan(op->cin, op->cout), B).total * sizeof(float);
}

extern "C" int interdiff_correction_finetune_grads(const idf_objproj *op, const float *params, const float *bn, const float *obj_angles,
                                                   const float *obj_trans, const float *markers, const int32_t *contact, const float *d_obj_pred,
                                                   int32_t B, int32_t T, int32_t initialize, const float *weights8, float *out9, float *grads, void *ws,
                                                   size_t ws_bytes, void *stream) {
    if (!params || !bn || !obj_angles || !obj_trans || !markers || !weights8 || !out9 || !grads || !ws) return IDF_E_INVAL;
    if (!initialize && !contact) return IDF_E_INVAL;
    if (ot_check(op, B) != IDF_OK || T != op->T) return IDF_E_INVAL;
    const FtPlan P = ot_plan(op->cin, op->cout);
    const FtWs W = ft_ws(P, B);
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
    if (idf_opt_in_lds(reinterpret_cast<const void *>(objproj_ft_clip_kernel), (int)OT_LDS, lds_ok) != IDF_OK) return IDF_E_LAUNCH;
    return stgcn_ft_launch_grads<NP>(P, W, base, B, lk, params, bn, out9, grads, st,
                                     [&] { hipLaunchKernelGGL(objproj_ft_clip_kernel, dim3(B), dim3(NTHR), OT_LDS, st, *op, P, a, B); });
}

extern "C" int interdiff_correction_finetune_step(const idf_objproj *op, float *arena, float *params, const float *bn, const float *grads, float *exp_avg,
                                                  float *exp_avg_sq, int32_t step, double lr, double beta1, double beta2, double eps, double weight_decay,
                                                  void *stream) {
    if (!arena || !params || !bn || !grads || !exp_avg || !exp_avg_sq || step < 1 || ot_check(op, 1) != IDF_OK) return IDF_E_INVAL;
    if (!(lr >= 0.0) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0) || !(weight_decay >= 0.0)) return IDF_E_INVAL;
    return stgcn_ft_launch_step<NP, VP>(*op, ot_plan(op->cin, op->cout), arena, params, bn, grads, exp_avg, exp_avg_sq,
                                        ft_adam_constants(step, lr, beta1, beta2, eps, weight_decay), idf_stream(stream));
}
