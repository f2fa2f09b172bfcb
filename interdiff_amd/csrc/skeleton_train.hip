// Fine-tuning of the skeleton correction predictor with frozen normalisation statistics: launchers of the clip kernel (csrc/skeleton_train.h) and of the
// kernels around it (csrc/stgcn_train.h) -- the fold of the per-clip partials in ascending clip order, the conversion of the folded convolutions' gradients
// to the reference parameters, Adam (torch.optim.Adam's order of operations) on the fp32 master parameters, and the re-fold into the arena the inference
// kernels read.
// Training with batch statistics and dropout (csrc/skeleton_bn_train.h): the phase launches; the mask generator and the batch statistics /
// running-buffer update are csrc/stgcn_bn_train.h's; it shares the fold over clips, Adam and the re-fold with the fine-tuner.
#include <math.h>
#include "skeleton_bn_train.h"

namespace {
using namespace idf_skel_train;
using namespace idf_stgcn_train;

__global__ __launch_bounds__(NTHR) void skel_ft_clip_kernel(const idf_skel_objproj op, const Src s, const FtPlan plan, const FtArgs a, int B) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    ft_clip_body(sm, op, s, plan, a, B, blockIdx.x);
}

// the channel widths the kernels were built for (all the parameter table needs)
int ft_check_widths(const idf_skel_objproj *op) {
    if (!op || op->n_pre != NP || op->T != NP || op->J != J) return IDF_E_INVAL;
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

int ft_check(const idf_skel_objproj *op, int B) {
    if (ft_check_widths(op) != IDF_OK || !op->arena || B < 1 || op->past_len < 1 || op->past_len > 10) return IDF_E_INVAL;
    for (int li = 0; li < 12; ++li)
        if (op->layer[li] < 0) return IDF_E_INVAL;
    return IDF_OK;
}

}  // namespace

extern "C" int interdiff_skeleton_finetune_param_table(const idf_skel_objproj *op, int32_t *table, int32_t *n_param, int32_t *n_bn) {
    if (!table || !n_param || !n_bn || ft_check_widths(op) != IDF_OK) return IDF_E_INVAL;
    ft_export_table(ft_plan(op->cin, op->cout), table, n_param, n_bn);
    return IDF_OK;
}

extern "C" size_t interdiff_skeleton_finetune_workspace_bytes(const idf_skel_objproj *op, int32_t B) {
    if (!op || B < 1) return 0;
    return ft_ws(ft_plan(op->cin, op->cout), B).total * sizeof(float);
}

extern "C" int interdiff_skeleton_finetune_grads(const idf_skel_objproj *op, const float *params, const float *bn, const float *obj_angles,
                                                 const float *obj_trans, const float *human_points, const float *pose_gt, int32_t B, int32_t T,
                                                 const float *weights8, float *out9, float *grads, void *ws, size_t ws_bytes, void *stream) {
    if (!params || !bn || !obj_angles || !obj_trans || !human_points || !pose_gt || !weights8 || !out9 || !grads || !ws) return IDF_E_INVAL;
    if (ft_check(op, B) != IDF_OK || T != op->T) return IDF_E_INVAL;
    const FtPlan P = ft_plan(op->cin, op->cout);
    const FtWs W = ft_ws(P, B);
    if (ws_bytes < W.total * sizeof(float)) return IDF_E_INVAL;
    float *base = static_cast<float *>(ws);
    hipStream_t st = idf_stream(stream);
    FtArgs a{};
    const LossK lk = ft_loss_constants(weights8, op->past_len, T, B, 4, a.coef);
    a.pose_gt = pose_gt;
    a.partials = base + W.partials;
    a.loss_part = base + W.loss_part;
    a.ws_clips = base + W.clips;
    Src s{};
    s.angles = obj_angles; s.trans = obj_trans; s.human = human_points;
    static std::atomic<uint64_t> lds_ok{0};
    if (idf_opt_in_lds(reinterpret_cast<const void *>(skel_ft_clip_kernel), (int)FT_LDS, lds_ok) != IDF_OK) return IDF_E_LAUNCH;
    return stgcn_ft_launch_grads<NP>(P, W, base, B, lk, params, bn, out9, grads, st,
                                     [&] { hipLaunchKernelGGL(skel_ft_clip_kernel, dim3(B), dim3(NTHR), FT_LDS, st, *op, s, P, a, B); });
}

extern "C" int interdiff_skeleton_finetune_step(const idf_skel_objproj *op, float *arena, float *params, const float *bn, const float *grads, float *exp_avg,
                                                float *exp_avg_sq, int32_t step, double lr, double beta1, double beta2, double eps, double weight_decay,
                                                void *stream) {
    if (!arena || !params || !bn || !grads || !exp_avg || !exp_avg_sq || step < 1 || ft_check(op, 1) != IDF_OK) return IDF_E_INVAL;
    if (!(lr >= 0.0) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0) || !(weight_decay >= 0.0)) return IDF_E_INVAL;
    return stgcn_ft_launch_step<NP, VP>(*op, ft_plan(op->cin, op->cout), arena, params, bn, grads, exp_avg, exp_avg_sq,
                                        ft_adam_constants(step, lr, beta1, beta2, eps, weight_decay), idf_stream(stream));
}

// ================= training with batch statistics and dropout =================
namespace {

__global__ __launch_bounds__(NTHR) void skel_tr_phase_kernel(const idf_skel_objproj op, const Src s, const FtPlan plan, const TrPlan tp, const FtArgs a,
                                                             const TrArgs t, int B, int phase) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    tr_phase_body(sm, op, s, plan, tp, a, t, B, blockIdx.x, phase);
}

}  // namespace

extern "C" size_t interdiff_skeleton_train_workspace_bytes(const idf_skel_objproj *op, int32_t B) {
    if (!op || B < 1 || ft_check_widths(op) != IDF_OK) return 0;
    const FtPlan P = ft_plan(op->cin, op->cout);
    return tr_ws(P, tr_plan(P), B, TR_SEAM).total * sizeof(float);
}

extern "C" int interdiff_skeleton_train_masks(const idf_skel_objproj *op, int32_t B, double p_drop, uint64_t seed, uint64_t step, uint8_t *masks_out,
                                              void *stream) {
    if (!masks_out || ft_check_widths(op) != IDF_OK || B < 1 || !(p_drop >= 0.0 && p_drop < 1.0)) return IDF_E_INVAL;
    const FtPlan P = ft_plan(op->cin, op->cout);
    stgcn_tr_launch_masks<NP>(P, tr_plan(P), B, p_drop, seed, step, masks_out, idf_stream(stream));
    IDF_CHECK_LAUNCH();
    return IDF_OK;
}

extern "C" int interdiff_skeleton_train_grads(const idf_skel_objproj *op, const float *params, float *bn, const float *obj_angles, const float *obj_trans,
                                              const float *human_points, const float *pose_gt, int32_t B, int32_t T, const float *weights8, double p_drop,
                                              const uint8_t *masks, uint64_t seed, uint64_t step, double momentum, int32_t update_running, float *out9,
                                              float *grads, float *batch_stats, void *ws, size_t ws_bytes, void *stream) {
    if (!params || !bn || !obj_angles || !obj_trans || !human_points || !pose_gt || !weights8 || !out9 || !grads || !ws) return IDF_E_INVAL;
    if (ft_check(op, B) != IDF_OK || T != op->T) return IDF_E_INVAL;
    if (!(p_drop >= 0.0 && p_drop < 1.0) || !(momentum >= 0.0 && momentum <= 1.0) || (update_running != 0 && update_running != 1)) return IDF_E_INVAL;
    const FtPlan P = ft_plan(op->cin, op->cout);
    const TrPlan TP = tr_plan(P);
    const TrWs W = tr_ws(P, TP, B, TR_SEAM);
    if (ws_bytes < W.total * sizeof(float)) return IDF_E_INVAL;
    float *base = static_cast<float *>(ws);
    hipStream_t st = idf_stream(stream);
    FtArgs a{};
    const LossK lk = ft_loss_constants(weights8, op->past_len, T, B, 4, a.coef);
    a.pose_gt = pose_gt;
    a.partials = base + W.partials;
    a.loss_part = base + W.loss_part;
    a.ws_clips = base + W.clips;
    Src s{};
    s.angles = obj_angles; s.trans = obj_trans; s.human = human_points;
    static std::atomic<uint64_t> lds_ok{0};
    if (idf_opt_in_lds(reinterpret_cast<const void *>(skel_tr_phase_kernel), (int)TR_LDS, lds_ok) != IDF_OK) return IDF_E_LAUNCH;
    return stgcn_tr_launch_grads<Tr, NP, MAXC>(P, TP, W, base, B, lk, params, bn, p_drop, masks, seed, step, momentum, update_running, out9, grads, batch_stats, st,
                                               [&](const TrArgs &t, int phase) {
                                                   hipLaunchKernelGGL(skel_tr_phase_kernel, dim3(B), dim3(NTHR), TR_LDS, st, *op, s, P, TP, a, t, B, phase);
                                               });
}
