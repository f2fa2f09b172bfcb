// HO-GCN skeleton mode: launchers of the correction predictor / correction hook (device code: csrc/skeleton.h) and the
// evaluation metrics calc_metric_single (eval_skeleton.py:46-68).
#include "skeleton.h"

namespace {
using namespace idf_skel_dev;

template <bool HOOK>
__global__ __launch_bounds__(NTHR) void skel_objproj_kernel(const idf_skel_objproj op, const Src s, int B) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    skel_body<HOOK>(sm, op, s, B, blockIdx.x);
}

constexpr int MET_THR = 256;

// calc_metric_single: four sums over frames >= f, each reduced in a fixed order (a strided per-thread walk, then a tree)
__global__ __launch_bounds__(MET_THR) void skel_metrics_kernel(const float *__restrict__ body_p, const float *__restrict__ body_g,
                                                              const float *__restrict__ obj_p, const float *__restrict__ obj_g,
                                                              const float *__restrict__ pose_p, const float *__restrict__ pose_g,
                                                              int T, int B, int f, float *__restrict__ out4) {
    __shared__ float red[4][MET_THR];
    const int tid = threadIdx.x;
    const int nf = (T - f) * B;                          // (frame, clip) pairs
    float sh = 0.f, so = 0.f, st = 0.f, sr = 0.f;
    for (int i = tid; i < nf * J; i += MET_THR) {       // mpjpe_h: L2 over the 21 joints
        const size_t e = ((size_t)f * B * J + i) * 3;
        const float dx = body_p[e] - body_g[e], dy = body_p[e + 1] - body_g[e + 1], dz = body_p[e + 2] - body_g[e + 2];
        sh += sqrtf(dx * dx + dy * dy + dz * dz);
    }
    for (int i = tid; i < nf * N_OBJ; i += MET_THR) {   // mpjpe_o: L2 over the 12 object keypoints
        const size_t e = ((size_t)f * B * N_OBJ + i) * 3;
        const float dx = obj_p[e] - obj_g[e], dy = obj_p[e + 1] - obj_g[e + 1], dz = obj_p[e + 2] - obj_g[e + 2];
        so += sqrtf(dx * dx + dy * dy + dz * dz);
    }
    for (int i = tid; i < nf; i += MET_THR) {           // translation_error, rotation_error (min over the quaternion's two signs, L1)
        const size_t e = ((size_t)f * B + i) * 7;
        const float dx = pose_p[e] - pose_g[e], dy = pose_p[e + 1] - pose_g[e + 1], dz = pose_p[e + 2] - pose_g[e + 2];
        st += sqrtf(dx * dx + dy * dy + dz * dz);
        float v1 = 0.f, v2 = 0.f;
#pragma unroll
        for (int k = 3; k < 7; ++k) {
            v1 += fabsf(pose_p[e + k] - pose_g[e + k]);
            v2 += fabsf(pose_p[e + k] + pose_g[e + k]);
        }
        sr += fminf(v1, v2);
    }
    red[0][tid] = sh; red[1][tid] = so; red[2][tid] = st; red[3][tid] = sr;
    __syncthreads();
    for (int h = MET_THR / 2; h > 0; h >>= 1) {
        if (tid < h)
#pragma unroll
            for (int m = 0; m < 4; ++m) red[m][tid] += red[m][tid + h];
        __syncthreads();
    }
    if (tid < 4) {
        const float n = (float)nf * (tid == 0 ? (float)J : tid == 1 ? (float)N_OBJ : 1.f);
        out4[tid] = red[tid][0] / n;
    }
}

int skel_check(const idf_skel_objproj *op, int B) {
    if (!op || !op->arena || B <= 0 || op->n_pre != NP || op->T != NP || op->J != J || op->past_len < 1 || op->past_len > 10) return IDF_E_INVAL;
    for (int st = 0; st < 3; ++st) {
        if (op->cin[st * 4] != CH || op->cout[st * 4 + 3] != CH) return IDF_E_INVAL;
        for (int l = 0; l < 4; ++l) {
            const int li = st * 4 + l;
            if (op->cin[li] < 1 || op->cin[li] > MAXC || op->cout[li] < 1 || op->cout[li] > MAXC || op->layer[li] < 0) return IDF_E_INVAL;
            if (l < 3 && op->cout[li] != op->cin[li + 1]) return IDF_E_INVAL;
        }
    }
    return IDF_OK;
}

template <bool HOOK>
int skel_launch(const idf_skel_objproj *op, const Src &s, int B, void *stream) {
    static std::atomic<uint64_t> lds_ok{0};
    if (idf_opt_in_lds(reinterpret_cast<const void *>(skel_objproj_kernel<HOOK>), (int)SKEL_LDS, lds_ok) != IDF_OK) return IDF_E_LAUNCH;
    idf_prof_mark(IDF_K_OBJPROJ, idf_stream(stream));
    hipLaunchKernelGGL(skel_objproj_kernel<HOOK>, dim3(B), dim3(NTHR), SKEL_LDS, idf_stream(stream), *op, s, B);
    idf_prof_mark(-1, idf_stream(stream));
    IDF_CHECK_LAUNCH();
    return IDF_OK;
}

}  // namespace

extern "C" int interdiff_skeleton_objprojector_sample(const idf_skel_objproj *op, const float *obj_angles, const float *obj_trans,
                                                      const float *human_points, int32_t B, float *quat_out, float *trans_out, void *stream) {
    if (!obj_angles || !obj_trans || !human_points || !quat_out || !trans_out || skel_check(op, B) != IDF_OK) return IDF_E_INVAL;
    Src s{};
    s.angles = obj_angles; s.trans = obj_trans; s.human = human_points;
    s.quat_out = quat_out; s.trans_out = trans_out;
    return skel_launch<false>(op, s, B, stream);
}

extern "C" int interdiff_skeleton_correction(const idf_skel_objproj *op, const float *x, const float *gt, const float *zero_pose_obj,
                                             int32_t B, int32_t T, float blend_t, float *out, void *stream) {
    if (!x || !gt || !zero_pose_obj || !out || skel_check(op, B) != IDF_OK || T != op->T) return IDF_E_INVAL;
    Src s{};
    s.x = x; s.gt = gt; s.zpo = zero_pose_obj; s.out = out; s.blend_t = blend_t;
    return skel_launch<true>(op, s, B, stream);
}

extern "C" int interdiff_skeleton_metrics(const float *body_pred, const float *body_gt, const float *obj_pred, const float *obj_gt,
                                          const float *pose_pred, const float *pose_gt, int32_t T, int32_t B, int32_t from_frame,
                                          float *out4, void *stream) {
    if (!body_pred || !body_gt || !obj_pred || !obj_gt || !pose_pred || !pose_gt || !out4 || B <= 0 || from_frame < 0 || from_frame >= T)
        return IDF_E_INVAL;
    idf_prof_mark(IDF_K_OTHER, idf_stream(stream));
    hipLaunchKernelGGL(skel_metrics_kernel, dim3(1), dim3(MET_THR), 0, idf_stream(stream), body_pred, body_gt, obj_pred, obj_gt, pose_pred, pose_gt,
                       T, B, from_frame, out4);
    idf_prof_mark(-1, idf_stream(stream));
    IDF_CHECK_LAUNCH();
    return IDF_OK;
}
