// Scoring of a skeleton diffusion checkpoint (forward only): the 13 terms of interdiff/train_diffusion_skeleton.py
//   forward_backward :100-143 (teacher-forced, on the model output) and calc_val_loss :190-229 (on a sample) -- the same arithmetic.
// Tokens are [B,1,C,T], C = n_body + 3 * n_points + 7: body | object keypoints | object translation 3 | object quaternion xyzw 4.
// Term order (= the reference's dict order):
//   0 body_past  1 body_future  2 obj_past  3 obj_future  4 loss_obj_nonrot_past  5 loss_obj_nonrot_future  6 loss_obj_rot_past
//   7 loss_obj_rot_future  8 quaternion_reg_loss  9 loss_obj_rot_v  10 loss_obj_nonrot_v  11 loss_body_v  12 loss_obj_v
// Every term is a mean of squares over its frames and channels; the velocity terms run over all T - 1 frame differences (no past /
// future split); quaternion_reg_loss is the mean over frames of (q.q - 1)^2 of the PREDICTION (the reference takes the norm and squares
// it again, :127 / :204: q.q to rounding).
// VALU / latency kernels: fp32, no MFMA, no float atomics, every sum in a fixed order (two calls give the same bits), and a clip's 13
// numbers are formed by its own workgroup from its own floats alone.
#include "common.h"

namespace {

constexpr int SKL_TERMS = 13, SKL_THREADS = 256, SKL_WAVES = SKL_THREADS / IDF_WAVE, SKL_ACC = 12;

// One workgroup per (sample, clip).  The clip's C * T floats of the prediction and of the ground truth are read once, lane after lane
// along the contiguous (channel, frame) index, so every load instruction of a wave covers 256 contiguous bytes; the frame before
// comes from the same cache lines.  A thread keeps twelve running sums, (channel group) x (past, future, velocity), and the quaternion
// regulariser; they meet by the DPP wave sum, then four wave results are added in wave order.
__global__ __launch_bounds__(SKL_THREADS) void skeleton_losses_kernel(const float *__restrict__ pred, const float *__restrict__ gt, int B, int C,
                                                                      int T, int P, int n_body, int n_obj, float *__restrict__ per_clip) {
    __shared__ float part[SKL_WAVES][SKL_TERMS];
    const int b = blockIdx.x % B, k = blockIdx.x / B;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float *x = pred + ((size_t)k * B + b) * C * T, *g = gt + (size_t)b * C * T;
    const int n = C * T, c_tr = n_body + n_obj, c_rot = c_tr + 3;
    float acc[SKL_ACC], qreg = 0.f;
#pragma unroll
    for (int a = 0; a < SKL_ACC; ++a) acc[a] = 0.f;
    for (int e = threadIdx.x; e < n; e += SKL_THREADS) {
        const int c = e / T, t = e - c * T;
        const int grp = c < n_body ? 0 : c < c_tr ? 1 : c < c_rot ? 2 : 3;
        const float xv = x[e], gv = g[e];
        const float d = xv - gv;
        float v = 0.f;
        if (t >= 1) v = (xv - x[e - 1]) - (gv - g[e - 1]);
        const int sel_d = 3 * grp + (t < P ? 0 : 1), sel_v = 3 * grp + 2;
        const float dd = d * d, vv = v * v;
#pragma unroll
        for (int a = 0; a < SKL_ACC; ++a) acc[a] += a == sel_d ? dd : a == sel_v ? vv : 0.f;      // (compile-time register indices: no scratch)
    }
    for (int t = threadIdx.x; t < T; t += SKL_THREADS) {
        const float *q = x + (size_t)c_rot * T + t;
        const float qx = q[0], qy = q[T], qz = q[2 * T], qw = q[3 * T];
        const float r = ((qx * qx + qy * qy) + (qz * qz + qw * qw)) - 1.0f;
        qreg += r * r;
    }
    // accumulator (group, kind) -> term of the reference's order
    constexpr int TERM_OF[SKL_ACC] = {0, 1, 11, 2, 3, 12, 4, 5, 10, 6, 7, 9};
#pragma unroll
    for (int a = 0; a < SKL_ACC; ++a) {
        const float s = wave_sum(acc[a]);
        if (lane == 0) part[wave][TERM_OF[a]] = s;
    }
    {
        const float s = wave_sum(qreg);
        if (lane == 0) part[wave][8] = s;
    }
    __syncthreads();
    if (threadIdx.x < SKL_TERMS) {
        const int j = threadIdx.x;
        float s = part[0][j];
#pragma unroll
        for (int w = 1; w < SKL_WAVES; ++w) s += part[w][j];
        const int feat = (j == 0 || j == 1 || j == 11) ? n_body : (j == 2 || j == 3 || j == 12) ? n_obj : (j == 4 || j == 5 || j == 10) ? 3 : 4;
        const int frames = (j == 0 || j == 2 || j == 4 || j == 6) ? P : (j == 1 || j == 3 || j == 5 || j == 7) ? T - P : T - 1;
        const float count = j == 8 ? (float)T : (float)frames * (float)feat;
        per_clip[((size_t)k * SKL_TERMS + j) * B + b] = s / count;
    }
}

// mean over the clips of every (sample, term): one workgroup; a wave takes a (sample, term) pair, its lanes walk the clips 64 apart,
// then the DPP wave sum -- the same order on every call
__global__ __launch_bounds__(SKL_THREADS) void skeleton_losses_finish_kernel(const float *__restrict__ per_clip, int K, int B,
                                                                             float *__restrict__ out_terms) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int p = wave; p < K * SKL_TERMS; p += SKL_WAVES) {               // (wave-uniform bounds: every lane of a wave reaches wave_sum)
        const float *row = per_clip + (size_t)p * B;
        float s = 0.f;
        for (int b = lane; b < B; b += IDF_WAVE) s += row[b];
        s = wave_sum(s);
        if (lane == 0) out_terms[p] = s / (float)B;
    }
}

inline int skl_check(int32_t K, int32_t B, int32_t C, int32_t T, int32_t past_len, int32_t n_body, int32_t n_points) {
    if (K <= 0 || B <= 0 || n_body <= 0 || n_points <= 0 || past_len < 1 || T < past_len + 1) return IDF_E_INVAL;
    if ((int64_t)C != (int64_t)n_body + 3 * (int64_t)n_points + 7) return IDF_E_INVAL;
    if ((int64_t)C * T > 0x7FFFFFFF || (int64_t)K * B > 0x7FFFFFFF || (int64_t)K * SKL_TERMS > 0x7FFFFFFF) return IDF_E_INVAL;
    return IDF_OK;
}

}  // namespace

extern "C" size_t interdiff_skeleton_sample_losses_workspace_bytes(int32_t K, int32_t B) {
    if (K <= 0 || B <= 0) return 0;
    return idf_align((size_t)K * SKL_TERMS * B * sizeof(float));
}

extern "C" int interdiff_skeleton_sample_losses(const float *pred, const float *gt, int32_t K, int32_t B, int32_t C, int32_t T, int32_t past_len,
                                                int32_t n_body, int32_t n_points, float *out_terms, float *out_per_clip, void *ws, size_t ws_bytes,
                                                void *stream) {
    if (!pred || !gt || !out_terms) return IDF_E_INVAL;
    const int rc = skl_check(K, B, C, T, past_len, n_body, n_points);
    if (rc != IDF_OK) return rc;
    float *per_clip = out_per_clip;
    if (!per_clip) {
        if (!ws) return IDF_E_INVAL;
        if (ws_bytes < interdiff_skeleton_sample_losses_workspace_bytes(K, B)) return IDF_E_NOMEM;
        per_clip = static_cast<float *>(ws);
    }
    hipLaunchKernelGGL(skeleton_losses_kernel, dim3((unsigned)(K * B)), dim3(SKL_THREADS), 0, idf_stream(stream), pred, gt, B, C, T, past_len, n_body,
                       3 * n_points, per_clip);
    IDF_CHECK_LAUNCH();
    hipLaunchKernelGGL(skeleton_losses_finish_kernel, dim3(1), dim3(SKL_THREADS), 0, idf_stream(stream), per_clip, K, B, out_terms);
    IDF_CHECK_LAUNCH();
    return IDF_OK;
}

extern "C" int interdiff_skeleton_denoising_losses(const float *pred, const float *target, int32_t B, int32_t T, int32_t past_len, int32_t n_body,
                                                   int32_t n_points, float *out, void *stream) {
    if (!pred || !target || !out) return IDF_E_INVAL;
    const int64_t C = (int64_t)n_body + 3 * (int64_t)n_points + 7;
    if (C > 0x7FFFFFFF) return IDF_E_INVAL;
    const int rc = skl_check(1, B, (int32_t)C, T, past_len, n_body, n_points);
    if (rc != IDF_OK) return rc;
    hipLaunchKernelGGL(skeleton_losses_kernel, dim3((unsigned)B), dim3(SKL_THREADS), 0, idf_stream(stream), pred, target, B, (int)C, T, past_len,
                       n_body, 3 * n_points, out);
    IDF_CHECK_LAUNCH();
    return IDF_OK;
}
