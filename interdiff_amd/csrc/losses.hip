// Checkpoint scoring (forward only): the forward diffusion q_sample, the 16 per-clip terms of the denoising objective and the
// 16 / 32 terms of validation_step / test_step.  Reference behaviour (interdiff/train_diffusion_smpl.py):
//   q_sample              diffusion/gaussian_diffusion.py:233-250, the inpainting of x_t :1264-1268
//   denoising_losses      LitInteraction.forward_backward :72-134 with l2 :54-58 (rot6d space, per-clip vectors [B])
//   sample_losses         _common_step :396-409 / :422-443 (rot6d -> matrix -> axis-angle, hands spliced in) + calc_val_loss :185-237
//                         / calc_loss :262-356 (axis-angle -> 3x3 through rotvec_to_rotmat, tools.py:88-90)
// Tokens are [B,1,144,T]: 22 x rot6d | body translation 3 | object rot6d | object translation 3.  Term order (= the reference's
// dict order): index = 4 * kind + group, kind in {past, v_past, future, v_future}, group in {body_rot, body_nonrot, obj_rot, obj_nonrot}.
// VALU / latency kernels: no MFMA, no float atomics, every sum in a fixed order (two calls give the same bits).
#include "common.h"
#include "philox.h"
#include "rot_math.h"

namespace {

constexpr int C_TOK = 144, C_BODY_ROT = 132, C_BODY_TR = 132, C_OBJ_ROT = 135, C_OBJ_TR = 141;
constexpr uint64_t Q_SAMPLE_STEP = 0xFFFFFFFEull;      // Philox step index of q_sample's noise (the sampler uses loop indices 0 .. steps - 1 and 0xFFFFFFFF for x_T)

// --------------------------------------------------------------------------------------------------------------- q_sample
// x_t = sqrt(abar_t) x0 + sqrt(1 - abar_t) eps: both products rounded on their own like the reference's tensor expression
__device__ __forceinline__ float q1(float a, float s, float x0, float e) {
#pragma clang fp contract(off)
    const float p = a * x0, q = s * e;
    return p + q;
}

template <bool GEN>
__global__ __launch_bounds__(256) void q_sample_kernel(float *__restrict__ xt, const float *__restrict__ x0, const float *__restrict__ noise,
                                                       const int64_t *__restrict__ ts, const float *__restrict__ sqrt_ac,
                                                       const float *__restrict__ sqrt_1mac, int n_steps, const float *__restrict__ gt,
                                                       const uint8_t *__restrict__ mask, int64_t n, int64_t per_clip, uint64_t seed, uint64_t g0) {
    const int64_t n4 = (n + 3) >> 2, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < n4; g += stride) {
        const int64_t i = g * 4;
        float ev[4];
        if constexpr (GEN) {
            const float4 e = randn4(seed, Q_SAMPLE_STEP, g0 + (uint64_t)g);
            ev[0] = e.x; ev[1] = e.y; ev[2] = e.z; ev[3] = e.w;
        }
        float r[4];
        for (int k = 0; k < 4 && i + k < n; ++k) {
            int64_t t = ts[(i + k) / per_clip];
            t = t < 0 ? 0 : (t >= n_steps ? n_steps - 1 : t);          // (a timestep outside the schedule must not read outside the tables)
            const float e = GEN ? ev[k] : noise[i + k];
            float v = q1(sqrt_ac[t], sqrt_1mac[t], x0[i + k], e);
            if (mask && mask[i + k]) v = gt[i + k];
            r[k] = v;
        }
        if (i + 3 < n) *reinterpret_cast<float4 *>(xt + i) = make_float4(r[0], r[1], r[2], r[3]);
        else
            for (int k = 0; k < 4 && i + k < n; ++k) xt[i + k] = r[k];
    }
}

// ------------------------------------------------------------------------------------------------------- denoising_losses
// One workgroup per clip, one thread per token channel walking the frames with the two previous predictions in registers.
// Six running sums per channel: value past / future, and for both velocity terms the two summands of the reference:
//   first summand   l2(X[t] - X[t-1], G[t] - G[t])   -- the ground-truth operand is zero, as the reference writes it (:91-115)
//   second summand  l2(X[t] - X[t-1], X[t+1] - X[t]) -- a second difference of the prediction alone
__global__ __launch_bounds__(256) void denoising_losses_kernel(const float *__restrict__ pred, const float *__restrict__ target, int B, int T,
                                                               int P, float *__restrict__ out) {
    __shared__ float part[6][C_TOK];
    const int b = blockIdx.x, c = threadIdx.x;
    if (c < C_TOK) {
        const float *x = pred + ((size_t)b * C_TOK + c) * T, *g = target + ((size_t)b * C_TOK + c) * T;
        float s_past = 0.f, s_fut = 0.f, s_vp1 = 0.f, s_vp2 = 0.f, s_vf1 = 0.f, s_vf2 = 0.f;
        float xm1 = 0.f, xm2 = 0.f;                                  // X[t-1], X[t-2]
        for (int t = 0; t < T; ++t) {
            const float xv = x[t], gv = g[t];
            const float d = xv - gv, gz = gv - gv;
            if (t < P) s_past += d * d; else s_fut += d * d;
            if (t >= 1) {
                const float v = (xv - xm1) - gz;                     // first summand at frame t
                if (t <= P) s_vp1 += v * v;
                if (t >= P) s_vf1 += v * v;
            }
            if (t >= 2) {                                            // second summand centred on u = t - 1
                const int u = t - 1;
                if (u <= P - 1) { const float e = (xm1 - xm2) - (xv - xm1); s_vp2 += e * e; }      // u = 1 .. P-1
                if (u >= P) { const float e = (xm2 - xm1) - (xm1 - xv); s_vf2 += e * e; }          // u = P .. T-2
            }
            xm2 = xm1;
            xm1 = xv;
        }
        part[0][c] = s_past; part[1][c] = s_vp1; part[2][c] = s_vp2; part[3][c] = s_fut; part[4][c] = s_vf1; part[5][c] = s_vf2;
    }
    __syncthreads();
    if (c < 16) {
        const int kind = c >> 2, group = c & 3;
        const int lo = group == 0 ? 0 : group == 1 ? C_BODY_TR : group == 2 ? C_OBJ_ROT : C_OBJ_TR;
        const int hi = group == 0 ? C_BODY_ROT : group == 1 ? C_OBJ_ROT : group == 2 ? C_OBJ_TR : C_TOK;
        const float feat = (float)(hi - lo);
        auto sum = [&](int row) {
            float s = 0.f;
            for (int i = lo; i < hi; ++i) s += part[row][i];
            return s;
        };
        float r;
        if (kind == 0) r = sum(0) / ((float)P * feat);
        else if (kind == 1) r = sum(1) / ((float)P * feat) + sum(2) / ((float)(P - 1) * feat);
        else if (kind == 2) r = sum(3) / ((float)(T - P) * feat);
        else r = sum(4) / ((float)(T - P) * feat) + sum(5) / ((float)(T - P - 1) * feat);
        out[(size_t)c * B + b] = r;
    }
}

// --------------------------------------------------------------------------------------------------------- sample_losses
// One workgroup per (clip, sample); its eight waves take contiguous runs of frames.  Lane roles inside a wave: 0..21 body joints
// (rot6d -> matrix -> axis-angle -> 3x3), 22..51 hand joints (axis-angle -> 3x3; prediction reads the frame idx_pad[t], ground truth
// frame t), 52 the object rotation, 53 / 54 the body / object translation.  A lane keeps the previous frame's prediction and
// ground truth in registers for the velocity terms (a wave recomputes the one frame in front of its run), so no [K,T,B,52*9]
// tensor exists anywhere.  Partial sums meet in LDS and are added in a fixed order.
constexpr int SL_WAVES = 8, SL_ROLES = 55;

__device__ __forceinline__ void six_d_to_rotmat(const float *__restrict__ x, int c0, int T, int t, float *m) {
    float d[6], r[9], a[3];
#pragma unroll
    for (int i = 0; i < 6; ++i) d[i] = x[(size_t)(c0 + i) * T + t];
    rot::rot6d_to_matrix(d, r);
    rot::matrix_to_axis_angle(r, a);
    rot::aa2matrot(a, m);
}

__device__ __forceinline__ void role_frame(int role, const float *__restrict__ xs, const float *__restrict__ xg, const float *__restrict__ hand,
                                           int b, int B, int T, int P, int t, float *pm, float *gm) {
    if (role < 22 || role == 52) {
        const int c0 = role < 22 ? 6 * role : C_OBJ_ROT;
        six_d_to_rotmat(xs, c0, T, t, pm);
        six_d_to_rotmat(xg, c0, T, t, gm);
    } else if (role < 52) {
        const int j = role - 22, tp = t < P ? t : P - 1;
        const float *hp = hand + ((size_t)tp * B + b) * 90 + 3 * j, *hg = hand + ((size_t)t * B + b) * 90 + 3 * j;
        const float ap[3] = {hp[0], hp[1], hp[2]}, ag[3] = {hg[0], hg[1], hg[2]};
        rot::aa2matrot(ap, pm);
        rot::aa2matrot(ag, gm);
    } else {
        const int c0 = role == 53 ? C_BODY_TR : C_OBJ_TR;
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            pm[i] = i < 3 ? xs[(size_t)(c0 + i) * T + t] : 0.f;
            gm[i] = i < 3 ? xg[(size_t)(c0 + i) * T + t] : 0.f;
        }
    }
}

__global__ __launch_bounds__(64 * SL_WAVES) void sample_losses_kernel(const float *__restrict__ samples, const float *__restrict__ gt,
                                                                      const float *__restrict__ hand, int K, int B, int T, int P, int test_variant,
                                                                      float *__restrict__ per_clip) {
    __shared__ float part[SL_WAVES][4][64];
    const int b = blockIdx.x % B, k = blockIdx.x / B;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float *xs = samples + ((size_t)k * B + b) * C_TOK * T, *xg = gt + (size_t)b * C_TOK * T;
    const int chunk = (T + SL_WAVES - 1) / SL_WAVES, t0 = wave * chunk, t1 = min(T, t0 + chunk);
    const int vf0 = test_variant ? P + 1 : P;                      // calc_loss's future velocity starts one frame later than calc_val_loss's
    float acc[4] = {0.f, 0.f, 0.f, 0.f};                           // past, v_past, future, v_future
    if (lane < SL_ROLES && t0 < t1) {
        float pm[9], gm[9], pp[9], gp[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) pp[i] = gp[i] = 0.f;
        if (t0 > 0) role_frame(lane, xs, xg, hand, b, B, T, P, t0 - 1, pp, gp);
        for (int t = t0; t < t1; ++t) {
            role_frame(lane, xs, xg, hand, b, B, T, P, t, pm, gm);
            float sv = 0.f, sd = 0.f;
#pragma unroll
            for (int i = 0; i < 9; ++i) {
                const float d = pm[i] - gm[i], e = (pm[i] - pp[i]) - (gm[i] - gp[i]);
                sv += d * d;
                sd += e * e;
                pp[i] = pm[i];
                gp[i] = gm[i];
            }
            if (t < P) acc[0] += sv; else acc[2] += sv;
            if (t >= 1 && t <= P) acc[1] += sd;
            if (t >= vf0) acc[3] += sd;
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) part[wave][q][lane] = acc[q];
    __syncthreads();
    if (threadIdx.x < 16) {
        const int kind = threadIdx.x >> 2, group = threadIdx.x & 3;
        const int lo = group == 0 ? 0 : group == 1 ? 53 : group == 2 ? 52 : 54;
        const int hi = group == 0 ? 52 : lo + 1;
        float s = 0.f;
        for (int w = 0; w < SL_WAVES; ++w)
            for (int l = lo; l < hi; ++l) s += part[w][kind][l];
        const float feat = group == 0 ? 468.f : group == 2 ? 9.f : 3.f;
        const int frames = kind == 0 ? P : kind == 1 ? P : kind == 2 ? T - P : T - vf0;
        per_clip[((size_t)k * 16 + threadIdx.x) * B + b] = s / ((float)frames * feat);
    }
}

// mean over (K, B) of every term, and for test_step the per-clip minimum over the K samples, then the mean over clips
__global__ __launch_bounds__(64) void sample_losses_finish_kernel(const float *__restrict__ per_clip, int K, int B, int test_variant,
                                                                  float *__restrict__ out_terms) {
    const int i = threadIdx.x;
    if (i >= 32) return;
    const int term = i & 15;
    float r = 0.f;
    if (i < 16) {
        for (int k = 0; k < K; ++k)
            for (int b = 0; b < B; ++b) r += per_clip[((size_t)k * 16 + term) * B + b];
        r /= (float)K * (float)B;
    } else if (test_variant) {
        for (int b = 0; b < B; ++b) {
            float m = per_clip[(size_t)term * B + b];
            for (int k = 1; k < K; ++k) m = fminf(m, per_clip[((size_t)k * 16 + term) * B + b]);
            r += m;
        }
        r /= (float)B;
    }
    out_terms[i] = r;
}

inline unsigned grid_for(int64_t work) {
    int64_t b = idf_cdiv(work, 256);
    return (unsigned)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}

}  // namespace

extern "C" int interdiff_q_sample(float *x_t, const float *x0, const float *noise, const int64_t *ts, const float *sqrt_ac,
                                  const float *sqrt_1mac, int32_t n_steps, const float *gt, const uint8_t *mask, int32_t B, int64_t per_clip,
                                  uint64_t seed, uint64_t elem0, void *stream) {
    if (!x_t || !x0 || !ts || !sqrt_ac || !sqrt_1mac || n_steps <= 0 || B <= 0 || per_clip <= 0 || (mask && !gt) || (elem0 & 3)) return IDF_E_INVAL;
    if (reinterpret_cast<uintptr_t>(x_t) & 15) return IDF_E_INVAL;
    const int64_t n = (int64_t)B * per_clip;
    const unsigned g = grid_for((n + 3) / 4);
    if (noise)
        hipLaunchKernelGGL((q_sample_kernel<false>), dim3(g), dim3(256), 0, idf_stream(stream), x_t, x0, noise, ts, sqrt_ac, sqrt_1mac, n_steps, gt,
                           mask, n, per_clip, seed, elem0 >> 2);
    else
        hipLaunchKernelGGL((q_sample_kernel<true>), dim3(g), dim3(256), 0, idf_stream(stream), x_t, x0, noise, ts, sqrt_ac, sqrt_1mac, n_steps, gt,
                           mask, n, per_clip, seed, elem0 >> 2);
    IDF_CHECK_LAUNCH();
    return IDF_OK;
}

extern "C" int interdiff_denoising_losses(const float *pred, const float *target, int32_t B, int32_t T, int32_t past_len, float *out,
                                          void *stream) {
    if (!pred || !target || !out || B <= 0 || past_len < 2 || T < past_len + 2) return IDF_E_INVAL;
    hipLaunchKernelGGL(denoising_losses_kernel, dim3((unsigned)B), dim3(256), 0, idf_stream(stream), pred, target, B, T, past_len, out);
    IDF_CHECK_LAUNCH();
    return IDF_OK;
}

extern "C" size_t interdiff_sample_losses_workspace_bytes(int32_t K, int32_t B) {
    if (K <= 0 || B <= 0) return 0;
    return idf_align((size_t)K * 16 * B * sizeof(float));
}

extern "C" int interdiff_sample_losses(const float *samples, const float *gt, const float *hand_pose, int32_t K, int32_t B, int32_t T,
                                       int32_t past_len, int32_t variant, float *out_terms, float *out_per_clip, void *ws, size_t ws_bytes,
                                       void *stream) {
    if (!samples || !gt || !hand_pose || !out_terms || K <= 0 || B <= 0 || past_len < 1 || T < past_len + 2) return IDF_E_INVAL;
    if (variant != IDF_LOSS_VAL && variant != IDF_LOSS_TEST) return IDF_E_INVAL;
    if (variant == IDF_LOSS_VAL && K != 1) return IDF_E_INVAL;
    if ((int64_t)K * B > 0x7FFFFFFF) return IDF_E_INVAL;
    float *per_clip = out_per_clip;
    if (!per_clip) {
        if (!ws) return IDF_E_INVAL;
        if (ws_bytes < interdiff_sample_losses_workspace_bytes(K, B)) return IDF_E_NOMEM;
        per_clip = static_cast<float *>(ws);
    }
    const int test_variant = variant == IDF_LOSS_TEST;
    hipLaunchKernelGGL(sample_losses_kernel, dim3((unsigned)(K * B)), dim3(64 * SL_WAVES), 0, idf_stream(stream), samples, gt, hand_pose, K, B, T,
                       past_len, test_variant, per_clip);
    IDF_CHECK_LAUNCH();
    hipLaunchKernelGGL(sample_losses_finish_kernel, dim3(1), dim3(64), 0, idf_stream(stream), per_clip, K, B, test_variant, out_terms);
    IDF_CHECK_LAUNCH();
    return IDF_OK;
}
