// Training of the HO-GCN skeleton denoiser (model/diffusion_skeleton.py MDM, --ff_size 256): one call is loss.backward() of LitInteraction._common_step(mode='train')
// (train_diffusion_skeleton.py:255-262 -> forward_backward :89-168) for all 230 parameter tensors -- MDM._get_embeddings (:194-215), MDM.forward (:231-257), the 13-term
// loss -- and interdiff_mdm_train_step is its torch.optim.AdamW (:181-184).  No seam is left: the conditioning is shapeEmbedding(zero_pose_obj), a linear layer.
//
// The two stacks are the SMPL trainer's at SKELETON_GEOM (csrc/mdm_train_stack.h; device code csrc/mdm_train.h, compiled in csrc/mdm_train.hip).  This file adds what
// is the skeleton model's own: the shape embedding in the place the SMPL encoder has pc_embedding, the keypoint head behind the two output linears with its backward,
// and the gradient of the 13-term loss.  Arithmetic contract of csrc/mdm_train.h: exact fp32 (every matrix product, the shape embedding's included, is
// mt_gemm_kernel), no float atomics, every sum owned by one thread in a fixed order -- two calls give the same bits, and the backward is linear in d_pred bit for bit.
#include "mdm_train_stack.h"

using namespace mdmtrain;

namespace {

constexpr Geom GEO = SKELETON_GEOM;
constexpr int CTOK = GEO.ctok, NBODY = GEO.hbody, NPTS = 12, NOBJ = 3 * NPTS, NPOSE = GEO.hobj, HEAD = GEO.head(), N_TERMS = 13;
static_assert(CTOK == NBODY + NOBJ + NPOSE && GEO.nobj == NOBJ, "token = body | object keypoints | pose");

// ------------------------------------------------------------------------------------------------------------------ head
// pytorch3d quaternion_to_matrix on (r, i, j, k) = (pose[6], pose[3], pose[4], pose[5]), NOT normalised: R = I + two_s N(q), two_s = 2 / (q . q), N quadratic in q.
struct Quat {
    float r, i, j, k, s2;
};
__device__ __forceinline__ Quat skt_quat(const float *pose) {
    Quat q{pose[6], pose[3], pose[4], pose[5], 0.f};
    q.s2 = 2.0f / ((q.r * q.r + q.i * q.i) + (q.j * q.j + q.k * q.k));
    return q;
}
__device__ __forceinline__ void skt_n(const Quat &q, float N[3][3]) {
    N[0][0] = -(q.j * q.j + q.k * q.k); N[0][1] = q.i * q.j - q.k * q.r;    N[0][2] = q.i * q.k + q.j * q.r;
    N[1][0] = q.i * q.j + q.k * q.r;    N[1][1] = -(q.i * q.i + q.k * q.k); N[1][2] = q.j * q.k - q.i * q.r;
    N[2][0] = q.i * q.k - q.j * q.r;    N[2][1] = q.j * q.k + q.i * q.r;    N[2][2] = -(q.i * q.i + q.j * q.j);
}
// calc_obj_pred (:218-229) behind the two output linears: one thread per token row r = b*T + t.  Y [M][70] = body 63 | pose 7 (translation 3, quaternion xyzw 4);
// pred [B][106][T] = body | R(q) zero_pose_obj + translation | pose.  Adjacent threads are adjacent frames: every store instruction of a wave is contiguous in t.
__global__ __launch_bounds__(64) void skt_head_fwd_kernel(const float *__restrict__ Y, const float *__restrict__ zpo, float *__restrict__ pred, int B, int T) {
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= B * T) return;
    const int b = r / T, t = r - b * T;
    const float *y = Y + (int64_t)r * HEAD;
    float *out = pred + (int64_t)b * CTOK * T + t;
    for (int c = 0; c < NBODY; ++c) out[(int64_t)c * T] = y[c];
    float pose[NPOSE];
#pragma unroll
    for (int c = 0; c < NPOSE; ++c) {
        pose[c] = y[NBODY + c];
        out[(int64_t)(NBODY + NOBJ + c) * T] = pose[c];
    }
    const Quat q = skt_quat(pose);
    float N[3][3];
    skt_n(q, N);
    const float *z = zpo + (int64_t)b * NOBJ;
    for (int p = 0; p < NPTS; ++p) {
        const float z0 = z[3 * p], z1 = z[3 * p + 1], z2 = z[3 * p + 2];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float rot = z[3 * p + a] + q.s2 * ((N[a][0] * z0 + N[a][1] * z1) + N[a][2] * z2);
            out[(int64_t)(NBODY + 3 * p + a) * T] = rot + pose[a];
        }
    }
}
// Backward of the head, one thread per token row: d_pred [B][106][T] -> dY [M][70].  d body passes through; d pose = d_pred[pose] + J^T d_pred[obj]:
// the translation takes the sum over the 12 points, the quaternion goes through dR[a][c] = sum_p d obj[p][a] z[p][c]:
//   d q_m = two_s <dR, dN/dq_m> + <dR, N> d two_s/dq_m,   d two_s/dq_m = -two_s^2 q_m.
// The 12-point sums are this thread's own, points in ascending order.
__global__ __launch_bounds__(64) void skt_head_bwd_kernel(const float *__restrict__ dpred, const float *__restrict__ Y, const float *__restrict__ zpo, float *__restrict__ dY,
                                                          int B, int T) {
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= B * T) return;
    const int b = r / T, t = r - b * T;
    const float *g = dpred + (int64_t)b * CTOK * T + t;
    float *dy = dY + (int64_t)r * HEAD;
    for (int c = 0; c < NBODY; ++c) dy[c] = g[(int64_t)c * T];
    float pose[NPOSE];
#pragma unroll
    for (int c = 0; c < NPOSE; ++c) pose[c] = Y[(int64_t)r * HEAD + NBODY + c];
    const float *z = zpo + (int64_t)b * NOBJ;
    float dR[3][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}}, dtr[3] = {0.f, 0.f, 0.f};
    for (int p = 0; p < NPTS; ++p) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float ga = g[(int64_t)(NBODY + 3 * p + a) * T];
            dtr[a] += ga;
#pragma unroll
            for (int c = 0; c < 3; ++c) dR[a][c] += ga * z[3 * p + c];
        }
    }
    const Quat q = skt_quat(pose);
    float N[3][3];
    skt_n(q, N);
    float dn = 0.f;                                               // <dR, N>
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int c = 0; c < 3; ++c) dn += dR[a][c] * N[a][c];
    // <dR, dN/dq_m>
    const float er = (q.k * (dR[1][0] - dR[0][1]) + q.j * (dR[0][2] - dR[2][0])) + q.i * (dR[2][1] - dR[1][2]);
    const float ei = ((q.j * (dR[0][1] + dR[1][0]) + q.k * (dR[0][2] + dR[2][0])) + q.r * (dR[2][1] - dR[1][2])) - 2.0f * q.i * (dR[1][1] + dR[2][2]);
    const float ej = ((q.i * (dR[0][1] + dR[1][0]) + q.k * (dR[1][2] + dR[2][1])) + q.r * (dR[0][2] - dR[2][0])) - 2.0f * q.j * (dR[0][0] + dR[2][2]);
    const float ek = ((q.i * (dR[0][2] + dR[2][0]) + q.j * (dR[1][2] + dR[2][1])) + q.r * (dR[1][0] - dR[0][1])) - 2.0f * q.k * (dR[0][0] + dR[1][1]);
    const float ds = -(q.s2 * q.s2) * dn;
    const float *gp = g + (int64_t)(NBODY + NOBJ) * T;
#pragma unroll
    for (int a = 0; a < 3; ++a) dy[NBODY + a] = gp[(int64_t)a * T] + dtr[a];
    dy[NBODY + 3] = gp[(int64_t)3 * T] + (q.s2 * ei + ds * q.i);
    dy[NBODY + 4] = gp[(int64_t)4 * T] + (q.s2 * ej + ds * q.j);
    dy[NBODY + 5] = gp[(int64_t)5 * T] + (q.s2 * ek + ds * q.k);
    dy[NBODY + 6] = gp[(int64_t)6 * T] + (q.s2 * er + ds * q.r);
}

// ---------------------------------------------------------------------------------------------------------- loss gradient
// d/d pred of mean_b sum_i w_i term_i[b], the 13 terms of csrc/skeleton_losses.hip (forward_backward :108-127).  One thread per element.  A channel is in one of
// four groups (body 63, object keypoints 36, translation 3, quaternion 4) and takes part in its group's past or future MSE, in its velocity MSE over all T - 1 frame
// differences v_t = (x_t - x_{t-1}) - (g_t - g_{t-1}) (as the end of v_t and the start of v_{t+1}), and, a quaternion channel, in mean_t (q.q - 1)^2.
struct Weights13 {
    float w[N_TERMS];
};
__global__ __launch_bounds__(256) void skt_loss_grad_kernel(const float *__restrict__ pred, const float *__restrict__ target, int B, int T, int P, const Weights13 W,
                                                            float *__restrict__ dpred) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)B * CTOK * T) return;
    const int t = (int)(i % T), c = (int)((i / T) % CTOK);
    const int grp = c < NBODY ? 0 : c < NBODY + NOBJ ? 1 : c < NBODY + NOBJ + 3 ? 2 : 3;
    const float feat = grp == 0 ? (float)NBODY : grp == 1 ? (float)NOBJ : grp == 2 ? 3.f : 4.f;
    const float wv = grp == 0 ? W.w[11] : grp == 1 ? W.w[12] : grp == 2 ? W.w[10] : W.w[9];
    const float *x = pred + (i - t), *g = target + (i - t);
    const float xt = x[t], gt = g[t];
    const float a_val = t < P ? W.w[2 * grp] / ((float)P * feat) : W.w[2 * grp + 1] / ((float)(T - P) * feat);
    const float a_v = wv / ((float)(T - 1) * feat);
    float acc = a_val * (xt - gt);
    if (t >= 1) acc += a_v * ((xt - x[t - 1]) - (gt - g[t - 1]));
    if (t + 1 < T) acc -= a_v * ((x[t + 1] - xt) - (g[t + 1] - gt));
    if (grp == 3) {
        const float *q = pred + (i - t) - (int64_t)(c - (NBODY + NOBJ + 3)) * T + t;
        const float qq = (q[0] * q[0] + q[T] * q[T]) + (q[2 * (int64_t)T] * q[2 * (int64_t)T] + q[3 * (int64_t)T] * q[3 * (int64_t)T]);
        acc += (2.f * W.w[8] / (float)T) * ((qq - 1.0f) * xt);
    }
    dpred[i] = 2.f * acc / (float)B;
}

inline unsigned blocks256(int64_t n) { return (unsigned)idf_cdiv(n, 256); }

int loss_grad(hipStream_t st, const float *pred, const float *target, int B, int T, int P, const float *w13, float *dpred) {
    Weights13 W;
    for (int i = 0; i < N_TERMS; ++i) W.w[i] = w13[i];
    hipLaunchKernelGGL(skt_loss_grad_kernel, dim3(blocks256((int64_t)B * CTOK * T)), dim3(256), 0, st, pred, target, B, T, P, W, dpred);
    IDF_CHECK_LAUNCH();
    return IDF_OK;
}

// ---- layout: the 144 + 84 tensors of the stacks at SKELETON_GEOM, then shapeEmbedding.weight [256][36] and .bias [256] ---------------------------------------
const Layout &layout() {
    static const Layout L = make_layout(GEO);
    return L;
}
const EncLayout &enc_layout() {
    static const EncLayout L = make_enc_layout(GEO, layout());
    return L;
}
inline int64_t shape_w_off() { return enc_layout().total; }
inline int64_t shape_b_off() { return shape_w_off() + (int64_t)D * NOBJ; }
inline int64_t n_param() { return shape_b_off() + D; }

// behind the two stacks' plans: the shape row and its gradient [B][256], d_cond [S][B][256]
struct SkelWs {
    float *shape, *d_shape, *d_cond;
    size_t floats;
};
SkelWs skel_plan(float *base, size_t at, int B, int S) {
    SkelWs w{};
    Carver take{base, at};
    w.shape = take((size_t)B * D); w.d_shape = take((size_t)B * D); w.d_cond = take((size_t)S * B * D);
    w.floats = take.at;
    return w;
}

}  // namespace

extern "C" int interdiff_skeleton_denoising_loss_grad(const float *pred, const float *target, int32_t B, int32_t T, int32_t past_len, const float *weights13,
                                                      float *d_pred, void *stream) {
    if (!pred || !target || !weights13 || !d_pred || B <= 0 || past_len < 1 || T < past_len + 1 || (int64_t)B * CTOK * T > 0x7FFFFFFF) return IDF_E_INVAL;
    return loss_grad(idf_stream(stream), pred, target, B, T, past_len, weights13, d_pred);
}

extern "C" int interdiff_skeleton_mdm_train_param_table(int64_t *offsets, int64_t *sizes, int32_t *n_tensors, int64_t *n_param_out) {
    const Layout &L = layout();
    const EncLayout &EL = enc_layout();
    const int64_t shape_off[2] = {shape_w_off(), shape_b_off()}, shape_size[2] = {(int64_t)D * NOBJ, D};
    return table_out({{L.off, L.size, N_TENSORS}, {EL.off, EL.size, N_ENC_TENSORS}, {shape_off, shape_size, 2}}, n_param(), offsets, sizes, n_tensors, n_param_out);
}

extern "C" size_t interdiff_skeleton_mdm_train_workspace_bytes(int32_t B, int32_t T, int32_t past_len) {
    if (!shape_ok(GEO, B, T, past_len, past_len)) return 0;
    return skel_plan(nullptr, full_plan(nullptr, GEO, layout(), B, T, past_len).e.floats, B, past_len).floats * sizeof(float);
}

extern "C" int interdiff_skeleton_mdm_train_grads(const float *params, const float *pe, int32_t pe_rows, const float *x_t, const int64_t *ts, const float *target,
                                                  const float *zero_pose_obj, int32_t B, int32_t T, int32_t past_len, const float *weights13, const float *d_pred_in,
                                                  float *grads, float *cond, float *pred, float *terms, void *ws, size_t ws_bytes, void *stream) {
    if (!params || !pe || !x_t || !ts || !target || !zero_pose_obj || !weights13 || !grads || !cond || !pred || !terms || !ws) return IDF_E_INVAL;
    if (!shape_ok(GEO, B, T, past_len, past_len) || pe_rows < T) return IDF_E_INVAL;
    MT_TRY(ws_check(ws, ws_bytes, interdiff_skeleton_mdm_train_workspace_bytes(B, T, past_len)));
    hipStream_t st = idf_stream(stream);
    const Layout &L = layout();
    const EncLayout &EL = enc_layout();
    float *base = static_cast<float *>(ws);
    const auto [w, e] = full_plan(base, GEO, L, B, T, past_len);
    const SkelWs k = skel_plan(base, e.floats, B, past_len);
    const int M = B * T;
    // _get_embeddings: the shape row takes the place pc_embedding has in the SMPL encoder
    MT_TRY(lin_fwd(st, zero_pose_obj, NOBJ, params + shape_w_off(), params + shape_b_off(), k.shape, D, nullptr, 0, B, D, NOBJ));
    MT_TRY(enc_forward(st, L, EL, w, e, params, pe, target, k.shape, B, T, past_len, cond));
    // MDM.forward: the decoder, the two output linears, the keypoint head
    MT_TRY(forward(st, L, w, params, pe, pe_rows, x_t, ts, cond, B, T, past_len));
    hipLaunchKernelGGL(skt_head_fwd_kernel, dim3((unsigned)idf_cdiv(M, 64)), dim3(64), 0, st, w.Y, zero_pose_obj, pred, B, T);
    IDF_CHECK_LAUNCH();
    MT_TRY(interdiff_skeleton_denoising_losses(pred, target, B, T, past_len, NBODY, NPTS, terms, stream));
    const float *dp = d_pred_in;
    if (!dp) {
        float *mine = w.g;                                        // (free between the forward and the backward; M * 256 >= B * 106 * T floats)
        MT_TRY(loss_grad(st, pred, target, B, T, past_len, weights13, mine));
        dp = mine;
    }
    hipLaunchKernelGGL(skt_head_bwd_kernel, dim3((unsigned)idf_cdiv(M, 64)), dim3(64), 0, st, dp, w.Y, zero_pose_obj, w.dY, B, T);
    IDF_CHECK_LAUNCH();
    MT_TRY(backward(st, L, w, params, cond, B, T, past_len, grads, k.d_cond));
    MT_TRY(enc_backward(st, L, EL, w, e, params, k.d_cond, B, past_len, grads, k.d_shape));
    // shapeEmbedding: weight = d_shape^T zero_pose_obj, bias = its column sum; zero_pose_obj is data
    return lin_param_grads(st, w, k.d_shape, D, zero_pose_obj, NOBJ, grads + shape_w_off(), grads + shape_b_off(), B, D, NOBJ);
}
