// The physics-informed correction hook `denoised_fn` (row C1 of SURVEY.md §8), fused.
//
// Behaviour restated from eval_smpl_short.py:84-130.  The reference builds the object point cloud
// [T,B,2048,3], all vertex normals (3 scatter-adds), both nearest-neighbour directions, and TWO
// [T,B,2048,67] marker-distance tensors (2 x 878 MB at B=16,T=100, via 2.6 GB temporaries).  Only
// the object->human signed distance, the per-frame minimum marker distance and the per-marker
// contact flag are ever consumed, so here one workgroup per frame
//   - parks the frame's 6890 vertices in LDS (110 KB of the CU's 160 KB),
//   - transforms its share of the canonical object points on the fly (never stored),
//   - scans the vertices for the exact nearest neighbour (same arithmetic as geometry.hip),
//   - evaluates the vertex normal ONLY at the nearest vertices, from LDS, through the adjacency,
//   - reduces loss / min-distance / contact flags in LDS and writes a few floats per frame.
// Frame index n = t*B + b everywhere (the reference's .view(T*B, ...)).
//
// This file is the hook (K1 prepare, K5 reduce, K7 blend, its workspace, correction_impl) and every definition with external linkage.  The kernel families
// it launches are headers of this ONE translation unit:
//   contact_scan.h   K3 / K4: the clips' point order, the nearest-vertex scan corr_contact_kernel<OPT, WITH_PRED>, ContactArgs and the one launch_contact
//   near_mask.h      the post-optimisation's contact-radius mask (opt_patch_kernel, opt_near_kernel)
//   corr_metrics.h   the evaluation metrics' kernels and the workspace they share with the stand-alone scan
// (vec3.h: ld3 / sub3 / cross3, shared with geometry.hip and optimize.hip.)  Each header is included where its kernels stood in this file, so the code
// object keeps its kernel order.
#include "common.h"
#include "objproj.h"
#include "rot_math.h"
#include <float.h>

namespace {

constexpr int NBODY = 22;              // body joints predicted as rot6d (smpl_dim = 132)
constexpr int CTOK = 144;

// ---- K1: tokens -> SMPL pose (axis-angle), translation, object rotation/translation -----------------
// one thread per (frame, slot): slots 0..21 body joints, 22 = hands + trans copy, 23 = object
__global__ __launch_bounds__(256) void corr_prepare_kernel(const float *__restrict__ x0, const float *__restrict__ gt,
                                                           const float *__restrict__ hand_pose, int B, int T,
                                                           float *__restrict__ pose, float *__restrict__ trans,
                                                           float *__restrict__ objR, float *__restrict__ objT,
                                                           float *__restrict__ gt_angles, float *__restrict__ gt_trans) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t N = (int64_t)B * T;
    if (i >= N * 24) return;
    const int64_t n = i / 24;
    const int slot = (int)(i - n * 24), t = (int)(n / B), b = (int)(n - (int64_t)t * B);
    const float *xb = x0 + (size_t)b * CTOK * T + t;                   // channel c at xb[c*T]
    if (slot < NBODY) {
        float d[6], m[9], a[3];
#pragma unroll
        for (int k = 0; k < 6; ++k) d[k] = xb[(size_t)(slot * 6 + k) * T];
        rot::rot6d_to_matrix(d, m);
        rot::matrix_to_axis_angle(m, a);
        float *p = pose + n * 156 + slot * 3;
        p[0] = a[0]; p[1] = a[1]; p[2] = a[2];
    } else if (slot == 22) {
        for (int k = 0; k < 90; ++k) pose[n * 156 + 66 + k] = hand_pose[n * 90 + k];
#pragma unroll
        for (int k = 0; k < 3; ++k) trans[n * 3 + k] = xb[(size_t)(132 + k) * T];
    } else {
        float d[6], m[9];
#pragma unroll
        for (int k = 0; k < 6; ++k) d[k] = xb[(size_t)(135 + k) * T];
        rot::rot6d_to_matrix(d, m);
#pragma unroll
        for (int k = 0; k < 9; ++k) objR[n * 9 + k] = m[k];
        const float *gb = gt + (size_t)b * CTOK * T + t;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            objT[n * 3 + k] = xb[(size_t)(141 + k) * T];
            gt_trans[n * 3 + k] = gb[(size_t)(141 + k) * T];
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) gt_angles[n * 6 + k] = gb[(size_t)(135 + k) * T];
    }
}

}  // namespace

#include "contact_scan.h"

namespace {

// ---- K5: per-clip decisions (eval_smpl_short.py:119-125) ---------------------------------------------
__global__ __launch_bounds__(128) void corr_reduce_kernel(const float *__restrict__ loss_sum, const float *__restrict__ min_dist,
                                                          const int32_t *__restrict__ label, int B, int T, int past, int P, int M,
                                                          uint8_t *__restrict__ condition, int32_t *__restrict__ contact,
                                                          float *__restrict__ distance_out, float *__restrict__ loss_out) {
    // the per-frame values are fetched by all threads at once (one memory round trip instead of T dependent ones: the serial loop
    // cost 60 us per call) and summed by thread 0 from LDS in the reference's order, frame by frame: the same bits as before
    extern __shared__ float fr[];                         // [T] loss sums | [T] minimum distances
    const int b = blockIdx.x, tid = threadIdx.x;
    for (int t = tid; t < T; t += 128) {
        fr[t] = loss_sum[(size_t)t * B + b];
        fr[T + t] = min_dist[(size_t)t * B + b];
    }
    if (tid < M) {
        int c = 0;
#pragma unroll 16
        for (int t = past; t < T; ++t) c += label[((size_t)t * B + b) * M + tid];           // independent loads: sixteen in flight
        contact[(size_t)b * M + tid] = c;
    }
    __syncthreads();
    if (tid == 0) {
        float ls = 0.f, ds = 0.f;
        for (int t = past; t < T; ++t) ls += fr[t] / (float)P;                             // mean over points, then frames
        for (int t = 0; t < T; ++t) ds += fr[T + t];
        const float loss = ls / (float)(T - past), dist = ds / (float)T;
        condition[b] = !((loss < 0.002f) && (dist < 0.02f));
        if (distance_out) distance_out[b] = dist;
        if (loss_out) loss_out[b] = loss;
    }
}

// ---- K7: blend (eval_smpl_short.py:127-129): x = a*x + (1-a)*[body, proj] where condition ------------
// a: the blend weight t / 1000 by value, or -- a_table != null -- read on the device as a_table[state[0] * 4 + 3] (the sampler's
// coefficient table and state: a captured hipGraph of a whole hook step then serves every timestep)
__global__ __launch_bounds__(256) void corr_blend_kernel(float *__restrict__ x0, const float *__restrict__ proj,
                                                         const uint8_t *__restrict__ condition, int B, int T, float a,
                                                         const float *__restrict__ a_table, const int64_t *__restrict__ a_state) {
    if (a_table) a = a_table[a_state[0] * 4 + 3];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)B * CTOK * T) return;
    const int b = (int)(i / (CTOK * T)), r = (int)(i - (int64_t)b * CTOK * T), c = r / T, t = r - c * T;
    if (!condition[b]) return;
    const float x = x0[i];
    const float other = c < 135 ? x : proj[((size_t)t * B + b) * 9 + (c - 135)];
    x0[i] = a * x + (1.0f - a) * other;
}

struct CorrWs {
    float *pose, *trans, *objR, *objT, *gt_angles, *gt_trans, *verts, *jtr, *markers, *loss_sum, *min_dist, *proj, *proj_keep;
    int32_t *label, *contact, *porder;
    uint8_t *condition;
    void *smpl_ws;
    size_t smpl_ws_bytes, total;
};

CorrWs carve(const idf_correction_ctx *c, int B, int T, void *ws) {
    const int64_t N = (int64_t)B * T;
    const int V = c->smpl->V, J = c->smpl->J, M = c->n_markers;
    char *p = reinterpret_cast<char *>(ws);
    size_t off = 0;
    auto take = [&](size_t bytes) { char *r = p ? p + off : nullptr; off += idf_align(bytes); return r; };
    CorrWs w;
    w.pose = (float *)take(N * 156 * 4);
    w.trans = (float *)take(N * 3 * 4);
    w.objR = (float *)take(N * 9 * 4);
    w.objT = (float *)take(N * 3 * 4);
    w.gt_angles = (float *)take(N * 6 * 4);
    w.gt_trans = (float *)take(N * 3 * 4);
    w.verts = (float *)take((size_t)N * V * 3 * 4);
    w.jtr = (float *)take((size_t)N * J * 3 * 4);
    w.markers = (float *)take((size_t)N * M * 3 * 4);
    w.loss_sum = (float *)take(N * 4);
    w.min_dist = (float *)take(N * 4);
    w.proj = (float *)take(N * 9 * 4);
    w.label = (int32_t *)take((size_t)N * M * 4);
    w.contact = (int32_t *)take((size_t)B * M * 4);
    w.condition = (uint8_t *)take(B);
    w.porder = (int32_t *)take((size_t)B * c->n_points * 4);
    w.proj_keep = (float *)take((size_t)B * idf_objproj_keep_floats() * 4);
    w.smpl_ws_bytes = interdiff_smpl_workspace_bytes(c->smpl, N);
    w.smpl_ws = take(w.smpl_ws_bytes);
    w.total = off;
    return w;
}

}  // namespace

#include "near_mask.h"

extern "C" size_t interdiff_correction_workspace_bytes(const idf_correction_ctx *c, int32_t B, int32_t T) {
    if (!c || !c->smpl || B <= 0 || T <= 0) return 0;
    return carve(c, B, T, nullptr).total;
}

static int correction_impl(const idf_correction_ctx *c, float *x0, const float *gt, const float *hand_pose,
                           const float *beta, const float *obj_points, int32_t B, int32_t T, float blend_t, const float *blend_table,
                           const int64_t *blend_state, uint8_t *condition, int32_t *contact, float *distance, float *loss, void *ws,
                           size_t ws_bytes, void *stream) {
    if (!c || !c->smpl || !c->objproj || !x0 || !gt || !hand_pose || !beta || !obj_points || !ws || B <= 0 || T <= 0) return IDF_E_INVAL;
    const int V = c->smpl->V, M = c->n_markers, P = c->n_points;
    if (c->smpl->J != 52 || c->smpl->n_betas != 10 || M > MAXM || M != c->objproj->P || P > MAXP || T != c->objproj->T ||
        c->past_len != c->objproj->past_len || c->past_len >= T)
        return IDF_E_INVAL;
    CorrWs w = carve(c, B, T, ws);
    if (ws_bytes < w.total) return IDF_E_NOMEM;
    hipStream_t s = idf_stream(stream);
    const int64_t N = (int64_t)B * T;
    // Round 6: the predictor's three stacks need the markers only -- the contact labels pick which node's IDCT is evaluated at the very end -- so they ride in the contact scan's
    // launch as B leading workgroups (corr_contact_kernel<false, true>) and only the pick + IDCT kernel follows the labels.  ctx.tune & 2 (A/B, tests): scan, then the one-launch
    // predictor.  Same arithmetic either way: same bits.
    const bool fused = (c->tune & 2) == 0 && idf_objproj_check(c->objproj) == IDF_OK;
    idf_prof_mark(IDF_K_CORR_PREPARE, s);
    hipLaunchKernelGGL(corr_prepare_kernel, dim3((unsigned)idf_cdiv(N * 24, 256)), dim3(256), 0, s, x0, gt, hand_pose, B, T, w.pose,
                       w.trans, w.objR, w.objT, w.gt_angles, w.gt_trans);
    int rc = interdiff_smpl_forward(c->smpl, w.pose, beta, w.trans, N, w.verts, w.jtr, nullptr, w.smpl_ws, w.smpl_ws_bytes, stream);
    if (rc) return rc;
    idf_prof_mark(IDF_K_CORR_CONTACT, s);
    // (the hook always launches the instantiation that CAN carry the predictor, with no predictor workgroups in the A/B form: two instantiations of the same source were seen to
    // differ in the last bit of a frame's loss -- the compiler contracts the normal / signed-distance expressions per instantiation)
    ContactArgs a{};
    a.verts = w.verts; a.V = V;
    a.obj_points = obj_points; a.P = P;
    a.porder = w.porder;
    a.objR = w.objR; a.objT = w.objT;
    a.ctx = c;
    a.B = B;
    a.markers = fused ? nullptr : w.markers;            // fused: the predictor's workgroups gather them
    a.loss_sum = w.loss_sum; a.min_dist = w.min_dist; a.label = w.label;
    a.nn_from = (int64_t)c->past_len * B;
    if (fused) {
        PredArgs &pred = a.pred;
        pred.op = *c->objproj;
        pred.obj_angles = w.gt_angles; pred.obj_trans = w.gt_trans;
        pred.markers_idx = c->markers_idx; pred.markers = w.markers; pred.keep = w.proj_keep;
        pred.nclips = B;
    }
    rc = launch_contact<false, true>(s, N, a);
    if (rc) return rc;
    uint8_t *cond = condition ? condition : w.condition;
    int32_t *cont = contact ? contact : w.contact;
    idf_prof_mark(IDF_K_CORR_REDUCE, s);
    hipLaunchKernelGGL(corr_reduce_kernel, dim3(B), dim3(128), 2 * (size_t)T * sizeof(float), s, w.loss_sum, w.min_dist, w.label, B, T, c->past_len, P, M, cond,
                       cont, distance, loss);
    if (fused) {
        idf_prof_mark(IDF_K_OBJPROJ, s);
        rc = idf_objproj_pick(c->objproj, w.proj_keep, cont, B, w.proj, s);
    } else {
        rc = interdiff_objprojector_sample(c->objproj, w.gt_angles, w.gt_trans, w.markers, cont, B, w.proj, stream);
    }
    if (rc) return rc;
    idf_prof_mark(IDF_K_CORR_BLEND, s);
    hipLaunchKernelGGL(corr_blend_kernel, dim3((unsigned)idf_cdiv((int64_t)B * CTOK * T, 256)), dim3(256), 0, s, x0, w.proj, cond, B, T,
                       blend_t, blend_table, blend_state);
    idf_prof_mark(-1, s);
    IDF_CHECK_LAUNCH();
    return IDF_OK;
}

extern "C" int interdiff_correction(const idf_correction_ctx *c, float *x0, const float *gt, const float *hand_pose,
                                    const float *beta, const float *obj_points, int32_t B, int32_t T, float blend_t,
                                    uint8_t *condition, int32_t *contact, float *distance, float *loss, void *ws,
                                    size_t ws_bytes, void *stream) {
    return correction_impl(c, x0, gt, hand_pose, beta, obj_points, B, T, blend_t, nullptr, nullptr, condition, contact, distance, loss, ws, ws_bytes, stream);
}

extern "C" int interdiff_correction_dev(const idf_correction_ctx *c, float *x0, const float *gt, const float *hand_pose,
                                        const float *beta, const float *obj_points, int32_t B, int32_t T, const float *table,
                                        const int64_t *state, void *ws, size_t ws_bytes, void *stream) {
    if (!table || !state) return IDF_E_INVAL;
    return correction_impl(c, x0, gt, hand_pose, beta, obj_points, B, T, 0.f, table, state, nullptr, nullptr, nullptr, nullptr, ws, ws_bytes, stream);
}

// ---- evaluation metrics (row E1, eval_smpl_short.py:24-81) --------------------------------------------------------
#include "corr_metrics.h"

// The scan's operands as both entries below give them: every frame scanned, markers / loss / labels into the workspace
static ContactArgs metrics_scan_args(const idf_correction_ctx *c, const MetWs &w, const float *verts, const float *obj_points, const float *objR, const float *objT, int B) {
    ContactArgs a{};
    a.verts = verts; a.V = c->smpl->V;
    a.obj_points = obj_points; a.P = c->n_points;
    a.porder = w.porder;
    a.objR = objR; a.objT = objT;
    a.ctx = c;
    a.B = B;
    a.markers = w.markers; a.loss_sum = w.loss_sum; a.min_dist = w.min_dist; a.label = w.label;
    return a;
}

// The contact scan on its own: signed object->human distance and nearest vertex of every object point of every frame
// (tools.point2point_signed's o2h half fused with the object transform, eval_smpl_short.py:107-112).  Frames n = t*B + b.
extern "C" size_t interdiff_contact_nn_workspace_bytes(const idf_correction_ctx *c, int32_t B, int32_t T) {
    if (!c || B <= 0 || T <= 0) return 0;
    return carve_metrics(c, B, T, nullptr).total;
}

extern "C" int interdiff_contact_nn(const idf_correction_ctx *c, const float *verts, const float *obj_points, const float *objR,
                                    const float *objT, int32_t B, int32_t T, float *o2h, int32_t *idx, uint64_t *stats, void *ws,
                                    size_t ws_bytes, void *stream) {
    if (!c || !c->smpl || !verts || !obj_points || !objR || !objT || !ws || B <= 0 || T <= 0 || (!o2h && !idx)) return IDF_E_INVAL;
    if (c->n_markers > MAXM || c->n_points > MAXP) return IDF_E_INVAL;
    MetWs w = carve_metrics(c, B, T, ws);
    if (ws_bytes < w.total) return IDF_E_NOMEM;
    hipStream_t s = idf_stream(stream);
    if (stats && hipMemsetAsync(stats, 0, IDF_CONTACT_STATS * sizeof(uint64_t), s) != hipSuccess) return IDF_E_LAUNCH;
    ContactArgs a = metrics_scan_args(c, w, verts, obj_points, objR, objT, B);
    a.o2h = o2h ? o2h : w.o2h; a.idx = idx;
    a.stats = reinterpret_cast<unsigned long long *>(stats);
    const int rc = launch_contact<false, false>(s, (int64_t)B * T, a);
    if (rc) return rc;
    IDF_CHECK_LAUNCH();
    return IDF_OK;
}

extern "C" size_t interdiff_metrics_workspace_bytes(const idf_correction_ctx *c, int32_t B, int32_t T) {
    if (!c || B <= 0 || T <= 0) return 0;
    return carve_metrics(c, B, T, nullptr).total;
}

extern "C" int interdiff_metrics(const idf_correction_ctx *c, const float *obj_pred, const float *jtr, const float *body_trans,
                                 const float *obj_gt, const float *jtr_gt, const float *body_trans_gt, const float *verts,
                                 const float *obj_points, int32_t B, int32_t T, int32_t J, float *out6, void *ws, size_t ws_bytes,
                                 void *stream) {
    if (!c || !c->smpl || !obj_pred || !jtr || !body_trans || !obj_gt || !jtr_gt || !body_trans_gt || !verts || !obj_points || !out6 ||
        !ws || B <= 0 || T <= 0 || J <= 0)
        return IDF_E_INVAL;
    const int M = c->n_markers, P = c->n_points;
    if (M > MAXM || P > MAXP) return IDF_E_INVAL;
    MetWs w = carve_metrics(c, B, T, ws);
    if (ws_bytes < w.total) return IDF_E_NOMEM;
    hipStream_t s = idf_stream(stream);
    const int64_t N = (int64_t)B * T;
    idf_prof_mark(IDF_K_OTHER, s);
    hipLaunchKernelGGL(metrics_prepare_kernel, dim3((unsigned)idf_cdiv(N, 256)), dim3(256), 0, s, obj_pred, N, w.objR, w.objT);
    ContactArgs a = metrics_scan_args(c, w, verts, obj_points, w.objR, w.objT, B);
    a.o2h = w.o2h;
    const int rc = launch_contact<false, false>(s, N, a);
    if (rc) return rc;
    hipLaunchKernelGGL(metrics_reduce_kernel, dim3(B), dim3(256), 0, s, obj_pred, jtr, body_trans, obj_gt, jtr_gt, body_trans_gt, w.o2h, B,
                       T, J, P, out6);
    idf_prof_mark(-1, s);
    IDF_CHECK_LAUNCH();
    return IDF_OK;
}

// ---- what optimize.hip calls (declared in common.h) ---------------------------------------------------------------
// (Last in the file on purpose: the scan's instantiations are emitted in the order of their first use -- hook, stand-alone scan, post-optimisation -- and with
// these three ahead of the hook, <false, false> and <true, false> compiled to DIFFERENT machine code: profiles/correction_split_ab.json.)
// The nearest-vertex half of the post-optimisation's scan (optimize.hip; declared in common.h): per transformed object point of
// every frame the nearest vertex.  Frames clip-major (n = b*T + t); `porder` [B][P] = idf_point_order of the clips' canonical points
// (they do not change over the iterations: computed once by interdiff_optimize_init).
int idf_point_order(hipStream_t s, const float *obj_points, int B, int P, int32_t *porder) {
    if (P > MAXP) return IDF_E_INVAL;
    hipLaunchKernelGGL(corr_point_order_kernel, dim3((unsigned)B), dim3(1024), 0, s, obj_points, P, porder);
    return IDF_OK;
}

int idf_nn_scan_opt(hipStream_t s, int64_t N, int frames_per_clip, const float *verts, int V, const float *pts_frame, const float *obj_points, int P,
                    const int32_t *porder, const idf_correction_ctx *c, int32_t *yidx) {
    ContactArgs a{};
    a.verts = verts; a.V = V;
    a.obj_points = obj_points; a.P = P;
    a.porder = const_cast<int32_t *>(porder);          // OPT only reads it
    a.ctx = c;
    a.B = (int)(N / frames_per_clip);
    a.idx = yidx;
    a.pts_frame = pts_frame; a.frames_per_clip = frames_per_clip;
    return launch_contact<true, false>(s, N, a);
}

// ... and the contact-radius mask: near[n][v] = 1 iff some object point of frame n lies within 0.5 m of vertex v (near_mask.h).
int idf_near_mask_opt(hipStream_t s, int64_t N, int frames_per_clip, const float *verts, int V, const float *pts_frame, int P, const int32_t *porder,
                      const int32_t *vorder, float *psort, float *pbox, int32_t *near) {
    return launch_near_mask(s, N, frames_per_clip, verts, V, pts_frame, P, porder, vorder, psort, pbox, near);
}
