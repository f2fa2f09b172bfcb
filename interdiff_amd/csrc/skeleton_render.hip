// Skeleton-mode clips (interdiff/render/viz_helper.py: visualize_skeleton, visualize_skeleton_pred_gt, restated without matplotlib).
// The contract of both stages -- record layout, draw order, 1/16-pixel grid, coverage rule, blend arithmetic, bit widths -- is the head comment of
// skeleton_render.h.
//
// LAUNCH PLAN, per chunk of frames (a frame = one image; the chunk is what the workspace holds):
//   sk_setup    one workgroup (128 lanes) per frame, the frame's state (SkFrame, 7 KB) in LDS.  Lane = point: fetch, finite test; lanes 0..5: min / max
//               over the points in LDS; lane = point: limits -> camera -> snap; lanes 0..1: depth range per scatter collection; lane = slot: the
//               record (markers: rank by counting, depth-shade alpha).  Records leave through LDS, 128 x 8 int32 per frame, in draw order.  fp32 ends here.
//   sk_raster   one workgroup (256 lanes) per (tile of 16 x 16 pixels, frame).  The frame's records sit in LDS (4 KB); lane k < count marks record k when
//               its pixel box reaches the tile; each lane then owns one pixel and folds the marked records in draw order (4 x 4 samples, integer "over").
// No atomics but the 32-bit integer add of the dropped counter; no cooperative launch, no spin.
#include "common.h"
#include "skeleton_render.h"
#include <algorithm>

namespace {

constexpr int SK_RASTER_THR = SK_TILE * SK_TILE;
static_assert(SK_RASTER_THR >= SK_MAX_REC, "one lane per record in the marking pass");

struct SkLayout { size_t hdr, rec, total; };

SkLayout sk_layout(int64_t c) {
    SkLayout L;
    size_t o = 0;
    L.hdr = o; o += 256;
    L.rec = o; o += idf_align((size_t)c * SK_MAX_REC * SK_REC * 4);
    L.total = o;
    return L;
}

__global__ __launch_bounds__(SK_LANES) void sk_setup_kernel(idf_skel_view v, const float *__restrict__ body, const float *__restrict__ obj,
                                                            const float *__restrict__ body_gt, const float *__restrict__ obj_gt,
                                                            const int32_t *__restrict__ wires, int n_wires, int64_t f0, int T, int T_gt,
                                                            int32_t *__restrict__ recs, int32_t *__restrict__ out_count,
                                                            int32_t *__restrict__ dropped) {
    __shared__ SkFrame f;
    const int lane = threadIdx.x;
    const int64_t fr = f0 + blockIdx.x, clip = fr / T;
    SkArgs a;
    a.body = body + (size_t)clip * T * SK_NB * 3; a.obj = obj + (size_t)clip * T * SK_NO * 3;
    a.body_gt = body_gt ? body_gt + (size_t)clip * T_gt * SK_NB * 3 : nullptr; a.obj_gt = obj_gt ? obj_gt + (size_t)clip * T_gt * SK_NO * 3 : nullptr;
    a.wires = wires; a.n_wires = n_wires; a.T = T; a.T_gt = T_gt; a.t = (int)(fr % T);
    for (int i = lane; i < SK_MAX_REC * SK_REC; i += SK_LANES) (&f.rec[0][0])[i] = 0;
    f.drop[lane] = 0;
    sk_phase_load(f, lane, v, a);
    __syncthreads();
    sk_phase_limits(f, lane);
    __syncthreads();
    sk_phase_project(f, lane, v);
    __syncthreads();
    if (v.style == IDF_SKEL_PLAIN) {
        sk_phase_groups(f, lane);
        __syncthreads();
    }
    sk_phase_emit(f, lane, v, a);
    __syncthreads();
    int32_t *out = recs + (size_t)blockIdx.x * SK_MAX_REC * SK_REC;
    const int32_t *src = &f.rec[0][0];
    for (int i = lane; i < SK_MAX_REC * SK_REC; i += SK_LANES) out[i] = src[i];
    if (lane == 0) {
        if (out_count) out_count[fr] = sk_count(v, n_wires);          // every frame uses the same number of slots (a group that is not drawn keeps its, empty)
        int nd = 0;
        for (int i = 0; i < SK_LANES; ++i) nd += f.drop[i];
        if (nd) atomicAdd(dropped, nd);
    }
}

__global__ __launch_bounds__(SK_RASTER_THR) void sk_raster_kernel(const int32_t *__restrict__ recs, int count, int H, int W, int tiles_x, int64_t f0,
                                                                  uint8_t *__restrict__ out_rgb) {
    __shared__ int32_t rec[SK_MAX_REC][SK_REC];
    __shared__ uint8_t hit[SK_MAX_REC];
    const int tid = threadIdx.x, tile = blockIdx.x, li = blockIdx.y;
    const int tx = tile % tiles_x, ty = tile / tiles_x;
    const int x0 = tx * SK_TILE, y0 = ty * SK_TILE, x1 = min(x0 + SK_TILE, W) - 1, y1 = min(y0 + SK_TILE, H) - 1;          // the tile's pixels, inclusive
    const int32_t *src = recs + (size_t)li * SK_MAX_REC * SK_REC;
    for (int i = tid; i < count * SK_REC; i += SK_RASTER_THR) (&rec[0][0])[i] = src[i];
    __syncthreads();
    if (tid < count) {
        int i0, i1, j0, j1;
        hit[tid] = sk_pixel_box(sk_load(rec[tid]), H, W, i0, i1, j0, j1) && i0 <= x1 && i1 >= x0 && j0 <= y1 && j1 >= y0;
    }
    __syncthreads();
    const int pi = x0 + (tid & (SK_TILE - 1)), pj = y0 + tid / SK_TILE;
    if (pi >= W || pj >= H) return;
    int32_t acc[3] = {255 << 8, 255 << 8, 255 << 8};
    for (int k = 0; k < count; ++k) {
        if (!hit[k]) continue;
        const SkPrim p = sk_load(rec[k]);
        int i0, i1, j0, j1;
        sk_pixel_box(p, H, W, i0, i1, j0, j1);
        if (pi < i0 || pi > i1 || pj < j0 || pj > j1) continue;
        const int n = sk_samples(p, pi, pj);
        if (n) sk_blend(acc, p, n);
    }
    uint8_t *o = out_rgb + (((size_t)(f0 + li) * H + pj) * W + pi) * 3;
    o[0] = (uint8_t)((acc[0] + 128) >> 8); o[1] = (uint8_t)((acc[1] + 128) >> 8); o[2] = (uint8_t)((acc[2] + 128) >> 8);
}

bool sk_aligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

int sk_check_view(const idf_skel_view *v, int32_t n_wires, int32_t T, int32_t T_gt, const void *body_gt, const void *obj_gt) {
    if (!v || (v->style != IDF_SKEL_PLAIN && v->style != IDF_SKEL_PREDGT)) return IDF_E_INVAL;
    if (v->line_wd < 1 || v->line_wd > SK_WD_MAX || v->disc_wd < 1 || v->disc_wd > SK_WD_MAX) return IDF_E_INVAL;
    if (n_wires < 0 || n_wires > IDF_SKEL_MAX_WIRES || T < 1 || T_gt < 0) return IDF_E_INVAL;
    if ((body_gt == nullptr) != (obj_gt == nullptr)) return IDF_E_INVAL;
    if (v->style == IDF_SKEL_PLAIN && (body_gt || n_wires)) return IDF_E_INVAL;
    if (body_gt && T_gt < 1) return IDF_E_INVAL;
    return IDF_OK;
}

}  // namespace

extern "C" size_t interdiff_skeleton_render_frames_workspace_bytes(int64_t n_frames) {
    if (n_frames <= 0) return 0;
    return sk_layout(n_frames).total;
}

extern "C" int interdiff_skeleton_render_frames(const idf_skel_view *view, const float *body, const float *obj, const float *body_gt, const float *obj_gt,
                                                const int32_t *wires, int32_t n_wires, int64_t B, int32_t T, int32_t T_gt, int32_t H, int32_t W,
                                                uint8_t *out_rgb, int32_t *out_setup, int32_t *out_count, int64_t *dropped, float *stage_ms, void *ws,
                                                size_t ws_bytes, void *stream) {
    const int rc = sk_check_view(view, n_wires, T, T_gt, body_gt, obj_gt);
    if (rc != IDF_OK) return rc;
    if (!body || !obj || !out_rgb || !ws || (n_wires > 0 && !wires)) return IDF_E_INVAL;
    if (!sk_aligned4(body) || !sk_aligned4(obj) || !sk_aligned4(body_gt) || !sk_aligned4(obj_gt) || !sk_aligned4(wires) || !sk_aligned4(out_setup) ||
        !sk_aligned4(out_count) || (reinterpret_cast<uintptr_t>(ws) & 255))
        return IDF_E_INVAL;
    if (B < 1 || B > (1 << 20) || T > (1 << 20) || H < 1 || W < 1 || H > IDF_RENDER_MAX_DIM || W > IDF_RENDER_MAX_DIM) return IDF_E_INVAL;
    const int64_t n_fr = B * T;
    if (ws_bytes < sk_layout(1).total) return IDF_E_NOMEM;
    int64_t chunk = std::min<int64_t>(n_fr, 0xFFFF);             // frames ride on gridDim.y of the raster launch
    chunk = std::min<int64_t>(chunk, (int64_t)((ws_bytes - 256) / ((size_t)SK_MAX_REC * SK_REC * 4)));
    while (chunk > 1 && sk_layout(chunk).total > ws_bytes) --chunk;
    const SkLayout L = sk_layout(chunk);
    hipStream_t s = idf_stream(stream);
    char *w8 = static_cast<char *>(ws);
    int32_t *hdr = reinterpret_cast<int32_t *>(w8 + L.hdr), *recs = reinterpret_cast<int32_t *>(w8 + L.rec);          // hdr[0]: dropped primitives
    if (hipMemsetAsync(hdr, 0, 256, s) != hipSuccess) return IDF_E_LAUNCH;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    float ms[2] = {0.f, 0.f};
    auto mark = [&](int i) { if (stage_ms) (void)hipEventRecord(ev[i], s); };
    auto cleanup = [&]() { for (auto &e : ev) if (e) { (void)hipEventDestroy(e); e = nullptr; } };
    if (stage_ms)
        for (auto &e : ev)
            if (hipEventCreate(&e) != hipSuccess) { e = nullptr; cleanup(); return IDF_E_LAUNCH; }
    const int tiles_x = (int)idf_cdiv(W, SK_TILE), tiles_y = (int)idf_cdiv(H, SK_TILE), count = sk_count(*view, n_wires);
    for (int64_t f0 = 0; f0 < n_fr; f0 += chunk) {
        const unsigned c = (unsigned)std::min<int64_t>(chunk, n_fr - f0);
        mark(0);
        hipLaunchKernelGGL(sk_setup_kernel, dim3(c), dim3(SK_LANES), 0, s, *view, body, obj, body_gt, obj_gt, wires, n_wires, f0, T, T_gt, recs, out_count, hdr);
        mark(1);
        hipLaunchKernelGGL(sk_raster_kernel, dim3((unsigned)(tiles_x * tiles_y), c), dim3(SK_RASTER_THR), 0, s, recs, count, H, W, tiles_x, f0, out_rgb);
        mark(2);
        if (hipGetLastError() != hipSuccess) { cleanup(); return IDF_E_LAUNCH; }
        if (out_setup && hipMemcpyAsync(out_setup + (size_t)f0 * SK_MAX_REC * SK_REC, recs, (size_t)c * SK_MAX_REC * SK_REC * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) {
            cleanup();
            return IDF_E_LAUNCH;
        }
        if (stage_ms) {
            if (hipStreamSynchronize(s) != hipSuccess) { cleanup(); return IDF_E_LAUNCH; }
            for (int i = 0; i < 2; ++i) {
                float t = 0.f;
                (void)hipEventElapsedTime(&t, ev[i], ev[i + 1]);
                ms[i] += t;
            }
        }
    }
    cleanup();
    int32_t host_hdr = 0;
    if (hipMemcpyAsync(&host_hdr, hdr, 4, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return IDF_E_LAUNCH;
    if (dropped) *dropped = host_hdr;
    if (stage_ms)
        for (int i = 0; i < 2; ++i) stage_ms[i] = ms[i];
    return IDF_OK;
}

extern "C" int interdiff_skeleton_raster_records(const int32_t *recs, int32_t count, int64_t n_frames, int32_t H, int32_t W, uint8_t *out_rgb, void *stream) {
    if (!recs || !out_rgb || !sk_aligned4(recs) || count < 0 || count > SK_MAX_REC || n_frames < 1 || n_frames > 0xFFFF) return IDF_E_INVAL;
    if (H < 1 || W < 1 || H > IDF_RENDER_MAX_DIM || W > IDF_RENDER_MAX_DIM) return IDF_E_INVAL;
    const int tiles_x = (int)idf_cdiv(W, SK_TILE), tiles_y = (int)idf_cdiv(H, SK_TILE);
    hipLaunchKernelGGL(sk_raster_kernel, dim3((unsigned)(tiles_x * tiles_y), (unsigned)n_frames), dim3(SK_RASTER_THR), 0, idf_stream(stream), recs, count, H, W,
                       tiles_x, (int64_t)0, out_rgb);
    IDF_CHECK_LAUNCH();
    return IDF_OK;
}

extern "C" int interdiff_debug_skeleton_setup(const idf_skel_view *view, const float *body, const float *obj, const float *body_gt, const float *obj_gt,
                                              const int32_t *wires, int32_t n_wires, int32_t T, int32_t T_gt, int32_t t, int32_t *rec, int32_t *count,
                                              int32_t *dropped) {
    const int rc = sk_check_view(view, n_wires, T, T_gt, body_gt, obj_gt);
    if (rc != IDF_OK) return rc;
    if (!body || !obj || !rec || !count || !dropped || t < 0 || t >= T || (n_wires > 0 && !wires)) return IDF_E_INVAL;
    static thread_local SkFrame f;
    SkArgs a{body, obj, body_gt, obj_gt, wires, n_wires, T, T_gt, t};
    for (int l = 0; l < SK_LANES; ++l) {
        for (int k = 0; k < SK_REC; ++k) f.rec[l][k] = 0;
        f.drop[l] = 0;
    }
    for (int l = 0; l < SK_LANES; ++l) sk_phase_load(f, l, *view, a);
    for (int l = 0; l < SK_LANES; ++l) sk_phase_limits(f, l);
    for (int l = 0; l < SK_LANES; ++l) sk_phase_project(f, l, *view);
    if (view->style == IDF_SKEL_PLAIN)
        for (int l = 0; l < SK_LANES; ++l) sk_phase_groups(f, l);
    for (int l = 0; l < SK_LANES; ++l) sk_phase_emit(f, l, *view, a);
    int nd = 0;
    for (int l = 0; l < SK_LANES; ++l) nd += f.drop[l];
    for (int i = 0; i < SK_MAX_REC * SK_REC; ++i) rec[i] = (&f.rec[0][0])[i];
    *count = sk_count(*view, n_wires);
    *dropped = nd;
    return IDF_OK;
}

extern "C" int interdiff_debug_skeleton_pixel(const int32_t *rec, int32_t n_rec, const int32_t *ij, int32_t *out, int32_t n) {
    if (!rec || !ij || !out || n < 0 || n_rec < 0 || n_rec > SK_MAX_REC) return IDF_E_INVAL;
    for (int q = 0; q < n; ++q) {
        int32_t acc[3] = {255 << 8, 255 << 8, 255 << 8};
        for (int k = 0; k < n_rec; ++k) {
            const SkPrim p = sk_load(rec + (size_t)SK_REC * k);
            if (p.kind == 0) continue;
            const int c = sk_samples(p, ij[2 * q], ij[2 * q + 1]);
            if (c) sk_blend(acc, p, c);
        }
        for (int k = 0; k < 3; ++k) out[3 * q + k] = (acc[k] + 128) >> 8;
    }
    return IDF_OK;
}
