// Tiled software rasteriser for the clips the package produces (interdiff/render/mesh_viz.py: visualize_body_obj, restated without pyrender).
// The contract of every stage -- record layout, 1/16-pixel grid, top-left fill rule, depth key, bit widths -- is the head comment of render.h.
//
// LAUNCH PLAN, per chunk of images (an image = one view of one frame; the chunk is what the workspace holds):
//   memset         tile counts, fill cursors, large-list lengths
//   rd_setup       one thread per (source triangle, image): pose / scene transform / shading per vertex (render.h rd_vertex), near-plane clip into the
//                  triangle's two slots, snap, quantise, write both setup records; then the BIN COUNT of its slots: a slot whose pixel box holds no
//                  pixel centre is not binned at all (most of a body's 1-2 pixel triangles at small sizes), one that touches <= RD_BIN_MAX tiles adds 1
//                  to each tile's count, a larger one goes on the image's LARGE LIST instead (the ground's screen-filling triangles: every tile reads
//                  that list, so nothing is stored per tile for them).  fp32 ends here.
//   rd_scan        one workgroup per image: exclusive scan of the tile counts.
//   rd_fill        one thread per (slot, image): the same decision again, slot ids into the tile lists.  A list has no capacity: the lists of an image
//                  hold <= RD_BIN_MAX entries per slot IN TOTAL, and a slot on more tiles than that is on the large list, which holds every slot if need be.
//                  The order inside a list comes from an integer atomic and never reaches the result (the depth key decides).
//   rd_tile        one workgroup (256 lanes) per (tile of 16 x 16 pixels, image).  LDS: 256 keys of 64 bits (2 KB) + a queue of 256 slot ids (1 KB) -- 3 KB
//                  per workgroup, occupancy is bounded by waves, not LDS.  The tile's list and the large list are walked 256 slots at a time, one slot
//                  per lane: a slot whose pixel box inside the tile is <= RD_SMALL pixels is rasterised by its lane (integer LDS min per covered pixel);
//                  a larger one is queued, and the whole workgroup then takes the queued slots one after the other, one pixel per lane, the running
//                  minimum in a register.  So a one-pixel triangle never gets a wave and a screen-filling one never sits on one lane.
//                  The resolve is the tail of the same kernel (the keys are already in LDS): winner's weights -> RGB8, id, depth.
// Integer atomics only; no cooperative launch, no spin.
#include "common.h"
#include "render.h"
#include <algorithm>

namespace {

constexpr int RD_THR = 256;
constexpr int RD_BIN_MAX = 16;       // a slot on more tiles than this goes on the image's large list
constexpr int RD_SMALL = 16;         // pixel-box area (inside the tile) up to which one lane rasterises the slot
constexpr unsigned long long RD_EMPTY = ~0ull;
static_assert(RD_TILE * RD_TILE == RD_THR, "one lane per pixel of a tile");

struct RdMeshTable {
    idf_render_mesh m[IDF_RENDER_MAX_MESHES];
    int32_t face_base[IDF_RENDER_MAX_MESHES + 1];
    int32_t n;
};

struct RdLayout {          // offsets into the workspace for a chunk of c images
    size_t hdr, zero, zero_bytes, counts, cursors, nlarge, offsets, rec, large, entries, total;
};

RdLayout rd_layout(int64_t c, int64_t S, int64_t nt) {
    RdLayout L;
    size_t o = 0;
    L.hdr = o; o += 256;
    L.zero = o;
    L.counts = o; o += idf_align((size_t)c * nt * 4);
    L.cursors = o; o += idf_align((size_t)c * nt * 4);
    L.nlarge = o; o += idf_align((size_t)c * 4);
    L.zero_bytes = o - L.zero;
    L.offsets = o; o += idf_align((size_t)c * nt * 4);
    L.rec = o; o += idf_align((size_t)c * S * RD_REC * 4);
    L.large = o; o += idf_align((size_t)c * S * 4);
    L.entries = o; o += idf_align((size_t)c * S * RD_BIN_MAX * 4);
    L.total = o;
    return L;
}

__global__ __launch_bounds__(RD_THR) void rd_check_faces_kernel(const int32_t *__restrict__ faces, int64_t n, int V, int32_t *__restrict__ bad) {
    const int64_t i = (int64_t)blockIdx.x * RD_THR + threadIdx.x;
    if (i < n && (faces[i] < 0 || faces[i] >= V)) atomicOr(bad, 1);
}

// tiles [tx0, tx1] x [ty0, ty1] the slot's pixel box touches; false: not binned
__device__ __forceinline__ bool rd_tile_box(const int32_t *rec, int H, int W, int &tx0, int &tx1, int &ty0, int &ty1) {
    int i0, i1, j0, j1;
    if (!rd_pixel_box(rec, H, W, i0, i1, j0, j1)) return false;
    tx0 = i0 / RD_TILE; tx1 = i1 / RD_TILE; ty0 = j0 / RD_TILE; ty1 = j1 / RD_TILE;
    return true;
}

__global__ __launch_bounds__(RD_THR) void rd_setup_kernel(idf_render_scene sc, RdMeshTable tab, int64_t img0, int views, int H, int W, int tiles_x,
                                                          int nt, int32_t *__restrict__ recs, int32_t *__restrict__ counts,
                                                          int32_t *__restrict__ nlarge, int32_t *__restrict__ large, int32_t *__restrict__ dropped) {
    const int tri = blockIdx.x * RD_THR + threadIdx.x;
    const int Ft = tab.face_base[tab.n];
    if (tri >= Ft) return;
    const int li = blockIdx.y;                       // image inside the chunk
    const int64_t img = img0 + li, n = img / views;
    const int view = (int)(img % views);
    int mi = 0;
    while (tri >= tab.face_base[mi + 1]) ++mi;
    const idf_render_mesh &m = tab.m[mi];
    const int32_t *f = m.faces + (size_t)(tri - tab.face_base[mi]) * 3;
    const size_t fr = m.frames > 1 ? (size_t)n * m.V * 3 : 0;
    const bool scene_space = (m.flags & IDF_RMESH_SCENE_SPACE) != 0, vrgb = (m.flags & IDF_RMESH_VERTEX_RGB) != 0;
    RdVert v[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int vi = f[k];
        const float *p = m.verts + fr + (size_t)vi * 3, *q = m.normals + fr + (size_t)vi * 3;
        const float *c = vrgb ? m.rgb + (size_t)vi * 3 : m.rgb + (size_t)n * 3;
        float px = p[0], py = p[1], pz = p[2], nx = q[0], ny = q[1], nz = q[2];
        if (m.R) {
#pragma clang fp contract(off)
            const float *R = m.R + (size_t)n * 9, *t = m.t + (size_t)n * 3;
            const float ox = ((R[0] * px + R[1] * py) + R[2] * pz) + t[0], oy = ((R[3] * px + R[4] * py) + R[5] * pz) + t[1],
                        oz = ((R[6] * px + R[7] * py) + R[8] * pz) + t[2];
            const float mx = (R[0] * nx + R[1] * ny) + R[2] * nz, my = (R[3] * nx + R[4] * ny) + R[5] * nz, mz = (R[6] * nx + R[7] * ny) + R[8] * nz;
            px = ox; py = oy; pz = oz; nx = mx; ny = my; nz = mz;
        }
        v[k] = rd_vertex(sc, view, scene_space, px, py, pz, nx, ny, nz, c[0], c[1], c[2]);
    }
    int32_t r0[RD_REC], r1[RD_REC];
    const int nd = rd_setup_triangle(sc, H, W, v, r0, r1);
    if (nd) atomicAdd(dropped, nd);
    int32_t *out = recs + ((size_t)li * Ft * 2 + (size_t)tri * 2) * RD_REC;
#pragma unroll
    for (int i = 0; i < RD_REC; ++i) { out[i] = r0[i]; out[RD_REC + i] = r1[i]; }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        int tx0, tx1, ty0, ty1;
        if (!rd_tile_box(s ? r1 : r0, H, W, tx0, tx1, ty0, ty1)) continue;
        if ((tx1 - tx0 + 1) * (ty1 - ty0 + 1) > RD_BIN_MAX) {
            const int pos = atomicAdd(nlarge + li, 1);
            large[(size_t)li * Ft * 2 + pos] = 2 * tri + s;
        } else {
            for (int ty = ty0; ty <= ty1; ++ty)
                for (int tx = tx0; tx <= tx1; ++tx) atomicAdd(counts + (size_t)li * nt + ty * tiles_x + tx, 1);
        }
    }
}

// exclusive scan of one image's tile counts; one workgroup per image
__global__ __launch_bounds__(RD_THR) void rd_scan_kernel(const int32_t *__restrict__ counts, int nt, int32_t *__restrict__ offsets) {
    __shared__ int32_t part[RD_THR];
    const int li = blockIdx.x, tid = threadIdx.x;
    const int per = (nt + RD_THR - 1) / RD_THR, a = min(tid * per, nt), b = min(a + per, nt);
    const int32_t *c = counts + (size_t)li * nt;
    int32_t s = 0;
    for (int i = a; i < b; ++i) s += c[i];
    part[tid] = s;
    __syncthreads();
    if (tid == 0) {
        int32_t run = 0;
        for (int i = 0; i < RD_THR; ++i) { const int32_t x = part[i]; part[i] = run; run += x; }
    }
    __syncthreads();
    int32_t run = part[tid];
    for (int i = a; i < b; ++i) { offsets[(size_t)li * nt + i] = run; run += c[i]; }
}

__global__ __launch_bounds__(RD_THR) void rd_fill_kernel(const int32_t *__restrict__ recs, int S, int H, int W, int tiles_x, int nt,
                                                         const int32_t *__restrict__ offsets, int32_t *__restrict__ cursors,
                                                         int32_t *__restrict__ entries) {
    const int slot = blockIdx.x * RD_THR + threadIdx.x, li = blockIdx.y;
    if (slot >= S) return;
    int tx0, tx1, ty0, ty1;
    if (!rd_tile_box(recs + ((size_t)li * S + slot) * RD_REC, H, W, tx0, tx1, ty0, ty1)) return;
    if ((tx1 - tx0 + 1) * (ty1 - ty0 + 1) > RD_BIN_MAX) return;
    for (int ty = ty0; ty <= ty1; ++ty)
        for (int tx = tx0; tx <= tx1; ++tx) {
            const size_t t = (size_t)li * nt + ty * tiles_x + tx;
            const int pos = offsets[t] + atomicAdd(cursors + t, 1);
            entries[(size_t)li * S * RD_BIN_MAX + pos] = slot;
        }
}

__global__ __launch_bounds__(RD_THR) void rd_tile_kernel(const int32_t *__restrict__ recs, int S, int H, int W, int tiles_x, int nt,
                                                         const int32_t *__restrict__ counts, const int32_t *__restrict__ offsets,
                                                         const int32_t *__restrict__ entries, const int32_t *__restrict__ nlarge,
                                                         const int32_t *__restrict__ large, int64_t img0, uchar4 bg, uint8_t *__restrict__ out_rgb,
                                                         int32_t *__restrict__ out_id, int32_t *__restrict__ out_depth) {
    __shared__ unsigned long long key[RD_THR];
    __shared__ int32_t queue[RD_THR];
    __shared__ int32_t qn;
    const int tid = threadIdx.x, tile = blockIdx.x, li = blockIdx.y;
    const int tx = tile % tiles_x, ty = tile / tiles_x;
    const int x0 = tx * RD_TILE, y0 = ty * RD_TILE, x1 = min(x0 + RD_TILE, W) - 1, y1 = min(y0 + RD_TILE, H) - 1;      // the tile's pixels, inclusive
    const int pi = x0 + (tid & (RD_TILE - 1)), pj = y0 + tid / RD_TILE;
    const bool live = pi < W && pj < H;
    const int32_t *rimg = recs + (size_t)li * S * RD_REC;
    const int32_t *ent = entries + (size_t)li * S * RD_BIN_MAX + offsets[(size_t)li * nt + tile];
    const int32_t *lg = large + (size_t)li * S;
    const int cnt = counts[(size_t)li * nt + tile], total = cnt + nlarge[li];
    key[tid] = RD_EMPTY;
    unsigned long long best = RD_EMPTY;
    for (int base = 0; base < total; base += RD_THR) {
        if (tid == 0) qn = 0;
        __syncthreads();
        const int idx = base + tid;
        if (idx < total) {
            const int slot = idx < cnt ? ent[idx] : lg[idx - cnt];
            const int32_t *rec = rimg + (size_t)slot * RD_REC;
            int i0, i1, j0, j1;
            if (rd_pixel_box(rec, H, W, i0, i1, j0, j1)) {
                i0 = max(i0, x0); i1 = min(i1, x1); j0 = max(j0, y0); j1 = min(j1, y1);
                if (i0 <= i1 && j0 <= j1) {
                    if ((i1 - i0 + 1) * (j1 - j0 + 1) <= RD_SMALL) {
                        RdTri t;
                        if (rd_load(rec, t))
                            for (int j = j0; j <= j1; ++j)
                                for (int i = i0; i <= i1; ++i) {
                                    int64_t w[3];
                                    if (rd_cover(t, i, j, w))
                                        atomicMin(&key[(j - y0) * RD_TILE + (i - x0)],
                                                  ((unsigned long long)(uint32_t)rd_depth(t, w) << 32) | (uint32_t)slot);
                                }
                    } else {
                        queue[atomicAdd(&qn, 1)] = slot;
                    }
                }
            }
        }
        __syncthreads();
        const int nq = qn;
        for (int q = 0; q < nq; ++q) {
            const int slot = queue[q];
            RdTri t;
            int64_t w[3];
            if (live && rd_load(rimg + (size_t)slot * RD_REC, t) && rd_cover(t, pi, pj, w)) {
                const unsigned long long k = ((unsigned long long)(uint32_t)rd_depth(t, w) << 32) | (uint32_t)slot;
                best = k < best ? k : best;
            }
        }
        __syncthreads();
    }
    __syncthreads();
    if (!live) return;
    unsigned long long k = key[tid];
    k = best < k ? best : k;
    // resolve: a pure integer function of the winner's record
    const size_t pix = ((size_t)(img0 + li) * H + pj) * W + pi;
    uint8_t r = bg.x, g = bg.y, b = bg.z;
    int32_t id = -1, depth = 0x7fffffff;
    if (k != RD_EMPTY) {
        id = (int32_t)(uint32_t)(k & 0xffffffffull);
        depth = (int32_t)(k >> 32);
        RdTri t;
        int64_t w[3];
        rd_load(rimg + (size_t)id * RD_REC, t);
        rd_cover(t, pi, pj, w);
        r = (uint8_t)rd_colour(t, w, 0); g = (uint8_t)rd_colour(t, w, 1); b = (uint8_t)rd_colour(t, w, 2);
    }
    out_rgb[pix * 3] = r; out_rgb[pix * 3 + 1] = g; out_rgb[pix * 3 + 2] = b;
    if (out_id) out_id[pix] = id;
    if (out_depth) out_depth[pix] = depth;
}

bool rd_aligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

int rd_check_args(const idf_render_scene *scene, const idf_render_mesh *meshes, int32_t n_meshes, int64_t N, int32_t views, int32_t H, int32_t W,
                  int64_t *Ft) {
    if (!scene || !meshes || n_meshes < 1 || n_meshes > IDF_RENDER_MAX_MESHES) return IDF_E_INVAL;
    if (N <= 0 || views < 1 || views > 4 || H < 1 || W < 1 || H > IDF_RENDER_MAX_DIM || W > IDF_RENDER_MAX_DIM) return IDF_E_INVAL;
    if (N > (1 << 24)) return IDF_E_INVAL;                   // image indices and pixel offsets stay far inside int64
    if (!(scene->znear > 0.f) || !(scene->focal > 0.f)) return IDF_E_INVAL;
    int64_t F = 0;
    for (int i = 0; i < n_meshes; ++i) {
        const idf_render_mesh &m = meshes[i];
        if (!m.verts || !m.normals || !m.faces || !m.rgb) return IDF_E_INVAL;
        if (!rd_aligned4(m.verts) || !rd_aligned4(m.normals) || !rd_aligned4(m.faces) || !rd_aligned4(m.rgb) || !rd_aligned4(m.R) || !rd_aligned4(m.t))
            return IDF_E_INVAL;
        if (m.V <= 0 || m.F <= 0 || (m.frames != 1 && m.frames != N)) return IDF_E_INVAL;
        if ((m.R == nullptr) != (m.t == nullptr)) return IDF_E_INVAL;
        F += m.F;
    }
    if (F * 2 > 0x3FFFFFF) return IDF_E_INVAL;               // slot ids, and slots * RD_BIN_MAX entries, stay inside int32
    *Ft = F;
    return IDF_OK;
}

}  // namespace

extern "C" size_t interdiff_render_frames_workspace_bytes(int64_t n_images, int64_t n_triangles, int32_t H, int32_t W) {
    if (n_images <= 0 || n_triangles <= 0 || H < 1 || W < 1 || H > IDF_RENDER_MAX_DIM || W > IDF_RENDER_MAX_DIM) return 0;
    const int64_t nt = idf_cdiv(W, RD_TILE) * idf_cdiv(H, RD_TILE);
    return rd_layout(n_images, 2 * n_triangles, nt).total;
}

extern "C" int interdiff_render_frames(const idf_render_scene *scene, const idf_render_mesh *meshes, int32_t n_meshes, int64_t N, int32_t views,
                                       int32_t H, int32_t W, uint8_t *out_rgb, int32_t *out_id, int32_t *out_depth, int32_t *out_setup,
                                       int64_t *dropped, float *stage_ms, void *ws, size_t ws_bytes, void *stream) {
    int64_t Ft = 0;
    const int rc = rd_check_args(scene, meshes, n_meshes, N, views, H, W, &Ft);
    if (rc != IDF_OK) return rc;
    if (!out_rgb || !ws || !rd_aligned4(out_id) || !rd_aligned4(out_depth) || !rd_aligned4(out_setup) || (reinterpret_cast<uintptr_t>(ws) & 255))
        return IDF_E_INVAL;
    const int64_t S = 2 * Ft, n_img = N * views;
    const int tiles_x = (int)idf_cdiv(W, RD_TILE), tiles_y = (int)idf_cdiv(H, RD_TILE), nt = tiles_x * tiles_y;
    if (ws_bytes < rd_layout(1, S, nt).total) return IDF_E_NOMEM;
    int64_t chunk = std::min<int64_t>(n_img, 0xFFFF);             // images ride on gridDim.y
    while (chunk > 1 && rd_layout(chunk, S, nt).total > ws_bytes) chunk = std::max<int64_t>(1, std::min(chunk - 1, chunk * (int64_t)ws_bytes / (int64_t)rd_layout(chunk, S, nt).total));
    const RdLayout L = rd_layout(chunk, S, nt);
    hipStream_t s = idf_stream(stream);
    char *w8 = static_cast<char *>(ws);
    int32_t *hdr = reinterpret_cast<int32_t *>(w8 + L.hdr);                 // [0] bad face index seen, [1] dropped slots
    if (hipMemsetAsync(hdr, 0, 256, s) != hipSuccess) return IDF_E_LAUNCH;
    RdMeshTable tab;
    tab.n = n_meshes;
    tab.face_base[0] = 0;
    for (int i = 0; i < n_meshes; ++i) {
        tab.m[i] = meshes[i];
        tab.face_base[i + 1] = tab.face_base[i] + meshes[i].F;
        const int64_t ne = (int64_t)meshes[i].F * 3;
        hipLaunchKernelGGL(rd_check_faces_kernel, dim3((unsigned)idf_cdiv(ne, RD_THR)), dim3(RD_THR), 0, s, meshes[i].faces, ne, meshes[i].V, hdr);
        IDF_CHECK_LAUNCH();
    }
    int32_t host_hdr[2] = {0, 0};
    if (hipMemcpyAsync(host_hdr, hdr, 8, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return IDF_E_LAUNCH;
    if (host_hdr[0]) return IDF_E_INVAL;

    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    float ms[3] = {0.f, 0.f, 0.f};
    auto mark = [&](int i) { if (stage_ms) (void)hipEventRecord(ev[i], s); };
    auto cleanup = [&]() { for (auto &e : ev) if (e) { (void)hipEventDestroy(e); e = nullptr; } };
    if (stage_ms)
        for (auto &e : ev)
            if (hipEventCreate(&e) != hipSuccess) { e = nullptr; cleanup(); return IDF_E_LAUNCH; }
    int32_t *counts = reinterpret_cast<int32_t *>(w8 + L.counts), *cursors = reinterpret_cast<int32_t *>(w8 + L.cursors);
    int32_t *nlarge = reinterpret_cast<int32_t *>(w8 + L.nlarge), *offsets = reinterpret_cast<int32_t *>(w8 + L.offsets);
    int32_t *recs = reinterpret_cast<int32_t *>(w8 + L.rec), *large = reinterpret_cast<int32_t *>(w8 + L.large);
    int32_t *entries = reinterpret_cast<int32_t *>(w8 + L.entries);
    const uchar4 bg = make_uchar4((unsigned char)rintf(fminf(fmaxf(scene->bg[0], 0.f), 1.f) * 255.f), (unsigned char)rintf(fminf(fmaxf(scene->bg[1], 0.f), 1.f) * 255.f),
                                  (unsigned char)rintf(fminf(fmaxf(scene->bg[2], 0.f), 1.f) * 255.f), 255);
    for (int64_t img0 = 0; img0 < n_img; img0 += chunk) {
        const unsigned c = (unsigned)std::min<int64_t>(chunk, n_img - img0);
        mark(0);
        if (hipMemsetAsync(w8 + L.zero, 0, L.zero_bytes, s) != hipSuccess) { cleanup(); return IDF_E_LAUNCH; }
        hipLaunchKernelGGL(rd_setup_kernel, dim3((unsigned)idf_cdiv(Ft, RD_THR), c), dim3(RD_THR), 0, s, *scene, tab, img0, views, H, W, tiles_x, nt, recs,
                           counts, nlarge, large, hdr + 1);
        mark(1);
        hipLaunchKernelGGL(rd_scan_kernel, dim3(c), dim3(RD_THR), 0, s, counts, nt, offsets);
        hipLaunchKernelGGL(rd_fill_kernel, dim3((unsigned)idf_cdiv(S, RD_THR), c), dim3(RD_THR), 0, s, recs, (int)S, H, W, tiles_x, nt, offsets, cursors,
                           entries);
        mark(2);
        hipLaunchKernelGGL(rd_tile_kernel, dim3((unsigned)nt, c), dim3(RD_THR), 0, s, recs, (int)S, H, W, tiles_x, nt, counts, offsets, entries, nlarge,
                           large, img0, bg, out_rgb, out_id, out_depth);
        mark(3);
        if (hipGetLastError() != hipSuccess) { cleanup(); return IDF_E_LAUNCH; }
        if (out_setup && hipMemcpyAsync(out_setup + (size_t)img0 * S * RD_REC, recs, (size_t)c * S * RD_REC * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) {
            cleanup();
            return IDF_E_LAUNCH;
        }
        if (stage_ms) {
            if (hipStreamSynchronize(s) != hipSuccess) { cleanup(); return IDF_E_LAUNCH; }
            for (int i = 0; i < 3; ++i) {
                float t = 0.f;
                (void)hipEventElapsedTime(&t, ev[i], ev[i + 1]);
                ms[i] += t;
            }
        }
    }
    cleanup();
    if (hipMemcpyAsync(host_hdr, hdr, 8, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return IDF_E_LAUNCH;
    if (dropped) *dropped = host_hdr[1];
    if (stage_ms)
        for (int i = 0; i < 3; ++i) stage_ms[i] = ms[i];
    return IDF_OK;
}

extern "C" int interdiff_debug_render_setup_vertex(const idf_render_scene *scene, int32_t view, int32_t scene_space, int32_t H, int32_t W,
                                                   const float *pos, const float *nrm, const float *rgb, float *out_f, int32_t *out_i, int32_t n) {
    if (!scene || !pos || !nrm || !rgb || !out_f || !out_i || n < 0 || H < 1 || W < 1) return IDF_E_INVAL;
    for (int i = 0; i < n; ++i) {
        const float *p = pos + 3 * i, *q = nrm + 3 * i, *c = rgb + 3 * i;
        const RdVert v = rd_vertex(*scene, view, scene_space != 0, p[0], p[1], p[2], q[0], q[1], q[2], c[0], c[1], c[2]);
        float *f = out_f + 6 * i;
        f[0] = v.xc; f[1] = v.yc; f[2] = v.d; f[3] = v.r; f[4] = v.g; f[5] = v.b;
        int32_t *o = out_i + 7 * i;
        for (int k = 0; k < 7; ++k) o[k] = 0;
        if (v.d >= scene->znear) {
            const RdSnap sn = rd_project(*scene, H, W, v);
            const float g = (float)RD_GUARD;
            o[0] = 1;
            o[1] = fabsf(sn.X) <= g ? (int32_t)sn.X : (sn.X > 0.f ? RD_GUARD + 1 : -RD_GUARD - 1);      // outside the band: pinned just past it (the kernel drops the slot)
            o[2] = fabsf(sn.Y) <= g ? (int32_t)sn.Y : (sn.Y > 0.f ? RD_GUARD + 1 : -RD_GUARD - 1);
            o[3] = sn.Z; o[4] = sn.R; o[5] = sn.G; o[6] = sn.B;
        }
    }
    return IDF_OK;
}

extern "C" int interdiff_debug_render_pixel(const int32_t *rec, const int32_t *ij, int32_t *out, int32_t n) {
    if (!rec || !ij || !out || n < 0) return IDF_E_INVAL;
    for (int i = 0; i < n; ++i) {
        RdTri t;
        int64_t w[3];
        int32_t *o = out + 5 * i;
        for (int k = 0; k < 5; ++k) o[k] = 0;
        if (rd_load(rec + (size_t)RD_REC * i, t) && rd_cover(t, ij[2 * i], ij[2 * i + 1], w)) {
            o[0] = 1; o[1] = rd_depth(t, w);
            for (int k = 0; k < 3; ++k) o[2 + k] = rd_colour(t, w, k);
        }
    }
    return IDF_OK;
}
