// Contact-label generation (interdiff/data/prepare_behave.py:32-52, get_contact_labels): per frame the signed distance of P object points
// to the body's triangle mesh, the object points closer than `thres`, and the body vertices within `thres` of one of those.  The reference calls
// igl.signed_distance (winding-number sign, 3-D); neither igl nor a stand-in exists here, so the contract is the restatement of SURVEY.md B.6:
//   d[p] = min over faces of the exact point-triangle distance (a zero-area face counts through its edges and corners; never a NaN)
//   w[p] = (1 / 4 pi) * sum over faces of the signed solid angle, van Oosterom-Strackee atan2 form (a zero-area face contributes 0)
//   S[p] = (1 - 2 w[p]) d[p];   obj_label[p] = S[p] < thres;   human_label[v] = exists p: obj_label[p] and |p - v| < thres
// fp32 throughout, no MFMA, no float atomics, no reduction across workgroups: two calls give the same bits.
//
// DISTANCE + WINDING PASS (ct_points_kernel): one workgroup per (frame, tile of 256 points), one point per lane, posed in registers
// (p R^T + t).  The faces stream through LDS in chunks of 256: thread j of the workgroup gathers the three corners of face c0 + j and writes one
// record of five float4 (corner a, edges ab / ac, normal ab x ac, the dot products and reciprocals the closest-point test reuses); the face loop
// then reads every record at a wave-uniform address (LDS broadcast, no bank conflicts).  ONE face loop does both sums: the record is shared, the
// solid angle needs every face, and the lanes that could skip it (d < thres) are a minority that is not wave-coherent -- so w is computed for every
// point and signed_dist is S everywhere.  The distance half of a chunk is skipped by a lane whose squared distance to the chunk's bounding box
// (ct_boxes_kernel, one small launch in front) is >= its running minimum: a box distance is a lower bound of every face distance in it, so the
// minimum is preserved exactly, whatever the face order.  The order only decides how much is skipped (the Python side sorts faces along a
// Morton curve of the centroids once per mesh).
// The solid angles are summed per chunk and the chunk sums into the total: <= 256 adds of small terms, then <= F / 256 adds -- the rounding
// of the sum stays near 1e-6 in w instead of growing with F.
// BODY-LABEL PASS (ct_body_kernel): one workgroup per (frame, 256 vertices).  The frame's labelled points are posed again and compacted into LDS
// 2048 at a time (24 KB; the slot order comes from an integer LDS counter and does not matter: the result is an OR), one vertex per lane takes the
// minimum squared distance.  No early exit: a labelled set is tens to hundreds of points and lanes of a wave would leave the loop together only
// when all 64 vertices are hits.
#include "common.h"
#include <float.h>
#include <math.h>

namespace {

constexpr int CT_THR = 256;          // lanes = points (or vertices) per workgroup
constexpr int CT_FC = 256;           // faces per LDS chunk: one record per thread
constexpr int CT_PC = 2048;          // labelled points per LDS round of the body pass
constexpr float CT_SIN2_MIN = 1e-10f;      // |ab x ac|^2 <= this * |ab|^2 |ac|^2  (sin <= 1e-5): the face is treated as zero-area

// r0 = a | ab.ab,  r1 = ab | ab.ac,  r2 = ac | ac.ac,  r3 = n = ab x ac | 1 / n.n (0: zero-area),  r4 = 1 / ab.ab, 1 / ac.ac, 1 / bc.bc (0 where the edge has no length), unused
struct CtRec { float4 r0, r1, r2, r3, r4; };

__host__ __device__ __forceinline__ float ct_dot(float ax, float ay, float az, float bx, float by, float bz) { return ax * bx + ay * by + az * bz; }
__host__ __device__ __forceinline__ float ct_clamp01(float x) { return fminf(fmaxf(x, 0.f), 1.f); }

__host__ __device__ __forceinline__ CtRec ct_make_rec(float ax, float ay, float az, float bx, float by, float bz, float cx, float cy, float cz) {
    CtRec r;
    const float ux = bx - ax, uy = by - ay, uz = bz - az, vx = cx - ax, vy = cy - ay, vz = cz - az;
    const float d00 = ct_dot(ux, uy, uz, ux, uy, uz), d01 = ct_dot(ux, uy, uz, vx, vy, vz), d11 = ct_dot(vx, vy, vz, vx, vy, vz);
    const float nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
    const float nn = ct_dot(nx, ny, nz, nx, ny, nz);
    const float wx = vx - ux, wy = vy - uy, wz = vz - uz, dbc = ct_dot(wx, wy, wz, wx, wy, wz);
    const bool flat = !(nn > CT_SIN2_MIN * d00 * d11);           // also catches NaN / zero edges
    r.r0 = make_float4(ax, ay, az, d00);
    r.r1 = make_float4(ux, uy, uz, d01);
    r.r2 = make_float4(vx, vy, vz, d11);
    r.r3 = make_float4(nx, ny, nz, flat ? 0.f : 1.f / nn);
    r.r4 = make_float4(d00 > 0.f ? 1.f / d00 : 0.f, d11 > 0.f ? 1.f / d11 : 0.f, dbc > 0.f ? 1.f / dbc : 0.f, 0.f);
    return r;
}

// squared distance of x (relative to the segment's origin) to the segment {s e : 0 <= s <= 1}; inv = 1 / e.e or 0
__host__ __device__ __forceinline__ float ct_seg2(float xx, float xy, float xz, float ex, float ey, float ez, float inv) {
    const float s = ct_clamp01(ct_dot(xx, xy, xz, ex, ey, ez) * inv);
    const float rx = xx - s * ex, ry = xy - s * ey, rz = xz - s * ez;
    return ct_dot(rx, ry, rz, rx, ry, rz);
}

// One (point, face) pair: adds the face's signed solid angle / 2 to `half_omega`, and, when want_d, folds the squared distance into `best`.
// Closest point by the Voronoi regions of the triangle (Ericson, Real-Time Collision Detection 5.1.5) on the record's shared dot products;
// inside the face region the distance is the plane distance (p - a).n / |n|, which needs no barycentric division.
__host__ __device__ __forceinline__ void ct_pair(const CtRec &r, float px, float py, float pz, bool want_d, float &best, float &half_omega) {
    const float apx = px - r.r0.x, apy = py - r.r0.y, apz = pz - r.r0.z;
    const float pn = ct_dot(apx, apy, apz, r.r3.x, r.r3.y, r.r3.z);
    const bool flat = r.r3.w == 0.f;
    if (!flat) {
        // corners seen from p: A = a - p, B = b - p, C = c - p;  tan(omega / 2) = A.(B x C) / (|A||B||C| + A.B |C| + B.C |A| + C.A |B|),  A.(B x C) = A.n
        const float bx = r.r1.x - apx, by = r.r1.y - apy, bz = r.r1.z - apz, cx = r.r2.x - apx, cy = r.r2.y - apy, cz = r.r2.z - apz;
        const float la = sqrtf(ct_dot(apx, apy, apz, apx, apy, apz)), lb = sqrtf(ct_dot(bx, by, bz, bx, by, bz)), lc = sqrtf(ct_dot(cx, cy, cz, cx, cy, cz));
        const float ab = -ct_dot(apx, apy, apz, bx, by, bz), ac = -ct_dot(apx, apy, apz, cx, cy, cz), bc = ct_dot(bx, by, bz, cx, cy, cz);
        const float den = la * lb * lc + ab * lc + bc * la + ac * lb;
        half_omega += atan2f(-pn, den);
    }
    if (!want_d) return;
    const float d00 = r.r0.w, d01 = r.r1.w, d11 = r.r2.w;
    const float d1 = ct_dot(apx, apy, apz, r.r1.x, r.r1.y, r.r1.z), d2 = ct_dot(apx, apy, apz, r.r2.x, r.r2.y, r.r2.z);
    float dd;
    if (flat) {
        // zero-area: the three edges as segments (an edge without length is its end point)
        const float bpx = apx - r.r1.x, bpy = apy - r.r1.y, bpz = apz - r.r1.z;
        const float e0 = ct_seg2(apx, apy, apz, r.r1.x, r.r1.y, r.r1.z, r.r4.x), e1 = ct_seg2(apx, apy, apz, r.r2.x, r.r2.y, r.r2.z, r.r4.y);
        const float e2 = ct_seg2(bpx, bpy, bpz, r.r2.x - r.r1.x, r.r2.y - r.r1.y, r.r2.z - r.r1.z, r.r4.z);
        dd = fminf(e0, fminf(e1, e2));
    } else {
        const float d3 = d1 - d00, d4 = d2 - d01, d5 = d1 - d01, d6 = d2 - d11;      // ab.bp, ac.bp, ab.cp, ac.cp
        const float va = d3 * d6 - d5 * d4, vb = d5 * d2 - d1 * d6, vc = d1 * d4 - d3 * d2;
        float s = 0.f, t = 0.f;                                                     // closest point a + s ab + t ac
        bool face = false;
        if (d1 <= 0.f && d2 <= 0.f) { }
        else if (d3 >= 0.f && d4 <= d3) s = 1.f;
        else if (d6 >= 0.f && d5 <= d6) t = 1.f;
        else if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) s = ct_clamp01(d1 * r.r4.x);
        else if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) t = ct_clamp01(d2 * r.r4.y);
        else if (va <= 0.f && d4 - d3 >= 0.f && d5 - d6 >= 0.f) { t = ct_clamp01((d4 - d3) * r.r4.z); s = 1.f - t; }
        else face = true;
        if (face) dd = pn * pn * r.r3.w;
        else {
            const float rx = apx - s * r.r1.x - t * r.r2.x, ry = apy - s * r.r1.y - t * r.r2.y, rz = apz - s * r.r1.z - t * r.r2.z;
            dd = ct_dot(rx, ry, rz, rx, ry, rz);
        }
    }
    best = fminf(best, dd);
}

// p' = p R^T + t, products and sums rounded one by one, left to right (what an elementwise restatement computes); RT = R row-major | t
__device__ __forceinline__ float3 ct_pose(const float *RT, bool posed, float px, float py, float pz) {
#pragma clang fp contract(off)
    if (!posed) return make_float3(px, py, pz);
    float3 o;
    o.x = ((RT[0] * px + RT[1] * py) + RT[2] * pz) + RT[9];
    o.y = ((RT[3] * px + RT[4] * py) + RT[5] * pz) + RT[10];
    o.z = ((RT[6] * px + RT[7] * py) + RT[8] * pz) + RT[11];
    return o;
}

__device__ __forceinline__ void ct_load_pose(float *RT, const float *objR, const float *objT, int64_t n) {
    if (!objR) return;
#pragma unroll
    for (int i = 0; i < 9; ++i) RT[i] = objR[n * 9 + i];
#pragma unroll
    for (int i = 0; i < 3; ++i) RT[9 + i] = objT[n * 3 + i];
}

// face index -> inside [0, V): the caller validates its mesh once (interdiff_amd/contact_labels.py); the clamp only keeps a bad index inside the frame
__device__ __forceinline__ int ct_vidx(int i, int V) { return min(max(i, 0), V - 1); }

// bounding box of every chunk of 256 faces of every frame: boxes [N][n_chunks][8] = min xyz, max xyz, 2 unused.  grid = N * n_chunks.
__global__ __launch_bounds__(CT_THR) void ct_boxes_kernel(const float *__restrict__ verts, int V, const int32_t *__restrict__ faces, int F, int n_chunks,
                                                          float *__restrict__ boxes) {
    __shared__ float red[6][CT_THR / 64];
    const int64_t n = blockIdx.x / n_chunks;
    const int ch = blockIdx.x % n_chunks, f = ch * CT_FC + threadIdx.x;
    const float *v = verts + (size_t)n * V * 3;
    float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    if (f < F) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float *p = v + (size_t)ct_vidx(faces[(size_t)f * 3 + k], V) * 3;
#pragma unroll
            for (int a = 0; a < 3; ++a) { lo[a] = fminf(lo[a], p[a]); hi[a] = fmaxf(hi[a], p[a]); }
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            lo[a] = fminf(lo[a], __shfl_xor(lo[a], o));
            hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], o));
        }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0)
#pragma unroll
        for (int a = 0; a < 3; ++a) { red[a][wave] = lo[a]; red[3 + a][wave] = hi[a]; }
    __syncthreads();
    if (threadIdx.x < 6) {
        float x = red[threadIdx.x][0];
        for (int w = 1; w < CT_THR / 64; ++w) x = threadIdx.x < 3 ? fminf(x, red[threadIdx.x][w]) : fmaxf(x, red[threadIdx.x][w]);
        boxes[(size_t)blockIdx.x * 8 + threadIdx.x] = x;
    }
}

__global__ __launch_bounds__(CT_THR) void ct_points_kernel(const float *__restrict__ verts, int V, const int32_t *__restrict__ faces, int F,
                                                           const float *__restrict__ points, int P, int64_t pstride, const float *__restrict__ objR,
                                                           const float *__restrict__ objT, float thres, const float *__restrict__ boxes, int n_chunks,
                                                           int n_tiles, uint8_t *__restrict__ obj_label, float *__restrict__ signed_dist) {
    __shared__ float4 rec[5][CT_FC];
    const int64_t n = blockIdx.x / n_tiles;
    const int tid = threadIdx.x, i = (blockIdx.x % n_tiles) * CT_THR + tid;
    const float *v = verts + (size_t)n * V * 3;
    const float *box = boxes + (size_t)n * n_chunks * 8;
    float RT[12];
    ct_load_pose(RT, objR, objT, n);
    float3 p = make_float3(0.f, 0.f, 0.f);
    if (i < P) {
        const float *q = points + (size_t)n * pstride + (size_t)i * 3;
        p = ct_pose(RT, objR != nullptr, q[0], q[1], q[2]);
    }
    float best = FLT_MAX, half_omega = 0.f;
    for (int ch = 0; ch < n_chunks; ++ch) {
        const int c0 = ch * CT_FC, cn = min(CT_FC, F - c0);
        __syncthreads();
        if (tid < cn) {
            const int32_t *f = faces + (size_t)(c0 + tid) * 3;
            const float *a = v + (size_t)ct_vidx(f[0], V) * 3, *b = v + (size_t)ct_vidx(f[1], V) * 3, *c = v + (size_t)ct_vidx(f[2], V) * 3;
            const CtRec r = ct_make_rec(a[0], a[1], a[2], b[0], b[1], b[2], c[0], c[1], c[2]);
            rec[0][tid] = r.r0; rec[1][tid] = r.r1; rec[2][tid] = r.r2; rec[3][tid] = r.r3; rec[4][tid] = r.r4;
        }
        __syncthreads();
        // squared distance to the chunk's box: a lower bound of the distance to every face in it
        const float *bx = box + (size_t)ch * 8;
        const float ex = fmaxf(fmaxf(bx[0] - p.x, p.x - bx[3]), 0.f), ey = fmaxf(fmaxf(bx[1] - p.y, p.y - bx[4]), 0.f), ez = fmaxf(fmaxf(bx[2] - p.z, p.z - bx[5]), 0.f);
        // the bound is shrunk by a part in 2^10 (its own rounding and that of the face distances are parts in 2^20 and less), so that a chunk
        // that holds the minimum is not skipped; costs no measurable culling
        const bool want_d = (ex * ex + ey * ey + ez * ez) * (1.f - 0x1p-10f) < best;
        float part = 0.f;
        for (int j = 0; j < cn; ++j) {
            CtRec r;
            r.r0 = rec[0][j]; r.r1 = rec[1][j]; r.r2 = rec[2][j]; r.r3 = rec[3][j]; r.r4 = rec[4][j];
            ct_pair(r, p.x, p.y, p.z, want_d, best, part);
        }
        half_omega += part;
    }
    if (i < P) {
        const float d = sqrtf(best), w = half_omega * (float)(1.0 / (2.0 * M_PI));       // w = (2 * sum atan2) / (4 pi)
        const float S = (1.f - 2.f * w) * d;
        obj_label[(size_t)n * P + i] = S < thres ? 1 : 0;
        if (signed_dist) signed_dist[(size_t)n * P + i] = S;
    }
}

__global__ __launch_bounds__(CT_THR) void ct_body_kernel(const float *__restrict__ verts, int V, const float *__restrict__ points, int P, int64_t pstride,
                                                         const float *__restrict__ objR, const float *__restrict__ objT, float thres, int n_tiles,
                                                         const uint8_t *__restrict__ obj_label, uint8_t *__restrict__ human_label) {
    __shared__ float sx[CT_PC], sy[CT_PC], sz[CT_PC];
    __shared__ int cnt;
    const int64_t n = blockIdx.x / n_tiles;
    const int tid = threadIdx.x, i = (blockIdx.x % n_tiles) * CT_THR + tid;
    float RT[12];
    ct_load_pose(RT, objR, objT, n);
    float vx = 0.f, vy = 0.f, vz = 0.f;
    if (i < V) {
        const float *q = verts + ((size_t)n * V + i) * 3;
        vx = q[0]; vy = q[1]; vz = q[2];
    }
    float best = FLT_MAX;
    for (int p0 = 0; p0 < P; p0 += CT_PC) {
        __syncthreads();
        if (tid == 0) cnt = 0;
        __syncthreads();
        for (int j = p0 + tid; j < min(P, p0 + CT_PC); j += CT_THR)
            if (obj_label[(size_t)n * P + j]) {
                const float *q = points + (size_t)n * pstride + (size_t)j * 3;
                const float3 p = ct_pose(RT, objR != nullptr, q[0], q[1], q[2]);
                const int slot = atomicAdd(&cnt, 1);                                   // integer, LDS: the order of the slots does not reach the result
                sx[slot] = p.x; sy[slot] = p.y; sz[slot] = p.z;
            }
        __syncthreads();
        const int m = cnt;
        for (int j = 0; j < m; ++j) {
            const float dx = vx - sx[j], dy = vy - sy[j], dz = vz - sz[j];
            best = fminf(best, ct_dot(dx, dy, dz, dx, dy, dz));
        }
    }
    if (i < V) human_label[(size_t)n * V + i] = sqrtf(best) < thres ? 1 : 0;
}

}  // namespace

extern "C" size_t interdiff_contact_labels_workspace_bytes(int64_t N, int32_t V, int32_t F, int32_t P) {
    if (N <= 0 || V <= 0 || F <= 0 || P <= 0) return 0;
    return idf_align((size_t)N * (size_t)idf_cdiv(F, CT_FC) * 8 * sizeof(float));
}

extern "C" int interdiff_contact_labels(const float *verts, int64_t N, int32_t V, const int32_t *faces, int32_t F, const float *points, int32_t P,
                                        int64_t point_frame_stride, const float *objR, const float *objT, float thres, uint8_t *obj_label,
                                        uint8_t *human_label, float *signed_dist, void *ws, size_t ws_bytes, void *stream) {
    if (!verts || !faces || !points || !obj_label || !human_label || !ws) return IDF_E_INVAL;
    if (N <= 0 || V <= 0 || F <= 0 || P <= 0 || !(thres > 0.f)) return IDF_E_INVAL;
    if (point_frame_stride != 0 && point_frame_stride != (int64_t)3 * P) return IDF_E_INVAL;
    if ((objR == nullptr) != (objT == nullptr)) return IDF_E_INVAL;                    // a pose is both or neither
    const int64_t n_chunks = idf_cdiv(F, CT_FC), tiles_p = idf_cdiv(P, CT_THR), tiles_v = idf_cdiv(V, CT_THR);
    if (N * n_chunks > 0x7FFFFFFF || N * tiles_p > 0x7FFFFFFF || N * tiles_v > 0x7FFFFFFF) return IDF_E_INVAL;      // frames ride on gridDim.x
    if (ws_bytes < interdiff_contact_labels_workspace_bytes(N, V, F, P)) return IDF_E_NOMEM;
    hipStream_t s = idf_stream(stream);
    float *boxes = static_cast<float *>(ws);
    hipLaunchKernelGGL(ct_boxes_kernel, dim3((unsigned)(N * n_chunks)), dim3(CT_THR), 0, s, verts, V, faces, F, (int)n_chunks, boxes);
    IDF_CHECK_LAUNCH();
    hipLaunchKernelGGL(ct_points_kernel, dim3((unsigned)(N * tiles_p)), dim3(CT_THR), 0, s, verts, V, faces, F, points, P, point_frame_stride, objR, objT,
                       thres, boxes, (int)n_chunks, (int)tiles_p, obj_label, signed_dist);
    IDF_CHECK_LAUNCH();
    hipLaunchKernelGGL(ct_body_kernel, dim3((unsigned)(N * tiles_v)), dim3(CT_THR), 0, s, verts, V, points, P, point_frame_stride, objR, objT, thres,
                       (int)tiles_v, obj_label, human_label);
    IDF_CHECK_LAUNCH();
    return IDF_OK;
}

// HOST-side instance of the per-pair device inline: n (point, triangle) pairs, tri [n][9] = a | b | c, p [n][3] -> out [n][2] = squared distance,
// signed solid angle.  Lets the CPU suite check the region logic and the zero-area path without a GPU.
extern "C" int interdiff_debug_point_triangle(const float *tri, const float *p, float *out, int32_t n) {
    if (!tri || !p || !out || n < 0) return IDF_E_INVAL;
    for (int i = 0; i < n; ++i) {
        const float *t = tri + 9 * i;
        const CtRec r = ct_make_rec(t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7], t[8]);
        float best = FLT_MAX, half_omega = 0.f;
        ct_pair(r, p[3 * i], p[3 * i + 1], p[3 * i + 2], true, best, half_omega);
        out[2 * i] = best;
        out[2 * i + 1] = 2.f * half_omega;
    }
    return IDF_OK;
}
