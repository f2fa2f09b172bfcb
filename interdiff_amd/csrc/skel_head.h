// Keypoint head of the HO-GCN skeleton denoiser (model/diffusion_skeleton.py:218-248) as an epilogue of the heads GEMM (gemm.h
// gemm_glds_kernel, 32 x 32 tile, 512 threads).
//
// The model's last linears give 70 values per token row: bodyFinalLinear (n_body = 63) and objFinalLinear (7 = translation xyz |
// quaternion xyzw).  x0 has 106 channels: 63 body | 36 object keypoints calc_obj_pred(pose, zero_pose_obj) = R(q) z_k + trans |
// 7 pose.  Every keypoint channel of a row needs that row's 7 pose values, so the packed weight (skeleton.py pack_skeleton_head)
// puts the 7 POSE ROWS FIRST IN EVERY 32-row column tile, followed by 25 body rows: 63 body rows take 3 tiles -- the same 3
// workgroups per row tile a plain 70-wide GEMM would launch -- and each workgroup holds the pose of its 32 token rows without a
// second launch or a trip through HBM (the pose rows are computed three times, in MFMA columns that were padding before).  Tile nt
// writes its 25 body channels, a third of the keypoints (n_points / tiles of them) and, tile 0 only, the 7 pose channels.
//
// After the k-loop the accumulator tile (+ bias) is parked in LDS ([32 rows][32 + 1]) next to the zero-pose keypoints of the clips
// the 32 rows belong to (fetched into registers before the k-loop, ONCE per workgroup); then every thread owns one (channel, four
// consecutive rows) item: 64 channel slots x 8 row groups = 512 threads.  With T % 4 == 0 the four rows are four frames of one clip
// = one aligned float4 of x0[b][c][t..t+3], and the fused step (E_SKEL_POST) applies inpainting, posterior mean and Philox noise to
// it exactly as gemm.h's epilogue_post does; other clip lengths take the per-element form.  The value of an x0 element is computed
// by ONE function (skel_value, contraction off) in every instantiation: forward + interdiff_posterior_step_dev and the fused step
// agree bit for bit.
//
// Operands ride in Args fields the heads GEMM does not use otherwise: resid = zero_pose_obj [B][n_points][3], Ka = n_body,
// n_steps = n_points, ldc = channels of x0 (n_body + 3 n_points + 7), N = 32 x tiles (rows of the packed weight).
#pragma once

namespace idf_gemm {

constexpr int SKH_POSE = 7, SKH_BODY = 32 - SKH_POSE;      // rows of a 32-row column tile: pose first, then body
constexpr int SKH_SLOTS = 64;                              // channel slots per tile: 32 linear outputs + up to 32 keypoint coordinates
constexpr int SKH_CS = 33;                                 // padded row stride of the parked tile
constexpr int SKH_ZMAX = 48;                               // 3 n_points at most: 32 clips x 48 floats = 3 prefetch registers per thread
constexpr int SKH_ZREG = 32 * SKH_ZMAX / 512;

static inline int skel_head_tiles(int n_body) { return (n_body + SKH_BODY - 1) / SKH_BODY; }
// shapes the epilogue serves: every tile's keypoint share fits its 32 spare slots, all of a clip's keypoints fit the prefetch registers
static inline bool skel_head_shape_ok(int n_body, int n_points, int n_tiles) {
    if (n_body < 1 || n_points < 1 || n_tiles != skel_head_tiles(n_body) || 3 * n_points > SKH_ZMAX) return false;
    return 3 * ((n_points + n_tiles - 1) / n_tiles) <= SKH_SLOTS - 32;
}

// slot ci of column tile nt -> channel of x0 (or -1: nothing to write); col = column of the parked tile for a linear output,
// k >= 0 / d: keypoint and coordinate for a derived one
__device__ __forceinline__ int skel_slot(const Args &g, int nt, int ci, int &col, int &k, int &d) {
    const int n_body = g.Ka, n_points = g.n_steps, ntile = g.N >> 5, kpt = (n_points + ntile - 1) / ntile;
    col = ci; k = -1; d = 0;
    if (ci < SKH_POSE) return nt == 0 ? n_body + 3 * n_points + ci : -1;
    if (ci < 32) {
        const int j = nt * SKH_BODY + ci - SKH_POSE;
        return j < n_body ? j : -1;
    }
    const int e = ci - 32, kk = e / 3;
    d = e - 3 * kk;
    k = nt * kpt + kk;
    if (kk >= kpt || k >= n_points) { k = -1; return -1; }
    return n_body + 3 * k + d;
}

// x0 value of one (row, slot): a linear output as it is, or coordinate d of keypoint k -- calc_obj_pred (diffusion_skeleton.py:218-229):
// the head's quaternion (x, y, z, w) reordered to (w, x, y, z) = pytorch3d's (r, i, j, k), quaternion_to_matrix WITHOUT normalising
// (two_s = 2 / (q . q)), row d of R times the zero-pose keypoint, plus the translation.  Every operation rounded on its own.
__device__ __forceinline__ float skel_value(const float *row, const float *z, int col, int k, int d) {
#pragma clang fp contract(off)
    if (k < 0) return row[col];
    const float i = row[3], j = row[4], kk = row[5], r = row[6];
    const float s2 = 2.0f / (((r * r + i * i) + j * j) + kk * kk);
    float m0, m1, m2;
    if (d == 0) { m0 = 1.0f - s2 * (j * j + kk * kk); m1 = s2 * (i * j - kk * r); m2 = s2 * (i * kk + j * r); }
    else if (d == 1) { m0 = s2 * (i * j + kk * r); m1 = 1.0f - s2 * (i * i + kk * kk); m2 = s2 * (j * kk - i * r); }
    else { m0 = s2 * (i * kk - j * r); m1 = s2 * (j * kk + i * r); m2 = 1.0f - s2 * (i * i + j * j); }
    const float *zk = z + 3 * k;
    return ((m0 * zk[0] + m1 * zk[1]) + m2 * zk[2]) + row[d];
}

// what a thread asks for BEFORE the k-loop: its share of the tile's zero-pose keypoints and, for the fused step with T % 4 == 0, the
// sampler operands of its item (state -> coefficient row -> x / gt / mask: three dependent round trips, plus ~500 VALU instructions
// of Philox + Box-Muller: behind the first operand fetches instead of behind the matrix work, as gemm.h post_prefetch)
struct SkelPre {
    float z[SKH_ZREG];
    float4 xv, gv, e;
    uchar4 mk;
    float c1, c2, sigma;
};

template <int EPI>
__device__ __forceinline__ void skel_prefetch(const Args &g, SkelPre &p, int m0, int nt, int tid) {
    const int zc = 3 * g.n_steps, b_first = m0 / g.T, b_last = min(m0 + 31, g.M - 1) / g.T, nz = (b_last - b_first + 1) * zc;
#pragma unroll
    for (int q = 0; q < SKH_ZREG; ++q) {
        const int idx = tid + 512 * q;
        p.z[q] = idx < nz ? g.resid[(size_t)b_first * zc + idx] : 0.f;
    }
    if constexpr (EPI == E_SKEL_POST) {
        const int64_t st = g.post_state[4];
        const uint64_t it = (uint64_t)g.post_state[5], seed = (uint64_t)g.post_state[2];
        const size_t elem0 = (size_t)g.post_state[6];
        p.c1 = g.post_table[st * 4]; p.c2 = g.post_table[st * 4 + 1]; p.sigma = g.post_table[st * 4 + 2];
        int col, k, d;
        const int ch = skel_slot(g, nt, tid >> 3, col, k, d), row0 = m0 + 4 * (tid & 7);
        p.xv = p.gv = p.e = zero4();
        p.mk = make_uchar4(0, 0, 0, 0);
        if (ch >= 0 && row0 < g.M) {
            const int b = row0 / g.T, t = row0 - b * g.T;
            const size_t flat = ((size_t)b * g.ldc + ch) * g.T + t;
            p.xv = ld4(g.post_x + flat);
            if (g.post_mask) {
                p.gv = ld4(g.post_gt + flat);
                p.mk = *reinterpret_cast<const uchar4 *>(g.post_mask + flat);
            }
            p.e = randn4(seed, it, (uint64_t)((flat + elem0) >> 2));
        }
        asm volatile("" : "+v"(p.e.x), "+v"(p.e.y), "+v"(p.e.z), "+v"(p.e.w));      // computed here, not sunk into the epilogue
    }
}

// cs: the tile's 32 x 32 linear outputs (+ bias), written by the caller, not yet synchronised; zs: room for 32 clips' keypoints
template <int EPI>
__device__ __forceinline__ void skel_epilogue(const Args &g, const float *cs, float *zs, const SkelPre &p, int m0, int nt, int tid) {
    const int T = g.T, M = g.M, Cout = g.ldc, zc = 3 * g.n_steps, b_first = m0 / T, b_last = min(m0 + 31, M - 1) / T, nz = (b_last - b_first + 1) * zc;
#pragma unroll
    for (int q = 0; q < SKH_ZREG; ++q) {
        const int idx = tid + 512 * q;
        if (idx < nz) zs[idx] = p.z[q];
    }
    __syncthreads();
    if (EPI == E_SKEL_POST || (EPI == E_SKEL && (T & 3) == 0)) {
        // one item per thread: slot tid >> 3, rows 4 (tid & 7) .. + 3 = four frames of one clip (M % 4 == 0: all four exist or none)
        int col, k, d;
        const int ch = skel_slot(g, nt, tid >> 3, col, k, d), r0 = 4 * (tid & 7), row0 = m0 + r0;
        if (ch < 0 || row0 >= M) return;
        const int b = row0 / T, t = row0 - b * T;
        const float *z = zs + (b - b_first) * zc;
        float4 pv = make_float4(skel_value(cs + r0 * SKH_CS, z, col, k, d), skel_value(cs + (r0 + 1) * SKH_CS, z, col, k, d),
                                skel_value(cs + (r0 + 2) * SKH_CS, z, col, k, d), skel_value(cs + (r0 + 3) * SKH_CS, z, col, k, d));
        const size_t flat = ((size_t)b * Cout + ch) * T + t;
        if constexpr (EPI == E_SKEL_POST) {
            const uchar4 m = p.mk;
            pv.x = m.x ? p.gv.x : pv.x; pv.y = m.y ? p.gv.y : pv.y; pv.z = m.z ? p.gv.z : pv.z; pv.w = m.w ? p.gv.w : pv.w;
            idf_store16_wt(g.post_x + flat, posterior4(p.c1, p.c2, p.sigma, pv, p.xv, p.e));      // the next step's embedding reads x from other XCDs
        } else {
            *reinterpret_cast<float4 *>(g.C + flat) = pv;
        }
    } else {
        // any clip length: one element at a time, 32 rows x 64 slots over the 512 threads; the fused step draws component (index & 3) of
        // Philox group (index >> 2), what interdiff_posterior_step_dev gives that element
        int64_t st = 0;
        uint64_t it = 0, seed = 0;
        size_t elem0 = 0;
        float c1 = 0.f, c2 = 0.f, sigma = 0.f;
        if constexpr (is_post(EPI)) {
            st = g.post_state[4]; it = (uint64_t)g.post_state[5]; seed = (uint64_t)g.post_state[2]; elem0 = (size_t)g.post_state[6];
            c1 = g.post_table[st * 4]; c2 = g.post_table[st * 4 + 1]; sigma = g.post_table[st * 4 + 2];
        }
        for (int item = tid; item < 32 * SKH_SLOTS; item += 512) {
            int col, k, d;
            const int r = item & 31, ch = skel_slot(g, nt, item >> 5, col, k, d), row = m0 + r;
            if (ch < 0 || row >= M) continue;
            const int b = row / T, t = row - b * T;
            float v = skel_value(cs + r * SKH_CS, zs + (b - b_first) * zc, col, k, d);
            const size_t flat = ((size_t)b * Cout + ch) * T + t;
            if constexpr (is_post(EPI)) {
                if (g.post_mask && g.post_mask[flat]) v = g.post_gt[flat];
                const size_t idx = flat + elem0;
                const float4 ec = randn4(seed, it, (uint64_t)(idx >> 2));
                idf_store4_wt(g.post_x + flat, posterior1(c1, c2, sigma, v, g.post_x[flat], sel8(ec, ec, (int)(idx & 3))));
            } else {
                g.C[flat] = v;
            }
        }
    }
}

}  // namespace idf_gemm
