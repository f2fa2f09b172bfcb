// The contact-radius mask of the physics post-optimisation (optimization.py:74-75): opt_patch_kernel, opt_near_kernel and their launcher.  It is the dual of
// the nearest-vertex scan and shares its constants (MAXP, v2f) and the clips' Morton point order, so it lives in the scan's translation unit (correction.hip);
// optimize.hip reaches it through idf_near_mask_opt (common.h).
#pragma once
#include "contact_scan.h"

namespace {

// ---- the contact-radius mask of the post-optimisation (optimization.py:74-75): per vertex, does ANY object point lie within 0.5 m? ----
// The dual of the scan (contact_scan.h): lanes are VERTICES, the frame's object points are cut into patches of 64 consecutive points of the
// clip's Morton order (compact under the frame's rigid transform) with their boxes; a patch is looked at only if its box comes
// closer than 0.5 m to some vertex of the wave that is still undecided (same monotone lower bound, so the cut is exact), and a
// wave leaves as soon as all its vertices have found a point.  K-A sorts the frame's points and boxes its patches, K-B answers.
constexpr int NPATCH = MAXP / 64;
__global__ __launch_bounds__(256) void opt_patch_kernel(const float *__restrict__ pts, int P, const int32_t *__restrict__ porder, int frames_per_clip,
                                                        float4 *__restrict__ psort /* [N][MAXP] */, float4 *__restrict__ pbox /* [N][NPATCH][2] */) {
    const int64_t n = blockIdx.x;
    const int b = (int)(n / frames_per_clip), tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float *pn = pts + (size_t)n * P * 3;
    for (int k = wave; k < NPATCH; k += 4) {
        const int sp = 64 * k + lane;
        float x = 3e18f, y = 3e18f, z = 3e18f;                              // slots past P: far away (never within the radius)
        float lx = FLT_MAX, ly = FLT_MAX, lz = FLT_MAX, hx = -FLT_MAX, hy = -FLT_MAX, hz = -FLT_MAX;
        if (sp < P) {
            const int i = porder[(size_t)b * P + sp];
            x = pn[3 * i]; y = pn[3 * i + 1]; z = pn[3 * i + 2];
            lx = hx = x; ly = hy = y; lz = hz = z;
        }
        psort[(size_t)n * MAXP + sp] = make_float4(x, y, z, 0.f);
        lx = -wave_max(-lx); ly = -wave_max(-ly); lz = -wave_max(-lz);
        hx = wave_max(hx); hy = wave_max(hy); hz = wave_max(hz);
        if (lane == 0) {
            pbox[((size_t)n * NPATCH + k) * 2] = make_float4(lx, ly, lz, 0.f);
            pbox[((size_t)n * NPATCH + k) * 2 + 1] = make_float4(hx, hy, hz, 0.f);
        }
    }
}

__global__ __launch_bounds__(256) void opt_near_kernel(const float *__restrict__ verts, int V, int P, const float4 *__restrict__ psort,
                                                       const float4 *__restrict__ pbox, const int32_t *__restrict__ vorder,
                                                       int32_t *__restrict__ near) {
    __shared__ float4 ps[MAXP];                                            // the frame's points, sorted
    __shared__ float4 bx[NPATCH * 2];
    const int64_t n = blockIdx.y;
    // a wave takes 64 consecutive vertices of the SCAN order (a compact clump of the body): its lanes agree on which patches matter
    const int tid = threadIdx.x, pos = blockIdx.x * 256 + tid, vid = vorder[min(pos, V - 1)];
    for (int i = tid; i < MAXP; i += 256) ps[i] = psort[(size_t)n * MAXP + i];
    if (tid < NPATCH * 2) bx[tid] = pbox[(size_t)n * NPATCH * 2 + tid];
    const bool valid = pos < V;
    const float *vp = verts + ((size_t)n * V + vid) * 3;
    const float vx = vp[0], vy = vp[1], vz = vp[2];
    __syncthreads();
    const int npatch = (P + 63) / 64;
    bool hit = false;
    {
#pragma clang fp contract(off)
        const v2f VX = v2f{vx, vx}, VY = v2f{vy, vy}, VZ = v2f{vz, vz};
        for (int k = 0; k < npatch; ++k) {
            if (__builtin_amdgcn_ballot_w64(valid && !hit) == 0ull) break;               // every vertex of the wave is decided
            const float4 lo = bx[2 * k], hi = bx[2 * k + 1];
            const float ex = fmaxf(fmaxf(lo.x - vx, vx - hi.x), 0.f), ey = fmaxf(fmaxf(lo.y - vy, vy - hi.y), 0.f), ez = fmaxf(fmaxf(lo.z - vz, vz - hi.z), 0.f);
            const float xx = ex * ex, yy = ey * ey, zz = ez * ez;
            if (__builtin_amdgcn_ballot_w64(valid && !hit && (xx + yy) + zz < 0.25f) == 0ull) continue;      // no undecided vertex can have a point of this patch in range
            const float4 *pp = ps + 64 * k;
            for (int j0 = 0; j0 < 64; j0 += 16) {                        // sixteen points, then ask again whether anybody is still undecided
#pragma unroll
                for (int j = j0; j < j0 + 16; j += 2) {
                    const float4 p = pp[j], q = pp[j + 1];
                    // sqrt(d2) < 0.5 (optimization.py:75) <=> d2 < 0.25 up to the rounding of the last ulp; d = point - vertex as in the brute force
                    const v2f dx = v2f{p.x, q.x} - VX, dy = v2f{p.y, q.y} - VY, dz = v2f{p.z, q.z} - VZ;
                    const v2f d2 = (dx * dx + dy * dy) + dz * dz;
                    hit = hit || d2.x < 0.25f || d2.y < 0.25f;
                }
                if (__builtin_amdgcn_ballot_w64(valid && !hit) == 0ull) break;
            }
        }
    }
    if (valid) near[(size_t)n * V + vid] = hit ? 1 : 0;
}

// near[n][v] = 1 iff some object point of frame n lies within 0.5 m of vertex v.  Frames clip-major; `porder` [B][P] as filled by idf_point_order for the same clips;
// psort [N][2048] float4 and pbox [N][32][2] float4 are scratch.
int launch_near_mask(hipStream_t s, int64_t N, int frames_per_clip, const float *verts, int V, const float *pts_frame, int P, const int32_t *porder,
                     const int32_t *vorder, float *psort, float *pbox, int32_t *near) {
    if (P > MAXP || !vorder) return IDF_E_INVAL;
    hipLaunchKernelGGL(opt_patch_kernel, dim3((unsigned)N), dim3(256), 0, s, pts_frame, P, porder, frames_per_clip, reinterpret_cast<float4 *>(psort),
                       reinterpret_cast<float4 *>(pbox));
    hipLaunchKernelGGL(opt_near_kernel, dim3((unsigned)idf_cdiv(V, 256), (unsigned)N), dim3(256), 0, s, verts, V, P, reinterpret_cast<const float4 *>(psort),
                       reinterpret_cast<const float4 *>(pbox), vorder, near);
    return IDF_OK;
}

}  // namespace
