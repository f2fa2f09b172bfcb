// Scoring of a correction-predictor checkpoint (forward only): the ten terms of LitInteraction.calc_loss_contact
// (interdiff/train_correction_smpl.py:103-185), the eight of calc_loss (:60-101) and of the skeleton trainer's calc_loss
// (train_correction_skeleton.py:85-126).  Term order = the reference's dict order:
//   0 penetration, 1 contact, 2 obj_rot_past, 3 obj_nonrot_past, 4 obj_rot_future, 5 obj_nonrot_future,
//   6 obj_rot_v_past, 7 obj_nonrot_v_past, 8 obj_rot_v_future, 9 obj_nonrot_v_future.
//
// GEOMETRY HALF (one launch, grid = (blocks per frame, T * B)).  Per frame the reference poses the P object points with the PREDICTED
// rotation / translation, runs point2point_signed between the V body vertices and the posed points (tools.py:11-76: nearest neighbour in
// both directions, sign of object->human from the body normal at the nearest vertex) and takes two masked means.  Here a workgroup owns
// 1024 queries of one frame and one direction:
//   object-query workgroups (the heavy ones, scheduled first): pose their points in registers, scan all V vertices through LDS chunks
//       with the project's exact argmin (d2 = (dx*dx + dy*dy) + dz*dz, no FMA, lowest index wins), then read position and normal of the
//       winner out of the interleaved [V][7] record:  sum 20 |o2h| [o2h < 0]
//   human-query workgroups: scan the P posed points (posed while they are written to LDS); only the minimum is needed (the human->object
//       distance is unsigned: y_normals is None at :131), then the label of the interleaved record:  sum |h2o| [|h2o| > 0.02 and label > 0.5]
// Nothing per pair, per vertex or per point goes to HBM: a workgroup writes (sum, count) -- two floats.  The posed points never exist in
// memory either.  Quirk kept: the reference's band 0 < o2h < 0.01 gets weight 0 (:141-143), i.e. nothing.
// REDUCTION HALF (one launch, ten workgroups): term i is folded by workgroup i -- strided per-thread sums in index order, then a fixed
// LDS tree.  No float atomics anywhere: two calls give the same bits.  In front of the two: one strided device copy and the rotation entry's launch
// (per-frame matrices, see the launcher).  The launch count does not depend on T * B.
#include "corr_geometry.h"
#include <float.h>

using namespace idf_corr_geometry;      // the tiling, cl_dist2, cl_pose, cl_tree: shared with the backward (csrc/corr_geometry_grad.hip)

namespace {

// (sum, count) of the workgroup in a fixed order: lanes by a shuffle tree, waves one after the other
__device__ __forceinline__ void cl_block_sum2(float s, float c, float *red, float *out2) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s += __shfl_down(s, o);
        c += __shfl_down(c, o);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { red[2 * wave] = s; red[2 * wave + 1] = c; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float ts = 0.f, tc = 0.f;
        for (int w = 0; w < CL_THR / 64; ++w) { ts += red[2 * w]; tc += red[2 * w + 1]; }
        out2[0] = ts;
        out2[1] = tc;
    }
}

__global__ __launch_bounds__(CL_THR) void corr_geometry_kernel(const float *__restrict__ obj_pred, const float *__restrict__ obj_points, int pstride,
                                                               const float *__restrict__ human_verts, const float *__restrict__ rotmat, int B, int V,
                                                               int P, int nbO, int nbH, float *__restrict__ partial) {
    __shared__ float4 rs[CL_RC];
    __shared__ float red[2 * CL_THR / 64];
    const int64_t n = blockIdx.y;                       // frame t * B + b
    const int bx = blockIdx.x, tid = threadIdx.x;
    const float *op = obj_points + (size_t)(n % B) * P * pstride;      // canonical points of the frame's clip
    float R[12];                                        // the frame's matrix (from interdiff_rotation_6d_to_matrix, see the launcher) and translation: uniform loads
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = rotmat[n * 9 + i];
#pragma unroll
    for (int i = 0; i < 3; ++i) R[9 + i] = obj_pred[n * 9 + 6 + i];
    const float *hv = human_verts + (size_t)n * V * HV;
    float *out2 = partial + ((size_t)n * (nbO + nbH) + bx) * 2;
    float qx[CL_QPT], qy[CL_QPT], qz[CL_QPT], best[CL_QPT];

    if (bx < nbO) {
        // ---------------------------------------------------------------- object -> human: exact argmin over the V vertices
        const int q0 = bx * CL_TILE + tid;
        int bi[CL_QPT];
#pragma unroll
        for (int k = 0; k < CL_QPT; ++k) {
            const int i = q0 + CL_THR * k;
            float3 p = make_float3(0.f, 0.f, 0.f);
            if (i < P) p = cl_pose(R, op[(size_t)i * pstride], op[(size_t)i * pstride + 1], op[(size_t)i * pstride + 2]);
            qx[k] = p.x; qy[k] = p.y; qz[k] = p.z;
            best[k] = FLT_MAX;
            bi[k] = 0;
        }
        for (int c0 = 0; c0 < V; c0 += CL_RC) {
            const int cn = min(CL_RC, V - c0);
            __syncthreads();
            for (int j = tid; j < cn; j += CL_THR) {
                const float *r = hv + (size_t)(c0 + j) * HV;
                rs[j] = make_float4(r[0], r[1], r[2], 0.f);
            }
            __syncthreads();
            for (int j = 0; j < cn; ++j) {
                const float4 p = rs[j];
#pragma unroll
                for (int k = 0; k < CL_QPT; ++k) {
                    const float d2 = cl_dist2(qx[k], qy[k], qz[k], p.x, p.y, p.z);
                    if (d2 < best[k]) { best[k] = d2; bi[k] = c0 + j; }
                }
            }
        }
        float s = 0.f, c = 0.f;
#pragma unroll
        for (int k = 0; k < CL_QPT; ++k) {
            const int i = q0 + CL_THR * k;
            if (i < P) {
                const float *r = hv + (size_t)bi[k] * HV;
                const float vx = qx[k] - r[0], vy = qy[k] - r[1], vz = qz[k] - r[2];
                const float d = sqrtf(vx * vx + vy * vy + vz * vz);
                const float dt = r[3] * vx + r[4] * vy + r[5] * vz;          // sign(normal . vector), tools.py:58-61
                if (dt < 0.f && d > 0.f) { s += d * 20.f; c += 1.f; }          // w = 20 where o2h_signed < 0 (:142-144)
            }
        }
        __syncthreads();
        cl_block_sum2(s, c, red, out2);
    } else {
        // ---------------------------------------------------------------- human -> object: the minimum over the P posed points
        const int q0 = (bx - nbO) * CL_TILE + tid;
#pragma unroll
        for (int k = 0; k < CL_QPT; ++k) {
            const int i = q0 + CL_THR * k;
            const bool ok = i < V;
            qx[k] = ok ? hv[(size_t)i * HV] : 0.f; qy[k] = ok ? hv[(size_t)i * HV + 1] : 0.f; qz[k] = ok ? hv[(size_t)i * HV + 2] : 0.f;
            best[k] = FLT_MAX;
        }
        for (int c0 = 0; c0 < P; c0 += CL_RC) {
            const int cn = min(CL_RC, P - c0);
            __syncthreads();
            for (int j = tid; j < cn; j += CL_THR) {
                const float *r = op + (size_t)(c0 + j) * pstride;
                const float3 p = cl_pose(R, r[0], r[1], r[2]);
                rs[j] = make_float4(p.x, p.y, p.z, 0.f);
            }
            __syncthreads();
            for (int j = 0; j < cn; ++j) {
                const float4 p = rs[j];
#pragma unroll
                for (int k = 0; k < CL_QPT; ++k) {
                    const float d2 = cl_dist2(qx[k], qy[k], qz[k], p.x, p.y, p.z);
                    best[k] = d2 < best[k] ? d2 : best[k];
                }
            }
        }
        float s = 0.f, c = 0.f;
#pragma unroll
        for (int k = 0; k < CL_QPT; ++k) {
            const int i = q0 + CL_THR * k;
            if (i < V) {
                const float d = sqrtf(best[k]);
                if (d > 0.02f && hv[(size_t)i * HV + 6] > 0.5f) { s += d; c += 1.f; }      // v_dist (:136)
            }
        }
        __syncthreads();
        cl_block_sum2(s, c, red, out2);
    }
}

// Ten workgroups, one per term.  0 / 1: per-frame sums of the geometry partials (a frame's workgroups in index order), written to
// out_frames [N][4] = (penetration sum, contact sum, penetration count, contact count) when asked for, then the mean over N * P / N * V.
// 2..9: the MSE terms on [T][B][W + 3] (rot = the leading W channels, nonrot = the trailing 3): thread i takes elements i, i + 256, ...
__global__ __launch_bounds__(CL_THR) void corr_finish_kernel(const float *__restrict__ x, const float *__restrict__ g, int T, int B, int W, int past,
                                                             const float *__restrict__ partial, int nbO, int nbH, int V, int P,
                                                             float *__restrict__ out_terms, float *__restrict__ out_frames) {
    __shared__ float sm[CL_THR];
    const int term = blockIdx.x, tid = threadIdx.x;
    const int C = W + 3;
    float acc = 0.f;
    if (term < 2) {
        if (!partial) {                                  // no geometry half (calc_loss, the skeleton trainer)
            if (tid == 0) out_terms[term] = 0.f;
            return;
        }
        const int N = T * B, nb = nbO + nbH;
        const int lo = term == 0 ? 0 : nbO, hi = term == 0 ? nbO : nb;
        for (int n = tid; n < N; n += CL_THR) {
            float s = 0.f, c = 0.f;
            for (int k = lo; k < hi; ++k) {
                s += partial[((size_t)n * nb + k) * 2];
                c += partial[((size_t)n * nb + k) * 2 + 1];
            }
            if (out_frames) {
                out_frames[(size_t)n * 4 + term] = s;
                out_frames[(size_t)n * 4 + 2 + term] = c;
            }
            acc += s;
        }
        const float tot = cl_tree(acc, sm);
        if (tid == 0) out_terms[term] = tot / ((float)N * (float)(term == 0 ? P : V));
        return;
    }
    const int k = term - 2;                              // 0 rot_past 1 nonrot_past 2 rot_future 3 nonrot_future 4 rot_v_past 5 nonrot_v_past 6 rot_v_future 7 nonrot_v_future
    const bool nonrot = k & 1, future = (k >> 1) & 1, vel = k >= 4;
    const int c0 = nonrot ? W : 0, cw = nonrot ? 3 : W;
    const int t0 = future ? past : 0, nt = future ? T - past : past;
    // velocity: past pairs frame t with t + 1 (t < past), future pairs frame t with t - 1 (t >= past: the first pair straddles the
    // past / future border, as the reference writes it)
    const int dt = future ? -1 : 1;
    const int per_t = B * cw, total = nt * per_t;
    for (int e = tid; e < total; e += CL_THR) {
        const int t = t0 + e / per_t, r = e - (e / per_t) * per_t, b = r / cw, c = c0 + (r - b * cw);
        const size_t i = ((size_t)t * B + b) * C + c;
        float d;
        if (!vel) d = x[i] - g[i];
        else {
            const size_t j = ((size_t)(t + dt) * B + b) * C + c;
            d = future ? (x[i] - x[j]) - (g[i] - g[j]) : (x[j] - x[i]) - (g[j] - g[i]);
        }
        acc += d * d;
    }
    const float tot = cl_tree(acc, sm);
    if (tid == 0) out_terms[term] = tot / (float)total;
}

}  // namespace

extern "C" size_t interdiff_correction_losses_workspace_bytes(int32_t T, int32_t B, int32_t V, int32_t P) {
    if (T <= 0 || B <= 0 || V <= 0 || P <= 0) return 0;
    const size_t nb = (size_t)idf_cdiv(P, CL_TILE) + (size_t)idf_cdiv(V, CL_TILE);
    return idf_align((size_t)T * B * nb * 2 * sizeof(float)) + idf_align((size_t)T * B * 6 * sizeof(float)) + idf_align((size_t)T * B * 9 * sizeof(float));
}

extern "C" int interdiff_correction_losses(const float *obj_pred, const float *obj_gt, const float *obj_points, int32_t point_stride,
                                           const float *human_verts, int32_t T, int32_t B, int32_t V, int32_t P, int32_t rot_width,
                                           int32_t past_len, float *out_terms, float *out_frames, void *ws, size_t ws_bytes, void *stream) {
    if (!obj_pred || !obj_gt || !out_terms || T <= 0 || B <= 0 || rot_width < 1 || rot_width > 64) return IDF_E_INVAL;
    if (past_len < 1 || T < past_len + 1) return IDF_E_INVAL;                 // the past velocity term reads frame past_len
    if ((int64_t)T * B * (rot_width + 3) > 0x7FFFFFFF) return IDF_E_INVAL;
    const bool geo = obj_points != nullptr || human_verts != nullptr;
    hipStream_t s = idf_stream(stream);
    float *partial = nullptr;
    int nbO = 0, nbH = 0;
    if (geo) {
        if (!obj_points || !human_verts || rot_width != 6 || V <= 0 || P <= 0 || point_stride < 3 || !ws) return IDF_E_INVAL;
        if ((int64_t)T * B > 65535) return IDF_E_INVAL;                       // frames ride on gridDim.y
        if (ws_bytes < interdiff_correction_losses_workspace_bytes(T, B, V, P)) return IDF_E_NOMEM;
        nbO = (int)idf_cdiv(P, CL_TILE);
        nbH = (int)idf_cdiv(V, CL_TILE);
        partial = static_cast<float *>(ws);
        // The per-frame matrices come from the library's own rotation entry, not from a second copy of its formula: the rot6d columns are gathered
        // into the workspace by a strided device copy and interdiff_rotation_6d_to_matrix converts them -- so this entry and a composition of that entry
        // with interdiff_point2point_signed pose the points from the same bits whatever the compiler contracts.
        const size_t N = (size_t)T * B;
        float *d6 = reinterpret_cast<float *>(static_cast<char *>(ws) + idf_align(N * (nbO + nbH) * 2 * sizeof(float)));
        float *rotmat = reinterpret_cast<float *>(reinterpret_cast<char *>(d6) + idf_align(N * 6 * sizeof(float)));
        if (hipMemcpy2DAsync(d6, 6 * sizeof(float), obj_pred, 9 * sizeof(float), 6 * sizeof(float), N, hipMemcpyDeviceToDevice, s) != hipSuccess) return IDF_E_LAUNCH;
        const int rc = interdiff_rotation_6d_to_matrix(d6, rotmat, (int64_t)N, stream);
        if (rc != IDF_OK) return rc;
        hipLaunchKernelGGL(corr_geometry_kernel, dim3((unsigned)(nbO + nbH), (unsigned)(T * B)), dim3(CL_THR), 0, s, obj_pred, obj_points,
                           point_stride, human_verts, rotmat, B, V, P, nbO, nbH, partial);
        IDF_CHECK_LAUNCH();
    } else if (out_frames) return IDF_E_INVAL;
    hipLaunchKernelGGL(corr_finish_kernel, dim3(10), dim3(CL_THR), 0, s, obj_pred, obj_gt, T, B, rot_width, past_len, partial, nbO, nbH, V, P, out_terms,
                       out_frames);
    IDF_CHECK_LAUNCH();
    return IDF_OK;
}
