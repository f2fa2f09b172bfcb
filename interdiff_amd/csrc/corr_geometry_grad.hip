// Backward pass of the two geometry terms of LitInteraction.calc_loss_contact (interdiff/train_correction_smpl.py:121-153): the gradient of
//     w_pen * penetration + w_con * contact
// at the prediction obj_pred [T][B][9] (rot6d | translation) -- what loss.backward() sends through torch.matmul(obj_points, obj_rot) + trans (:126),
// rotation_6d_to_matrix (:121) and tools.point2point_signed (tools.py:11-76) into the network's output.  The forward of the two terms is
// corr_geometry_kernel (csrc/corr_losses.hip); this file mirrors it.
//
// With y_j = M p_j + t the posed object point, x_i a body vertex, i(j) / j(i) the nearest neighbours and every mask a constant:
//     penetration = 1/(N P) sum_{n,j} 20 |y_j - x_i(j)|  over the points behind their nearest vertex (normal . (y - x) < 0)
//     contact     = 1/(N V) sum_{n,i} |x_i - y_j(i)|     over the labelled vertices farther than 2 cm
// a penetrating point contributes g = 20 (y_j - x_i) / |y_j - x_i| with p = p_j, a contact vertex g = -(x_i - y_j(i)) / |x_i - y_j(i)| with p = p_j(i); each adds
// g to dL/dt and the outer product g p^T to dL/dM.  The pose is 12 numbers per frame, so nothing per point is scattered.
//
// SCAN (one launch, grid = (workgroups per frame, T * B)): a workgroup owns 1024 queries of one frame and one direction, exactly as in the forward kernel --
// the same LDS chunk scan, the same exact argmin (d2 = (dx*dx + dy*dy) + dz*dz, no FMA, lowest index wins), points posed on the fly from the same matrix
// bits (interdiff_rotation_6d_to_matrix).  The human-side scan carries the argmin INDEX as well (the forward keeps only the minimum).  A workgroup writes, in a
// fixed order, its two forward partials (sum, count: fp32, the forward kernel's arithmetic) and its 12 gradient partials (double: lanes by a shuffle tree,
// waves one after the other).
// FINISH (one launch): block 0 folds the two term values in the forward's order; every other block takes 256 frames, one per thread: the frame's workgroups in
// index order, the weights w_pen / (N P) and w_con / (N V), and the backward of the Gram-Schmidt construction in double
//     b1 = a1 / |a1|,  c = a2 - (b1 . a2) b1,  b2 = c / |c|,  b3 = b1 x b2        (pytorch3d rotation_6d_to_matrix, F.normalize's eps 1e-12)
// -> d_obj_pred [N][9], rounded once.  No float atomics: two calls give the same bits.  The launch count does not depend on T * B.
#include "corr_geometry.h"
#include <float.h>

using namespace idf_corr_geometry;      // the forward's tiling, cl_dist2, cl_pose, cl_tree

namespace {

constexpr int CG_WAVES = CL_THR / 64;
constexpr int CG_G = 12;                                               // dL/dM [3][3] row-major | dL/dt [3]

// acc += scale * v / |v| (x) (p | 1): the unit vector in double from the fp32 difference
__device__ __forceinline__ void cg_add(double *acc, double scale, float vx, float vy, float vz, float px, float py, float pz) {
    const double x = (double)vx, y = (double)vy, z = (double)vz;
    const double r = scale / sqrt(x * x + y * y + z * z);
    const double g[3] = {x * r, y * r, z * r};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        acc[3 * i] += g[i] * (double)px;
        acc[3 * i + 1] += g[i] * (double)py;
        acc[3 * i + 2] += g[i] * (double)pz;
        acc[9 + i] += g[i];
    }
}

// the workgroup's (sum, count) and 12 gradient sums in a fixed order: lanes by a shuffle tree, waves one after the other
__device__ __forceinline__ void cg_block_sum(float s, float c, double *acc, float *redf, double *redd, float *out2, double *out12) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s += __shfl_down(s, o);
        c += __shfl_down(c, o);
#pragma unroll
        for (int i = 0; i < CG_G; ++i) acc[i] += __shfl_down(acc[i], o);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        redf[2 * wave] = s;
        redf[2 * wave + 1] = c;
#pragma unroll
        for (int i = 0; i < CG_G; ++i) redd[wave * CG_G + i] = acc[i];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float ts = 0.f, tc = 0.f;
        for (int w = 0; w < CG_WAVES; ++w) { ts += redf[2 * w]; tc += redf[2 * w + 1]; }
        out2[0] = ts;
        out2[1] = tc;
    }
    if ((int)threadIdx.x < CG_G) {
        double t = 0.0;
        for (int w = 0; w < CG_WAVES; ++w) t += redd[w * CG_G + threadIdx.x];
        out12[threadIdx.x] = t;
    }
}

__global__ __launch_bounds__(CL_THR) void corr_geometry_grad_kernel(const float *__restrict__ obj_pred, const float *__restrict__ obj_points, int pstride,
                                                                    const float *__restrict__ human_verts, const float *__restrict__ rotmat, int B, int V,
                                                                    int P, int nbO, int nbH, float *__restrict__ partial, double *__restrict__ gpart) {
    __shared__ float4 rs[CL_RC];
    __shared__ float redf[2 * CG_WAVES];
    __shared__ double redd[CG_G * CG_WAVES];
    const int64_t n = blockIdx.y;                       // frame t * B + b
    const int bx = blockIdx.x, tid = threadIdx.x;
    const float *op = obj_points + (size_t)(n % B) * P * pstride;      // canonical points of the frame's clip
    float R[12];
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = rotmat[n * 9 + i];
#pragma unroll
    for (int i = 0; i < 3; ++i) R[9 + i] = obj_pred[n * 9 + 6 + i];
    const float *hv = human_verts + (size_t)n * V * HV;
    const size_t slot = (size_t)n * (nbO + nbH) + bx;
    float qx[CL_QPT], qy[CL_QPT], qz[CL_QPT], best[CL_QPT];
    int bi[CL_QPT];
    double acc[CG_G];
#pragma unroll
    for (int i = 0; i < CG_G; ++i) acc[i] = 0.0;
    float s = 0.f, c = 0.f;

    if (bx < nbO) {
        // ---------------------------------------------------------------- object -> human: exact argmin over the V vertices
        const int q0 = bx * CL_TILE + tid;
        float cx[CL_QPT], cy[CL_QPT], cz[CL_QPT];       // the canonical points: the p of the outer product
#pragma unroll
        for (int k = 0; k < CL_QPT; ++k) {
            const int i = q0 + CL_THR * k;
            cx[k] = cy[k] = cz[k] = 0.f;
            if (i < P) { cx[k] = op[(size_t)i * pstride]; cy[k] = op[(size_t)i * pstride + 1]; cz[k] = op[(size_t)i * pstride + 2]; }
            float3 p = make_float3(0.f, 0.f, 0.f);
            if (i < P) p = cl_pose(R, cx[k], cy[k], cz[k]);
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
#pragma unroll
        for (int k = 0; k < CL_QPT; ++k) {
            const int i = q0 + CL_THR * k;
            if (i < P) {
                const float *r = hv + (size_t)bi[k] * HV;
                const float vx = qx[k] - r[0], vy = qy[k] - r[1], vz = qz[k] - r[2];
                const float d = sqrtf(vx * vx + vy * vy + vz * vz);
                const float dt = r[3] * vx + r[4] * vy + r[5] * vz;          // sign(normal . vector), tools.py:58-61
                if (dt < 0.f && d > 0.f) {                                    // w = 20 where o2h_signed < 0 (:142-144)
                    s += d * 20.f;
                    c += 1.f;
                    cg_add(acc, 20.0, vx, vy, vz, cx[k], cy[k], cz[k]);
                }
            }
        }
    } else {
        // ---------------------------------------------------------------- human -> object: minimum AND index over the P posed points
        const int q0 = (bx - nbO) * CL_TILE + tid;
#pragma unroll
        for (int k = 0; k < CL_QPT; ++k) {
            const int i = q0 + CL_THR * k;
            const bool ok = i < V;
            qx[k] = ok ? hv[(size_t)i * HV] : 0.f; qy[k] = ok ? hv[(size_t)i * HV + 1] : 0.f; qz[k] = ok ? hv[(size_t)i * HV + 2] : 0.f;
            best[k] = FLT_MAX;
            bi[k] = 0;
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
                    if (d2 < best[k]) { best[k] = d2; bi[k] = c0 + j; }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < CL_QPT; ++k) {
            const int i = q0 + CL_THR * k;
            if (i < V) {
                const float d = sqrtf(best[k]);
                if (d > 0.02f && hv[(size_t)i * HV + 6] > 0.5f) {            // v_dist (:136)
                    s += d;
                    c += 1.f;
                    const float *r = op + (size_t)bi[k] * pstride;           // bi < P: the scan saw at least one point
                    const float px = r[0], py = r[1], pz = r[2];
                    const float3 y = cl_pose(R, px, py, pz);
                    cg_add(acc, -1.0, qx[k] - y.x, qy[k] - y.y, qz[k] - y.z, px, py, pz);
                }
            }
        }
    }
    __syncthreads();
    cg_block_sum(s, c, acc, redf, redd, partial + slot * 2, gpart + slot * CG_G);
}

__device__ __forceinline__ double cg_dot(const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
__device__ __forceinline__ void cg_cross(const double *a, const double *b, double *o) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

// block 0: the two term values (per-frame sums in workgroup order, frames strided over the threads, LDS tree: corr_finish_kernel's order);
// block 1 + k: frames 256 k .. 256 k + 255, one per thread
__global__ __launch_bounds__(CL_THR) void corr_geometry_grad_finish_kernel(const float *__restrict__ obj_pred, const float *__restrict__ partial,
                                                                           const double *__restrict__ gpart, int N, int nbO, int nbH, int V, int P, double w_pen,
                                                                           double w_con, float *__restrict__ d_obj_pred, float *__restrict__ terms2,
                                                                           float *__restrict__ out_frames) {
    __shared__ float sm[CL_THR];
    const int tid = threadIdx.x, nb = nbO + nbH;
    if (blockIdx.x == 0) {
        for (int term = 0; term < 2; ++term) {
            const int lo = term == 0 ? 0 : nbO, hi = term == 0 ? nbO : nb;
            float acc = 0.f;
            for (int n = tid; n < N; n += CL_THR) {
                float s = 0.f;
                for (int k = lo; k < hi; ++k) s += partial[((size_t)n * nb + k) * 2];
                acc += s;
            }
            const float tot = cl_tree(acc, sm);
            if (tid == 0) terms2[term] = tot / ((float)N * (float)(term == 0 ? P : V));
            __syncthreads();                             // (every thread has read sm[0] before the next term's tree writes it)
        }
        return;
    }
    const int n = (blockIdx.x - 1) * CL_THR + tid;
    if (n >= N) return;
    double G[CG_G];
#pragma unroll
    for (int i = 0; i < CG_G; ++i) G[i] = 0.0;
    float fs[2] = {0.f, 0.f}, fc[2] = {0.f, 0.f};
    for (int term = 0; term < 2; ++term) {
        const int lo = term == 0 ? 0 : nbO, hi = term == 0 ? nbO : nb;
        const double w = term == 0 ? w_pen / ((double)N * (double)P) : w_con / ((double)N * (double)V);
        double g[CG_G];
#pragma unroll
        for (int i = 0; i < CG_G; ++i) g[i] = 0.0;
        for (int k = lo; k < hi; ++k) {
            const size_t slot = (size_t)n * nb + k;
            fs[term] += partial[slot * 2];
            fc[term] += partial[slot * 2 + 1];
#pragma unroll
            for (int i = 0; i < CG_G; ++i) g[i] += gpart[slot * CG_G + i];
        }
#pragma unroll
        for (int i = 0; i < CG_G; ++i) G[i] += w * g[i];
    }
    if (out_frames) {
        out_frames[(size_t)n * 4] = fs[0];
        out_frames[(size_t)n * 4 + 1] = fs[1];
        out_frames[(size_t)n * 4 + 2] = fc[0];
        out_frames[(size_t)n * 4 + 3] = fc[1];
    }
    float *out = d_obj_pred + (size_t)n * 9;
    if (w_pen == 0.0 && w_con == 0.0) {                  // the terms are off: exact zeros whatever the partials hold
#pragma unroll
        for (int i = 0; i < 9; ++i) out[i] = 0.f;
        return;
    }
    // ---- Gram-Schmidt backward.  rows of M: b1, b2, b3; G[0..2] = dL/db1, G[3..5] = dL/db2, G[6..8] = dL/db3
    double a1[3], a2[3], b1[3], b2[3], cv[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) { a1[i] = (double)obj_pred[(size_t)n * 9 + i]; a2[i] = (double)obj_pred[(size_t)n * 9 + 3 + i]; }
    const double n1 = fmax(sqrt(cg_dot(a1, a1)), 1e-12);
#pragma unroll
    for (int i = 0; i < 3; ++i) b1[i] = a1[i] / n1;
    const double sp = cg_dot(b1, a2);
#pragma unroll
    for (int i = 0; i < 3; ++i) cv[i] = a2[i] - sp * b1[i];
    const double n2 = fmax(sqrt(cg_dot(cv, cv)), 1e-12);
#pragma unroll
    for (int i = 0; i < 3; ++i) b2[i] = cv[i] / n2;
    double db1[3] = {G[0], G[1], G[2]}, db2[3] = {G[3], G[4], G[5]}, db3[3] = {G[6], G[7], G[8]}, x1[3], x2[3], dc[3], da1[3], da2[3];
    cg_cross(b2, db3, x1);                               // b3 = b1 x b2
    cg_cross(db3, b1, x2);
#pragma unroll
    for (int i = 0; i < 3; ++i) { db1[i] += x1[i]; db2[i] += x2[i]; }
    const double p2 = cg_dot(b2, db2);
#pragma unroll
    for (int i = 0; i < 3; ++i) dc[i] = (db2[i] - b2[i] * p2) / n2;
    const double pc = cg_dot(b1, dc);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        da2[i] = dc[i] - b1[i] * pc;
        db1[i] += -sp * dc[i] - a2[i] * pc;
    }
    const double p1 = cg_dot(b1, db1);
#pragma unroll
    for (int i = 0; i < 3; ++i) da1[i] = (db1[i] - b1[i] * p1) / n1;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        out[i] = (float)da1[i];
        out[3 + i] = (float)da2[i];
        out[6 + i] = (float)G[9 + i];
    }
}

struct CgWs {
    size_t partial, gpart, d6, rotmat, total;
};
inline CgWs cg_ws(size_t N, size_t nb) {
    CgWs w{};
    w.partial = w.total; w.total += idf_align(N * nb * 2 * sizeof(float));
    w.gpart = w.total;   w.total += idf_align(N * nb * CG_G * sizeof(double));
    w.d6 = w.total;      w.total += idf_align(N * 6 * sizeof(float));
    w.rotmat = w.total;  w.total += idf_align(N * 9 * sizeof(float));
    return w;
}

}  // namespace

extern "C" size_t interdiff_correction_geometry_grads_workspace_bytes(int32_t T, int32_t B, int32_t V, int32_t P) {
    if (T <= 0 || B <= 0 || V <= 0 || P <= 0) return 0;
    return cg_ws((size_t)T * B, (size_t)idf_cdiv(P, CL_TILE) + (size_t)idf_cdiv(V, CL_TILE)).total;
}

extern "C" int interdiff_correction_geometry_grads(const float *obj_pred, const float *obj_points, int32_t point_stride, const float *human_verts, int32_t T,
                                                   int32_t B, int32_t V, int32_t P, double w_penetration, double w_contact, float *d_obj_pred_out,
                                                   float *terms2_out, float *frames_out, void *ws, size_t ws_bytes, void *stream) {
    if (!obj_pred || !obj_points || !human_verts || !d_obj_pred_out || !terms2_out || !ws) return IDF_E_INVAL;
    if (T <= 0 || B <= 0 || V <= 0 || P <= 0 || point_stride < 3) return IDF_E_INVAL;
    if ((int64_t)T * B > 65535) return IDF_E_INVAL;                           // frames ride on gridDim.y
    if (!(w_penetration >= 0.0 && w_penetration <= DBL_MAX) || !(w_contact >= 0.0 && w_contact <= DBL_MAX)) return IDF_E_INVAL;
    if (ws_bytes < interdiff_correction_geometry_grads_workspace_bytes(T, B, V, P)) return IDF_E_NOMEM;
    hipStream_t s = idf_stream(stream);
    const int nbO = (int)idf_cdiv(P, CL_TILE), nbH = (int)idf_cdiv(V, CL_TILE);
    const size_t N = (size_t)T * B;
    const CgWs W = cg_ws(N, (size_t)nbO + nbH);
    char *base = static_cast<char *>(ws);
    float *partial = reinterpret_cast<float *>(base + W.partial), *d6 = reinterpret_cast<float *>(base + W.d6), *rotmat = reinterpret_cast<float *>(base + W.rotmat);
    double *gpart = reinterpret_cast<double *>(base + W.gpart);
    // the per-frame matrices from the library's own rotation entry, as interdiff_correction_losses takes them: both passes pose the points from the same bits
    if (hipMemcpy2DAsync(d6, 6 * sizeof(float), obj_pred, 9 * sizeof(float), 6 * sizeof(float), N, hipMemcpyDeviceToDevice, s) != hipSuccess) return IDF_E_LAUNCH;
    const int rc = interdiff_rotation_6d_to_matrix(d6, rotmat, (int64_t)N, stream);
    if (rc != IDF_OK) return rc;
    hipLaunchKernelGGL(corr_geometry_grad_kernel, dim3((unsigned)(nbO + nbH), (unsigned)N), dim3(CL_THR), 0, s, obj_pred, obj_points, point_stride, human_verts,
                       rotmat, B, V, P, nbO, nbH, partial, gpart);
    IDF_CHECK_LAUNCH();
    hipLaunchKernelGGL(corr_geometry_grad_finish_kernel, dim3(1 + (unsigned)idf_cdiv(N, CL_THR)), dim3(CL_THR), 0, s, obj_pred, partial, gpart, (int)N, nbO, nbH,
                       V, P, w_penetration, w_contact, d_obj_pred_out, terms2_out, frames_out);
    IDF_CHECK_LAUNCH();
    return IDF_OK;
}
