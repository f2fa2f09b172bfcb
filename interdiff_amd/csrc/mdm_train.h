// Training of the SMPL denoiser's decoder: device code of the forward with saves, the backward of MDM.forward (model/diffusion_smpl.py:226-246: embedding,
// timestep MLP, [std, QaN x6, std] decoder layers, the two output heads) under the loss of LitInteraction.forward_backward (train_diffusion_smpl.py:60-166),
// and AdamW (:177-183); and of the encoder side, MDM._get_embeddings from pc_embedding on (:217-221), which runs the same sublayers on past_len tokens per clip.
// Launchers: csrc/mdm_train.hip; they take a geometry (csrc/mdm_train_stack.h) and also run the skeleton denoiser's stacks (csrc/skeleton_mdm_train.hip).
// Arithmetic: exact fp32 only -- every matrix product is v_mfma_f32_16x16x4_f32 (a k-ordered fp32 fma chain, four independent accumulators per wave), everything
// else VALU.  No f16 MFMA, so the exclusive-CU rule (common.h) puts no obligation on these kernels.  No float atomics: a sum across workgroups is a partial-slab store
// plus a fixed-order reducer (mt_colsum_*), every other sum is owned by one thread or one wave -- two calls give the same bits.
// Token rows are clip-major: row r = b * T + t of an [M = B*T, 256] matrix; memory rows are cond's own [S][B] order, row s * B + b.
#pragma once
#include "mdm_train_stack.h"                                      // the constants, the geometry (feed-forward and token widths) the launchers take

namespace mdmtrain {

// ------------------------------------------------------------------------------------------------------------------ GEMM
// C[M,N] = sum_k A(i,k) B(k,j) (+ bias[j]) (+ R[i,j]) with free strides on both operands, so one kernel is the NT product of a forward linear (Y = X W^T), the NN
// product dX = dY W and the transposed-operand product dW = dY^T X (A(i,k) = dY[k][i]): no transpose of an activation is ever materialised.
// One wave per workgroup, a 32 x 32 tile as 2 x 2 MFMA tiles (four independent accumulators), operands staged through LDS 16 k at a time with the unit-stride index
// on the lanes.  32 x 32 tiles make the 1024 x 256 weight gradients 256 workgroups.  R may alias C (each element is read and written by the same lane).
struct Gemm {
    const float *A;
    int64_t sam, sak;
    const float *B;
    int64_t sbk, sbn;
    float *C;
    int64_t ldc;
    const float *bias, *R;
    int64_t ldr;
    int M, N, K;
};

__global__ __launch_bounds__(64) void mt_gemm_kernel(const Gemm g) {
    __shared__ float As[32][17];
    __shared__ float Bs[16][33];
    const int lane = threadIdx.x, m0 = blockIdx.y * 32, n0 = blockIdx.x * 32;
    const bool a_k = g.sak == 1, b_k = g.sbk == 1;
    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < g.K; k0 += 16) {
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int e = lane + 64 * r;
            const int ai = a_k ? e >> 4 : e & 31, ak = a_k ? e & 15 : e >> 5;
            const int gm = m0 + ai, gk = k0 + ak;
            As[ai][ak] = (gm < g.M && gk < g.K) ? g.A[(int64_t)gm * g.sam + (int64_t)gk * g.sak] : 0.f;
            const int bn = b_k ? e >> 4 : e & 31, bk = b_k ? e & 15 : e >> 5;
            const int gn = n0 + bn, gk2 = k0 + bk;
            Bs[bk][bn] = (gn < g.N && gk2 < g.K) ? g.B[(int64_t)gk2 * g.sbk + (int64_t)gn * g.sbn] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const int k = kk * 4 + (lane >> 4), c = lane & 15;
            const float a0 = As[c][k], a1 = As[16 + c][k], b0 = Bs[k][c], b1 = Bs[k][16 + c];
            acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
        }
        __syncthreads();
    }
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int row = m0 + mi * 16 + (lane >> 4) * 4 + reg, col = n0 + ni * 16 + (lane & 15);
                if (row < g.M && col < g.N) {
                    float v = acc[mi][ni][reg];
                    if (g.bias) v += g.bias[col];
                    if (g.R) v += g.R[(int64_t)row * g.ldr + col];
                    g.C[(int64_t)row * g.ldc + col] = v;
                }
            }
}

// ------------------------------------------------------------------------------------------------ column sums over rows
// out[j] = sum_m A[m][j] (* Bm[m][j]): bias gradients, LayerNorm's d gamma / d beta, d wk.  Stage 1: a workgroup sums a slab of 64 rows x 64 columns (four row groups,
// added in order through LDS) and stores partial[slab][j]; stage 2 adds the slabs in ascending order.
__global__ __launch_bounds__(256) void mt_colsum_partial_kernel(const float *__restrict__ A, int64_t lda, const float *__restrict__ Bm, int64_t ldb, int M, int N,
                                                                float *__restrict__ partial) {
    __shared__ float part[4][64];
    const int c = threadIdx.x & 63, rg = threadIdx.x >> 6, col = blockIdx.x * 64 + c, slab = blockIdx.y;
    float s = 0.f;
    if (col < N)
        for (int i = 0; i < 16; ++i) {
            const int m = slab * 64 + rg * 16 + i;
            if (m < M) {
                const float a = A[(int64_t)m * lda + col];
                s += Bm ? a * Bm[(int64_t)m * ldb + col] : a;
            }
        }
    part[rg][c] = s;
    __syncthreads();
    if (rg == 0 && col < N) partial[(int64_t)slab * N + col] = ((part[0][c] + part[1][c]) + part[2][c]) + part[3][c];
}
__global__ __launch_bounds__(256) void mt_colsum_reduce_kernel(const float *__restrict__ partial, int slabs, int N, float *__restrict__ out) {
    const int col = blockIdx.x * 256 + threadIdx.x;
    if (col >= N) return;
    float s = 0.f;
    for (int i = 0; i < slabs; ++i) s += partial[(int64_t)i * N + col];
    out[col] = s;
}

// ---------------------------------------------------------------------------------------------------------- elementwise
__device__ __forceinline__ float mt_gelu(float z) { return 0.5f * z * (1.0f + erff(z * 0.70710678118654752440f)); }
__device__ __forceinline__ float mt_gelu_grad(float z) {
    return 0.5f * (1.0f + erff(z * 0.70710678118654752440f)) + z * 0.39894228040143267794f * expf(-0.5f * z * z);
}
__global__ __launch_bounds__(256) void mt_gelu_kernel(const float *__restrict__ z, float *__restrict__ g, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) g[i] = mt_gelu(z[i]);
}
__global__ __launch_bounds__(256) void mt_gelu_bwd_kernel(const float *__restrict__ z, float *__restrict__ dg, int64_t n) {      // dg <- dg * gelu'(z), in place
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dg[i] = dg[i] * mt_gelu_grad(z[i]);
}
__global__ __launch_bounds__(256) void mt_silu_kernel(const float *__restrict__ z, float *__restrict__ s, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) s[i] = z[i] / (1.0f + expf(-z[i]));
}
__global__ __launch_bounds__(256) void mt_silu_bwd_kernel(const float *__restrict__ z, float *__restrict__ ds, int64_t n) {      // ds <- ds * silu'(z), in place
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        const float sg = 1.0f / (1.0f + expf(-z[i]));
        ds[i] = ds[i] * (sg * (1.0f + z[i] * (1.0f - sg)));
    }
}
// [B][C][T] tokens <-> [B*T][C] rows, C channels per token
__global__ __launch_bounds__(256) void mt_tokens_to_rows_kernel(const float *__restrict__ x, float *__restrict__ rows, int B, int T, int C) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)B * T * C) return;
    const int c = (int)(i % C);
    const int64_t r = i / C;
    const int t = (int)(r % T), b = (int)(r / T);
    rows[i] = x[((int64_t)b * C + c) * T + t];
}
__global__ __launch_bounds__(256) void mt_rows_to_tokens_kernel(const float *__restrict__ rows, float *__restrict__ x, int B, int T, int C) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)B * T * C) return;
    const int t = (int)(i % T);
    const int64_t bc = i / T;
    const int c = (int)(bc % C), b = (int)(bc / C);
    x[i] = rows[((int64_t)b * T + t) * C + c];
}
// input of the timestep MLP: pe[ts[b]] (layers.py:42-43); a timestep outside the table must not read outside it
__global__ __launch_bounds__(256) void mt_gather_pe_kernel(const float *__restrict__ pe, int pe_rows, const int64_t *__restrict__ ts, float *__restrict__ out) {
    int64_t t = ts[blockIdx.x];
    t = t < 0 ? 0 : (t >= pe_rows ? pe_rows - 1 : t);
    out[(int64_t)blockIdx.x * D + threadIdx.x] = pe[t * D + threadIdx.x];
}
// h[r] += temb[b] + pe[t].  Second use: the encoder's input embedding, with pc_embedding [B][256] as temb and T = past_len (diffusion_smpl.py:219-220)
__global__ __launch_bounds__(256) void mt_add_temb_pe_kernel(float *__restrict__ h, const float *__restrict__ temb, const float *__restrict__ pe, int T) {
    const int r = blockIdx.x, b = r / T, t = r % T, c = threadIdx.x;
    h[(int64_t)r * D + c] = (h[(int64_t)r * D + c] + temb[(int64_t)b * D + c]) + pe[(int64_t)t * D + c];
}
// d temb[b] = sum_t d h[b*T + t], frames in ascending order.  Second use: d pc_embedding[b] = the encoder's d embedding summed over a clip's past_len tokens
__global__ __launch_bounds__(256) void mt_sum_frames_kernel(const float *__restrict__ dh, float *__restrict__ out, int T) {
    const int b = blockIdx.x, c = threadIdx.x;
    float s = 0.f;
    for (int t = 0; t < T; ++t) s += dh[((int64_t)b * T + t) * D + c];
    out[(int64_t)b * D + c] = s;
}
// the QaN layer's tgt + (x - tgt) (sublayers.py:338-339 with stochastic depth at rate 0): kept as the reference rounds it; its backward is the identity on x
__global__ __launch_bounds__(256) void mt_round_trip_kernel(const float *__restrict__ tgt, const float *__restrict__ x, float *__restrict__ out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        const float d = x[i] - tgt[i];
        out[i] = tgt[i] + d;
    }
}

// ------------------------------------------------------------------------------------------------------------ LayerNorm
// one wave per 256-wide row (four values per lane).  Forward leaves the normalised row and 1 / sigma for the backward.
__global__ __launch_bounds__(256) void mt_ln_fwd_kernel(const float *__restrict__ s, const float *__restrict__ gamma, const float *__restrict__ beta, float *__restrict__ xhat,
                                                        float *__restrict__ rstd, float *__restrict__ y, int M) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= M) return;
    const float4 v = *reinterpret_cast<const float4 *>(s + (int64_t)r * D + lane * 4);
    const float mean = wave_sum((v.x + v.y) + (v.z + v.w)) * (1.0f / D);
    const float a = v.x - mean, b = v.y - mean, c = v.z - mean, d = v.w - mean;
    const float var = wave_sum((a * a + b * b) + (c * c + d * d)) * (1.0f / D);
    const float rs = 1.0f / sqrtf(var + LN_EPS);
    const float4 g = *reinterpret_cast<const float4 *>(gamma + lane * 4), be = *reinterpret_cast<const float4 *>(beta + lane * 4);
    const float4 xh = make_float4(a * rs, b * rs, c * rs, d * rs);
    *reinterpret_cast<float4 *>(xhat + (int64_t)r * D + lane * 4) = xh;
    *reinterpret_cast<float4 *>(y + (int64_t)r * D + lane * 4) = make_float4(xh.x * g.x + be.x, xh.y * g.y + be.y, xh.z * g.z + be.z, xh.w * g.w + be.w);
    if (lane == 0) rstd[r] = rs;
}
// dx = rstd (g - mean(g) - xhat mean(g xhat)), g = dy gamma
__global__ __launch_bounds__(256) void mt_ln_bwd_kernel(const float *__restrict__ dy, const float *__restrict__ xhat, const float *__restrict__ rstd,
                                                        const float *__restrict__ gamma, float *__restrict__ dx, int M) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= M) return;
    const float4 d = *reinterpret_cast<const float4 *>(dy + (int64_t)r * D + lane * 4), xh = *reinterpret_cast<const float4 *>(xhat + (int64_t)r * D + lane * 4);
    const float4 ga = *reinterpret_cast<const float4 *>(gamma + lane * 4);
    const float g0 = d.x * ga.x, g1 = d.y * ga.y, g2 = d.z * ga.z, g3 = d.w * ga.w;
    const float m1 = wave_sum((g0 + g1) + (g2 + g3)) * (1.0f / D);
    const float m2 = wave_sum((g0 * xh.x + g1 * xh.y) + (g2 * xh.z + g3 * xh.w)) * (1.0f / D);
    const float rs = rstd[r];
    *reinterpret_cast<float4 *>(dx + (int64_t)r * D + lane * 4) =
        make_float4(rs * ((g0 - m1) - xh.x * m2), rs * ((g1 - m1) - xh.y * m2), rs * ((g2 - m1) - xh.z * m2), rs * ((g3 - m1) - xh.w * m2));
}

// ------------------------------------------------------------------------------------------- self-attention (layers 0, 7)
// One workgroup per (clip, head), T <= 128, thread i owns query row i.  qkv [M][768] = q | k | v, head h in columns h*64 ..; logits q.k / 8.
// Forward: K and V of the head in LDS, online softmax; leaves o (head-concatenated, before out_proj) and the per-row log-sum-exp.
__global__ __launch_bounds__(128) void mt_self_attn_fwd_kernel(const float *__restrict__ qkv, float *__restrict__ o, float *__restrict__ lse, int T) {
    extern __shared__ float mt_sm[];
    float *Ks = mt_sm, *Vs = mt_sm + T * HD;
    const int b = blockIdx.x >> 2, h = blockIdx.x & 3, tid = threadIdx.x;
    const float *base = qkv + (int64_t)b * T * 768 + h * HD;
    for (int e = tid; e < T * HD; e += 128) {
        const int j = e >> 6, d = e & 63;
        Ks[e] = base[(int64_t)j * 768 + 256 + d];
        Vs[e] = base[(int64_t)j * 768 + 512 + d];
    }
    __syncthreads();
    if (tid >= T) return;
    float q[HD], acc[HD];
#pragma unroll
    for (int d = 0; d < HD; ++d) { q[d] = base[(int64_t)tid * 768 + d]; acc[d] = 0.f; }
    float mx = -INFINITY, l = 0.f;
    for (int j = 0; j < T; ++j) {
        float s = 0.f;
#pragma unroll
        for (int d = 0; d < HD; ++d) s += q[d] * Ks[j * HD + d];
        s *= 0.125f;
        const float mn = fmaxf(mx, s), sc = expf(mx - mn), p = expf(s - mn);
        l = l * sc + p;
#pragma unroll
        for (int d = 0; d < HD; ++d) acc[d] = acc[d] * sc + p * Vs[j * HD + d];
        mx = mn;
    }
    const float inv = 1.0f / l;
    float *orow = o + ((int64_t)b * T + tid) * D + h * HD;
#pragma unroll
    for (int d = 0; d < HD; ++d) orow[d] = acc[d] * inv;
    lse[((int64_t)b * HEADS + h) * T + tid] = mx + logf(l);
}
// Backward, five products with P recomputed from the stored log-sum-exp.  Phase 1 (thread i = query row): S, P, dP = dO V^T, dS = P (dP - rowsum(dO o)) / 8,
// dq_i = sum_j dS_ij k_j; P and dS of this (clip, head) go to a [T][T] scratch.  Phase 2 (thread j = key row): dv_j = sum_i P_ij dO_i, dk_j = sum_i dS_ij q_i with
// Q and dO in LDS.  Every sum is owned by one thread, rows in ascending order.  dqkv [M][768] = dq | dk | dv.
__global__ __launch_bounds__(128) void mt_self_attn_bwd_kernel(const float *__restrict__ qkv, const float *__restrict__ o, const float *__restrict__ lse,
                                                               const float *__restrict__ dO, float *__restrict__ dqkv, float *__restrict__ Pbuf, float *__restrict__ dSbuf,
                                                               int T) {
    extern __shared__ float mt_sm[];
    float *Ks = mt_sm, *Vs = mt_sm + T * HD;
    const int b = blockIdx.x >> 2, h = blockIdx.x & 3, tid = threadIdx.x;
    const float *base = qkv + (int64_t)b * T * 768 + h * HD;
    const float *dob = dO + (int64_t)b * T * D + h * HD;
    float *P = Pbuf + (int64_t)blockIdx.x * T * T, *dS = dSbuf + (int64_t)blockIdx.x * T * T;
    for (int e = tid; e < T * HD; e += 128) {
        const int j = e >> 6, d = e & 63;
        Ks[e] = base[(int64_t)j * 768 + 256 + d];
        Vs[e] = base[(int64_t)j * 768 + 512 + d];
    }
    __syncthreads();
    if (tid < T) {
        float q[HD], g[HD], dq[HD];
        const float *orow = o + ((int64_t)b * T + tid) * D + h * HD;
        float delta = 0.f;
#pragma unroll
        for (int d = 0; d < HD; ++d) {
            q[d] = base[(int64_t)tid * 768 + d];
            g[d] = dob[(int64_t)tid * D + d];
            dq[d] = 0.f;
            delta += g[d] * orow[d];
        }
        const float L = lse[((int64_t)b * HEADS + h) * T + tid];
        for (int j = 0; j < T; ++j) {
            float s = 0.f, dp = 0.f;
#pragma unroll
            for (int d = 0; d < HD; ++d) { s += q[d] * Ks[j * HD + d]; dp += g[d] * Vs[j * HD + d]; }
            const float p = expf(s * 0.125f - L), ds = p * (dp - delta) * 0.125f;
#pragma unroll
            for (int d = 0; d < HD; ++d) dq[d] += ds * Ks[j * HD + d];
            P[tid * T + j] = p;
            dS[tid * T + j] = ds;
        }
        float *dqrow = dqkv + ((int64_t)b * T + tid) * 768 + h * HD;
#pragma unroll
        for (int d = 0; d < HD; ++d) dqrow[d] = dq[d];
    }
    __threadfence_block();
    __syncthreads();
    for (int e = tid; e < T * HD; e += 128) {                    // Q and dO take the place of K and V
        const int j = e >> 6, d = e & 63;
        Ks[e] = base[(int64_t)j * 768 + d];
        Vs[e] = dob[(int64_t)j * D + d];
    }
    __syncthreads();
    if (tid < T) {
        float dk[HD], dv[HD];
#pragma unroll
        for (int d = 0; d < HD; ++d) dk[d] = dv[d] = 0.f;
        for (int i = 0; i < T; ++i) {
            const float p = P[i * T + tid], ds = dS[i * T + tid];
#pragma unroll
            for (int d = 0; d < HD; ++d) { dk[d] += ds * Ks[i * HD + d]; dv[d] += p * Vs[i * HD + d]; }
        }
        float *row = dqkv + ((int64_t)b * T + tid) * 768 + h * HD;
#pragma unroll
        for (int d = 0; d < HD; ++d) { row[256 + d] = dk[d]; row[512 + d] = dv[d]; }
    }
}

// ---------------------------------------------------------------------------------------------------- cross-attention
// S <= 16 memory rows.  One thread per (token row, head); q [M][256], kv [S*B][512] = k | v of the memory, row s*B + b.  The slot loops are unrolled to MAX_MEM
// with a guard so that the logits stay in registers.
__device__ __forceinline__ void mt_cross_probs(const float *q, const float *__restrict__ kv, int b, int B, int h, int S, float *p) {
    float mx = -INFINITY;
#pragma unroll
    for (int s = 0; s < MAX_MEM; ++s) {
        p[s] = -INFINITY;
        if (s < S) {
            const float *k = kv + ((int64_t)s * B + b) * 512 + h * HD;
            float a = 0.f;
#pragma unroll
            for (int d = 0; d < HD; ++d) a += q[d] * k[d];
            p[s] = a * 0.125f;
            mx = fmaxf(mx, p[s]);
        }
    }
    float l = 0.f;
#pragma unroll
    for (int s = 0; s < MAX_MEM; ++s) {
        p[s] = s < S ? expf(p[s] - mx) : 0.f;
        l += p[s];
    }
    const float inv = 1.0f / l;
#pragma unroll
    for (int s = 0; s < MAX_MEM; ++s) p[s] *= inv;
}
__global__ __launch_bounds__(256) void mt_cross_attn_fwd_kernel(const float *__restrict__ q2, const float *__restrict__ kv, float *__restrict__ o, int B, int T, int S) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= B * T * HEADS) return;
    const int r = idx >> 2, h = idx & 3, b = r / T;
    float q[HD], p[MAX_MEM], acc[HD];
#pragma unroll
    for (int d = 0; d < HD; ++d) { q[d] = q2[(int64_t)r * D + h * HD + d]; acc[d] = 0.f; }
    mt_cross_probs(q, kv, b, B, h, S, p);
#pragma unroll
    for (int s = 0; s < MAX_MEM; ++s)
        if (s < S) {
            const float *v = kv + ((int64_t)s * B + b) * 512 + 256 + h * HD;
#pragma unroll
            for (int d = 0; d < HD; ++d) acc[d] += p[s] * v[d];
        }
#pragma unroll
    for (int d = 0; d < HD; ++d) o[(int64_t)r * D + h * HD + d] = acc[d];
}
// backward, token side: probabilities recomputed; dq, and P / dS [M][4][MAX_MEM] for the memory side
__global__ __launch_bounds__(256) void mt_cross_attn_bwd_q_kernel(const float *__restrict__ q2, const float *__restrict__ kv, const float *__restrict__ dO,
                                                                  float *__restrict__ dq, float *__restrict__ Pc, float *__restrict__ dSc, int B, int T, int S) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= B * T * HEADS) return;
    const int r = idx >> 2, h = idx & 3, b = r / T;
    float q[HD], g[HD], p[MAX_MEM], dp[MAX_MEM], acc[HD];
#pragma unroll
    for (int d = 0; d < HD; ++d) { q[d] = q2[(int64_t)r * D + h * HD + d]; g[d] = dO[(int64_t)r * D + h * HD + d]; acc[d] = 0.f; }
    mt_cross_probs(q, kv, b, B, h, S, p);
    float delta = 0.f;
#pragma unroll
    for (int s = 0; s < MAX_MEM; ++s) {
        dp[s] = 0.f;
        if (s < S) {
            const float *v = kv + ((int64_t)s * B + b) * 512 + 256 + h * HD;
            float a = 0.f;
#pragma unroll
            for (int d = 0; d < HD; ++d) a += g[d] * v[d];
            dp[s] = a;
            delta += p[s] * a;
        }
    }
#pragma unroll
    for (int s = 0; s < MAX_MEM; ++s) {
        const float ds = s < S ? p[s] * (dp[s] - delta) * 0.125f : 0.f;
        Pc[(int64_t)idx * MAX_MEM + s] = p[s];
        dSc[(int64_t)idx * MAX_MEM + s] = ds;
        if (s < S) {
            const float *k = kv + ((int64_t)s * B + b) * 512 + h * HD;
#pragma unroll
            for (int d = 0; d < HD; ++d) acc[d] += ds * k[d];
        }
    }
#pragma unroll
    for (int d = 0; d < HD; ++d) dq[(int64_t)r * D + h * HD + d] = acc[d];
}
// backward, memory side: dkv[s*B + b][c] = sum_t dS q (c < 256) | sum_t P dO (c >= 256), frames in ascending order
__global__ __launch_bounds__(256) void mt_cross_attn_bwd_kv_kernel(const float *__restrict__ q2, const float *__restrict__ dO, const float *__restrict__ Pc,
                                                                   const float *__restrict__ dSc, float *__restrict__ dkv, int B, int T, int S) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= S * B * 512) return;
    const int c = idx & 511, sb = idx >> 9, b = sb % B, s = sb / B, col = c & 255, h = col >> 6;
    const float *w = c < 256 ? dSc : Pc, *x = c < 256 ? q2 : dO;
    float a = 0.f;
    for (int t = 0; t < T; ++t) {
        const int64_t r = (int64_t)b * T + t;
        a += w[(r * HEADS + h) * MAX_MEM + s] * x[r * D + col];
    }
    dkv[idx] = a;
}

// ------------------------------------------------------------------------------------------------------------ QaN block
// sublayers.py:343-352 around LocalAttention (window 1, look +-1): token t has three key slots j = 0..2 = frames t-1, t, t+1 of its clip (a slot outside the clip is masked),
// NQ learned queries n, logits sim[n][j] = (R_2 qs_n) . (R_j x_{t-1+j}) with R_p the rotary rotation at position p (keys by slot, the query by the LAST row) and
// qs_n = queries[n] per head / (|.| + 1e-6) / sqrt(64) * 256^-1/2.  R_j^T R_2 = R_{2-j}, so sim[n][j] = G[n][j] . x_{t-1+j} with the per-layer constant
// G[n][j] = R_{2-j} qs_n; out_t = sum_j c_j x_{t-1+j}, c_j = sum_n wk[n] softmax_j(sim[n])[j].
__device__ __forceinline__ float mt_rot_inv_freq(int d) { return powf(10000.0f, -(float)(2 * (d & 127)) / 256.0f); }
// G [NQ][SLOTS][256] from queries [NQ][256]: one workgroup per query
__global__ __launch_bounds__(256) void mt_qan_prep_kernel(const float *__restrict__ queries, float *__restrict__ G) {
    __shared__ float sq[D], qs[D];
    const int n = blockIdx.x, d = threadIdx.x;
    const float q = queries[n * D + d];
    sq[d] = q * q;
    __syncthreads();
    float nn = 0.f;
    for (int i = 0; i < HD; ++i) nn += sq[(d & ~63) + i];
    qs[d] = q / (sqrtf(nn) + 1e-6f) * (0.125f * 0.0625f);
    __syncthreads();
    const float f = mt_rot_inv_freq(d);
    for (int j = 0; j < SLOTS; ++j) {
        const float a = (float)(2 - j) * f, c = cosf(a), s = sinf(a);
        const float v = d < 128 ? qs[d] * c - qs[d + 128] * s : qs[d] * c + qs[d - 128] * s;
        G[(n * SLOTS + j) * D + d] = v;
    }
}
// per-token attention weights (all lanes of the wave hold the same values); xv[j] = this lane's four values of the slot's frame (zero when masked)
__device__ __forceinline__ void mt_qan_attn(const float *__restrict__ G, const float4 *xv, const bool *valid, int lane, float attn[NQ][SLOTS]) {
#pragma unroll
    for (int n = 0; n < NQ; ++n) {
        float sim[SLOTS], mx = -INFINITY;
#pragma unroll
        for (int j = 0; j < SLOTS; ++j) {
            const float4 g = *reinterpret_cast<const float4 *>(G + (n * SLOTS + j) * D + lane * 4);
            sim[j] = wave_sum((g.x * xv[j].x + g.y * xv[j].y) + (g.z * xv[j].z + g.w * xv[j].w));
            if (valid[j]) mx = fmaxf(mx, sim[j]);
        }
        float l = 0.f;
#pragma unroll
        for (int j = 0; j < SLOTS; ++j) {
            attn[n][j] = valid[j] ? expf(sim[j] - mx) : 0.f;
            l += attn[n][j];
        }
        const float inv = 1.0f / l;
#pragma unroll
        for (int j = 0; j < SLOTS; ++j) attn[n][j] *= inv;
    }
}
__device__ __forceinline__ void mt_qan_slots(const float *__restrict__ x, int r, int T, int lane, float4 *xv, bool *valid) {
    const int t = r % T;
#pragma unroll
    for (int j = 0; j < SLOTS; ++j) {
        valid[j] = t - 1 + j >= 0 && t - 1 + j < T;
        xv[j] = valid[j] ? *reinterpret_cast<const float4 *>(x + (int64_t)(r - 1 + j) * D + lane * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}
// forward: s1[r] = x[r] + block(x)[r], one wave per token
__global__ __launch_bounds__(256) void mt_qan_fwd_kernel(const float *__restrict__ x, const float *__restrict__ G, const float *__restrict__ wk, float *__restrict__ s1, int M,
                                                         int T) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= M) return;
    float4 xv[SLOTS];
    bool valid[SLOTS];
    float attn[NQ][SLOTS];
    mt_qan_slots(x, r, T, lane, xv, valid);
    mt_qan_attn(G, xv, valid, lane, attn);
    float4 out = xv[1];
    float4 blk = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int j = 0; j < SLOTS; ++j) {
        float c = 0.f;
#pragma unroll
        for (int n = 0; n < NQ; ++n) c += wk[n] * attn[n][j];
        blk.x += c * xv[j].x; blk.y += c * xv[j].y; blk.z += c * xv[j].z; blk.w += c * xv[j].w;
    }
    out.x += blk.x; out.y += blk.y; out.z += blk.z; out.w += blk.w;
    *reinterpret_cast<float4 *>(s1 + (int64_t)r * D + lane * 4) = out;
}
// backward, per token t (one wave): with d = d block[t]:  dc_j = d . x_{t-1+j};  d attn[n][j] = wk[n] dc_j;  dsim = softmax backward;  d wk[n] (this token's
// share) = sum_j attn[n][j] dc_j.  Leaves dsim [M][NQ][SLOTS], c [M][SLOTS] and dwk_tok [M][NQ] for the gather kernel, the d G products and the column sum.
__global__ __launch_bounds__(256) void mt_qan_bwd_token_kernel(const float *__restrict__ x, const float *__restrict__ G, const float *__restrict__ wk,
                                                               const float *__restrict__ dblk, float *__restrict__ dsim, float *__restrict__ cj, float *__restrict__ dwk_tok,
                                                               int M, int T) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= M) return;
    float4 xv[SLOTS];
    bool valid[SLOTS];
    float attn[NQ][SLOTS], dc[SLOTS];
    mt_qan_slots(x, r, T, lane, xv, valid);
    mt_qan_attn(G, xv, valid, lane, attn);
    const float4 d = *reinterpret_cast<const float4 *>(dblk + (int64_t)r * D + lane * 4);
#pragma unroll
    for (int j = 0; j < SLOTS; ++j) dc[j] = wave_sum((d.x * xv[j].x + d.y * xv[j].y) + (d.z * xv[j].z + d.w * xv[j].w));
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < SLOTS; ++j) {
            float c = 0.f;
#pragma unroll
            for (int n = 0; n < NQ; ++n) c += wk[n] * attn[n][j];
            cj[(int64_t)r * SLOTS + j] = c;
        }
#pragma unroll
        for (int n = 0; n < NQ; ++n) {
            const float w = wk[n];
            float dot = 0.f, dw = 0.f;
#pragma unroll
            for (int j = 0; j < SLOTS; ++j) { dot += attn[n][j] * (w * dc[j]); dw += attn[n][j] * dc[j]; }
#pragma unroll
            for (int j = 0; j < SLOTS; ++j) dsim[((int64_t)r * NQ + n) * SLOTS + j] = attn[n][j] * (w * dc[j] - dot);
            dwk_tok[(int64_t)r * NQ + n] = dw;
        }
    }
}
// backward, gather per frame u (one wave): dx[u] = d s1[u] (the residual) + sum_j over the tokens t = u + 1 - j of u's clip that see u in slot j:
// c_j(t) d block[t] (value role) + sum_n dsim[t][n][j] G[n][j] (key role)
__global__ __launch_bounds__(256) void mt_qan_bwd_gather_kernel(const float *__restrict__ ds1, const float *__restrict__ G, const float *__restrict__ dsim,
                                                                const float *__restrict__ cj, float *__restrict__ dx, int M, int T) {
    const int u = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (u >= M) return;
    const int tu = u % T;
    float4 acc = *reinterpret_cast<const float4 *>(ds1 + (int64_t)u * D + lane * 4);
#pragma unroll
    for (int j = 0; j < SLOTS; ++j) {
        const int tt = tu + 1 - j;
        if (tt < 0 || tt >= T) continue;
        const int64_t t = (int64_t)u + 1 - j;
        const float c = cj[t * SLOTS + j];
        const float4 d = *reinterpret_cast<const float4 *>(ds1 + t * D + lane * 4);
        acc.x += c * d.x; acc.y += c * d.y; acc.z += c * d.z; acc.w += c * d.w;
        for (int n = 0; n < NQ; ++n) {
            const float w = dsim[(t * NQ + n) * SLOTS + j];
            const float4 g = *reinterpret_cast<const float4 *>(G + (n * SLOTS + j) * D + lane * 4);
            acc.x += w * g.x; acc.y += w * g.y; acc.z += w * g.z; acc.w += w * g.w;
        }
    }
    *reinterpret_cast<float4 *>(dx + (int64_t)u * D + lane * 4) = acc;
}
// d queries [NQ][256] from dG [SLOTS][NQ][256] (the three transposed-operand products): d qs_n = sum_j R_{2-j}^T dG[j][n], then the per-head normalisation
// y = alpha q / (|q| + 1e-6):  dq = alpha (dy / (r + eps) - q (dy . q) / ((r + eps)^2 r)).  One workgroup per query.
__global__ __launch_bounds__(256) void mt_qan_dqueries_kernel(const float *__restrict__ queries, const float *__restrict__ dG, float *__restrict__ dqueries) {
    __shared__ float sq[D], sdot[D];
    const int n = blockIdx.x, d = threadIdx.x;
    const float f = mt_rot_inv_freq(d);
    float dy = 0.f;
    for (int j = 0; j < SLOTS; ++j) {
        const float a = (float)(2 - j) * f, c = cosf(a), s = sinf(a);
        const float *g = dG + ((int64_t)j * NQ + n) * D;
        dy += d < 128 ? g[d] * c + g[d + 128] * s : g[d] * c - g[d - 128] * s;
    }
    const float q = queries[n * D + d];
    sq[d] = q * q;
    sdot[d] = dy * q;
    __syncthreads();
    float nn = 0.f, dot = 0.f;
    for (int i = 0; i < HD; ++i) { nn += sq[(d & ~63) + i]; dot += sdot[(d & ~63) + i]; }
    const float r = sqrtf(nn), re = r + 1e-6f, alpha = 0.125f * 0.0625f;
    dqueries[n * D + d] = alpha * (dy / re - q * dot / (re * re * r));
}

// ---------------------------------------------------------------------------------------------------------- loss gradient
// d/d pred of mean_b sum_i w_i term_i[b] for the 16 terms of csrc/losses.hip denoising_losses_kernel, as the reference writes them (:91-115): the ground-truth operand of
// every velocity term is identically zero, so each _v_ term is an MSE of first differences (frames 1..P | P..T-1) plus an MSE of the second-difference form
// e_u = 2 x_u - x_{u-1} - x_{u+1} (u = 1..P-1 | P..T-2).  One thread per element, a handful of neighbours in t.
struct Weights16 {
    float w[16];
};
__global__ __launch_bounds__(256) void mt_loss_grad_kernel(const float *__restrict__ pred, const float *__restrict__ target, int B, int T, int P, const Weights16 W,
                                                           float *__restrict__ dpred) {
    constexpr int CTOK = SMPL_GEOM.ctok;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)B * CTOK * T) return;
    const int t = (int)(i % T), c = (int)((i / T) % CTOK);
    const int g = c < 132 ? 0 : c < 135 ? 1 : c < 141 ? 2 : 3;
    const float feat = g == 0 ? 132.f : g == 2 ? 6.f : 3.f;
    const float *x = pred + (i - t);
    const float xt = x[t];
    const float a_val = t < P ? W.w[g] / ((float)P * feat) : W.w[8 + g] / ((float)(T - P) * feat);
    const float a1p = W.w[4 + g] / ((float)P * feat), a1f = W.w[12 + g] / ((float)(T - P) * feat);
    const float a2p = W.w[4 + g] / ((float)(P - 1) * feat), a2f = W.w[12 + g] / ((float)(T - P - 1) * feat);
    float acc = a_val * (xt - target[i]);
    if (t >= 1) {                                                 // first differences that end at t
        const float d = xt - x[t - 1];
        if (t <= P) acc += a1p * d;
        if (t >= P) acc += a1f * d;
    }
    if (t + 1 < T) {                                              // ... and the one that starts at t
        const float d = x[t + 1] - xt;
        if (t + 1 <= P) acc -= a1p * d;
        if (t + 1 >= P) acc -= a1f * d;
    }
    auto coef = [&](int u) { return (u >= 1 && u <= P - 1) ? a2p : (u >= P && u <= T - 2) ? a2f : 0.f; };
    auto e = [&](int u) { return 2.f * x[u] - x[u - 1] - x[u + 1]; };       // only called where coef(u) != 0: 1 <= u <= T-2
    const float c0 = coef(t), cm = coef(t - 1), cp = coef(t + 1);
    if (c0 != 0.f) acc += 2.f * c0 * e(t);
    if (cm != 0.f) acc -= cm * e(t - 1);
    if (cp != 0.f) acc -= cp * e(t + 1);
    dpred[i] = 2.f * acc / (float)B;
}

// ---------------------------------------------------------------------------------------------- encoder (_get_embeddings)
// The encoder's token input is the past frames of x_start: rows[b*S + s][c] = target[b][c][s] of a [B][C][T] tensor (clip-major rows, like the decoder's).
__global__ __launch_bounds__(256) void mt_gather_past_kernel(const float *__restrict__ target, float *__restrict__ rows, int B, int T, int S, int C) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)B * S * C) return;
    const int c = (int)(i % C);
    const int64_t r = i / C;
    const int s = (int)(r % S), b = (int)(r / S);
    rows[i] = target[((int64_t)b * C + c) * T + s];
}
// [P][Q] rows of 256 -> [Q][P]: the encoder's clip-major output to cond's [S][B] order, and d_cond back
__global__ __launch_bounds__(256) void mt_swap_rows_kernel(const float *__restrict__ in, float *__restrict__ out, int P, int Q) {
    const int r = blockIdx.x, p = r / Q, q = r % Q, c = threadIdx.x;
    out[((int64_t)q * P + p) * D + c] = in[(int64_t)r * D + c];
}
// dst[i] = dst[i] + src[i]: the encoder path's gradient of the shared bodyEmbedding / objEmbedding added to the decoder path's, in that order
__global__ __launch_bounds__(256) void mt_add_into_kernel(float *__restrict__ dst, const float *__restrict__ src, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = dst[i] + src[i];
}

// ------------------------------------------------------------------------------------------------------------------ AdamW
// torch.optim.AdamW (_single_tensor_adamw): p *= 1 - lr wd; exp_avg.lerp_(g, 1 - beta1); exp_avg_sq = beta2 exp_avg_sq + (1 - beta2) g^2;
// denom = sqrt(exp_avg_sq) / sqrt(1 - beta2^step) + eps; p += -(lr / (1 - beta1^step)) exp_avg / denom
struct AdamWK {
    float decay, w1, beta2, w2, step_size, bc2_sqrt, eps;
};
__global__ __launch_bounds__(256) void mt_adamw_kernel(float *__restrict__ p, const float *__restrict__ grad, float *__restrict__ m, float *__restrict__ v, int64_t n,
                                                       const AdamWK k) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float g = grad[i];
    float pi = p[i] * k.decay, mi = m[i], vi = v[i];
    mi = mi + k.w1 * (g - mi);
    vi = vi * k.beta2 + k.w2 * g * g;
    const float denom = sqrtf(vi) / k.bc2_sqrt + k.eps;
    m[i] = mi;
    v[i] = vi;
    p[i] = pi + (-k.step_size) * (mi / denom);
}

}  // namespace mdmtrain
