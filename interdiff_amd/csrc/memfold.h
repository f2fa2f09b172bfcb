// Per-sample folding of the cross-attention memory (interdiff_mdm_prepare_memory): cond [mem_len][B][256] (the encoder's frame-major output) is projected once per
// sample and folded with every layer's query / output weights, so that the row block computes scores = x.G^T + g0 and out = P.VW (rowblock.h, which also lists the
// fragment orders written here).  Result: memctx, in the column layout MemLay<MS> (denoiser_common.h), carved by memctx_carve below.
#pragma once
#include "rowblock.h"

namespace {

// kv[l][r][c] = cond[r][:] . Wkv_l[c][:] + bkv_l[c];  r = m*B + b (reference layout [mem_len,B,D]), c < 512
__global__ __launch_bounds__(256) void mem_kv_kernel(const float *__restrict__ arena, const idf_mdm_weights w,
                                                     const float *__restrict__ cond, int R, float *__restrict__ kv) {
    const int l = blockIdx.z, r = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
    __shared__ float xr[D];
    xr[threadIdx.x] = cond[(size_t)r * D + threadIdx.x];
    __syncthreads();
    const float *Wr = arena + w.layer[l].ca_kv_w + (size_t)c * D;
    float s = 0.f;
    for (int k = 0; k < D; k += 4) {
        const float4 wv = *reinterpret_cast<const float4 *>(Wr + k);
        s += xr[k] * wv.x + xr[k + 1] * wv.y + xr[k + 2] * wv.z + xr[k + 3] * wv.w;
    }
    kv[((size_t)l * R + r) * 512 + c] = s + arena[w.layer[l].ca_kv_b + c];
}

// fragment order of the fp32 forms (see G_FRAG): the reader's lane is kq * 16 + li; NCT = column tiles of the layout (MemLay)
template <int NCT>
__device__ __forceinline__ int g_slot(int col, int k) {            // score column col (0 .. 16 NCT - 1), feature k (0..255)
    const int ks = k >> 4, kq = (k >> 2) & 3, e = k & 3, ct = col >> 4, li = col & 15;
    return ((ks * NCT + ct) * 64 + kq * 16 + li) * 4 + e;
}
template <int NCT>
__device__ __forceinline__ int vw_slot(int o, int col) {           // output feature o (0..255), probability column col (0 .. 16 NCT - 1)
    const int wave = o >> 6, c = (o >> 4) & 3, li = o & 15, sidx = col >> 4, kq = (col >> 2) & 3, e = col & 3;
    return (((wave * NCT + sidx) * 4 + c) * 64 + kq * 16 + li) * 4 + e;
}

// G[l][b][h*MEM+m][i] = 1/8 sum_d Wq[h*64+d][i] K[m,b][h*64+d];  g0 = 1/8 sum_d bq[h*64+d] K[..]
// VWT[l][b][o][h*MEM+m] = sum_d V[m,b][h*64+d] Wo[o][h*64+d]   (columns 40..47 zero)
// grid (H * mem_len, B, L), 256 threads (thread = i / o).  Generic layout (MS == MEMX): the buffers were zeroed by the caller, only the columns of present slots are written.
template <int MS>
__global__ __launch_bounds__(256) void mem_fold_kernel(const float *__restrict__ arena, const idf_mdm_weights w,
                                                       const float *__restrict__ kv, int B, float *__restrict__ G,
                                                       float *__restrict__ g0, float *__restrict__ VWT, int mem_len) {
    using ML = MemLay<MS>;
    const int mlen = ML::GEN ? mem_len : MEM;
    const int hm = blockIdx.x, b = blockIdx.y, l = blockIdx.z, h = hm / mlen, m = hm - h * mlen, i = threadIdx.x, col = ML::col(h, m);
    __shared__ float kd[HD], vd[HD];
    const float *row = kv + ((size_t)l * (mlen * B) + (size_t)m * B + b) * 512;
    if (i < HD) kd[i] = row[h * HD + i];
    else if (i < 2 * HD) vd[i - HD] = row[D + h * HD + (i - HD)];
    __syncthreads();
    const float *Wq = arena + w.layer[l].ca_q_w, *bq = arena + w.layer[l].ca_q_b, *Wo = arena + w.layer[l].ca_out_w;
    float sg = 0.f, sv = 0.f;
    for (int d = 0; d < HD; ++d) {
        sg += Wq[(size_t)(h * HD + d) * D + i] * kd[d];
        sv += vd[d] * Wo[(size_t)i * D + h * HD + d];
    }
    float *Gf = G + ((size_t)l * B + b) * ML::G_FRAG, *Vf = VWT + ((size_t)l * B + b) * ML::VWT_F;
    Gf[g_slot<ML::NCT>(col, i)] = sg * 0.125f;
    Vf[vw_slot<ML::NCT>(i, col)] = sv;
    if (!ML::GEN && hm < HMP - HM) {
        Gf[g_slot<ML::NCT>(HM + hm, i)] = 0.f;
        Vf[vw_slot<ML::NCT>(i, HM + hm)] = 0.f;
    }
    if (i == 0) {
        float s = 0.f;
        for (int d = 0; d < HD; ++d) s += bq[h * HD + d] * kd[d];
        g0[((size_t)l * B + b) * ML::G0N + col] = s * 0.125f;
    }
}

// The folded memory as split-f16 plane fragments (rowblock_kernel<.., H2>; layouts at G_H2).  Its values are data (encoder output folded with
// weights), so each (layer, clip) matrix is divided by a power of two that puts its largest magnitude in [2^13, 2^14) -- exact, the f16 pair then keeps
// 22 bits of every element down to 2^-27 of the largest -- and the row block multiplies the fp32 result back (sc[l][b] = {2^eG, 2^eV}).
// grid (B, L), 256 threads; once per sample.
template <int MS>
__global__ __launch_bounds__(256) void mem_fold_h2_kernel(const float *__restrict__ G, const float *__restrict__ VWT, int B,
                                                          float *__restrict__ Gh2, float *__restrict__ VWh2, float *__restrict__ sc) {
    using ML = MemLay<MS>;
    constexpr int NCT = ML::NCT, HMPX = ML::HMPX;
    const int b = blockIdx.x, l = blockIdx.y, tid = threadIdx.x;
    const float *Gf = G + ((size_t)l * B + b) * ML::G_FRAG, *Vf = VWT + ((size_t)l * B + b) * ML::VWT_F;
    __shared__ float red[2][256];
    float ag = 0.f, av = 0.f;
    for (int i = tid; i < ML::G_FRAG; i += 256) ag = fmaxf(ag, fabsf(Gf[i]));
    for (int i = tid; i < ML::VWT_F; i += 256) av = fmaxf(av, fabsf(Vf[i]));
    red[0][tid] = ag;
    red[1][tid] = av;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st) {
            red[0][tid] = fmaxf(red[0][tid], red[0][tid + st]);
            red[1][tid] = fmaxf(red[1][tid], red[1][tid + st]);
        }
        __syncthreads();
    }
    // amax 2^-e in [2^13, 2^14); a matrix of zeros (or non-finite values, which then stay what they are) is left alone
    const int eg = (red[0][0] > 0.f && red[0][0] < INFINITY) ? ilogbf(red[0][0]) - 13 : 0, ev = (red[1][0] > 0.f && red[1][0] < INFINITY) ? ilogbf(red[1][0]) - 13 : 0;
    const float dg = ldexpf(1.0f, -eg), dv = ldexpf(1.0f, -ev);
    float *Go = Gh2 + ((size_t)l * B + b) * ML::G_H2, *Vo = VWh2 + ((size_t)l * B + b) * VW_H2;
    for (int it = tid; it < 4 * 2 * NCT * 64; it += 256) {
        const int lane = it & 63, ct = (it >> 6) % NCT, s2 = (it / (64 * NCT)) & 1, wv = it / (128 * NCT), kq = lane >> 4, li = lane & 15;
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = Gf[g_slot<NCT>(16 * ct + li, 64 * wv + 32 * s2 + 8 * kq + e)] * dg;
        uint2 h0, l0, h1, l1;
        idf_ffn_h2::split4(make_float4(v[0], v[1], v[2], v[3]), h0, l0);
        idf_ffn_h2::split4(make_float4(v[4], v[5], v[6], v[7]), h1, l1);
        uint4 *dst = reinterpret_cast<uint4 *>(Go) + (((wv * 2 + s2) * NCT + ct) * 2) * 64 + lane;
        dst[0] = make_uint4(h0.x, h0.y, h1.x, h1.y);
        dst[64] = make_uint4(l0.x, l0.y, l1.x, l1.y);
    }
    for (int it = tid; it < 4 * 2 * 4 * 64; it += 256) {
        const int lane = it & 63, c = (it >> 6) & 3, s2 = (it >> 8) & 1, wv = it >> 9, kq = lane >> 4, li = lane & 15;
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int col = 32 * s2 + 8 * kq + e;
            v[e] = col < HMPX ? Vf[vw_slot<NCT>(64 * wv + 16 * c + li, min(col, HMPX - 1))] * dv : 0.f;
        }
        uint2 h0, l0, h1, l1;
        idf_ffn_h2::split4(make_float4(v[0], v[1], v[2], v[3]), h0, l0);
        idf_ffn_h2::split4(make_float4(v[4], v[5], v[6], v[7]), h1, l1);
        uint4 *dst = reinterpret_cast<uint4 *>(Vo) + (((wv * 2 + s2) * 4 + c) * 2) * 64 + lane;
        dst[0] = make_uint4(h0.x, h0.y, h1.x, h1.y);
        dst[64] = make_uint4(l0.x, l0.y, l1.x, l1.y);
    }
    if (tid == 0) {
        sc[((size_t)l * B + b) * 2] = ldexpf(1.0f, eg);
        sc[((size_t)l * B + b) * 2 + 1] = ldexpf(1.0f, ev);
    }
}

// memctx: G | VWT | g0 (fp32 forms) | G planes | VWT planes | scales (split-f16 forms, always folded: the arithmetic is chosen per forward)
struct MemCtx {
    const float *G, *VWT, *g0, *Gh2, *VWh2, *sc;
};
template <int MS>
static inline MemCtx memctx_carve(const float *m, int B) {
    using ML = MemLay<MS>;
    MemCtx c;
    c.G = m;
    c.VWT = c.G + (size_t)L * B * ML::G_FRAG;
    c.g0 = c.VWT + (size_t)L * B * ML::VWT_F;
    c.Gh2 = c.g0 + (size_t)L * B * ML::G0N;
    c.VWh2 = c.Gh2 + (size_t)L * B * ML::G_H2;
    c.sc = c.VWh2 + (size_t)L * B * VW_H2;
    return c;
}
template <int MS>
static inline size_t memctx_floats_t(int32_t B) {
    using ML = MemLay<MS>;
    return (size_t)L * B * (ML::G_FRAG + ML::VWT_F + ML::G0N + ML::G_H2 + VW_H2 + 2);
}
// memory length of a handle: w->mem_len (0 = the default IDF_MDM_MEM); the compact layout serves exactly IDF_MDM_MEM, the generic one every 1 .. IDF_MDM_MEM_MAX
static inline int idf_mem_len(const idf_mdm_weights *w) { return w->mem_len ? w->mem_len : MEM; }

template <int MS>
int prepare_memory_t(const idf_mdm_weights *w, const float *cond, int32_t B, float *memctx, void *ws, size_t ws_bytes, hipStream_t s) {
    const int mlen = idf_mem_len(w);
    if (ws_bytes < (size_t)L * mlen * B * 512 * sizeof(float)) return IDF_E_NOMEM;
    float *kv = reinterpret_cast<float *>(ws);
    const MemCtx mc = memctx_carve<MS>(memctx, B);
    float *G = const_cast<float *>(mc.G), *VWT = const_cast<float *>(mc.VWT), *g0 = const_cast<float *>(mc.g0);
    idf_prof_mark(IDF_K_MEM_PREP, s);
    if (MemLay<MS>::GEN) {       // generic layout: only the columns of present slots are written below
        if (hipMemsetAsync(memctx, 0, memctx_floats_t<MS>(B) * sizeof(float), s) != hipSuccess) return IDF_E_LAUNCH;
    }
    hipLaunchKernelGGL(mem_kv_kernel, dim3(2, mlen * B, L), dim3(256), 0, s, w->arena, *w, cond, mlen * B, kv);
    hipLaunchKernelGGL(mem_fold_kernel<MS>, dim3(H * mlen, B, L), dim3(256), 0, s, w->arena, *w, kv, B, G, g0, VWT, mlen);
    hipLaunchKernelGGL(mem_fold_h2_kernel<MS>, dim3(B, L), dim3(256), 0, s, G, VWT, B, const_cast<float *>(mc.Gh2), const_cast<float *>(mc.VWh2), const_cast<float *>(mc.sc));
    idf_prof_mark(-1, s);
    IDF_CHECK_LAUNCH();
    return IDF_OK;
}
}  // namespace
