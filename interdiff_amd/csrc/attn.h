// Temporal self-attention of the two standard layers on the fp32 MFMA: softmax(Q K^T / 8) V per (clip, head), with the head's slice of the out-projection -- the exact
// form, and what runs where attn_h2.h's split-f16 kernel does not (clips beyond its LDS budget, a device where it does not get its CU).  qkv [N][768] in (row = b*T + t),
// H partial slabs [N][256] out, which the row block sums.  self_attn_kernel: a clip's K and V in LDS (T <= ATTN_MAX_T), grid (ceil(T/QT), H, B) flattened, 256 threads,
// LDS: K,V [TP][68], Q [QT][68], S [QT][TP+4]; TP = T rounded up to 16, QT = 16 or 32 query rows.  self_attn_tiled_kernel: 64-key tiles, any longer clip.
#pragma once
#include <float.h>
#include "denoiser_common.h"

#ifndef IDF_AT_STAMP
#define IDF_AT_STAMP(i) do { } while (0)        // phase stamps exist only in tools/rowblock_probe.hip (which defines the macro before including denoiser.hip)
#endif

namespace {

constexpr int AS = HD + 4;            // row stride (floats) of the V image: its P.V operand reads are scalar (4 k rows x 16 columns per instruction: 68 keeps the four 16-lane groups on disjoint banks)
constexpr int SPAD = 8;               // padding of a score row (floats)
constexpr int ASK = HD + 8;           // row stride of the Q and K images: their S = Q K^T operands are ds_read_b128 of lane (li, kq) -> row li, slot s0 + kq, and a stride of 2 slots mod 16
                                      // makes those conflict-free (see the row block's HS; round 4 used 68 for all three: every Q / K fragment read took twice its LDS cycles)
constexpr int ATTN_MAX_T = 208;
constexpr int ATTN_RT = 1;            // 16-query tiles per workgroup of the fused attention + out-projection kernel

// OUTPROJ: the workgroup also multiplies its [32 x 64] context tile with its head's 64 rows of W_o^T (K = 64, wave w owns output
// columns [64w, 64w+64)) and writes a [32 x 256] PARTIAL of the out-projection into slab `head` of `slabs`; the row block that follows
// sums the H slabs + residual + bias (one launch, one kernel boundary and the ctx round trip less than a separate GEMM).
// wo_frag: this layer's W_o in fragment order [head][wave][k-group of 16][column tile][lane][4] (mdm.py sa_out_fragments).
// RT: 16-query tiles per workgroup (grid.x = ceil(T / (16 RT))).  RT = 1 halves a workgroup's LDS image (73 KB at T = 100), so that two
// workgroups share a CU and one's loads / softmax run beside the other's MFMA phases.
template <bool OUTPROJ, int RT>
__global__ __launch_bounds__(256) void self_attn_kernel(const float *__restrict__ qkv, float *__restrict__ ctx, int T, int nwg,
                                                        const float *__restrict__ wo_frag, float *__restrict__ slabs, size_t pstride) {
    // 1-D grid of nwg = ceil(T / QT) * H * B workgroups; all twelve argument dwords arrive preloaded in SGPRs (build.py): no argument-segment read, no gridDim
    extern __shared__ __attribute__((aligned(16))) float smx[];
    IDF_AT_STAMP(0);
    const int TP = (T + 15) & ~15, SS = TP + SPAD;       // (TP + 8: the same 2-slots-mod-16 rule for the P.V A-operand reads of the score rows)
    constexpr int QT = 16 * RT;
    float *Ks = smx, *Vs = Ks + TP * ASK, *Qs = Vs + TP * AS, *Ss = Qs + QT * ASK;
    const int xq = nwg >> 3, xr = nwg & 7, xcd = (int)blockIdx.x & 7;                   // XCD-affine logical id (xcd_logical_id)
    const int lid = (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + ((int)blockIdx.x >> 3);
    const int nqt = (T + QT - 1) / QT, b = lid / (nqt * H), h = (lid / nqt) % H, q0 = (lid % nqt) * QT, tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6, li = lane & 15, kq = lane >> 4;
    const size_t rowbase = (size_t)b * T;
    // Operand fetch, all requests of a batch in flight together: clamped (always valid) addresses, no guard around a load -- a guarded
    // load inside a run-time loop costs one full memory round trip per iteration (7 at T = 100).  TP * 16 is a multiple of 256, so a
    // sweep `it` covers key rows 16 it .. 16 it + 15 for the whole workgroup; 8 sweeps per batch (T <= 128: one batch).
    float4 qreg[RT];
#pragma unroll
    for (int u = 0; u < RT; ++u) {
        const int i = tid + 256 * u, r = i >> 4, d4 = (i & 15) * 4;
        qreg[u] = ld4(qkv + (rowbase + min(q0 + r, T - 1)) * (3 * D) + h * HD + d4);
    }
    const int nsweep = TP >> 4;
    for (int it0 = 0; it0 < nsweep; it0 += 8) {
        float4 kreg[8], vreg[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = tid + 256 * (it0 + u), j = i >> 4, d4 = (i & 15) * 4;
            const float *src = qkv + (rowbase + min(j, T - 1)) * (3 * D) + h * HD + d4;
            kreg[u] = ld4(src + D);
            vreg[u] = ld4(src + 2 * D);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = tid + 256 * (it0 + u), j = i >> 4, d4 = (i & 15) * 4;
            if (it0 + u < nsweep) {                                    // workgroup-uniform
                *reinterpret_cast<float4 *>(Ks + j * ASK + d4) = j < T ? kreg[u] : zero4();
                *reinterpret_cast<float4 *>(Vs + j * AS + d4) = j < T ? vreg[u] : zero4();
            }
        }
    }
    float4 wo[4][4];                                     // out-projection fragments: requested now (behind K / V, pinned), consumed after P V
    if constexpr (OUTPROJ) {
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int sidx = 0; sidx < 4; ++sidx)
#pragma unroll
            for (int c = 0; c < 4; ++c) wo[sidx][c] = ld4(wo_frag + ((((size_t)(h * 4 + wave) * 4 + sidx) * 4 + c) * 64 + lane) * 4);
    }
#pragma unroll
    for (int u = 0; u < RT; ++u) {
        const int i = tid + 256 * u, r = i >> 4, d4 = (i & 15) * 4;
        *reinterpret_cast<float4 *>(Qs + r * ASK + d4) = q0 + r < T ? qreg[u] : zero4();
    }
    __syncthreads();
    IDF_AT_STAMP(1);                                     // K, V, Q in LDS
    // S = Q K^T / 8: wave w owns key tiles w, w+4, ... for both 16-query tiles
    for (int ct = wave; ct < TP / 16; ct += 4) {
        f32x4 acc[RT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) acc[rt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < HD / 16; ++s) {
            const int koff = 16 * s + 4 * kq;
            const float4 kv = ld4(Ks + (ct * 16 + li) * ASK + koff);
            float4 a[RT], bb[RT];
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) { a[rt] = ld4(Qs + (rt * 16 + li) * ASK + koff); bb[rt] = kv; }
            mma_rounds<RT>(acc, a, bb);
        }
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int r = 0; r < 4; ++r) Ss[(rt * 16 + kq * 4 + r) * SS + ct * 16 + li] = acc[rt][r] * 0.125f;
    }
    __syncthreads();
    IDF_AT_STAMP(2);                                     // S = Q K^T
    {   // row softmax: one 16-lane group per row, 16 rows per sweep; lane l16 owns columns l16, 16+l16, ... and keeps them in
        // registers between the max, the exp/sum and the normalisation (one LDS read and one write per element; three run-time loops
        // over LDS took 7.2 k of the kernel's 19 k cycles)
        constexpr int NC = ATTN_MAX_T / 16, NC0 = 8;     // columns per lane at the longest clip; the first NC0 cover T <= 128
        const int ncol = TP >> 4;
        const bool tail = ncol > NC0;                    // workgroup-uniform: ONE branch around the columns past 128
        for (int i = wave * 4 + kq; i < QT; i += 16) {
            float *row = Ss + i * SS;
            float v[NC], mx = -FLT_MAX;
            // reads are unconditional with clamped addresses (a guard per column makes the compiler wait for every read separately)
#pragma unroll
            for (int c = 0; c < NC0; ++c) {
                const int j = 16 * c + li;
                v[c] = row[min(j, TP - 1)];
                v[c] = j < T ? v[c] : -FLT_MAX;
            }
            if (tail) {
#pragma unroll
                for (int c = NC0; c < NC; ++c) {
                    const int j = 16 * c + li;
                    v[c] = row[min(j, TP - 1)];
                    v[c] = j < T ? v[c] : -FLT_MAX;
                }
            } else {
#pragma unroll
                for (int c = NC0; c < NC; ++c) v[c] = -FLT_MAX;
            }
#pragma unroll
            for (int c = 0; c < NC; ++c) mx = fmaxf(mx, v[c]);
            mx = row16_max(mx);
            float sum = 0.f;
#pragma unroll
            for (int c = 0; c < NC0; ++c) {
                v[c] = 16 * c + li < T ? __expf(v[c] - mx) : 0.f;
                sum += v[c];
            }
            if (tail) {
#pragma unroll
                for (int c = NC0; c < NC; ++c) {
                    v[c] = 16 * c + li < T ? __expf(v[c] - mx) : 0.f;
                    sum += v[c];
                }
            }
            const float inv = __builtin_amdgcn_rcpf(row16_sum(sum));
#pragma unroll
            for (int c = 0; c < NC0; ++c)
                if (16 * c + li < TP) row[16 * c + li] = v[c] * inv;
            if (tail) {
#pragma unroll
                for (int c = NC0; c < NC; ++c)
                    if (16 * c + li < TP) row[16 * c + li] = v[c] * inv;
            }
        }
    }
    __syncthreads();
    IDF_AT_STAMP(3);                                     // softmax
    {   // ctx = P V: wave w owns the 16 head-dim columns [16w, 16w+16) for both query tiles
        f32x4 acc[RT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) acc[rt] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int dcol = wave * 16 + li;
        for (int s = 0; s < TP / 16; ++s) {
            const int koff = 16 * s + 4 * kq;
            const float *vp = Vs + koff * AS + dcol;
            const float4 vv = make_float4(vp[0], vp[AS], vp[2 * AS], vp[3 * AS]);
            float4 a[RT], bb[RT];
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) { a[rt] = ld4(Ss + (rt * 16 + li) * SS + koff); bb[rt] = vv; }
            mma_rounds<RT>(acc, a, bb);
        }
        if constexpr (!OUTPROJ) {
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int t = q0 + rt * 16 + kq * 4 + r;
                    if (t < T) idf_store4_wt(ctx + (rowbase + t) * D + h * HD + dcol, acc[rt][r]);
                }
        } else {
            // context tile -> LDS in A-operand (row-major) form; the Q image is dead since the S phase
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int r = 0; r < 4; ++r) Qs[(rt * 16 + kq * 4 + r) * ASK + dcol] = acc[rt][r];
        }
    }
    IDF_AT_STAMP(4);                                     // P V (+ store)
    if constexpr (OUTPROJ) {
        __syncthreads();
        IDF_AT_STAMP(7);                                 // (probe) context tile in LDS, every wave there
        f32x4 o[4 * RT];
#pragma unroll
        for (int i = 0; i < 4 * RT; ++i) o[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int sidx = 0; sidx < 4; ++sidx) {
            const int koff = 16 * sidx + 4 * kq;
            float4 a[4 * RT], bb[4 * RT];
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                const float4 av = ld4(Qs + (rt * 16 + li) * ASK + koff);
#pragma unroll
                for (int c = 0; c < 4; ++c) { a[rt * 4 + c] = av; bb[rt * 4 + c] = wo[sidx][c]; }
            }
            mma_rounds<4 * RT>(o, a, bb);
        }
        IDF_AT_STAMP(6);                                 // (probe) out-projection MFMAs issued
        float *slab = slabs + (size_t)h * pstride;
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int t = q0 + rt * 16 + kq * 4 + r;
                if (t < T) {
#pragma unroll
                    for (int c = 0; c < 4; ++c) idf_store4_wt(slab + (rowbase + t) * D + (wave * 4 + c) * 16 + li, o[rt * 4 + c][r]);
                }
            }
        IDF_AT_STAMP(5);                                 // out-projection partial + store
    }
}

// ------------------------------------------------------------------------------------
// Clips longer than ATTN_MAX_T frames: the same attention with K / V streamed through LDS in tiles of 64 keys and a running row maximum / sum
// ("flash" form), fp32 MFMA, the out-projection partial in its tail like self_attn_kernel<true, 1>.  The one-shot kernel parks K and V of a whole
// (clip, head) in LDS (149 KiB at T = 208); the reference's own bound is its positional table, PositionalEncoding(max_len = 5000) (model/layers.py:10).
// A correct path for every length the table allows, not a tuned one: per key tile four barriers and one pass over S; the shipped shapes never take it.
// grid (ceil(T/16), H, B), 256 threads; static LDS ~45 KiB.
// ------------------------------------------------------------------------------------
constexpr int KT = 64;                       // keys per tile
__global__ __launch_bounds__(256) void self_attn_tiled_kernel(const float *__restrict__ qkv, int T, const float *__restrict__ wo_frag,
                                                              float *__restrict__ slabs, size_t pstride) {
    __shared__ __attribute__((aligned(16))) float Ks[KT * ASK], Vs[KT * AS], Qs[16 * ASK], Ss[16 * (KT + 8)];
    __shared__ float m_run[16], l_run[16], alpha[16];
    constexpr int SS = KT + 8;
    idf_args_now(qkv, T, wo_frag, slabs, pstride, gridDim.x);
    const int lid = xcd_logical_id(), nqt = gridDim.x, b = lid / (nqt * H), h = (lid / nqt) % H, q0 = (lid % nqt) * 16, tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6, li = lane & 15, kq = lane >> 4;
    const size_t rowbase = (size_t)b * T;
    float4 wo[4][4];
#pragma unroll
    for (int sidx = 0; sidx < 4; ++sidx)
#pragma unroll
        for (int c = 0; c < 4; ++c) wo[sidx][c] = ld4(wo_frag + ((((size_t)(h * 4 + wave) * 4 + sidx) * 4 + c) * 64 + lane) * 4);
    {   // the 16 query rows (zero past the clip), running statistics
        const int r = tid >> 4, d4 = (tid & 15) * 4;
        const float4 qv = ld4(qkv + (rowbase + min(q0 + r, T - 1)) * (3 * D) + h * HD + d4);
        *reinterpret_cast<float4 *>(Qs + r * ASK + d4) = q0 + r < T ? qv : zero4();
        if (tid < 16) { m_run[tid] = -FLT_MAX; l_run[tid] = 0.f; }
    }
    f32x4 o_acc = {0.f, 0.f, 0.f, 0.f};                  // O[16 queries][16 head-dim columns of this wave]: lane (li = column, kq) holds rows 4 kq .. 4 kq + 3
    const int dcol = wave * 16 + li;
    for (int k0 = 0; k0 < T; k0 += KT) {
        __syncthreads();                                 // the previous tile's P.V reads of Ks / Vs / Ss are done (first pass: Qs, statistics written)
#pragma unroll
        for (int u = 0; u < KT / 16; ++u) {
            const int i = tid + 256 * u, j = i >> 4, d4 = (i & 15) * 4;
            const float *src = qkv + (rowbase + min(k0 + j, T - 1)) * (3 * D) + h * HD + d4;
            const float4 kv = ld4(src + D), vv = ld4(src + 2 * D);
            *reinterpret_cast<float4 *>(Ks + j * ASK + d4) = k0 + j < T ? kv : zero4();
            *reinterpret_cast<float4 *>(Vs + j * AS + d4) = k0 + j < T ? vv : zero4();
        }
        __syncthreads();
        {   // S tile = Q K^T / 8: wave w owns key tile w of the four
            f32x4 acc[1] = {{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
            for (int sg = 0; sg < HD / 16; ++sg) {
                const int koff = 16 * sg + 4 * kq;
                const float4 a[1] = {ld4(Qs + li * ASK + koff)}, bb[1] = {ld4(Ks + (wave * 16 + li) * ASK + koff)};
                mma_rounds<1>(acc, a, bb);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) Ss[(kq * 4 + r) * SS + wave * 16 + li] = k0 + wave * 16 + li < T ? acc[0][r] * 0.125f : -FLT_MAX;
        }
        __syncthreads();
        {   // running softmax: the 16-lane group of row i holds columns li, 16 + li, 32 + li, 48 + li of the tile
            const int i = wave * 4 + kq;
            float *row = Ss + i * SS;
            float v[4], mx = -FLT_MAX;
#pragma unroll
            for (int c = 0; c < 4; ++c) { v[c] = row[16 * c + li]; mx = fmaxf(mx, v[c]); }
            mx = row16_max(mx);
            const float m_old = m_run[i], m_new = fmaxf(m_old, mx);
            float sum = 0.f;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                v[c] = k0 + 16 * c + li < T ? __expf(v[c] - m_new) : 0.f;
                sum += v[c];
                row[16 * c + li] = v[c];
            }
            sum = row16_sum(sum);
            if (li == 0) {
                const float al = __expf(m_old - m_new);     // first tile: exp(-FLT_MAX - m) = 0
                alpha[i] = al;
                l_run[i] = l_run[i] * al + sum;
                m_run[i] = m_new;
            }
        }
        __syncthreads();
        {   // O = O alpha + P V
#pragma unroll
            for (int r = 0; r < 4; ++r) o_acc[r] *= alpha[kq * 4 + r];
            f32x4 acc[1] = {o_acc};
#pragma unroll
            for (int sg = 0; sg < KT / 16; ++sg) {
                const int koff = 16 * sg + 4 * kq;
                const float *vp = Vs + koff * AS + dcol;
                const float4 a[1] = {ld4(Ss + li * SS + koff)}, bb[1] = {make_float4(vp[0], vp[AS], vp[2 * AS], vp[3 * AS])};
                mma_rounds<1>(acc, a, bb);
            }
            o_acc = acc[0];
        }
    }
    __syncthreads();                                     // every wave is past its reads of Qs (S phase of the last tile)
#pragma unroll
    for (int r = 0; r < 4; ++r) Qs[(kq * 4 + r) * ASK + dcol] = o_acc[r] * __builtin_amdgcn_rcpf(l_run[kq * 4 + r]);       // context tile, A-operand (row-major) form
    __syncthreads();
    f32x4 o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int sidx = 0; sidx < 4; ++sidx) {
        const float4 av = ld4(Qs + li * ASK + 16 * sidx + 4 * kq);
        const float4 a[4] = {av, av, av, av};
        mma_rounds<4>(o, a, wo[sidx]);
    }
    float *slab = slabs + (size_t)h * pstride;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int t = q0 + kq * 4 + r;
        if (t < T) {
#pragma unroll
            for (int c = 0; c < 4; ++c) idf_store4_wt(slab + (rowbase + t) * D + (wave * 4 + c) * 16 + li, o[c][r]);
        }
    }
}

inline size_t attn_lds_bytes(int T, int rt) {
    const int TP = (T + 15) & ~15;
    return ((size_t)TP * (ASK + AS) + 16 * rt * ASK + 16 * rt * (TP + SPAD)) * sizeof(float);
}
// self_attn_kernel needs more than 64 KiB of dynamic LDS for long clips: per-device opt-in (common.h)
int attn_opt_in() {
    static std::atomic<uint64_t> lds_ok{0};
    return idf_opt_in_lds(reinterpret_cast<const void *>(self_attn_kernel<true, ATTN_RT>), (int)attn_lds_bytes(ATTN_MAX_T, ATTN_RT), lds_ok);
}

// self-attention + out-projection partials of one standard layer: the one-shot kernel up to ATTN_MAX_T frames, the K/V-tiled one beyond
inline void launch_self_attn_outproj(hipStream_t s, const float *qkv, int B, int T, const float *wo_frag, float *parts, size_t pstride) {
    if (T <= ATTN_MAX_T)
        hipLaunchKernelGGL((self_attn_kernel<true, ATTN_RT>), dim3((unsigned)(idf_cdiv(T, 16 * ATTN_RT) * H * B)), dim3(256), attn_lds_bytes(T, ATTN_RT), s, qkv, nullptr, T,
                           (int)(idf_cdiv(T, 16 * ATTN_RT) * H * B), wo_frag, parts, pstride);
    else
        hipLaunchKernelGGL(self_attn_tiled_kernel, dim3((unsigned)idf_cdiv(T, 16), H, B), dim3(256), 0, s, qkv, T, wo_frag, parts, pstride);
}

}  // namespace
