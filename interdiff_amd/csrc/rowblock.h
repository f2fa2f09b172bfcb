// Row block shared by QaN layers and standard layers -- everything between two feed-forward blocks in ONE launch, 16 (or 8) tokens of one clip per workgroup:
//   [QAN]  x = LN_prev(u_in rows t-1 .. t+16);  logits[t][n][j] = <Qc[n][j], x[t+j-1]>  (MFMA, K split over waves)
//          u1 = x_t + sum_j c_j(t) x_{t+j-1},  c_j = sum_n wk[n] softmax_j(logits[t][n][:])
//   [!QAN] u1 = u_in row  (+ sa_resid row + sa_bias: the slabs are the self-attention's out-projection partials)
//   x1 = LN1(u1);  scores = x1.G^T + g0 (MFMA);  P = softmax per head;  u2 = x1 + P.VW + b_out (MFMA)      [CROSS; G / g0 / VW: the folded memory of memfold.h]
//   x2 = LN2(u2)  -> HBM (the FFN input AND its residual)
// u_in: NP partial slabs [N][256] u_pstride floats apart, rows clip-major (row = b*T + t).  rowblock_kernel: grid (ceil(T/16), B), 256 threads -- the exact fp32-MFMA
// form and, with H2, round 4's split-f16 form; rowblock8_kernel: eight waves, the shipped split-f16 form.  The launchers, the route between the forms and the
// exclusive-CU checks of the split-f16 ones are at the end of this file.
#pragma once
#include <float.h>
#include "denoiser_common.h"

#ifndef IDF_RB_STAMP
#define IDF_RB_STAMP(i) do { } while (0)        // phase stamps exist only in tools/rowblock_probe.hip (which defines the macro before including denoiser.hip)
#endif

namespace {

constexpr int TR = 16;
// MFMA B-operand fragments of the row block are stored IN FRAGMENT ORDER -- [wave = K quarter][k-group of 16][tile][lane][4 floats] --
// so that one wave load instruction reads 1 KiB contiguous (8 cache lines).  Fetched from the row-major matrices the same
// instruction gathered sixteen 64-byte pieces, and the kernel spent 5.9 k of its 20 k cycles just ISSUING its first batch of
// requests (tools/rowblock_probe.hip): the vector memory pipe handles about one line request every two cycles.
//   Qc  (weights, mdm.py qan_fragments):      [4][4][3 taps][4 kq][NQ][4]: only lanes li < NQ fetch (logit columns >= NQ are never read)
//   G   (per sample, mem_fold_kernel):        [4][4][3 column tiles][64][4], column = 16 ct + li of the 40 (head, slot) pairs (+8 zero)
//   VWT (per sample, mem_fold_kernel):        [4 waves = output column quarter][3 k-groups][4 tiles][64][4]
//   (sizes per (layer, clip): MemLay<MS>::G_FRAG / G_H2 / VWT_F -- 12288 / 12288 / 12288 floats in the compact layout)
// split-f16 forms (rowblock_kernel<.., H2>): 16-byte plane fragments = the v_mfma_f32_16x16x32_f16 operand of a lane (8 halves, k = 8 kq .. 8 kq + 7 of a K = 32 step)
//   Qc  (mdm.py qan_fragments_h2):            [4 waves = K quarter][2 K steps][3 taps][2 planes][4 kq][NQ][8 halves]
//   G   (mem_fold_h2_kernel):                 [4 waves = K quarter][2 K steps][3 column tiles][2 planes][64 lanes][8 halves], values divided by 2^e
//   VWT (mem_fold_h2_kernel):                 [4 waves = output column quarter][2 K steps (probability columns 0..63, zero from 40)][4 tiles][2 planes][64][8 halves]
constexpr int VW_H2 = 4 * 2 * 4 * 2 * 64 * 4;  // 16384 floats
constexpr int RS = D + 4;             // LDS row stride of token rows (floats)

// H2 (decoder layers, tune[IDF_TUNE_FFN_MATH] == 1 and the packer's range proof): the three contractions on the f16 matrix pipe with every fp32
// operand as two f16 planes (ffn_h2.h: v = hi + lo' 2^-11, three v_mfma_f32_16x16x32_f16 per product, fp32 accumulate).  48 fp32 MFMAs of 32 cycles per
// wave and contraction -- 1 536 of the ~2 000 cycles each of those three phases took -- become 18 / 18 / 24 of 16.  Qc / G / VWT then point at the
// plane fragments (mdm.py qan_fragments_h2; mem_fold_h2_kernel) and h2_scale[b][2] holds the powers of two that G[b] / VW[b] were divided by.
// Token rows need no scaling: they are LayerNorm outputs, bounded by 16 max|gamma| + max|beta| (the packer checks that against the f16 range).
template <bool QAN, bool CROSS = true, int NP = 1, bool H2 = false, int MS = MEM>
__global__ __launch_bounds__(256) void rowblock_kernel(const float *__restrict__ u_in, const float *__restrict__ lnp_w,
                                                       const float *__restrict__ lnp_b, const float *__restrict__ Qc,
                                                       const float *__restrict__ wk, const float *__restrict__ ln1_w,
                                                       const float *__restrict__ ln1_b, const float *__restrict__ G,
                                                       const float *__restrict__ g0, const float *__restrict__ VWT,
                                                       const float *__restrict__ bout, const float *__restrict__ ln2_w,
                                                       const float *__restrict__ ln2_b, float *__restrict__ x2_out, int T,
                                                       int out_frame_major /* encoder output: row = t*B + b */,
                                                       size_t u_pstride /* NP > 1: u_in is NP partial slabs this many floats apart */,
                                                       const float *__restrict__ sa_resid /* !QAN, nullable: u1 = sum(u_in slabs) + sa_resid row + sa_bias */,
                                                       const float *__restrict__ sa_bias, const float *__restrict__ h2_scale = nullptr,
                                                       int mem_len = MEM /* MS == MEMX: slots per head actually present (1..16) */) {
    static_assert(!H2 || CROSS, "the split-f16 form exists for the decoder's row blocks");
    using idf_ffn_h2::h8;
    using ML = MemLay<MS>;
    constexpr int NCT = ML::NCT, HMPX = ML::HMPX, NSLOT = ML::NSLOT, PSX = HMPX + 4;
    const int mlen = ML::GEN ? mem_len : MEM;
    constexpr int XS = QAN ? (TR + 2) * RS : 0;
    // Row strides (halves) of the token-row planes / probability planes.  A fragment read is one ds_read_b128 per lane, lane (li, kq) -> row li, 16-byte slot s0 + kq;
    // the instruction is served in lane groups {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, ... (MI355X_MICROARCH.md, LDS table), i.e. rows {0-3, 12-15} at slot s and
    // rows {4-11} at slot s + 1 together.  With a row stride of 2 slots mod 16 (32 bytes mod 256) the first set lands on the even slots and the second on the odd ones:
    // conflict-free.  (Round 4 had a stride of 1 slot -- D + 8 halves, 64 + 8 -- where row 12 at slot s and row 11 at slot s + 1 collide in every group: 2 x the LDS cycles.)
    constexpr int HS = D + 16, PHS = 64 + 16;
    __shared__ __attribute__((aligned(16))) _Float16 xpl[H2 ? 2 * (TR + 2) * HS : 8];       // [hi | lo'][TR+2][HS]: LN_prev rows for the logits, then x1 for the scores
    __shared__ __attribute__((aligned(16))) _Float16 ppl[H2 ? 2 * TR * PHS : 8];            // [hi | lo'][TR][PHS]: probabilities, columns >= HM stay zero
    _Float16 *const xh = xpl, *const xl = xpl + (H2 ? (TR + 2) * HS : 0), *const ph = ppl, *const pl = ppl + (H2 ? TR * PHS : 0);
    __shared__ __attribute__((aligned(1024))) float prm[8 * 256];        // LN_prev / LN1 / LN2 gamma, beta + cross-attention output bias + self-attention output bias (DMA targets)
    __shared__ __attribute__((aligned(16))) float sm[XS + TR * RS + 4 * (NCT > 3 ? NCT : 3) * 256 + TR * PSX];
    float *xs = sm;                               // [TR+2][RS]  LN_prev rows t0-1 .. t0+16 (QAN)
    float *x1s = sm + XS;                         // [TR][RS]    x1, then u2 in place
    float *part = x1s + TR * RS;                  // [4 waves][3 taps | NCT score tiles][16x16] K-split partial tiles
    float *Ps = part + 4 * (NCT > 3 ? NCT : 3) * 256;               // [TR][PSX]

    idf_args_now(u_in, lnp_w, lnp_b, Qc, wk, ln1_w, ln1_b, G, g0, VWT, bout, ln2_w, ln2_b, x2_out, T, out_frame_major, u_pstride, sa_resid, sa_bias, h2_scale, mem_len, gridDim.x, gridDim.y);
    const int lid = xcd_logical_id(), b = lid / (int)gridDim.x, t0 = (lid - b * (int)gridDim.x) * TR;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, kq = lane >> 4;
    const size_t rowbase = (size_t)b * T;
    // row passes (LayerNorms): every 16-lane group owns one token row, four rows per wave, all 16 rows in one sweep
    const int rown = wave * 4 + kq;
    const float *Gb = CROSS ? G + (size_t)b * (H2 ? ML::G_H2 : ML::G_FRAG) : nullptr, *g0b = CROSS ? g0 + b * ML::G0N : nullptr;
    const float *VWTb = CROSS ? VWT + (size_t)b * (H2 ? VW_H2 : ML::VWT_F) : nullptr;
    IDF_RB_STAMP(0);
    if constexpr (H2) {
        // EXCLUSIVE CU, like the other kernels that issue the f16 MFMA (ffn_h2.h "exclusive CU": next to such a kernel, workgroups of OTHER kernels on the same CU
        // have been seen to compute wrong values -- again with this kernel before it took its CU: the staggered-chains bit-identity test at B = 32).  The whole
        // register file (one wave per SIMD x 512 registers) and, by the dynamic LDS the launcher adds, all 160 KiB of LDS: nothing else can be resident here.
        asm volatile("" ::: "v255", "a255");
        // probability planes: the columns past HM are never written again
        for (int i = threadIdx.x; i < 2 * TR * PHS / 8; i += 256) reinterpret_cast<float4 *>(ppl)[i] = zero4();
    }

    // ---- Operand fetch, organised for memory-level parallelism: everything is requested with clamped (always valid) addresses and
    // no lane-divergent guard around a load, in three batches that each have whole phases of work to hide behind --
    //   entry:            token rows (all slabs), the learned-query fragments, and by DMA the small shared vectors (LayerNorm
    //                     gamma / beta x3, output bias) into LDS;
    //   after barrier 1:  the folded-score fragments G (used two phases later);
    //   after barrier 2:  the P.VW fragments (used four phases later).
    // An earlier version fetched operands "one phase ahead" behind per-lane guards; the compiler parked a full s_waitcnt vmcnt(0)
    // at every guard and the kernel made ~15 dependent round trips to L2 / Infinity Cache (tools/rowblock_probe.hip: 18 k of its
    // 26 k cycles).  Rows / columns duplicated by the clamps are never consumed (logit columns >= NQ, score columns >= HM) or are
    // zeroed below.
    {
        const float *srcs[8] = {lnp_w ? lnp_w : ln1_w, lnp_w ? lnp_b : ln1_b, ln1_w, ln1_b, CROSS ? ln2_w : ln1_w, CROSS ? ln2_b : ln1_b,
                                CROSS ? bout : ln1_b, sa_bias ? sa_bias : ln1_b};
        const uint32_t prm_lds = idf_lds_addr(prm);
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if ((i & 3) == wave) idf_dma16_s(idf_uniform_ptr(srcs[i]), (uint32_t)(lane << 4), prm_lds + (uint32_t)(i * 1024));
    }
    Row16 ra, rb;
    float4 q[4][3], gv[4][NCT], vw[NCT][4];      // fp32 fragments; H2: the same registers hold 16-byte plane fragments -- q[2 s + pl][j], gv[2 s + pl][ct], vw2[s][c][pl]
    float4 vw2[2][4][2];
    float wk_n = 0.f, g0v[NSLOT], gsc = 1.f, vsc = 1.f;                     // g0 of (head = wave, memory slots q, q+4, q+8 with q = lane & 3)
    const int ta = QAN ? t0 - 1 + rown : t0 + rown, tb = t0 + 15 + kq;
    const bool va = ta >= 0 && ta < T, vb = QAN && wave == 0 && kq < 2 && tb < T;
    Row16Raw<NP> raw_a, raw_b;
    // issue order is pinned (sched_barrier) because the wait below COUNTS: small vectors, then the token rows, then -- youngest -- the
    // twelve learned-query fragments, which are not needed before the logits and may keep flying across the first barrier
    if constexpr (QAN) wk_n = wk[min(li, NQ - 1)];
    if constexpr (CROSS) {
#pragma unroll
        for (int i = 0; i < NSLOT; ++i) g0v[i] = g0b[ML::col(wave, min((lane & 3) + 4 * i, mlen - 1))];
    }
    if constexpr (H2) {
        gsc = h2_scale[2 * b];
        vsc = h2_scale[2 * b + 1];
    }
    if constexpr (QAN) {
        if (wave == 0 && kq < 2) raw_b.request(u_in + (rowbase + min(tb, T - 1)) * D, li, u_pstride);     // halo rows t0+15, t0+16: two lane groups of wave 0 (exec-masked loads)
    }
    raw_a.request(u_in + (rowbase + min(max(ta, 0), T - 1)) * D, li, u_pstride);
    Row16Raw<1> raw_r;                            // standard layers with the out-projection folded into the attention kernel: the residual row
    if constexpr (!QAN) {
        if (sa_resid) raw_r.request(sa_resid + (rowbase + min(max(ta, 0), T - 1)) * D, li, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (QAN) {
#pragma unroll
        for (int ss = 0; ss < 4; ++ss)
#pragma unroll
            for (int j = 0; j < 3; ++j) q[ss][j] = zero4();
        if (li < NQ) {                                   // compact fragment order: only the NQ valid query columns are stored and fetched
#pragma unroll
            for (int ss = 0; ss < 4; ++ss)               // (H2: ss = 2 s + plane of [wave][K step s][tap][plane][kq][NQ][8 halves] -- the same twelve 16-byte loads)
#pragma unroll
                for (int j = 0; j < 3; ++j)
                    q[ss][j] = H2 ? ld4(Qc + (((((wave * 2 + (ss >> 1)) * 3 + j) * 2 + (ss & 1)) * 4 + kq) * NQ + li) * 4)
                                  : ld4(Qc + (((wave * 4 + ss) * 3 + j) * (4 * NQ) + kq * NQ + li) * 4);
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    auto fetch_g = [&]() {
        if constexpr (CROSS) {
#pragma unroll
            for (int ss = 0; ss < 4; ++ss)               // (H2: ss = 2 s + plane of [wave][K step s][column tile][plane][lane][8 halves])
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct)
                    gv[ss][ct] = H2 ? ld4(Gb + (((((wave * 2 + (ss >> 1)) * NCT + ct) * 2 + (ss & 1)) * 64) + lane) * 4)
                                    : ld4(Gb + (((wave * 4 + ss) * NCT + ct) * 64 + lane) * 4);
        }
    };
    auto fetch_vw = [&]() {
        if constexpr (H2) {                              // [wave = output column quarter][K step s][column tile c][plane][lane][8 halves]
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
                for (int c = 0; c < 4; ++c)
#pragma unroll
                    for (int pl2 = 0; pl2 < 2; ++pl2) vw2[s2][c][pl2] = ld4(VWTb + (((((wave * 2 + s2) * 4 + c) * 2 + pl2) * 64) + lane) * 4);
        } else if constexpr (CROSS) {
#pragma unroll
            for (int sidx = 0; sidx < NCT; ++sidx)
#pragma unroll
                for (int c = 0; c < 4; ++c) vw[sidx][c] = ld4(VWTb + (((wave * NCT + sidx) * 4 + c) * 64 + lane) * 4);
        }
    };
    // the DMA'd vectors must have landed for every wave before anyone reads them: each wave drains its own queue (its rows come
    // with it -- they are needed now anyway), then one barrier
    // (H2 owns the whole register file, so the G / VW fragments could be requested here as well: measured, slower -- the CU's address path takes ~16 cycles per
    //  sixteen-byte wave load whoever waits for it, a wave cannot start waiting for its rows before it has issued everything, and the first phase grew from
    //  7.5 k to 9.0 k cycles, the kernel from 15.6 k to 16.6 k: the three batches stay.  This kernel moves ~330 KB per workgroup through that path: 5.2 k of its cycles.)
    IDF_RB_STAMP(9);                                     // every request of the first batch issued
    if constexpr (QAN) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");      // everything older than the 12 Qc fragment loads has landed
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    IDF_RB_STAMP(10);                                    // this wave's share has landed
    __syncthreads();
    raw_a.reduce(ra);
    if constexpr (QAN) {
        if (wave == 0) raw_b.reduce(rb);
    }
    const float *P_lnp_w = prm, *P_lnp_b = prm + 256, *P_ln1_w = prm + 512, *P_ln1_b = prm + 768, *P_ln2_w = prm + 1024, *P_ln2_b = prm + 1280,
                *P_bout = prm + 1536, *P_sab = prm + 1792;

    if constexpr (QAN) {
        // rows t0-1 .. t0+14 by all groups, halo rows t0+15, t0+16 by the first two groups of wave 0
        if (lnp_w) {
            ln_row16_lds(ra, P_lnp_w, P_lnp_b, li);
            if (wave == 0) ln_row16_lds(rb, P_lnp_w, P_lnp_b, li);
        }
        if (!va) row16_zero(ra);
        if (!vb) row16_zero(rb);
        row16_store(ra, xs + rown * RS, li);
        if (wave == 0 && kq < 2) row16_store(rb, xs + (16 + kq) * RS, li);
        if constexpr (H2) {
            row16_store_planes(ra, xh + rown * HS, xl + rown * HS, li);
            if (wave == 0 && kq < 2) row16_store_planes(rb, xh + (16 + kq) * HS, xl + (16 + kq) * HS, li);
        }
        fetch_g();
        __syncthreads();
        IDF_RB_STAMP(1);                                 // rows loaded (+ slab sum), LN_prev
        // logits: three 16x16 tiles (j = 0,1,2), each wave contracts a 64-wide slice of K
        f32x4 acc[3] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
        if constexpr (H2) {
            f32x4 acc_c[3] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                const int koff = 64 * wave + 32 * s2 + 8 * kq;
                h8 ah[3], al[3];
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    ah[j] = *reinterpret_cast<const h8 *>(xh + (li + j) * HS + koff);
                    al[j] = *reinterpret_cast<const h8 *>(xl + (li + j) * HS + koff);
                }
                mma_h2<3>(acc, acc_c, ah, al, q[2 * s2], q[2 * s2 + 1]);
            }
#pragma unroll
            for (int j = 0; j < 3; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[j][r] += acc_c[j][r] * idf_ffn_h2::LO_UNSCALE;
        } else {
#pragma unroll
            for (int ss = 0; ss < 4; ++ss) {
                const int koff = 16 * (wave * 4 + ss) + 4 * kq;
                float4 a[3];
#pragma unroll
                for (int j = 0; j < 3; ++j) a[j] = ld4(xs + (li + j) * RS + koff);
                mma_rounds<3>(acc, a, q[ss]);
            }
        }
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) part[(wave * 3 + j) * 256 + (kq * 4 + r) * 16 + li] = acc[j][r];
        fetch_vw();
        __syncthreads();
        IDF_RB_STAMP(2);                                 // logits MFMA
        // tap softmax + coefficients: the 16-lane group of token `rown` holds query n = li; c_j = sum_n wk[n] softmax_j(logits) is a
        // row reduction on the DPP path, so the coefficients stay in the registers of the group that applies them below (an earlier
        // version went (t, n) -> LDS -> barrier -> 64 threads summing over n -> LDS -> barrier)
        float c0, c1, c2;
        {
            const int t = rown, n = min(li, NQ - 1);
            float l[3];
#pragma unroll
            for (int j = 0; j < 3; ++j)
                l[j] = (part[(0 * 3 + j) * 256 + t * 16 + n] + part[(1 * 3 + j) * 256 + t * 16 + n]) +
                       (part[(2 * 3 + j) * 256 + t * 16 + n] + part[(3 * 3 + j) * 256 + t * 16 + n]);
            const int tg = t0 + t;
            if (tg <= 0) l[0] = -FLT_MAX;
            if (tg + 1 >= T) l[2] = -FLT_MAX;
            const float mx = fmaxf(l[0], fmaxf(l[1], l[2]));
            const float e0 = __expf(l[0] - mx), e1 = __expf(l[1] - mx), e2 = __expf(l[2] - mx);
            const float w = li < NQ ? wk_n / (e0 + e1 + e2) : 0.f;
            c0 = row16_sum(w * e0);
            c1 = row16_sum(w * e1);
            c2 = row16_sum(w * e2);
        }
        IDF_RB_STAMP(3);                                 // tap softmax + coefficient sums
        {   // u1 = x_t + sum_j c_j x_{t+j-1} ;  x1 = LN1(u1)
            Row16 xm, xc, xp;
            row16_load(xm, xs + rown * RS, li);
            row16_load(xc, xs + (rown + 1) * RS, li);
            row16_load(xp, xs + (rown + 2) * RS, li);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                xc.c[i].x = xc.c[i].x + (c0 * xm.c[i].x + c1 * xc.c[i].x + c2 * xp.c[i].x);
                xc.c[i].y = xc.c[i].y + (c0 * xm.c[i].y + c1 * xc.c[i].y + c2 * xp.c[i].y);
                xc.c[i].z = xc.c[i].z + (c0 * xm.c[i].z + c1 * xc.c[i].z + c2 * xp.c[i].z);
                xc.c[i].w = xc.c[i].w + (c0 * xm.c[i].w + c1 * xc.c[i].w + c2 * xp.c[i].w);
            }
            ln_row16_lds(xc, P_ln1_w, P_ln1_b, li);
            if constexpr (H2) row16_store_planes(xc, xh + rown * HS, xl + rown * HS, li);      // (the logits' reads of these planes ended at the barrier above)
            if constexpr (CROSS) row16_store(xc, x1s + rown * RS, li);
            else if (t0 + rown < T) row16_store(xc, x2_out + (out_frame_major ? (size_t)(t0 + rown) * gridDim.y + b : rowbase + t0 + rown) * D, li);
        }
    } else {
        const int t = t0 + rown;
        if (sa_resid) {                               // u1 = (head partials) + xn + b_o   (workgroup-uniform branch)
            Row16 rr;
            raw_r.reduce(rr);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float4 bo = *reinterpret_cast<const float4 *>(P_sab + (i * 16 + li) * 4);
                ra.c[i].x += rr.c[i].x + bo.x;
                ra.c[i].y += rr.c[i].y + bo.y;
                ra.c[i].z += rr.c[i].z + bo.z;
                ra.c[i].w += rr.c[i].w + bo.w;
            }
        }
        if (!va) row16_zero(ra);
        fetch_g();
        fetch_vw();
        ln_row16_lds(ra, P_ln1_w, P_ln1_b, li);
        if constexpr (H2) row16_store_planes(ra, xh + rown * HS, xl + rown * HS, li);
        if constexpr (CROSS) row16_store(ra, x1s + rown * RS, li);
        else if (t < T) row16_store(ra, x2_out + (out_frame_major ? (size_t)t * gridDim.y + b : rowbase + t) * D, li);
    }
    if constexpr (!CROSS) return;                  // encoder layers: no memory to attend to, x1 is the FFN input
    __syncthreads();
    IDF_RB_STAMP(4);                                     // stencil + LN1
    {   // folded cross-attention scores: NCT 16x16 tiles over the (head, memory slot) columns (compact layout: three tiles over 40 columns)
        f32x4 acc[NCT];
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
        if constexpr (H2) {
            f32x4 acc_c[NCT];
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) acc_c[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                const int koff = 64 * wave + 32 * s2 + 8 * kq;
                const h8 a_h = *reinterpret_cast<const h8 *>(xh + li * HS + koff), a_l = *reinterpret_cast<const h8 *>(xl + li * HS + koff);
                h8 ah[NCT], al[NCT];
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct) { ah[ct] = a_h; al[ct] = a_l; }
                mma_h2<NCT>(acc, acc_c, ah, al, gv[2 * s2], gv[2 * s2 + 1]);
            }
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[ct][r] = (acc[ct][r] + acc_c[ct][r] * idf_ffn_h2::LO_UNSCALE) * gsc;      // G[b] was divided by gsc (a power of two)
        } else {
#pragma unroll
            for (int ss = 0; ss < 4; ++ss) {
                const float4 av = ld4(x1s + li * RS + 16 * (wave * 4 + ss) + 4 * kq);
                float4 a[NCT];
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct) a[ct] = av;
                mma_rounds<NCT>(acc, a, gv[ss]);
            }
        }
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r) part[(wave * NCT + ct) * 256 + (kq * 4 + r) * 16 + li] = acc[ct][r];
    }
    __syncthreads();
    IDF_RB_STAMP(5);                                     // folded scores MFMA
    {   // softmax over the MEM memory slots of each head: wave = head, token = lane >> 2, the four lanes of a quad take slots
        // q, q+4, q+8 and combine by two quad permutes (all 256 lanes busy; one wave doing all 40 columns of its 16 tokens took 2 k cycles)
        static_assert(H == 4 && MEM <= 12 && MEMX <= 16, "one wave per head, <= 3 (compact) / 4 (generic) slots per lane");
#define IDF_QUAD_XOR1(v) __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xf, 0xf, false))
#define IDF_QUAD_XOR2(v) __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xf, 0xf, false))
        const int tq = lane >> 2, qd = lane & 3;
        float sc[NSLOT], mx = -FLT_MAX;
#pragma unroll
        for (int i = 0; i < NSLOT; ++i) {
            const int m = qd + 4 * i, idx = ML::col(wave, min(m, mlen - 1)), ct = idx >> 4, cl = idx & 15, o = tq * 16 + cl;
            const float v = ((part[(0 * NCT + ct) * 256 + o] + part[(1 * NCT + ct) * 256 + o]) +
                             (part[(2 * NCT + ct) * 256 + o] + part[(3 * NCT + ct) * 256 + o])) + g0v[i];
            sc[i] = m < mlen ? v : -FLT_MAX;
            mx = fmaxf(mx, sc[i]);
        }
        mx = fmaxf(mx, IDF_QUAD_XOR1(mx));
        mx = fmaxf(mx, IDF_QUAD_XOR2(mx));
        float sum = 0.f;
#pragma unroll
        for (int i = 0; i < NSLOT; ++i) {
            sc[i] = qd + 4 * i < mlen ? __expf(sc[i] - mx) : 0.f;
            sum += sc[i];
        }
        sum += IDF_QUAD_XOR1(sum);
        sum += IDF_QUAD_XOR2(sum);
        const float inv = __builtin_amdgcn_rcpf(sum);
#pragma unroll
        for (int i = 0; i < NSLOT; ++i)
            if (qd + 4 * i < (ML::GEN ? MEMX : MEM)) {        // (generic layout: a head's 16 columns are all written -- zero past mem_len; the planes of the split form were zeroed at entry)
                const float pv = qd + 4 * i < mlen ? sc[i] * inv : 0.f;
                if constexpr (H2) {
                    _Float16 hv, lv;
                    idf_ffn_h2::split1_nf(pv, hv, lv);
                    ph[tq * PHS + ML::col(wave, qd + 4 * i)] = hv;
                    pl[tq * PHS + ML::col(wave, qd + 4 * i)] = lv;
                } else {
                    Ps[tq * PSX + ML::col(wave, qd + 4 * i)] = pv;
                }
            }
        if (!ML::GEN && !H2 && wave == 0 && qd < (HMP - HM + 3) / 4) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (HM + qd * 4 + i < HMP) Ps[tq * PSX + HM + qd * 4 + i] = 0.f;
        }
    }
    __syncthreads();
    IDF_RB_STAMP(6);                                     // head softmax
    {   // u2 = x1 + P.VW + b_out : wave w owns output columns [64w, 64w+64)
        f32x4 acc[4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
        if constexpr (H2) {
            f32x4 acc_c[4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                const h8 p_h = *reinterpret_cast<const h8 *>(ph + li * PHS + 32 * s2 + 8 * kq), p_l = *reinterpret_cast<const h8 *>(pl + li * PHS + 32 * s2 + 8 * kq);
                const h8 ah[4] = {p_h, p_h, p_h, p_h}, al[4] = {p_l, p_l, p_l, p_l};
                const float4 bh[4] = {vw2[s2][0][0], vw2[s2][1][0], vw2[s2][2][0], vw2[s2][3][0]}, bl[4] = {vw2[s2][0][1], vw2[s2][1][1], vw2[s2][2][1], vw2[s2][3][1]};
                mma_h2<4>(acc, acc_c, ah, al, bh, bl);
            }
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[c][r] = (acc[c][r] + acc_c[c][r] * idf_ffn_h2::LO_UNSCALE) * vsc;       // VW[b] was divided by vsc
        } else {
#pragma unroll
            for (int s = 0; s < NCT; ++s) {
                const float4 pv = ld4(Ps + li * PSX + 16 * s + 4 * kq);
                float4 a[4] = {pv, pv, pv, pv};
                mma_rounds<4>(acc, a, vw[s]);
            }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int col = (wave * 4 + c) * 16 + li;
#pragma unroll
            for (int r = 0; r < 4; ++r) x1s[(kq * 4 + r) * RS + col] += acc[c][r] + P_bout[col];
        }
    }
    __syncthreads();
    IDF_RB_STAMP(7);                                     // P.VW MFMA
    {
        const int t = t0 + rown;
        Row16 r;
        row16_load(r, x1s + rown * RS, li);
        ln_row16_lds(r, P_ln2_w, P_ln2_b, li);
        if (t < T) row16_store_wt(r, x2_out + (rowbase + t) * D, li);
    }
    IDF_RB_STAMP(8);                                     // LN2 + store
}

// ------------------------------------------------------------------------------------
// The split-f16 row block on EIGHT waves (round 5).  Same arithmetic per product, operand layouts, grid and outputs as rowblock_kernel<QAN, true, NP, true, MS>;
// what differs is how a workgroup's work is cut.  Round 4's kernel (four waves, one per SIMD) was a chain of short phases -- 15.6 k cycles per workgroup of which the
// matrix pipe ran 0.4 k -- on 112 of 256 CUs; its phases are latency chains over whatever one wave holds:
//   * row passes (slab sums, the three LayerNorms, the stencil, the f16 splits): one token row per 32 lanes (two 16-byte chunks per lane) instead of per 16 lanes
//     (four) -- every pass is half as deep; a row's reductions are a 16-lane DPP reduction + one ds_swizzle exchange with the other half;
//   * the logits and scores contractions split K over eight waves (one K = 32 step each: three / NCT dependent-free MFMA groups instead of two rounds), P.VW gives a wave
//     two output tiles instead of four; every wave fetches half the fragments (the fragment orders in memory are unchanged: [K quarter][K step] IS [K eighth]);
//   * two waves per SIMD: one's loads and LDS traffic run beside the other's VALU work.
// It still owns its CU (512 threads x 256 registers = the register file, LDS topped up to 160 KiB by the launcher).  Results differ from the four-wave kernel by
// summation order only (eight K partials instead of four; 32-lane LayerNorm sums); every route of a process takes the same kernel, so bit-identity between routes holds.
// Reference work being replaced: model/sublayers.py:311-352 (QaN block + cross-attention + the two LayerNorms around them).
// ------------------------------------------------------------------------------------
// Token rows of the eight-wave row block: LPR lanes per row (32 with 16 tokens per workgroup, 64 with 8), lane lr owns the 4-float chunks lr, LPR + lr, ...
// The two forms compute the SAME bits: every per-element operation is the same, and a row's two LayerNorm sums are taken over ONE fixed tree whatever LPR is --
// leaves = the 64 chunks' partial sums; T_r = the 16-lane rotation tree (row16_sum) over chunks 16 r .. 16 r + 15, r = 0..3; sum = (T0 + T1) + (T2 + T3) -- so the number
// of tokens a workgroup takes is a pure performance choice (like the row tile of ffn_h2.h): shards / chains of a batch that pick differently still agree bit for bit.
// With 64 lanes per row that tree is common.h's wave_sum (DPP + four v_readlane: no LDS-crossbar instruction on the row passes' critical path -- a first version
// exchanged halves with ds_bpermute / ds_swizzle and spent ~250 cycles per reduction, six reductions per workgroup in a row); with 32 lanes a lane's two chunks belong
// to T_r and T_(r+2), so both are reduced over the 16-lane row and the halves exchanged with one ds_swizzle each.
template <int LPR>
struct RowL {
    static constexpr int CPL = 64 / LPR;          // chunks per lane: 2 or 1
    float4 c[CPL];
};
#define IDF_SWZ_XOR16(v) __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, v), 0x401F))      // lane i <- lane i ^ 16 (bit-mask mode: and 0x1f, or 0, xor 0x10)
// p0 / p1: this lane's partial sums of its chunk(s) (p1 only with two chunks per lane)
template <int LPR>
__device__ __forceinline__ float rowl_tree(float p0, float p1) {
    if constexpr (LPR == 64) {
        return wave_sum(p0);                      // row16_sum, then (T0 + T1) + (T2 + T3) through scalar registers
    } else {
        const float t0 = row16_sum(p0), t1 = row16_sum(p1);      // lanes 0..15: T0, T2; lanes 16..31: T1, T3
        const float s01 = t0 + IDF_SWZ_XOR16(t0), s23 = t1 + IDF_SWZ_XOR16(t1);
        return s01 + s23;
    }
}
template <int LPR, int NP>
struct RowLRaw {
    static constexpr int CPL = 64 / LPR;
    float4 t[CPL][NP];
    __device__ __forceinline__ void request(const float *__restrict__ row, int lr, size_t stride) {
#pragma unroll
        for (int i = 0; i < CPL; ++i)
#pragma unroll
            for (int sl = 0; sl < NP; ++sl) t[i][sl] = ld4(row + sl * stride + (i * LPR + lr) * 4);
    }
    __device__ __forceinline__ void reduce(RowL<LPR> &r) const {      // slabs summed in the order of common.h ld4_sum
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
            float4 v = t[i][0];
#pragma unroll
            for (int sl = 1; sl < NP; ++sl) { v.x += t[i][sl].x; v.y += t[i][sl].y; v.z += t[i][sl].z; v.w += t[i][sl].w; }
            r.c[i] = v;
        }
    }
};
template <int LPR>
__device__ __forceinline__ void ln_rowl_lds(RowL<LPR> &r, const float *w, const float *b, int lr) {
    // no FMA contraction in the row passes of this kernel: WHICH product of `a * a + b * b` (or of a * b + c written over two statements) the backend fuses is its own choice per
    // instantiation, and the 8- and the 16-token form must round alike (every product and every sum rounded on its own, like the sampler update of gemm.h)
#pragma clang fp contract(off)
    constexpr int CPL = 64 / LPR;
    float p[2] = {0.f, 0.f};
#pragma unroll
    for (int i = 0; i < CPL; ++i) p[i] = (r.c[i].x + r.c[i].y) + (r.c[i].z + r.c[i].w);
    const float mean = rowl_tree<LPR>(p[0], p[1]) * (1.0f / 256.0f);
    float q[2] = {0.f, 0.f};
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
        const float a0 = r.c[i].x - mean, a1 = r.c[i].y - mean, a2 = r.c[i].z - mean, a3 = r.c[i].w - mean;
        q[i] = (a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3);
    }
    const float rstd = __builtin_amdgcn_rsqf(rowl_tree<LPR>(q[0], q[1]) * (1.0f / 256.0f) + 1e-5f);
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
        const float4 g = *reinterpret_cast<const float4 *>(w + (i * LPR + lr) * 4), be = *reinterpret_cast<const float4 *>(b + (i * LPR + lr) * 4);
        r.c[i].x = (r.c[i].x - mean) * rstd * g.x + be.x;
        r.c[i].y = (r.c[i].y - mean) * rstd * g.y + be.y;
        r.c[i].z = (r.c[i].z - mean) * rstd * g.z + be.z;
        r.c[i].w = (r.c[i].w - mean) * rstd * g.w + be.w;
    }
}
// The same LayerNorm on TWO independent rows at once (a token row and a halo row of the same lanes): same operations per row in the same order -- same bits as two
// calls --, written side by side so that the two rows' reduction chains overlap instead of following each other behind a branch (the waves that own a halo row were
// the last to reach the barrier: tools/rowblock_probe.hip).
template <int LPR>
__device__ __forceinline__ void ln2_rowl_lds(RowL<LPR> &ra, RowL<LPR> &rb, const float *w, const float *b, int lr) {
#pragma clang fp contract(off)
    constexpr int CPL = 64 / LPR;
    float pa[2] = {0.f, 0.f}, pb[2] = {0.f, 0.f};
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
        pa[i] = (ra.c[i].x + ra.c[i].y) + (ra.c[i].z + ra.c[i].w);
        pb[i] = (rb.c[i].x + rb.c[i].y) + (rb.c[i].z + rb.c[i].w);
    }
    const float ma = rowl_tree<LPR>(pa[0], pa[1]) * (1.0f / 256.0f), mb = rowl_tree<LPR>(pb[0], pb[1]) * (1.0f / 256.0f);
    float qa[2] = {0.f, 0.f}, qb[2] = {0.f, 0.f};
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
        const float a0 = ra.c[i].x - ma, a1 = ra.c[i].y - ma, a2 = ra.c[i].z - ma, a3 = ra.c[i].w - ma;
        const float b0 = rb.c[i].x - mb, b1 = rb.c[i].y - mb, b2 = rb.c[i].z - mb, b3 = rb.c[i].w - mb;
        qa[i] = (a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3);
        qb[i] = (b0 * b0 + b1 * b1) + (b2 * b2 + b3 * b3);
    }
    const float rsa = __builtin_amdgcn_rsqf(rowl_tree<LPR>(qa[0], qa[1]) * (1.0f / 256.0f) + 1e-5f), rsb = __builtin_amdgcn_rsqf(rowl_tree<LPR>(qb[0], qb[1]) * (1.0f / 256.0f) + 1e-5f);
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
        const float4 g = *reinterpret_cast<const float4 *>(w + (i * LPR + lr) * 4), be = *reinterpret_cast<const float4 *>(b + (i * LPR + lr) * 4);
        ra.c[i].x = (ra.c[i].x - ma) * rsa * g.x + be.x;
        ra.c[i].y = (ra.c[i].y - ma) * rsa * g.y + be.y;
        ra.c[i].z = (ra.c[i].z - ma) * rsa * g.z + be.z;
        ra.c[i].w = (ra.c[i].w - ma) * rsa * g.w + be.w;
        rb.c[i].x = (rb.c[i].x - mb) * rsb * g.x + be.x;
        rb.c[i].y = (rb.c[i].y - mb) * rsb * g.y + be.y;
        rb.c[i].z = (rb.c[i].z - mb) * rsb * g.z + be.z;
        rb.c[i].w = (rb.c[i].w - mb) * rsb * g.w + be.w;
    }
}
template <int LPR>
__device__ __forceinline__ void rowl_load(RowL<LPR> &r, const float *row, int lr) {
#pragma unroll
    for (int i = 0; i < 64 / LPR; ++i) r.c[i] = *reinterpret_cast<const float4 *>(row + (i * LPR + lr) * 4);
}
template <int LPR>
__device__ __forceinline__ void rowl_store(const RowL<LPR> &r, float *row, int lr) {
#pragma unroll
    for (int i = 0; i < 64 / LPR; ++i) *reinterpret_cast<float4 *>(row + (i * LPR + lr) * 4) = r.c[i];
}
template <int LPR>
__device__ __forceinline__ void rowl_store_wt(const RowL<LPR> &r, float *row, int lr) {
#pragma unroll
    for (int i = 0; i < 64 / LPR; ++i) idf_store16_wt(row + (i * LPR + lr) * 4, r.c[i]);
}
template <int LPR>
__device__ __forceinline__ void rowl_zero(RowL<LPR> &r) {
#pragma unroll
    for (int i = 0; i < 64 / LPR; ++i) r.c[i] = zero4();
}
template <int LPR>
__device__ __forceinline__ void rowl_store_planes(const RowL<LPR> &r, _Float16 *hi_row, _Float16 *lo_row, int lr) {
#pragma unroll
    for (int i = 0; i < 64 / LPR; ++i) {
        uint2 h, l;
        idf_ffn_h2::split4_pk(r.c[i], h, l);
        *reinterpret_cast<uint2 *>(hi_row + (i * LPR + lr) * 4) = h;
        *reinterpret_cast<uint2 *>(lo_row + (i * LPR + lr) * 4) = l;
    }
}

// TV = tokens per workgroup: 16 (grid ceil(T/16) x B) or 8 (grid ceil(T/8) x B).  The row passes are bound by the CU's VALU issue (tools/rowblock_probe.hip: eight waves
// instead of four changed them by 6 % -- the same instructions on the same four SIMDs), so what shortens them is FEWER ROWS PER CU: with eight tokens the launch is
// 208 workgroups at B = 16, T = 100 -- one round on 256 CUs instead of 112 -- each with half the row work; the MFMA tiles stay 16 rows tall (rows >= TV + 2 of the A
// operands are whatever LDS holds: they only reach output rows nobody stores).  The launcher takes 8 whenever the launch still fits the chip in one round.
template <bool QAN, int NP, int MS = MEM, int TV = 16>
__global__ __launch_bounds__(512) void rowblock8_kernel(const float *__restrict__ u_in, int T, int ntile, int nclip, int mem_len, size_t u_pstride,
                                                        const float *__restrict__ sa_resid, const float *__restrict__ Qc,
                                                        const float *__restrict__ lnp_w, const float *__restrict__ lnp_b,
                                                        const float *__restrict__ wk, const float *__restrict__ ln1_w,
                                                        const float *__restrict__ ln1_b, const float *__restrict__ G,
                                                        const float *__restrict__ g0, const float *__restrict__ VWT,
                                                        const float *__restrict__ bout, const float *__restrict__ ln2_w,
                                                        const float *__restrict__ ln2_b, float *__restrict__ x2_out,
                                                        const float *__restrict__ sa_bias, const float *__restrict__ h2_scale) {
    // Argument order: what the token-row addresses need comes first -- the library is built with kernel-argument preloading (build.py), the leading 14 dwords are in
    // SGPRs when the wave starts, and the rows are requested before anything else is even read from the argument segment.  1-D grid of ntile * nclip workgroups.
#pragma clang fp contract(off)                    // (see ln_rowl_lds: the two token counts must compute the same bits)
    using idf_ffn_h2::h8;
    using ML = MemLay<MS>;
    static_assert(TV == 16 || TV == 8, "tokens per workgroup");
    constexpr int NCT = ML::NCT, NSLOT = ML::NSLOT, NW8 = 8, NPT = NCT > 3 ? NCT : 3;
    constexpr int LPR = 512 / TV;                 // lanes per token row in the row passes
    constexpr int PTR = 20, PTS = 16 * PTR;       // K-split partial tiles: row stride 20 floats.  The MFMA result layout stores row 4 kq + r, column li per lane: 4 rows = 80 floats = 16 banks
                                                  // further, so the four kq groups of a store cover 64 different banks (17 put them 4 banks apart: up to 4 lanes per bank, ~0.6 k conflict
                                                  // cycles per workgroup = most of the kernel's SQ_LDS_BANK_CONFLICT); the head softmax's column-wise reads (token = lane >> 2: 20 tq mod 64 are
                                                  // the sixteen multiples of 4) and the tap softmax's row reads stay conflict-free
    constexpr int XS = QAN ? (TR + 2) * RS : 0;
    constexpr int HS = D + 16, PHS = 64 + 16;     // plane strides: conflict-free fragment reads (rowblock_kernel)
    __shared__ __attribute__((aligned(16))) _Float16 xpl[2 * (TR + 2) * HS];       // [hi | lo'][TR+2][HS]: LN_prev rows for the logits, then x1 for the scores (TV + 2 rows are written)
    __shared__ __attribute__((aligned(16))) _Float16 ppl[2 * TR * PHS];            // [hi | lo'][TR][PHS]: probabilities, unwritten columns stay zero
    _Float16 *const xh = xpl, *const xl = xpl + (TR + 2) * HS, *const ph = ppl, *const pl = ppl + TR * PHS;
    __shared__ __attribute__((aligned(1024))) float prm[8 * 256];        // LN_prev / LN1 / LN2 gamma, beta + cross-attention output bias + self-attention output bias (DMA targets)
    __shared__ __attribute__((aligned(16))) float sm[XS + TR * RS + NW8 * NPT * PTS];
    float *xs = sm;                               // [TV+2 of TR+2][RS]  LN_prev rows t0-1 .. t0+TV (QAN)
    float *x1s = sm + XS;                         // [TR][RS]    x1, then u2 in place
    float *part = x1s + TR * RS;                  // [8 waves][3 taps | NCT score tiles][16][17] K-split partial tiles

    IDF_RB_STAMP(0);
    asm volatile("" ::: "v255");                  // EXCLUSIVE CU (ffn_h2.h): 2 waves per SIMD x 256 registers = the register file; the launcher tops the LDS up to 160 KiB
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rg = tid / LPR, lr = tid % LPR;     // row passes: token row rg of the TV, lane lr of its LPR; threads of rows 0 and 1 also take the two halo rows (QAN)
    // ---- first batch of requests (pinned order, the wait below counts).  Oldest: the token rows (five slabs each; behind them everything else of the prologue runs
    // while they are in flight); then the shared vectors by DMA, the scalars, and -- youngest -- the learned-query fragments
    const int nwg = ntile * nclip, xq = nwg >> 3, xr = nwg & 7, xcd = (int)blockIdx.x & 7;      // XCD-affine logical id (xcd_logical_id) from the preloaded counts
    const int lid = (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + ((int)blockIdx.x >> 3);
    const int b = lid / ntile, t0 = (lid - b * ntile) * TV;
    const size_t rowbase = (size_t)b * T;
    const int ta = QAN ? t0 - 1 + rg : t0 + rg, tb = t0 + TV - 1 + rg;
    const bool halo = QAN && rg < 2;
    const bool va = ta >= 0 && ta < T, vb = halo && tb < T;
    RowLRaw<LPR, NP> raw_a, raw_b;
    RowLRaw<LPR, 1> raw_r;
    if constexpr (QAN) {
        if (halo) raw_b.request(u_in + (rowbase + min(tb, T - 1)) * D, lr, u_pstride);     // halo rows t0 + TV - 1, t0 + TV: the threads of rows 0 and 1 (wave-uniform: LPR >= 32)
    }
    raw_a.request(u_in + (rowbase + min(max(ta, 0), T - 1)) * D, lr, u_pstride);
    if constexpr (!QAN) {
        if (sa_resid) raw_r.request(sa_resid + (rowbase + min(max(ta, 0), T - 1)) * D, lr, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
    IDF_RB_STAMP(9);                                     // token rows requested (from the preloaded arguments alone)
    idf_args_now(lnp_b, wk, ln1_w, ln1_b, G, g0, VWT, bout, ln2_w, ln2_b, x2_out, sa_bias, h2_scale);
#ifdef IDF_RB_STAMP_ARGS
    IDF_RB_STAMP(14);                                    // (probe variant) the rest of the argument segment has arrived
#endif
    const int li = lane & 15, kq = lane >> 4;
    const int mlen = ML::GEN ? mem_len : MEM;
    const float *Gb = G + (size_t)b * ML::G_H2, *g0b = g0 + b * ML::G0N, *VWTb = VWT + (size_t)b * VW_H2;
    {   // wave w brings shared vector w (a scalar choice: one DMA instruction per wave)
        const int ws = __builtin_amdgcn_readfirstlane(wave);
        const float *src = ws == 0 ? (lnp_w ? lnp_w : ln1_w) : ws == 1 ? (lnp_w ? lnp_b : ln1_b) : ws == 2 ? ln1_w : ws == 3 ? ln1_b : ws == 4 ? ln2_w : ws == 5 ? ln2_b
                         : ws == 6 ? bout : (sa_bias ? sa_bias : ln1_b);
        idf_dma16_s(idf_uniform_ptr(src), (uint32_t)(lane << 4), idf_lds_addr(prm) + (uint32_t)(ws * 1024));
    }
    float4 q[2][3], gv[2][NCT], vw2[2][2][2];     // plane fragments: q[plane][tap], gv[plane][column tile] of this wave's K step; vw2[K step][tile][plane] of its two output tiles
    float wk_n = 0.f, g0v[NSLOT];
    const float gsc = h2_scale[2 * b], vsc = h2_scale[2 * b + 1];
    const int hh = wave & 3;                      // head softmax: waves 0..3, wave = head
    RowL<LPR> ra, rb;
    if constexpr (QAN) wk_n = wk[min(li, NQ - 1)];
#pragma unroll
    for (int i = 0; i < NSLOT; ++i) g0v[i] = g0b[ML::col(hh, min((lane & 3) + 4 * i, mlen - 1))];
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (QAN) {
#pragma unroll
        for (int p2 = 0; p2 < 2; ++p2)
#pragma unroll
            for (int j = 0; j < 3; ++j) q[p2][j] = zero4();
        if (li < NQ) {                            // [K eighth = wave][tap][plane][kq][NQ][8 halves]
#pragma unroll
            for (int p2 = 0; p2 < 2; ++p2)
#pragma unroll
                for (int j = 0; j < 3; ++j) q[p2][j] = ld4(Qc + ((((wave * 3 + j) * 2 + p2) * 4 + kq) * NQ + li) * 4);
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    for (int i = tid; i < 2 * TR * PHS / 8; i += 512) reinterpret_cast<float4 *>(ppl)[i] = zero4();
    IDF_RB_STAMP(15);                                    // the rest of the argument segment read, every request of the first batch issued
    // (A CU's vector-memory path accepts ~64 B per clock for all its waves and a wave waits in its issue slot until its request is taken: the ~100 KB of this batch keep
    // wave 0 here until ~4.4 k cycles.  Sending the learned-query fragments behind the barrier below instead moved that wait into the LayerNorm pass, same total:
    // tools/rowblock_probe.hip, profiles/r05_rowblock_probe.txt.  The kernel's ~200 KB of operands per workgroup are ~3.2 k cycles of such issue time.)
    if constexpr (QAN) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");       // everything older than the six learned-query fragment loads has landed
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    IDF_RB_STAMP(10);                                    // this wave's share has landed
    __syncthreads();
    IDF_RB_STAMP(11);                                    // every wave's share has landed
    auto fetch_g = [&]() {                        // [K eighth = wave][column tile][plane][lane][8 halves]
#pragma unroll
        for (int p2 = 0; p2 < 2; ++p2)
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) {
                gv[p2][ct] = ld4(Gb + ((((wave * NCT + ct) * 2 + p2) * 64) + lane) * 4);
            }
    };
    raw_a.reduce(ra);
    if constexpr (QAN) {
        if (halo) raw_b.reduce(rb);
        else rowl_zero<LPR>(rb);                  // (waves without a halo row run the two-row LayerNorm below on zeros: a few VALU slots, no second latency chain)
    }
    const float *P_lnp_w = prm, *P_lnp_b = prm + 256, *P_ln1_w = prm + 512, *P_ln1_b = prm + 768, *P_ln2_w = prm + 1024, *P_ln2_b = prm + 1280,
                *P_bout = prm + 1536, *P_sab = prm + 1792;
    auto fetch_vw = [&]() {                       // [output column quarter = wave >> 1][K step][column tile 2 (wave & 1) + c][plane][lane][8 halves]
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int p2 = 0; p2 < 2; ++p2) {
                    vw2[s2][c][p2] = ld4(VWTb + ((((((wave >> 1) * 2 + s2) * 4 + 2 * (wave & 1) + c) * 2 + p2) * 64) + lane) * 4);
                }
    };

    if constexpr (QAN) {
        if (lnp_w) {
            if (halo) ln2_rowl_lds<LPR>(ra, rb, P_lnp_w, P_lnp_b, lr);      // its own row and its halo row side by side (same bits as two single-row calls)
            else ln_rowl_lds<LPR>(ra, P_lnp_w, P_lnp_b, lr);
        }
        if (!va) rowl_zero<LPR>(ra);
        if (!vb) rowl_zero<LPR>(rb);
        rowl_store<LPR>(ra, xs + rg * RS, lr);
        rowl_store_planes<LPR>(ra, xh + rg * HS, xl + rg * HS, lr);
        if (halo) {
            rowl_store<LPR>(rb, xs + (TV + rg) * RS, lr);
            rowl_store_planes<LPR>(rb, xh + (TV + rg) * HS, xl + (TV + rg) * HS, lr);
        }
        fetch_g();
        IDF_RB_STAMP(12);                                // this wave is done with its LN_prev rows (before the barrier)
        __syncthreads();
        IDF_RB_STAMP(1);                                 // rows loaded (+ slab sum), LN_prev, planes
        {   // logits: three 16x16 tiles (taps), this wave contracts K = [32 wave, 32 wave + 32)
            f32x4 acc[3] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}}, acc_c[3] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
            const int koff = 32 * wave + 8 * kq;
            h8 ah[3], al[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                ah[j] = *reinterpret_cast<const h8 *>(xh + (li + j) * HS + koff);
                al[j] = *reinterpret_cast<const h8 *>(xl + (li + j) * HS + koff);
            }
            mma_h2<3>(acc, acc_c, ah, al, q[0], q[1]);
            IDF_RB_STAMP(13);                                // (probe) logits: operands read, MFMAs issued
#pragma unroll
            for (int j = 0; j < 3; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) part[(wave * 3 + j) * PTS + (kq * 4 + r) * PTR + li] = acc[j][r] + acc_c[j][r] * idf_ffn_h2::LO_UNSCALE;
        }
        fetch_vw();
#ifndef IDF_RB_STAMP_ARGS
        IDF_RB_STAMP(14);                                // (probe) logits: partial tiles stored, VW requested
#endif
        __syncthreads();
        IDF_RB_STAMP(2);                                 // logits MFMA
        float c0, c1, c2;
        {   // tap softmax + coefficients: every 16-lane group of a row computes them (query n = lane & 15), so no exchange is needed before the stencil
            const int n = min(li, NQ - 1);
            float l[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const float *pp = part + j * PTS + rg * PTR + n;
                constexpr int WS3 = 3 * PTS;
                l[j] = ((pp[0 * WS3] + pp[1 * WS3]) + (pp[2 * WS3] + pp[3 * WS3])) + ((pp[4 * WS3] + pp[5 * WS3]) + (pp[6 * WS3] + pp[7 * WS3]));
            }
            const int tg = t0 + rg;
            if (tg <= 0) l[0] = -FLT_MAX;
            if (tg + 1 >= T) l[2] = -FLT_MAX;
            const float mx = fmaxf(l[0], fmaxf(l[1], l[2]));
            const float e0 = __expf(l[0] - mx), e1 = __expf(l[1] - mx), e2 = __expf(l[2] - mx);
            const float w = li < NQ ? wk_n / (e0 + e1 + e2) : 0.f;
            c0 = row16_sum(w * e0);
            c1 = row16_sum(w * e1);
            c2 = row16_sum(w * e2);
        }
        IDF_RB_STAMP(3);                                 // tap softmax + coefficient sums
        {   // u1 = x_t + sum_j c_j x_{t+j-1} ;  x1 = LN1(u1)
            RowL<LPR> xm, xc, xp;
            rowl_load<LPR>(xm, xs + rg * RS, lr);
            rowl_load<LPR>(xc, xs + (rg + 1) * RS, lr);
            rowl_load<LPR>(xp, xs + (rg + 2) * RS, lr);
#pragma unroll
            for (int i = 0; i < 64 / LPR; ++i) {
                xc.c[i].x = xc.c[i].x + (c0 * xm.c[i].x + c1 * xc.c[i].x + c2 * xp.c[i].x);
                xc.c[i].y = xc.c[i].y + (c0 * xm.c[i].y + c1 * xc.c[i].y + c2 * xp.c[i].y);
                xc.c[i].z = xc.c[i].z + (c0 * xm.c[i].z + c1 * xc.c[i].z + c2 * xp.c[i].z);
                xc.c[i].w = xc.c[i].w + (c0 * xm.c[i].w + c1 * xc.c[i].w + c2 * xp.c[i].w);
            }
            ln_rowl_lds<LPR>(xc, P_ln1_w, P_ln1_b, lr);
            rowl_store_planes<LPR>(xc, xh + rg * HS, xl + rg * HS, lr);      // (the logits' reads of these planes ended at the barrier above)
            rowl_store<LPR>(xc, x1s + rg * RS, lr);
        }
    } else {
        if (sa_resid) {                               // u1 = (head partials) + xn + b_o   (workgroup-uniform branch)
            RowL<LPR> rr;
            raw_r.reduce(rr);
#pragma unroll
            for (int i = 0; i < 64 / LPR; ++i) {
                const float4 bo = *reinterpret_cast<const float4 *>(P_sab + (i * LPR + lr) * 4);
                ra.c[i].x += rr.c[i].x + bo.x;
                ra.c[i].y += rr.c[i].y + bo.y;
                ra.c[i].z += rr.c[i].z + bo.z;
                ra.c[i].w += rr.c[i].w + bo.w;
            }
        }
        if (!va) rowl_zero<LPR>(ra);
        fetch_g();
        fetch_vw();
        ln_rowl_lds<LPR>(ra, P_ln1_w, P_ln1_b, lr);
        rowl_store_planes<LPR>(ra, xh + rg * HS, xl + rg * HS, lr);
        rowl_store<LPR>(ra, x1s + rg * RS, lr);
    }
    __syncthreads();
    IDF_RB_STAMP(4);                                     // stencil + LN1
    {   // folded cross-attention scores: NCT 16x16 tiles, this wave's K step
        f32x4 acc[NCT], acc_c[NCT];
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) acc[ct] = acc_c[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int koff = 32 * wave + 8 * kq;
        const h8 a_h = *reinterpret_cast<const h8 *>(xh + li * HS + koff), a_l = *reinterpret_cast<const h8 *>(xl + li * HS + koff);
        h8 ah[NCT], al[NCT];
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) { ah[ct] = a_h; al[ct] = a_l; }
        mma_h2<NCT>(acc, acc_c, ah, al, gv[0], gv[1]);
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r) part[(wave * NCT + ct) * PTS + (kq * 4 + r) * PTR + li] = (acc[ct][r] + acc_c[ct][r] * idf_ffn_h2::LO_UNSCALE) * gsc;      // G[b] was divided by gsc (a power of two)
    }
    __syncthreads();
    IDF_RB_STAMP(5);                                     // folded scores MFMA
    if (wave < 4) {   // softmax over the memory slots of each head: wave = head, token = lane >> 2, the four lanes of a quad take slots q, q+4, ... (rowblock_kernel)
        const int tq = lane >> 2, qd = lane & 3;
        float sc[NSLOT], mx = -FLT_MAX;
#pragma unroll
        for (int i = 0; i < NSLOT; ++i) {
            const int m = qd + 4 * i, idx = ML::col(wave, min(m, mlen - 1)), ct = idx >> 4, cl = idx & 15;
            const float *pp = part + ct * PTS + tq * PTR + cl;
            constexpr int WS8 = NCT * PTS;
            const float v = (((pp[0 * WS8] + pp[1 * WS8]) + (pp[2 * WS8] + pp[3 * WS8])) + ((pp[4 * WS8] + pp[5 * WS8]) + (pp[6 * WS8] + pp[7 * WS8]))) + g0v[i];
            sc[i] = m < mlen ? v : -FLT_MAX;
            mx = fmaxf(mx, sc[i]);
        }
        mx = fmaxf(mx, IDF_QUAD_XOR1(mx));
        mx = fmaxf(mx, IDF_QUAD_XOR2(mx));
        float sum = 0.f;
#pragma unroll
        for (int i = 0; i < NSLOT; ++i) {
            sc[i] = qd + 4 * i < mlen ? __expf(sc[i] - mx) : 0.f;
            sum += sc[i];
        }
        sum += IDF_QUAD_XOR1(sum);
        sum += IDF_QUAD_XOR2(sum);
        const float inv = __builtin_amdgcn_rcpf(sum);
#pragma unroll
        for (int i = 0; i < NSLOT; ++i)
            if (qd + 4 * i < (ML::GEN ? MEMX : MEM)) {
                _Float16 hv, lv;
                idf_ffn_h2::split1_nf(qd + 4 * i < mlen ? sc[i] * inv : 0.f, hv, lv);
                ph[tq * PHS + ML::col(wave, qd + 4 * i)] = hv;
                pl[tq * PHS + ML::col(wave, qd + 4 * i)] = lv;
            }
    }
    __syncthreads();
    IDF_RB_STAMP(6);                                     // head softmax
    {   // u2 = x1 + P.VW + b_out : wave w owns output columns [32 w, 32 w + 32)
        f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}}, acc_c[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            const h8 p_h = *reinterpret_cast<const h8 *>(ph + li * PHS + 32 * s2 + 8 * kq), p_l = *reinterpret_cast<const h8 *>(pl + li * PHS + 32 * s2 + 8 * kq);
            const h8 ah[2] = {p_h, p_h}, al[2] = {p_l, p_l};
            const float4 bh[2] = {vw2[s2][0][0], vw2[s2][1][0]}, bl[2] = {vw2[s2][0][1], vw2[s2][1][1]};
            mma_h2<2>(acc, acc_c, ah, al, bh, bl);
        }
        if (TV == 16 || kq * 4 < TV) {            // (8 tokens: rows 0..7 = the lanes of kq 0, 1.  ONE branch around all eight updates: a guard per element made eight serial LDS round trips)
            float xo[2][4], bo[2];
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int col = (wave * 2 + c) * 16 + li;
                bo[c] = P_bout[col];
#pragma unroll
                for (int r = 0; r < 4; ++r) xo[c][r] = x1s[(kq * 4 + r) * RS + col];
            }
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int col = (wave * 2 + c) * 16 + li;
#pragma unroll
                for (int r = 0; r < 4; ++r) x1s[(kq * 4 + r) * RS + col] = xo[c][r] + ((acc[c][r] + acc_c[c][r] * idf_ffn_h2::LO_UNSCALE) * vsc + bo[c]);       // VW[b] was divided by vsc
            }
        }
    }
    __syncthreads();
    IDF_RB_STAMP(7);                                     // P.VW MFMA
    {
        const int t = t0 + rg;
        RowL<LPR> r;
        rowl_load<LPR>(r, x1s + rg * RS, lr);
        ln_rowl_lds<LPR>(r, P_ln2_w, P_ln2_b, lr);
        if (t < T) rowl_store_wt<LPR>(r, x2_out + (rowbase + t) * D, lr);
    }
    IDF_RB_STAMP(8);                                     // LN2 + store
}

// ------------------------------------------------------------------------------------
// Host side: the operands of a launch, ONE launcher per kernel template, the exclusive-CU check of the split-f16 forms and the route between the forms.
// Null = absent: lnp_w (nothing pending on the input), qc (standard layer), sa_resid (QaN layer), G (encoder: no cross attention; ln2_* / ca_out_b unused).
// Operands that exist in two forms are both named; a launcher hands its kernel the form that kernel reads.
// ------------------------------------------------------------------------------------
struct RowBlockArgs {
    const float *u_in; int np; size_t pstride;          // input: np partial slabs pstride floats apart (np = 1: a plain matrix)
    const float *lnp_w, *lnp_b;                         // LayerNorm still to be applied to u_in
    const float *qc, *qc_h2, *wk;                       // learned queries in fp32 / split-f16 fragment order, tap weights
    const float *ln1_w, *ln1_b, *ln2_w, *ln2_b, *ca_out_b;
    const float *G, *VWT, *g0, *Gh2, *VWh2, *sc;        // this layer's folded memory (memfold.h MemCtx): fp32 fragments | split-f16 planes and their scales
    int mem_len;
    float *out; int frame_major;                        // frame_major (the encoder's output): row = t*B + b
    const float *sa_resid, *sa_bias;                    // standard layer: u1 = sum(u_in slabs) + sa_resid row + sa_bias
    int B, T;
};
template <bool QAN, bool CROSS, int NP, bool H2, int MS>
void launch_rowblock(hipStream_t s, const RowBlockArgs &a, int dyn_lds = 0) {
    rowblock_kernel<QAN, CROSS, NP, H2, MS><<<dim3((unsigned)idf_cdiv(a.T, TR), a.B), dim3(256), (size_t)dyn_lds, s>>>(
        a.u_in, a.lnp_w, a.lnp_b, H2 ? a.qc_h2 : a.qc, a.wk, a.ln1_w, a.ln1_b, H2 ? a.Gh2 : a.G, a.g0, H2 ? a.VWh2 : a.VWT, a.ca_out_b, a.ln2_w, a.ln2_b, a.out, a.T,
        a.frame_major, a.pstride, a.sa_resid, a.sa_bias, H2 ? a.sc : nullptr, a.mem_len);
}
template <bool QAN, int NP, int MS, int TV>
void launch_rowblock8(hipStream_t s, const RowBlockArgs &a, int dyn_lds) {
    const int ntile = (int)idf_cdiv(a.T, TV);
    rowblock8_kernel<QAN, NP, MS, TV><<<dim3((unsigned)ntile * a.B), dim3(512), (size_t)dyn_lds, s>>>(
        a.u_in, a.T, ntile, a.B, a.mem_len, a.pstride, a.sa_resid, a.qc_h2, a.lnp_w, a.lnp_b, a.wk, a.ln1_w, a.ln1_b, a.Gh2, a.g0, a.VWh2, a.ca_out_b, a.ln2_w, a.ln2_b,
        a.out, a.sa_bias, a.sc);
}
// the exact form of a QaN layer, whose input is a plain matrix (layer 0) or the feed-forward's slabs
template <bool CROSS, int MS>
void launch_rowblock_qan_f32(hipStream_t s, const RowBlockArgs &a) {
    if (a.np == NSL) launch_rowblock<true, CROSS, NSL, false, MS>(s, a);
    else launch_rowblock<true, CROSS, 1, false, MS>(s, a);
}

// Dynamic LDS that tops a split-f16 row block's static LDS up to the CU's whole 160 KiB (exclusive CU, see the kernels), verified per (kernel, device): -1 = the
// kernel does not get its CU there (common.h idf_exclusive_cu) and the route below moves on.  WAVES: 8 = rowblock8_kernel at TV tokens per workgroup (the shipped
// split-f16 row block since round 5), 4 = rowblock_kernel<.., H2> (round 4's kernel, its fallback).  A QaN layer's input is NSL slabs, a standard layer's H.
template <bool QAN, int MS, int WAVES, int TV = 16>
int rb_exclusive_dyn() {
    static_assert(WAVES == 8 || (WAVES == 4 && TV == 16), "kernel form");
    static idf_excl_cache excl;
    static const std::string name = std::string(WAVES == 8 ? "rowblock8_kernel<" : "rowblock_kernel<") + (QAN ? "QaN" : "std") + ", split-f16" +
                                    (WAVES == 4 ? "" : TV == 8 ? ", 8 tokens" : ", 16 tokens") + (MS == MEM ? "" : ", any memory length") + ">";
    constexpr int NP = QAN ? NSL : H;
    if constexpr (WAVES == 8) return idf_exclusive_cu(reinterpret_cast<const void *>(rowblock8_kernel<QAN, NP, MS, TV>), name.c_str(), 512, excl);
    else return idf_exclusive_cu(reinterpret_cast<const void *>(rowblock_kernel<QAN, true, NP, true, MS>), name.c_str(), 256, excl);
}
// both layer kinds of one form at each of the token counts TV (interdiff_exclusive_cu_report)
template <int WAVES, int MS, int... TV>
void rb_exclusive_forms() {
    ((rb_exclusive_dyn<true, MS, WAVES, TV>(), rb_exclusive_dyn<false, MS, WAVES, TV>()), ...);
}

// tokens per workgroup of the eight-wave row block: w->rb_tokens (8 / 16), or 0 = eight whenever the launch still fits the chip in one round of workgroups (the two forms
// compute the same bits: rowblock8_kernel)
inline int rb8_tokens(const idf_mdm_weights *w, int B, int T) {
    if (w->rb_tokens == 8 || w->rb_tokens == 16) return w->rb_tokens;
    return (int64_t)B * idf_cdiv(T, 8) <= idf_cu_count() ? 8 : 16;
}

// The route of a decoder row block, in order of preference: eight waves at tv8 tokens, four waves split-f16, exact fp32.  split_f16: the arithmetic is selected and
// the packer proved the layer's range (the caller's rb_h2); a split-f16 form must also get its CU here, and dyn_lds is what it is launched with.
enum class RbRoute { W8_T8, W8_T16, W4_H2, F32 };
template <bool QAN, int MS>
RbRoute rowblock_route(bool split_f16, int tv8, int &dyn_lds) {
    if (split_f16 && (dyn_lds = tv8 == 8 ? rb_exclusive_dyn<QAN, MS, 8, 8>() : rb_exclusive_dyn<QAN, MS, 8, 16>()) >= 0) return tv8 == 8 ? RbRoute::W8_T8 : RbRoute::W8_T16;
    if (split_f16 && (dyn_lds = rb_exclusive_dyn<QAN, MS, 4>()) >= 0) return RbRoute::W4_H2;
    dyn_lds = 0;
    return RbRoute::F32;
}
template <bool QAN, int MS>
void run_rowblock(hipStream_t s, const RowBlockArgs &a, bool split_f16, int tv8) {
    constexpr int NP = QAN ? NSL : H;
    int dyn = 0;
    switch (rowblock_route<QAN, MS>(split_f16, tv8, dyn)) {
    case RbRoute::W8_T8: launch_rowblock8<QAN, NP, MS, 8>(s, a, dyn); break;
    case RbRoute::W8_T16: launch_rowblock8<QAN, NP, MS, 16>(s, a, dyn); break;
    case RbRoute::W4_H2: launch_rowblock<QAN, true, NP, true, MS>(s, a, dyn); break;
    case RbRoute::F32:
        if constexpr (QAN) launch_rowblock_qan_f32<true, MS>(s, a);
        else launch_rowblock<false, true, H, false, MS>(s, a);
    }
}

}  // namespace
