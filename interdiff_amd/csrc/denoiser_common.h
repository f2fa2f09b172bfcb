// What the denoiser's kernel families (rowblock.h, attn.h, memfold.h) and its host code (denoiser.hip) share: the model's dimensions, the layout of the folded
// cross-attention memory (MemLay), the XCD-affine workgroup order and the MFMA round helpers.  Everything sits in the anonymous namespace of the ONE product
// translation unit that includes these headers (denoiser.hip; tools/rowblock_probe.hip includes that file whole).
#pragma once
#include "common.h"
#include "gemm.h"
#include "ffn_h2.h"

namespace {

using namespace idf_gemm;

constexpr int D = IDF_MDM_D;          // 256
constexpr int H = IDF_MDM_HEADS;      // 4
constexpr int HD = D / H;             // 64
constexpr int NQ = IDF_MDM_NQ;        // 10
constexpr int MEM = IDF_MDM_MEM;      // 10: the memory length of every BASELINE config -- the COMPACT layout of the folded memory below
constexpr int MEMX = IDF_MDM_MEM_MAX; // 16: longest memory the generic layout takes (eval_smpl_short.py:376 --past_len is a CLI argument)
constexpr int HM = H * MEM;           // 40
constexpr int HMP = 48;               // HM padded to a multiple of 16 (k-groups of the P.VW contraction)
// Layout of the folded memory's (head, slot) score columns, by the template parameter MS of the kernels that touch it:
//   MS == MEM (compact, the shipped fast path):  column = head * 10 + slot, 40 columns in 3 tiles of 16 (8 zero columns);
//   MS == MEMX (generic, any memory length 1..16 given at run time):  column = head * 16 + slot, one 16-column tile per head, slots >= mem_len masked.
// Everything that depends on it -- fragment sizes, column tiles, slots per softmax lane -- comes from here; with MS == MEM every expression below folds to
// the constants the kernels had before the generic path existed (same instructions, same bits).
template <int MS>
struct MemLay {
    static_assert(MS == MEM || MS == MEMX, "compact or generic");
    static constexpr bool GEN = MS != MEM;
    static constexpr int NCT = GEN ? 4 : 3;                 // 16-column tiles of the score matrix
    static constexpr int HMPX = 16 * NCT;                   // padded score columns = K of the P.VW contraction (fp32 form)
    static constexpr int NSLOT = GEN ? 4 : 3;               // memory slots per lane of the head softmax (quad q takes slots q, q + 4, ...)
    static constexpr int G0N = GEN ? 64 : HM;               // g0 floats per (layer, clip), indexed like the columns
    static constexpr int G_FRAG = 4 * 4 * NCT * 64 * 4;     // fp32 G fragments per (layer, clip)
    static constexpr int G_H2 = 4 * 2 * NCT * 2 * 64 * 4;   // split-f16 G plane fragments (as floats)
    static constexpr int VWT_F = D * HMPX;                  // fp32 VW fragments
    __host__ __device__ static constexpr int col(int h, int m) { return GEN ? h * 16 + m : h * MEM + m; }
};
constexpr int L = IDF_MDM_LAYERS;
constexpr int NSL = IDF_FFN_SLICES;   // partial output slabs of the fused FFN (ffn.h)

// XCD-affine workgroup order for the kernels below (speed only; any order is correct): workgroup `id` of a launch runs on XCD
// id % 8 and every XCD has its own L2, so the LOGICAL index is permuted to make one XCD work through consecutive logical
// workgroups -- the 7 token tiles of a clip (which all read the clip's folded memory G[b] / VW[b]) or the 4 query tiles of a
// (clip, head) (which all read its K and V) then fetch those operands into ONE L2 instead of up to eight.  Each XCD reaches
// HBM / Infinity Cache at only ~1/8 of the chip's rate, and at one workgroup per CU that fetch is most of what these kernels wait for.
__device__ __forceinline__ int xcd_logical_id() {
    const int nwg = gridDim.x * gridDim.y * gridDim.z, id = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
    const int q = nwg >> 3, r = nwg & 7, xcd = id & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (id >> 3);
}

// four dependent-free rounds of MFMAs over NA accumulators: acc[i] += a[i](k-group) . b[i](k-group)
template <int NA>
__device__ __forceinline__ void mma_rounds(f32x4 (&acc)[NA], const float4 (&a)[NA], const float4 (&b)[NA]) {
#pragma unroll
    for (int i = 0; i < NA; ++i) IDF_MFMA4(acc[i], a[i].x, b[i].x);
#pragma unroll
    for (int i = 0; i < NA; ++i) IDF_MFMA4(acc[i], a[i].y, b[i].y);
#pragma unroll
    for (int i = 0; i < NA; ++i) IDF_MFMA4(acc[i], a[i].z, b[i].z);
#pragma unroll
    for (int i = 0; i < NA; ++i) IDF_MFMA4(acc[i], a[i].w, b[i].w);
}

// LayerNorm with gamma / beta read from LDS (staged there by DMA at kernel entry; same arithmetic as common.h ln_row16): lane l16
// of a 16-lane row group handles the chunks {l16, 16+l16, 32+l16, 48+l16} of its row
__device__ __forceinline__ void ln_row16_lds(Row16 &r, const float *w, const float *b, int l16) {
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) sum += (r.c[i].x + r.c[i].y) + (r.c[i].z + r.c[i].w);
    const float mean = row16_sum(sum) * (1.0f / 256.0f);
    float qv = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float a0 = r.c[i].x - mean, a1 = r.c[i].y - mean, a2 = r.c[i].z - mean, a3 = r.c[i].w - mean;
        qv += (a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3);
    }
    const float rstd = __builtin_amdgcn_rsqf(row16_sum(qv) * (1.0f / 256.0f) + 1e-5f);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float4 g = *reinterpret_cast<const float4 *>(w + (i * 16 + l16) * 4), be = *reinterpret_cast<const float4 *>(b + (i * 16 + l16) * 4);
        r.c[i].x = (r.c[i].x - mean) * rstd * g.x + be.x;
        r.c[i].y = (r.c[i].y - mean) * rstd * g.y + be.y;
        r.c[i].z = (r.c[i].z - mean) * rstd * g.z + be.z;
        r.c[i].w = (r.c[i].w - mean) * rstd * g.w + be.w;
    }
}

using idf_ffn_h2::row16_store_planes;
// one K = 32 step of a split-f16 product on NA tiles: main += ah.bh, corr += ah.bl' + al'.bh   (result = main + corr 2^-11)
template <int NA>
__device__ __forceinline__ void mma_h2(f32x4 (&am)[NA], f32x4 (&ac)[NA], const idf_ffn_h2::h8 (&ah)[NA], const idf_ffn_h2::h8 (&al)[NA],
                                       const float4 (&bh)[NA], const float4 (&bl)[NA]) {
    using idf_ffn_h2::h8;
#pragma unroll
    for (int i = 0; i < NA; ++i) IDF_H2_MFMA(am[i], ah[i], __builtin_bit_cast(h8, bh[i]));
#pragma unroll
    for (int i = 0; i < NA; ++i) IDF_H2_MFMA(ac[i], ah[i], __builtin_bit_cast(h8, bl[i]));
#pragma unroll
    for (int i = 0; i < NA; ++i) IDF_H2_MFMA(ac[i], al[i], __builtin_bit_cast(h8, bh[i]));
}

}  // namespace
