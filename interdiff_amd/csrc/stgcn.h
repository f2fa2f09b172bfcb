// The ST-GCN layer (model/layers.py:339-345, sublayers.py:415-419,511-516) of the two correction predictors, the SMPL contact-frame
// one (csrc/objproj.h: 10 DCT coefficients, 68 nodes) and the HO-GCN skeleton one (csrc/skeleton.h: 20 coefficients, 22 nodes): the
// arena layer block and the three products of a layer.  Each predictor keeps its own layer schedule (two buffers / in place) around them.
// Activations are channel-major planes [c][k][node] in LDS, fp32 throughout; a 1024-thread workgroup (16 waves) runs every piece together.
//   - the 1x1 convolutions ([positions x cin] . [cin x cout]) and the per-coefficient adjacency product ([channels x nodes] . A_t)
//     run on the fp32 MFMA, the NP x NP temporal mix on the VALU,
//   - eval-mode BatchNorm is folded into the 1x1 convolutions on the host (interdiff_amd/stgcn_pack.py, which writes the block).
// Arena layer block (floats) of a layer with cin/cout channels over `nodes` nodes, cinp/coutp = channels rounded up to 16 (zero padded):
//   version 0 (stacks 0, 1): Tm[NP][NP]                               } rounded up to a multiple of 16 floats (zero padded):
//   version 2 (stack 2):     Tm[nodes][NP][NP]                        } NP = 10: 100 -> 112
//   version 2 only:          AT[NP][VP][VP]  (A transposed: [t][w][v], nodes zero padded to VP = whole MFMA tiles)
//   then Wt[coutp][cinp], bt[coutp], Wr[coutp][cinp], br[coutp], prelu[1]
#pragma once
#include "common.h"

namespace idf_stgcn {

constexpr int NTHR = 1024, NWAVE = NTHR / 64;

__device__ __forceinline__ int pad16(int x) { return (x + 15) & ~15; }
__device__ __forceinline__ float4 ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }

struct LayerP {
    const float *Tm, *AT, *Wt, *bt, *Wr, *br;
    float prelu;
};

template <int NP, int VP>
__device__ __forceinline__ LayerP layer_params(const float *blk, int cin, int cout, int nodes, bool v2) {
    // blocks start on 16 floats (the packer's add) and every piece is a multiple of 16 floats long: the float4 loads of AT and W are aligned
    static_assert(VP % 16 == 0, "the adjacency operand is whole MFMA tiles");
    const int cinp = pad16(cin), coutp = pad16(cout);
    LayerP p;
    p.Tm = blk;
    blk += pad16((v2 ? nodes : 1) * NP * NP);
    p.AT = v2 ? blk : nullptr;
    if (v2) blk += NP * VP * VP;
    p.Wt = blk; blk += coutp * cinp;
    p.bt = blk; blk += coutp;
    p.Wr = blk; blk += coutp * cinp;
    p.br = blk; blk += coutp;
    p.prelu = blk[0];
    return p;
}

// one 16x16 tile of a 1x1 convolution over channel-major planes: out[o][pos] = sum_c W[o][c] in[c][pos] (no bias)
// M = positions mt*16.., N = output channels nt*16.., K = input channels (zero-padded weights); lane (li, kq) gets
// rows mt*16 + kq*4 + r, column nt*16 + li.
__device__ __forceinline__ f32x4 conv_tile(const float *in, const float *W, int cin, int npos, int mt, int nt) {
    const int lane = threadIdx.x & 63, li = lane & 15, kq = lane >> 4;
    const int cinp = pad16(cin), pos = min(mt * 16 + li, npos - 1);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int c0 = 4 * kq; c0 < cinp; c0 += 16) {
        const float4 w = ld4(W + (nt * 16 + li) * cinp + c0);
        const float a0 = c0 + 0 < cin ? in[(c0 + 0) * npos + pos] : 0.f;
        const float a1 = c0 + 1 < cin ? in[(c0 + 1) * npos + pos] : 0.f;
        const float a2 = c0 + 2 < cin ? in[(c0 + 2) * npos + pos] : 0.f;
        const float a3 = c0 + 3 < cin ? in[(c0 + 3) * npos + pos] : 0.f;
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, w.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, w.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a2, w.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a3, w.w, acc, 0, 0, 0);
    }
    return acc;
}

// temporal mixing, in place on cin planes of NP * nodes floats: y[q] = sum_t x[t] Tm[(v)][t][q], t ascending (v2: one Tm per node)
template <int NP>
__device__ __forceinline__ void temporal_mix(float *buf, const float *Tm, int cin, int nodes, bool v2) {
    constexpr int W = NP % 4 == 0 ? 4 : 2;          // rows of Tm are NP floats apart: 16-byte aligned only when NP % 4 == 0
    static_assert(NP % W == 0, "Tm rows are read as float4 / float2");
    for (int i = threadIdx.x; i < cin * nodes; i += NTHR) {
        const int c = i / nodes, v = i - c * nodes;
        float *col = buf + c * NP * nodes + v;
        const float *tmv = Tm + (v2 ? v * NP * NP : 0);
        float y[NP];
#pragma unroll
        for (int q = 0; q < NP; ++q) y[q] = 0.f;
#pragma unroll 5
        for (int t = 0; t < NP; ++t) {              // x[t] read as it is needed, 5 per trip: unrolled fully, the loop spills in the skeleton
                                                    // layer (28 residual registers live) and in the contact scan that carries the SMPL stacks
            const float xt = col[t * nodes];
#pragma unroll
            for (int q = 0; q < NP; q += W) {
                typedef float row_t __attribute__((ext_vector_type(W)));
                const row_t tm = *reinterpret_cast<const row_t *>(tmv + t * NP + q);
#pragma unroll
                for (int e = 0; e < W; ++e) y[q + e] += xt * tm[e];
            }
        }
#pragma unroll
        for (int q = 0; q < NP; ++q) col[q * nodes] = y[q];
    }
}

// spatial mixing on the MFMA, in place: per coefficient t, Y[c][w] = sum_v X[c][t][v] A[t][v][w] (AT = A transposed, see above).
// One wave owns the rows (16 channels, one t) it writes and holds their X fragments in registers before it writes: no barrier inside.
template <int NP, int VP>
__device__ __forceinline__ void spatial_mix(float *buf, const float *AT, int cin, int nodes) {
    constexpr int NT = VP / 16;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, kq = lane >> 4;
    const int MT = pad16(cin) >> 4;
    for (int item = wave; item < MT * NP; item += NWAVE) {
        const int mt = item / NP, t = item - mt * NP, c = mt * 16 + li;
        float a[NT][4];
#pragma unroll
        for (int s4 = 0; s4 < NT; ++s4)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int v = 16 * s4 + 4 * kq + e;
                a[s4][e] = (c < cin && v < nodes) ? buf[(c * NP + t) * nodes + v] : 0.f;
            }
        f32x4 acc[NT];
#pragma unroll
        for (int wt = 0; wt < NT; ++wt) acc[wt] = f32x4{0.f, 0.f, 0.f, 0.f};
        const float *At = AT + (size_t)t * VP * VP;
#pragma unroll
        for (int s4 = 0; s4 < NT; ++s4) {
            f32x4 bw[NT];
#pragma unroll
            for (int wt = 0; wt < NT; ++wt) bw[wt] = *reinterpret_cast<const f32x4 *>(At + (wt * 16 + li) * VP + 16 * s4 + 4 * kq);
#pragma unroll
            for (int e = 0; e < 4; ++e)             // every acc[wt] sees s4 ascending, then .x .y .z .w: that order fixes the bits
#pragma unroll
                for (int wt = 0; wt < NT; ++wt) acc[wt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s4][e], bw[wt][e], acc[wt], 0, 0, 0);
        }
#pragma unroll
        for (int wt = 0; wt < NT; ++wt) {
            const int w = wt * 16 + li;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int cc = mt * 16 + kq * 4 + r;
                if (cc < cin && w < nodes) buf[(cc * NP + t) * nodes + w] = acc[wt][r];
            }
        }
    }
}

}  // namespace idf_stgcn
