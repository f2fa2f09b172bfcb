// MDM denoiser, decoder path, for gfx950 (rows A1-A4 of SURVEY.md §8).
//
// Reference behaviour restated: model/diffusion_smpl.py:226-246 (_decode/forward),
// model/sublayers.py:311-375 (QaN layer), torch.nn.TransformerDecoderLayer (post-norm, gelu).
// NOT a translation: the reference runs ~40 eager torch kernels per layer over [T,B,D]
// tensors and re-projects the constant memory every step.  Here
//   * tokens are clip-major rows (row = b*T + t) of [N,256] fp32 matrices that stay L2-resident,
//   * EVERY contraction runs on the matrix pipe.  Exact form: the fp32 MFMA (v_mfma_f32_16x16x4_f32) -- the six token GEMMs (gemm.h), the temporal
//     self-attention (QK^T and PV), and the whole "row block" between two FFNs: learned-query local attention, LayerNorms and the cross attention to the
//     10-token memory.  Shipped form (tune[IDF_TUNE_FFN_MATH] = 1, round 4): the feed-forward block, the QKV projection, the row block's contractions and the
//     two token GEMMs at the ends of a step as split-f16 products on v_mfma_f32_16x16x32_f16 (ffn_h2.h, tail_h2.h: every fp32 operand as two f16 planes, three
//     MFMAs per product, fp32 accumulate: fp32-grade results); the self-attention stays on the fp32 MFMA (attn_h2.h: its split-f16 form measured slower),
//   * the learned-query local attention collapses to a [16 x 256] x [256 x 30] contraction with
//     constant pre-rotated queries Qc (interdiff_amd/mdm.py: qan_constants) + a 3-tap stencil,
//   * cross-attention to the constant memory is folded per sample into
//     scores = x.G^T + g0 and out = P.VW (interdiff_mdm_prepare_memory),
//   * LayerNorm never gets its own launch: the row-block kernel owns whole rows (LN_prev on load,
//     LN1, LN2 in place) and the QKV / heads kernels normalise on load.
//   * the feed-forward block is ONE launch (ffn.h / ffn_h2.h): linear1 -> gelu -> linear2 per (32-row tile, hidden slice), the hidden
//     activations never leave the CU; it leaves IDF_FFN_SLICES partial slabs that the next reader sums on load.
// Per step: embedding + 2 x 4 (standard layers: QKV, self-attention + out-projection, row block, FFN) + 6 x 2 (QaN layers: row block, FFN) + heads = 22 launches;
// 21 inside a captured run of plain steps, where a step's last launch also computes the next step's embedding (tail_h2.h).
// This file: workspace carving, the encoder and decoder loops, the C entry points.  The kernels live next to their launchers, one header per family:
// gemm.h, ffn.h / ffn_h2.h, tail_h2.h, attn_h2.h and -- the families that are this translation unit's own -- rowblock.h, attn.h, memfold.h.
#include "common.h"
#include "gemm.h"
#include "ffn.h"
#include "ffn_h2.h"
#include "tail_h2.h"
#include "attn_h2.h"
#include "denoiser_common.h"
#include "rowblock.h"
#include "attn.h"            // (memfold.h: further down, between the explicit instantiations)

// tune entries other than IDF_TUNE_FFN and IDF_TUNE_FFN_MATH are reserved (include/interdiff_hip.h): a handle that sets one is refused
static inline bool idf_tune_reserved_clear(const idf_mdm_weights *w) {
    for (int i = 0; i < 8; ++i)
        if (i != IDF_TUNE_FFN && i != IDF_TUNE_FFN_MATH && w->tune[i] != 0) return false;
    return true;
}

// the feed-forward block of one layer: arithmetic by tune[IDF_TUNE_FFN_MATH] (and whether the packer set the layer's split-f16 stream),
// row tile by tune[IDF_TUNE_FFN] (0: by this launch's rows)
static inline int idf_launch_layer_ffn(hipStream_t s, const idf_mdm_layer &ly, const float *ar, const int32_t *tune, const float *x2, int M, float *parts) {
    int rows = idf_ffn::ffn_rows_of_tune(tune[IDF_TUNE_FFN]);
    if (tune[IDF_TUNE_FFN_MATH] != 0 && ly.ffn_pack_h2 != 0) {
        const int rc = idf_ffn_h2::launch_ffn_h2(s, x2, M, ar + ly.ffn_pack_h2, ar + ly.ffn_b1p, ar + ly.ff2_b, parts, rows ? rows : idf_ffn::ffn_tile_for_rows(M));
        if (rc != IDF_NOT_EXCLUSIVE) return rc;        // (the kernel does not get its CU on this device -- common.h idf_exclusive_cu: the exact kernel below)
    }
    idf_ffn::launch_ffn(s, x2, M, ar + ly.ffn_pack, ar + ly.ffn_b1p, ar + ly.ff2_b, parts, rows);
    return IDF_OK;
}

namespace {

struct Ws {
    float *uA, *uB, *xn, *x2, *ctx, *qkv, *parts;
};
constexpr size_t WS_ROW_FLOATS = (size_t)(5 + 3 + NSL) * D;      // uA uB xn x2 ctx | qkv | FFN partial slabs
Ws carve(void *ws, int64_t N) {
    float *p = reinterpret_cast<float *>(ws);
    Ws r;
    r.uA = p; p += N * D;
    r.uB = p; p += N * D;
    r.xn = p; p += N * D;
    r.x2 = p; p += N * D;
    r.ctx = p; p += N * D;
    r.qkv = p; p += N * 3 * D;
    r.parts = p;
    return r;
}

// tile configurations of the standalone token GEMM (interdiff_gemm_f32: the LDS-DMA pipeline of gemm.h).  The default per
// epilogue was picked on MI355X with tools/gemm_probe.hip + tools/kbench.py (profiles/).  Config ids: BM x BN, waves,
// k-slices per workgroup (ks), chunk depth (kc).
template <int APRO, int EPI, int NP = 1>
void run_gemm(int cfg, hipStream_t s, const Args &g) {
    switch (cfg) {
    case 1: launch_glds<32, 64, 2, 2, 1, 32, APRO, EPI, 3, NP>(s, g); break;
    case 2: launch_glds<32, 64, 2, 2, 1, 64, APRO, EPI, 3, NP>(s, g); break;
    case 3: launch_glds<32, 64, 2, 2, 2, 64, APRO, EPI, 3, NP>(s, g); break;
    case 4: launch_glds<64, 64, 2, 2, 1, 32, APRO, EPI, 3, NP>(s, g); break;
    case 5: launch_glds<32, 32, 2, 2, 1, 64, APRO, EPI, 3, NP>(s, g); break;
    case 6: launch_glds<32, 32, 2, 2, 2, 64, APRO, EPI, 3, NP>(s, g); break;
    case 7: launch_glds<64, 32, 2, 2, 1, 32, APRO, EPI, 3, NP>(s, g); break;
    case 8: launch_glds<64, 32, 2, 2, 2, 64, APRO, EPI, 3, NP>(s, g); break;
    case 9: launch<32, 64, 2, 2, 32, APRO, EPI, NP>(s, g); break;               // register-staged double buffer
    default: launch_glds<32, 64, 2, 2, 1, 32, APRO, EPI, 3, NP>(s, g); break;
    }
}
constexpr int CFG_FFN1 = 7, CFG_FFN2 = 6;
inline int pick(int cfg, int dflt) { return cfg ? cfg : dflt; }
// the heads GEMM of the fp32 route (A_LN: the layer input is one matrix or the previous layer's NSL partial slabs), configuration 6 of run_gemm; with the sampler
// update in its epilogue (gemm.h E_HEADS_POST) when post is set -- clip lengths that are not a multiple of 4 take the per-row form of the update
template <int NP>
void run_heads_np(hipStream_t s, const Args &g, bool post) {
    if (!post) launch_glds<32, 32, 2, 2, 2, 64, A_LN, E_HEADS, 3, NP>(s, g);
    else if (g.T & 3) launch_glds<32, 32, 2, 2, 2, 64, A_LN, E_HEADS_POST_RAGGED, 3, NP>(s, g);
    else launch_glds<32, 32, 2, 2, 2, 64, A_LN, E_HEADS_POST, 3, NP>(s, g);
}
void run_heads(hipStream_t s, const Args &g, int np, bool post) {
    if (np == NSL) run_heads_np<NSL>(s, g, post);
    else run_heads_np<1>(s, g, post);
}
// the same GEMM with the skeleton denoiser's keypoint head in its epilogue (skel_head.h); the layer input is always the feed-forward's NSL slabs
void run_skel_heads(hipStream_t s, const Args &g, bool post) {
    if (!post) launch_glds<32, 32, 2, 2, 2, 64, A_LN, E_SKEL, 3, NSL>(s, g);
    else if (g.T & 3) launch_glds<32, 32, 2, 2, 2, 64, A_LN, E_SKEL_POST_RAGGED, 3, NSL>(s, g);
    else launch_glds<32, 32, 2, 2, 2, 64, A_LN, E_SKEL_POST, 3, NSL>(s, g);
}
// QKV projection: the LayerNorm+linear kernel of ffn.h
// step_state != null (layer 0 of interdiff_mdm_forward_step): one thread of the launch does the step's sampler bookkeeping (philox.h)
// pack_h2 != null: the split-f16 form (ffn_h2.h ln_linear_h2_kernel: tune[IDF_TUNE_FFN_MATH] == 1 and the layer's sa_in_pack_h2 is set)
// planes / scales != null (with pack_h2): the output leaves as the self-attention's f16 plane pairs + per-row scales instead of fp32 rows (ffn_h2.h ln_linear_h2_kernel<.., PLANES>);
// the caller has checked (qkv_planes_ok) that this kernel and the attention kernel that reads the planes both run here -- there is no fp32 fallback behind a planes launch
int run_qkv(hipStream_t s, const Args &g, const float *pack, int np, int64_t *step_state = nullptr, int64_t *step_ts = nullptr,
            int step_B = 0, const float *pack_h2 = nullptr, float *planes = nullptr, float *scales = nullptr, const int64_t *step_tmap = nullptr) {
    if (planes) {
        if (!pack_h2) return IDF_E_INVAL;
        const int rc = np == NSL ? idf_ffn_h2::launch_ln_linear_h2<NSL>(s, g.A, g.a_pstride, g.lnw, g.lnb, g.M, g.N, pack_h2, g.bias, g.C, g.ldc, g.xn_out, step_state, step_ts, step_B, planes, scales, step_tmap)
                                 : idf_ffn_h2::launch_ln_linear_h2<1>(s, g.A, g.a_pstride, g.lnw, g.lnb, g.M, g.N, pack_h2, g.bias, g.C, g.ldc, g.xn_out, step_state, step_ts, step_B, planes, scales, step_tmap);
        return idf_public_rc(rc);
    }
    if (pack_h2) {
        const int rc = np == NSL ? idf_ffn_h2::launch_ln_linear_h2<NSL>(s, g.A, g.a_pstride, g.lnw, g.lnb, g.M, g.N, pack_h2, g.bias, g.C, g.ldc, g.xn_out, step_state, step_ts, step_B, nullptr, nullptr, step_tmap)
                                 : idf_ffn_h2::launch_ln_linear_h2<1>(s, g.A, g.a_pstride, g.lnw, g.lnb, g.M, g.N, pack_h2, g.bias, g.C, g.ldc, g.xn_out, step_state, step_ts, step_B, nullptr, nullptr, step_tmap);
        if (rc != IDF_NOT_EXCLUSIVE) return rc;        // (not exclusive on this device: the fp32 kernel below)
    }
    if (np == NSL)
        idf_ffn::launch_ln_linear<NSL>(s, g.A, g.a_pstride, g.lnw, g.lnb, g.M, g.N, pack, g.bias, g.C, g.ldc, g.xn_out, step_state, step_ts, step_B, step_tmap);
    else
        idf_ffn::launch_ln_linear<1>(s, g.A, g.a_pstride, g.lnw, g.lnb, g.M, g.N, pack, g.bias, g.C, g.ldc, g.xn_out, step_state, step_ts, step_B, step_tmap);
    return IDF_OK;
}


// May the QKV projection of a standard layer hand the self-attention PLANES (np = slabs of its input, T = clip length)?  Both kernels of the pair must get their CUs here.
bool qkv_planes_ok(int np, int B, int T) {
    float dummy = 0.f;
    const int rq = np == NSL ? idf_ffn_h2::launch_ln_linear_h2<NSL>(nullptr, nullptr, 0, nullptr, nullptr, 0, 3 * D, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, &dummy, &dummy)
                             : idf_ffn_h2::launch_ln_linear_h2<1>(nullptr, nullptr, 0, nullptr, nullptr, 0, 3 * D, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, &dummy, &dummy);
    return rq == IDF_OK && idf_attn_h2::launch_self_attn_h2(nullptr, nullptr, B, T, nullptr, nullptr, 0, nullptr, true) == IDF_OK;
}

// ---- The seven kernels of a plain denoising step at the shipped shapes, instantiated HERE, next to each other (two inside this namespace, five right behind it).  Explicit
// instantiations are emitted where they stand, so the seven end up CONTIGUOUS in the code object (57 KB); implicit ones land wherever the compiler gets to them -- scattered over
// this file's 1.1 MB of code, where 16-39 % of their cache lines shared an instruction-cache set with more lines than it has ways (64 KB per CU pair; a step cycles through all
// seven kernels, 22 launches at a time: with LRU such a set misses on every pass).  Contiguous code maps onto the cache without a collision.
// (Which instantiations: mdm_forward_impl_t at B = 16, T = 100, memory length 10.)
template __global__ void rowblock8_kernel<false, H, MEM, 8>(const float *, int, int, int, int, size_t, const float *, const float *, const float *, const float *, const float *, const float *,
                                                            const float *, const float *, const float *, const float *, const float *, const float *, const float *, float *, const float *,
                                                            const float *);
template __global__ void rowblock8_kernel<true, NSL, MEM, 8>(const float *, int, int, int, int, size_t, const float *, const float *, const float *, const float *, const float *, const float *,
                                                             const float *, const float *, const float *, const float *, const float *, const float *, const float *, float *, const float *,
                                                             const float *);
}  // namespace
// memfold.h is included HERE, not with the other headers: its mem_kv_kernel is not a template, so it is emitted where its namespace closes -- behind the two
// instantiations above and ahead of the five below, where it stood when all of this was one file: the code object keeps its layout.  Nothing above uses the header.
#include "memfold.h"
template __global__ void idf_attn_h2::self_attn_h2_kernel<0, true>(const float *, int, int, const float *, float *, size_t, const float *);
template __global__ void idf_ffn_h2::ffn_h2_kernel<2, 4, 0, 8>(const float *, int, int, const float *, const float *, const float *, float *, int);
template __global__ void idf_ffn_h2::ln_linear_h2_kernel<1, true>(const float *, size_t, int, int, const float *, const float *, const float *, int, int, const float *, float *, int, int, float *,
                                                                  int64_t *, int64_t *, float *, float *, const int64_t *);
template __global__ void idf_ffn_h2::ln_linear_h2_kernel<IDF_FFN_SLICES, true>(const float *, size_t, int, int, const float *, const float *, const float *, int, int, const float *, float *, int,
                                                                               int, float *, int64_t *, int64_t *, float *, float *, const int64_t *);
template __global__ void idf_tail_h2::step_tail_h2_kernel<3, false>(const float *, size_t, const float *, int, int, int, int, const idf_tail_h2::TailArgs);

extern "C" int interdiff_mdm_ffn(const idf_mdm_weights *w, int32_t layer, int32_t encoder, const float *x2, int32_t M, float *parts,
                                 void *stream) {
    if (!w || !x2 || !parts || M <= 0 || layer < 0 || layer >= L || (encoder && !w->has_encoder) || !idf_tune_reserved_clear(w)) return IDF_E_INVAL;
    if ((reinterpret_cast<uintptr_t>(x2) & 15) || (reinterpret_cast<uintptr_t>(parts) & 15)) return IDF_E_INVAL;
    const idf_mdm_layer &ly = encoder ? w->enc_layer[layer] : w->layer[layer];
    const int rc = idf_launch_layer_ffn(idf_stream(stream), ly, w->arena, w->tune, x2, M, parts);
    if (rc != IDF_OK) return rc;
    IDF_CHECK_LAUNCH();
    return IDF_OK;
}

// C[M,N] = epi(A[M,K] . W[N,K]^T + bias): the token GEMM of the denoiser as a standalone op (fp32 MFMA, LDS-DMA
// pipeline).  epi: 0 bias, 1 bias + erf-GELU, 2 bias + residual (resid has leading dimension ldc).  cfg 0 = the tile
// configuration the FFN call sites ship with.  K % 64 == 0, N % 16 == 0, lda / ldc % 4 == 0, A / C 16-byte aligned.
extern "C" int interdiff_gemm_f32(const float *A, int32_t lda, const float *W, const float *bias, const float *resid, float *C,
                                  int32_t ldc, int32_t M, int32_t N, int32_t K, int32_t epi, int32_t cfg, void *stream) {
    if (!A || !W || !C || M <= 0 || N <= 0 || K <= 0 || (K & 63) || (N & 15) || (epi == 2 && !resid) || epi < 0 || epi > 2) return IDF_E_INVAL;
    if ((ldc & 3) || (lda & 3) || (reinterpret_cast<uintptr_t>(C) & 15) || (reinterpret_cast<uintptr_t>(A) & 15)) return IDF_E_INVAL;   // 16-B row stores / loads
    Args g{};
    g.A = A; g.lda = lda; g.K = K; g.W = W; g.bias = bias; g.C = C; g.ldc = ldc; g.M = M; g.N = N; g.resid = resid; g.T = 1;
    hipStream_t s = idf_stream(stream);
    if (epi == 0) run_gemm<A_PLAIN, E_BIAS>(pick(cfg, CFG_FFN2), s, g);
    else if (epi == 1) run_gemm<A_PLAIN, E_GELU>(pick(cfg, CFG_FFN1), s, g);
    else run_gemm<A_PLAIN, E_RESID>(pick(cfg, CFG_FFN2), s, g);
    IDF_CHECK_LAUNCH();
    return IDF_OK;
}

extern "C" size_t interdiff_mdm_memctx_floats(int32_t B) { return memctx_floats_t<MEM>(B); }
extern "C" size_t interdiff_mdm_memctx_floats_for(int32_t B, int32_t mem_len) {
    if (mem_len < 1 || mem_len > MEMX) return 0;
    return mem_len == MEM ? memctx_floats_t<MEM>(B) : memctx_floats_t<MEMX>(B);
}

extern "C" size_t interdiff_mdm_workspace_bytes(int32_t B, int32_t T) {
    const size_t N = (size_t)B * T;
    const size_t fwd = N * WS_ROW_FLOATS * sizeof(float);
    const size_t prep = (size_t)L * MEMX * B * 512 * sizeof(float);         // interdiff_mdm_prepare_memory's K/V projections at the longest memory
    return idf_align(fwd > prep ? fwd : prep);
}


// cond [mem_len,B,256] with mem_len = w->mem_len (0 = IDF_MDM_MEM = 10): the reference takes the memory length from the command line (eval_smpl_short.py:376
// --past_len; model/diffusion_smpl.py:195-223 encodes that many past frames).  Length 10 -- every BASELINE config -- takes the compact layout of the folded memory
// (40 score columns); any other length 1 .. IDF_MDM_MEM_MAX a generic one (64 columns, one 16-column tile per head, absent slots masked): same kernels, one more
// column tile in the row block.  memctx must hold interdiff_mdm_memctx_floats_for(B, mem_len) floats.
extern "C" int interdiff_mdm_prepare_memory(const idf_mdm_weights *w, const float *cond, int32_t B, float *memctx,
                                            void *ws, size_t ws_bytes, void *stream) {
    if (!w || !cond || !memctx || !ws || B <= 0 || w->mem_len < 0 || w->mem_len > MEMX) return IDF_E_INVAL;
    return idf_mem_len(w) == MEM ? prepare_memory_t<MEM>(w, cond, B, memctx, ws, ws_bytes, idf_stream(stream))
                                 : prepare_memory_t<MEMX>(w, cond, B, memctx, ws, ws_bytes, idf_stream(stream));
}

namespace {
__global__ void iota_kernel(int64_t *p, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = i;
}
}  // namespace

extern "C" size_t interdiff_mdm_encode_workspace_bytes(int32_t B, int32_t Tp) {
    const size_t N = (size_t)B * Tp;
    return idf_align(N * WS_ROW_FLOATS * sizeof(float)) + idf_align((size_t)B * sizeof(int64_t));
}

// Encoder side: u0 = [body | obj].W_in^T + b_in + pc[b] + pe[t] over the Tp past frames, then the 8 encoder layers
// (model/diffusion_smpl.py:217-221).  Same kernels as the decoder; the row block runs without the cross-attention
// phases, the last LayerNorm writes the frame-major [Tp,B,256] layout the decoder's memory folding expects.
extern "C" int interdiff_mdm_encode(const idf_mdm_weights *w, const float *pc, const float *x_past, int32_t B, int32_t Tp,
                                    float *cond, void *ws, size_t ws_bytes, void *stream) {
    if (!w || !pc || !x_past || !cond || !ws || B <= 0 || Tp <= 0) return IDF_E_INVAL;
    if (!w->has_encoder || Tp > w->max_T || w->C > 256 || w->C < 1 || !idf_tune_reserved_clear(w)) return IDF_E_INVAL;
    if (ws_bytes < interdiff_mdm_encode_workspace_bytes(B, Tp)) return IDF_E_NOMEM;
    hipStream_t s = idf_stream(stream);
    const float *ar = w->arena;
    const int N = B * Tp, C = w->C, T = Tp;
    Ws k = carve(ws, N);
    int64_t *iota = reinterpret_cast<int64_t *>(reinterpret_cast<char *>(ws) + idf_align((size_t)N * WS_ROW_FLOATS * sizeof(float)));
    hipLaunchKernelGGL(iota_kernel, dim3((unsigned)idf_cdiv(B, 256)), dim3(256), 0, s, iota, B);
    {
        Args g{};
        g.A = x_past; g.K = (C + 3) & ~3; g.Ka = C; g.W = ar + w->in_w; g.bias = ar + w->in_b; g.C = k.uA; g.ldc = D; g.M = N; g.N = D; g.T = T;
        g.ts = iota; g.temb = pc; g.pe = ar + w->pe; g.n_steps = B;            // "+ temb[ts[b]]" adds pc[b]
        if (C & 3) launch<32, 64, 2, 2, 32, A_TOKT_R, E_EMBED>(s, g);           // (W_in is packed with its rows zero-padded to a multiple of 4: mdm.py)
        else launch<32, 64, 2, 2, 32, A_TOKT, E_EMBED>(s, g);
    }
    const float *u_in = k.uA;                  // layer input: plain [N,256] for layer 0, then the FFN's partial slabs
    int u_np = 1;
    const size_t pstride = (size_t)N * D;
    const float *lnp_w = nullptr, *lnp_b = nullptr;
    if (attn_opt_in() != IDF_OK) return IDF_E_LAUNCH;
    RowBlockArgs rb0{};                        // no cross attention here: the folded memory, LN2 and the output bias stay null
    rb0.pstride = pstride; rb0.mem_len = MEM; rb0.out = k.x2; rb0.B = B; rb0.T = T;
    for (int l = 0; l < L; ++l) {
        const idf_mdm_layer &ly = w->enc_layer[l];
        RowBlockArgs rb = rb0;
        rb.ln1_w = ar + ly.ln_w[0]; rb.ln1_b = ar + ly.ln_b[0];
        if (ly.is_qan) {
            rb.u_in = u_in; rb.np = u_np; rb.lnp_w = lnp_w; rb.lnp_b = lnp_b; rb.qc = ar + ly.qc; rb.wk = ar + ly.wk;
            launch_rowblock_qan_f32<false, MEM>(s, rb);
        } else {
            Args g{};
            g.A = u_in; g.lda = D; g.K = D; g.lnw = lnp_w; g.lnb = lnp_b; g.W = ar + ly.sa_in_w; g.bias = ar + ly.sa_in_b;
            g.C = k.qkv; g.ldc = 3 * D; g.M = N; g.N = 3 * D; g.xn_out = k.xn; g.T = T; g.a_pstride = pstride;
            if (const int rc = run_qkv(s, g, ar + ly.sa_in_pack, u_np, nullptr, nullptr, 0,
                                       (w->tune[IDF_TUNE_FFN_MATH] != 0 && ly.sa_in_pack_h2) ? ar + ly.sa_in_pack_h2 : nullptr); rc != IDF_OK) return rc;
            launch_self_attn_outproj(s, k.qkv, B, T, ar + ly.sa_out_frag, k.parts, pstride);
            rb.u_in = k.parts; rb.np = H; rb.sa_resid = k.xn; rb.sa_bias = ar + ly.sa_out_b;
            launch_rowblock<false, false, H, false, MEM>(s, rb);
        }
        if (const int rc = idf_launch_layer_ffn(s, ly, ar, w->tune, k.x2, N, k.parts); rc != IDF_OK) return rc;
        u_in = k.parts;
        u_np = NSL;
        lnp_w = ar + ly.ln_w[1];
        lnp_b = ar + ly.ln_b[1];
    }
    // cond[t][b][:] = LN2_last(u[b*T + t])
    RowBlockArgs rb = rb0;
    rb.u_in = u_in; rb.np = NSL;                   // after 8 layers u_in is always the slabs
    rb.ln1_w = lnp_w; rb.ln1_b = lnp_b; rb.out = cond; rb.frame_major = 1;
    launch_rowblock<false, false, NSL, false, MEM>(s, rb);
    IDF_CHECK_LAUNCH();
    return IDF_OK;
}

namespace {
// the sampler-step operands of interdiff_mdm_forward_step (null x: plain forward, x0 written out)
struct StepPost {
    float *x;
    const float *gt;
    const uint8_t *mask;
    const float *table;
    int64_t *state, *ts;
    const int64_t *tmap;          // respaced schedule: the model's timestep of every loop-side step (philox.h); null = identity
};
// the skeleton model's head (interdiff_skeleton_mdm_*): null h = the two plain linears of idf_mdm_weights
struct SkelHead {
    const idf_skel_head *h;
    const float *zero_pose_obj;
};

template <int MS>
int mdm_forward_impl_t(const idf_mdm_weights *w, const float *memctx, const float *x, const int64_t *ts, int32_t B, int32_t T, float *x0,
                       void *ws, size_t ws_bytes, void *stream, const StepPost &post, int32_t flags, const SkelHead &sk) {
    using ML = MemLay<MS>;
    constexpr int G_FRAG = ML::G_FRAG, G_H2 = ML::G_H2;
    const int mlen = idf_mem_len(w);
    if (!w || !memctx || !x || !ts || (!x0 && !post.x) || !ws || B <= 0 || T <= 0) return IDF_E_INVAL;
    if (T > w->max_T || w->C > 256 || w->C < 1 || mlen < 1 || mlen > MEMX || (MS == MEM) != (mlen == MEM)) return IDF_E_INVAL;
    if (ws_bytes < interdiff_mdm_workspace_bytes(B, T)) return IDF_E_NOMEM;
    hipStream_t s = idf_stream(stream);
    const float *ar = w->arena;
    const int N = B * T, C = w->C;
    Ws k = carve(ws, N);
    const MemCtx mc = memctx_carve<MS>(memctx, B);
    const int32_t *tune = w->tune;

    // The two ends of the step as split-f16 "step tail" launches (tail_h2.h): with the split arithmetic, the SMPL token width and the packer's plane
    // fragments.  flags (interdiff_mdm_forward_step_ex) then chain consecutive plain steps: IDF_STEP_EMBED_READY = the previous call's tail has already
    // written this step's embedding into the workspace, IDF_STEP_EMBED_NEXT = this call's tail writes the next step's.  Ignored otherwise.
    const bool tail_h2 = !sk.h && tune[IDF_TUNE_FFN_MATH] != 0 && w->out_w_h2 != 0 && w->in_w_h2 != 0 && C == idf_tail_h2::CW && w->tail_h2_ok != 0 && idf_tail_h2::tail_exclusive_ok((T & 3) != 0);
    idf_tail_h2::TailArgs ta{};
    if (tail_h2) {
        ta.win = ar + w->in_w_h2; ta.in_b = ar + w->in_b; ta.temb = ar + w->temb_table; ta.pe = ar + w->pe; ta.ts = ts; ta.n_steps = w->n_steps;
        ta.u0 = k.uA; ta.M = N; ta.T = T; ta.x_tok = x;
        if (!(post.x && (flags & IDF_STEP_EMBED_READY))) {
            idf_prof_mark(IDF_K_EMBED, s);
            if (const int rc = idf_tail_h2::launch_tail(s, 0, ta); rc != IDF_OK) return idf_public_rc(rc);      // (tail_exclusive_ok was asked first: IDF_NOT_EXCLUSIVE cannot come back, and never leaves the library if it does)
        }
    } else
    {   // u0 = [x_body | x_obj].W_in^T + b_in + temb[ts] + pe   (tokens gathered from x[b][c][t])
        Args g{};
        // token width C: any (BASELINE config #1, the HO-GCN skeleton tokens of model/diffusion_skeleton.py:236-253, has C = 106); W_in is packed
        // with rows of (C + 3) & ~3 floats, zero-padded (mdm.py), and a width that is no multiple of 4 takes the guarded gather (gemm.h A_TOKT_R)
        g.A = x; g.K = (C + 3) & ~3; g.Ka = C; g.W = ar + w->in_w; g.bias = ar + w->in_b; g.C = k.uA; g.ldc = D; g.M = N; g.N = D; g.T = T;
        g.ts = ts; g.temb = ar + w->temb_table; g.pe = ar + w->pe; g.n_steps = w->n_steps;
        idf_prof_mark(IDF_K_EMBED, s);
        if (C & 3) launch<32, 64, 2, 2, 32, A_TOKT_R, E_EMBED>(s, g);
        else launch<32, 64, 2, 2, 32, A_TOKT, E_EMBED>(s, g);
    }
    const float *u_in = k.uA;                  // layer input (pre-norm sum of the previous layer): plain for layer 0, then FFN partial slabs
    int u_np = 1;
    const size_t pstride = (size_t)N * D;
    const float *lnp_w = nullptr, *lnp_b = nullptr;   // LayerNorm still to be applied to u_in (none for layer 0)
    if (attn_opt_in() != IDF_OK) return IDF_E_LAUNCH;
    const int tv8 = rb8_tokens(w, B, T);
    RowBlockArgs rb0{};
    rb0.pstride = pstride; rb0.mem_len = mlen; rb0.out = k.x2; rb0.B = B; rb0.T = T;
    for (int l = 0; l < L; ++l) {
        const idf_mdm_layer &ly = w->layer[l];
        // split-f16 row block: tune[IDF_TUNE_FFN_MATH] == 1 (2 = split-f16 feed-forward and QKV only), for layers whose LayerNorm outputs the packer proved to stay in the f16 range
        const bool rb_h2 = tune[IDF_TUNE_FFN_MATH] == 1 && ly.rb_h2_ok != 0 && (!ly.is_qan || (ly.qc_h2 != 0 && u_np == NSL));
        RowBlockArgs rb = rb0;
        rb.ln1_w = ar + ly.ln_w[0]; rb.ln1_b = ar + ly.ln_b[0]; rb.ln2_w = ar + ly.ln_w[1]; rb.ln2_b = ar + ly.ln_b[1]; rb.ca_out_b = ar + ly.ca_out_b;
        rb.G = mc.G + (size_t)l * B * G_FRAG; rb.VWT = mc.VWT + (size_t)l * B * ML::VWT_F; rb.g0 = mc.g0 + (size_t)l * B * ML::G0N;
        rb.Gh2 = mc.Gh2 + (size_t)l * B * G_H2; rb.VWh2 = mc.VWh2 + (size_t)l * B * VW_H2; rb.sc = mc.sc + (size_t)l * B * 2;
        if (ly.is_qan) {
            idf_prof_mark(IDF_K_ROWBLOCK_QAN, s);
            rb.u_in = u_in; rb.np = u_np; rb.lnp_w = lnp_w; rb.lnp_b = lnp_b; rb.qc = ar + ly.qc; rb.qc_h2 = ar + ly.qc_h2; rb.wk = ar + ly.wk;
            run_rowblock<true, MS>(s, rb, rb_h2, tv8);
        } else {
            // xn = LN_prev(u_in) ; qkv = xn.Win^T + b
            Args g{};
            g.A = u_in; g.lda = D; g.K = D; g.lnw = lnp_w; g.lnb = lnp_b; g.W = ar + ly.sa_in_w; g.bias = ar + ly.sa_in_b;
            g.C = k.qkv; g.ldc = 3 * D; g.M = N; g.N = 3 * D; g.xn_out = k.xn; g.T = T; g.a_pstride = pstride;
            idf_prof_mark(IDF_K_GEMM_QKV, s);
            const float *qkv_h2 = (tune[IDF_TUNE_FFN_MATH] != 0 && ly.sa_in_pack_h2) ? ar + ly.sa_in_pack_h2 : nullptr;
            // Round 5: when the split-f16 self-attention follows, the projection writes the attention's f16 plane pairs (+ per-row scales, in the unused context buffer) instead of
            // fp32 rows -- the four query tiles of a (clip, head) then fetch planes instead of each splitting K and V again.
            const bool attn_h2 = tune[IDF_TUNE_FFN_MATH] != 0 && ly.sa_out_frag_h2 != 0 && T <= idf_attn_h2::MAX_T;
            const bool planes = attn_h2 && qkv_h2 && ly.qkv_bounds_ok != 0 && qkv_planes_ok(u_np, B, T);
            const bool step0 = post.x && l == 0;
            if (const int rc = run_qkv(s, g, ar + ly.sa_in_pack, u_np, step0 ? post.state : nullptr, step0 ? post.ts : nullptr, step0 ? B : 0, qkv_h2, planes ? k.qkv : nullptr,
                                       planes ? k.ctx : nullptr, step0 ? post.tmap : nullptr); rc != IDF_OK) return rc;
            idf_prof_mark(IDF_K_SELF_ATTN, s);
            // u1 = xn + ctx.Wo^T + bo with the product taken per head inside the attention kernel: H partial slabs in the FFN's
            // slab buffer (its previous contents were consumed by the QKV kernel), summed with xn + bo by the row block
            int rc_ah2 = IDF_NOT_EXCLUSIVE;
            // the split-f16 form (attn_h2.h: 32 queries per workgroup, one workgroup per CU) is the default since round 5 (row-major V planes read with the transposing LDS read:
            // -1.2 % per step against the fp32 kernel, profiles/r05_attn_split_f16_ab.txt); clips longer than its LDS budget
            // (T > 192), the exact arithmetic and a device where it does not get its CU take the fp32 kernel
            if (attn_h2) {
                rc_ah2 = idf_attn_h2::launch_self_attn_h2(s, k.qkv, B, T, ar + ly.sa_out_frag_h2, k.parts, pstride, planes ? k.ctx : nullptr);
                if (rc_ah2 != IDF_OK && (rc_ah2 != IDF_NOT_EXCLUSIVE || planes)) return idf_public_rc(rc_ah2);
            }
            if (rc_ah2 == IDF_NOT_EXCLUSIVE) launch_self_attn_outproj(s, k.qkv, B, T, ar + ly.sa_out_frag, k.parts, pstride);
            idf_prof_mark(IDF_K_ROWBLOCK_STD, s);
            rb.u_in = k.parts; rb.np = H; rb.sa_resid = k.xn; rb.sa_bias = ar + ly.sa_out_b;
            run_rowblock<false, MS>(s, rb, rb_h2, tv8);
        }
        // u3 = x2 + linear2(gelu(linear1(x2))) as NSL partial slabs (ffn.h); their sum is taken by the next reader
        idf_prof_mark(IDF_K_FFN_FUSED, s);
        if (const int rc = idf_launch_layer_ffn(s, ly, ar, tune, k.x2, N, k.parts); rc != IDF_OK) return rc;
        u_in = k.parts;
        u_np = NSL;
        lnp_w = ar + ly.ln_w[2];
        lnp_b = ar + ly.ln_b[2];
    }
    if (tail_h2) {
        ta.u_in = u_in; ta.pstride = pstride; ta.ln_w = lnp_w; ta.ln_b = lnp_b; ta.wout = ar + w->out_w_h2; ta.out_b = ar + w->out_b; ta.x0 = x0;
        idf_prof_mark(IDF_K_GEMM_HEADS, s);
        int mode = 1;
        if (post.x) {
            ta.post.N = C; ta.post.M = N; ta.post.T = T;
            ta.post.post_x = post.x; ta.post.post_gt = post.gt; ta.post.post_mask = post.mask; ta.post.post_table = post.table; ta.post.post_state = post.state;
            mode = (flags & IDF_STEP_EMBED_NEXT) ? 3 : 2;
        }
        if (const int rc = idf_tail_h2::launch_tail(s, mode, ta); rc != IDF_OK) return idf_public_rc(rc);
    } else
    {   // heads: x0[b][c][t] = LN3_last(u).Wout^T + b
        Args g{};
        g.A = u_in; g.lda = D; g.K = D; g.lnw = lnp_w; g.lnb = lnp_b; g.W = ar + w->out_w; g.bias = ar + w->out_b; g.C = x0;
        g.ldc = C; g.M = N; g.N = C; g.T = T; g.a_pstride = pstride;
        idf_prof_mark(IDF_K_GEMM_HEADS, s);
        if (post.x) {
            g.post_x = post.x; g.post_gt = post.gt; g.post_mask = post.mask; g.post_table = post.table; g.post_state = post.state;
        }
        if (sk.h) {      // keypoint head: the packed [pose | body] tiles, x0 = body | R(q) zero_pose_obj + trans | pose (skel_head.h)
            g.W = ar + sk.h->out_w; g.bias = ar + sk.h->out_b; g.N = 32 * sk.h->n_tiles;
            g.resid = sk.zero_pose_obj; g.Ka = sk.h->n_body; g.n_steps = sk.h->n_points;
            run_skel_heads(s, g, post.x != nullptr);
        } else {
            run_heads(s, g, u_np, post.x != nullptr);
        }
    }
    idf_prof_mark(-1, s);
    IDF_CHECK_LAUNCH();
    return IDF_OK;
}
int mdm_forward_impl(const idf_mdm_weights *w, const float *memctx, const float *x, const int64_t *ts, int32_t B, int32_t T, float *x0,
                     void *ws, size_t ws_bytes, void *stream, const StepPost &post, int32_t flags = 0, const SkelHead &sk = SkelHead{}) {
    if (!w || w->mem_len < 0 || w->mem_len > MEMX || !idf_tune_reserved_clear(w)) return IDF_E_INVAL;
    return idf_mem_len(w) == MEM ? mdm_forward_impl_t<MEM>(w, memctx, x, ts, B, T, x0, ws, ws_bytes, stream, post, flags, sk)
                                 : mdm_forward_impl_t<MEMX>(w, memctx, x, ts, B, T, x0, ws, ws_bytes, stream, post, flags, sk);
}
// a skeleton head the epilogue serves, on a handle of the matching token width
bool skel_head_ok(const idf_mdm_weights *w, const idf_skel_head *h, const float *z) {
    if (!w || !h || !z || h->reserved != 0 || !skel_head_shape_ok(h->n_body, h->n_points, h->n_tiles)) return false;
    if (w->C != h->n_body + 3 * h->n_points + 7 || ((3 * h->n_points) & 3) || (reinterpret_cast<uintptr_t>(z) & 15)) return false;
    return h->out_w > 0 && h->out_b > 0;
}
}  // namespace

// What every fused-step entry point refuses before the forward sees its operands (IDF_E_INVAL; IDF_OK otherwise)
static int step_args_check(const idf_mdm_weights *w, const float *x, const int64_t *ts, int32_t T, const float *gt, const uint8_t *mask, const float *table,
                           const int64_t *state) {
    if (!x || !ts || !table || !state || (mask && !gt) || T <= 0) return IDF_E_INVAL;
    // T % 4 == 0: the update is one aligned 16-byte access per lane; other clip lengths take the per-row form of the epilogue (gemm.h)
    if (!(T & 3) && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(gt)) & 15 || (reinterpret_cast<uintptr_t>(mask) & 3))) return IDF_E_INVAL;
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(gt)) & 3) return IDF_E_INVAL;
    if (!w || w->layer[0].is_qan) return IDF_E_INVAL;         // the step bookkeeping rides on layer 0's QKV kernel
    return IDF_OK;
}

extern "C" int interdiff_mdm_forward(const idf_mdm_weights *w, const float *memctx, const float *x, const int64_t *ts,
                                     int32_t B, int32_t T, float *x0, void *ws, size_t ws_bytes, void *stream) {
    if (!x0) return IDF_E_INVAL;
    return mdm_forward_impl(w, memctx, x, ts, B, T, x0, ws, ws_bytes, stream, StepPost{});
}

// One plain DDPM reverse step in the denoiser's own launches: the forward above with the x0 tile of the last GEMM consumed in its
// epilogue (inpaint, posterior mean, in-kernel noise) -- x is updated in place and the sampler state advanced, exactly what
// interdiff_mdm_forward + interdiff_posterior_step_dev(ts != NULL) do in two more HBM passes and one more launch.
extern "C" int interdiff_mdm_forward_step(const idf_mdm_weights *w, const float *memctx, float *x, int64_t *ts, int32_t B, int32_t T,
                                          const float *gt, const uint8_t *mask, const float *table, int64_t *state, void *ws,
                                          size_t ws_bytes, void *stream) {
    if (const int rc = step_args_check(w, x, ts, T, gt, mask, table, state); rc != IDF_OK) return rc;
    return mdm_forward_impl(w, memctx, x, ts, B, T, nullptr, ws, ws_bytes, stream, StepPost{x, gt, mask, table, state, ts, nullptr});
}

// The same under a respaced schedule: tmap = the model's timestep of every loop-side step, so layer 0's step bookkeeping writes ts[b] = tmap[max(t - 1, 0)]
// (philox.h; null = identity: the plain step).  flags as for interdiff_mdm_forward_step_ex below, which is this entry without a map.
extern "C" int interdiff_mdm_forward_step_map(const idf_mdm_weights *w, const float *memctx, float *x, int64_t *ts, int32_t B, int32_t T,
                                              const float *gt, const uint8_t *mask, const float *table, const int64_t *tmap, int64_t *state,
                                              void *ws, size_t ws_bytes, int32_t flags, void *stream) {
    if (flags & ~(IDF_STEP_EMBED_READY | IDF_STEP_EMBED_NEXT)) return IDF_E_INVAL;
    if (const int rc = step_args_check(w, x, ts, T, gt, mask, table, state); rc != IDF_OK) return rc;
    return mdm_forward_impl(w, memctx, x, ts, B, T, nullptr, ws, ws_bytes, stream, StepPost{x, gt, mask, table, state, ts, tmap}, flags);
}

// The plain step with flags that chain CONSECUTIVE steps on one workspace (include/interdiff_hip.h IDF_STEP_*): a step's last launch then also computes
// the next step's embedding from the token rows it has just updated (tail_h2.h), and the next call starts at its QKV projection.
extern "C" int interdiff_mdm_forward_step_ex(const idf_mdm_weights *w, const float *memctx, float *x, int64_t *ts, int32_t B, int32_t T,
                                             const float *gt, const uint8_t *mask, const float *table, int64_t *state, void *ws,
                                             size_t ws_bytes, int32_t flags, void *stream) {
    return interdiff_mdm_forward_step_map(w, memctx, x, ts, B, T, gt, mask, table, nullptr, state, ws, ws_bytes, flags, stream);
}

// The skeleton denoiser (model/diffusion_skeleton.py MDM.forward): the forward above with the keypoint head (skel_head.h) in the last GEMM's epilogue
extern "C" int interdiff_skeleton_mdm_forward(const idf_mdm_weights *w, const idf_skel_head *head, const float *memctx, const float *x,
                                              const int64_t *ts, const float *zero_pose_obj, int32_t B, int32_t T, float *x0,
                                              void *ws, size_t ws_bytes, void *stream) {
    if (!x0 || !skel_head_ok(w, head, zero_pose_obj)) return IDF_E_INVAL;
    if (!(T & 3) && (reinterpret_cast<uintptr_t>(x0) & 15)) return IDF_E_INVAL;
    return mdm_forward_impl(w, memctx, x, ts, B, T, x0, ws, ws_bytes, stream, StepPost{}, 0, SkelHead{head, zero_pose_obj});
}

// ... and its fused plain step: the update covers all C channels of x, the derived keypoint channels included
extern "C" int interdiff_skeleton_mdm_forward_step_map(const idf_mdm_weights *w, const idf_skel_head *head, const float *memctx, float *x,
                                                       int64_t *ts, const float *zero_pose_obj, int32_t B, int32_t T, const float *gt,
                                                       const uint8_t *mask, const float *table, const int64_t *tmap, int64_t *state, void *ws,
                                                       size_t ws_bytes, void *stream) {
    if (!skel_head_ok(w, head, zero_pose_obj)) return IDF_E_INVAL;          // (null w is refused here, ahead of the read of w->layer)
    if (const int rc = step_args_check(w, x, ts, T, gt, mask, table, state); rc != IDF_OK) return rc;
    return mdm_forward_impl(w, memctx, x, ts, B, T, nullptr, ws, ws_bytes, stream, StepPost{x, gt, mask, table, state, ts, tmap}, 0, SkelHead{head, zero_pose_obj});
}

extern "C" int interdiff_skeleton_mdm_forward_step(const idf_mdm_weights *w, const idf_skel_head *head, const float *memctx, float *x,
                                                   int64_t *ts, const float *zero_pose_obj, int32_t B, int32_t T, const float *gt,
                                                   const uint8_t *mask, const float *table, int64_t *state, void *ws, size_t ws_bytes,
                                                   void *stream) {
    return interdiff_skeleton_mdm_forward_step_map(w, head, memctx, x, ts, zero_pose_obj, B, T, gt, mask, table, nullptr, state, ws, ws_bytes, stream);
}

// Encoder side of the skeleton model (MDM._get_embeddings): pc[b] = shapeEmbedding(zero_pose_obj[b]) by the register-staged fp32-MFMA GEMM
// (K = 3 n_points is no multiple of the LDS-DMA kernel's chunk) into the tail of the workspace, then interdiff_mdm_encode
extern "C" size_t interdiff_skeleton_mdm_encode_workspace_bytes(int32_t B, int32_t Tp) {
    return interdiff_mdm_encode_workspace_bytes(B, Tp) + idf_align((size_t)(B > 0 ? B : 0) * D * sizeof(float));
}
extern "C" int interdiff_skeleton_mdm_encode(const idf_mdm_weights *w, const idf_skel_head *head, const float *zero_pose_obj,
                                             const float *x_past, int32_t B, int32_t Tp, float *cond, void *ws, size_t ws_bytes,
                                             void *stream) {
    if (!x_past || !cond || !ws || B <= 0 || Tp <= 0 || !skel_head_ok(w, head, zero_pose_obj) || !w->has_encoder || head->shape_w <= 0 || head->shape_b <= 0) return IDF_E_INVAL;
    if (ws_bytes < interdiff_skeleton_mdm_encode_workspace_bytes(B, Tp)) return IDF_E_NOMEM;
    const size_t enc = interdiff_mdm_encode_workspace_bytes(B, Tp);
    float *pc = reinterpret_cast<float *>(reinterpret_cast<char *>(ws) + enc);
    Args g{};
    g.A = zero_pose_obj; g.lda = 3 * head->n_points; g.K = 3 * head->n_points; g.W = w->arena + head->shape_w; g.bias = w->arena + head->shape_b;
    g.C = pc; g.ldc = D; g.M = B; g.N = D; g.T = 1;
    launch<32, 64, 2, 2, 32, A_PLAIN, E_BIAS>(idf_stream(stream), g);
    return interdiff_mdm_encode(w, pc, x_past, B, Tp, cond, ws, enc, stream);
}

// 1 when interdiff_mdm_forward_step_ex honours its flags for this handle (split arithmetic selected, token width 144, plane fragments packed); 0: they are ignored
extern "C" int interdiff_mdm_step_chaining(const idf_mdm_weights *w) {
    return w && w->tune[IDF_TUNE_FFN_MATH] != 0 && w->out_w_h2 != 0 && w->in_w_h2 != 0 && w->C == idf_tail_h2::CW && w->tail_h2_ok != 0 &&
                   idf_tail_h2::tail_exclusive_ok(false) && idf_tail_h2::tail_exclusive_ok(true) ? 1 : 0;
}

// DEBUG (tests only): kernels whose name -- as interdiff_exclusive_cu_report prints it -- contains one of the comma-separated patterns are treated as NOT getting their CU from now on,
// so that the fp32 kernel behind every split-f16 launcher can be executed on a device where all claims hold; null / "" clears the list.  Process-wide; not for product use.
extern "C" int interdiff_debug_deny_exclusive(const char *patterns) {
    idf_excl_set_deny(patterns);
    return IDF_OK;
}

// Verdicts of the exclusive-CU check (common.h idf_exclusive_cu) for EVERY kernel of the library that issues the f16 MFMA, on the current device: forces
// the check for each (no launch), writes one text line per kernel into buf (<= cap bytes, NUL-terminated) and returns the number of kernels that do NOT
// get their CU to themselves (those run as their fp32-MFMA counterparts), or a negative IDF_E_* code.
extern "C" int interdiff_exclusive_cu_report(char *buf, int32_t cap) {
    if (!buf || cap <= 0) return IDF_E_INVAL;
    {
        static idf_excl_cache c[6];
        using namespace idf_ffn_h2;
        idf_exclusive_cu(reinterpret_cast<const void *>(&ffn_h2_kernel<1, FFN_H2_SLOTS, 0>), "ffn_h2_kernel<16 rows>", NT, c[0]);
        idf_exclusive_cu(reinterpret_cast<const void *>(&ffn_h2_kernel<2, FFN_H2_SLOTS, 0, 8>), "ffn_h2_kernel<32 rows, loader waves>", NT + 512, c[1]);
        idf_exclusive_cu(reinterpret_cast<const void *>(&ffn_h2_kernel<4, 2, 0>), "ffn_h2_kernel<64 rows>", NT, c[2]);
        idf_exclusive_cu(reinterpret_cast<const void *>(&ln_linear_h2_kernel<1, false>), "ln_linear_h2_kernel<1 slab>", NT, c[3]);
        idf_exclusive_cu(reinterpret_cast<const void *>(&ln_linear_h2_kernel<IDF_FFN_SLICES, false>), "ln_linear_h2_kernel<5 slabs>", NT, c[4]);
        idf_exclusive_cu(reinterpret_cast<const void *>(&idf_attn_h2::self_attn_h2_kernel<0, false>), "self_attn_h2_kernel", idf_attn_h2::NTH, c[5]);
    }
    qkv_planes_ok(1, 1, 16);
    qkv_planes_ok(NSL, 1, 16);
    rb_exclusive_forms<4, MEM, 16>();
    rb_exclusive_forms<4, MEMX, 16>();
    rb_exclusive_forms<8, MEM, 16, 8>();
    rb_exclusive_forms<8, MEMX, 16, 8>();
    idf_tail_h2::tail_exclusive_ok(false);
    idf_tail_h2::tail_exclusive_ok(true);
    return idf_excl_report(buf, cap);
}
