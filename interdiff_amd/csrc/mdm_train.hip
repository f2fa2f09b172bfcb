// Training of the SMPL denoiser's decoder (launchers; device code and the arithmetic contract: csrc/mdm_train.h).  Replaces, for the 144 tensors MDM.forward reads,
// loss.backward() on LitInteraction.forward_backward (train_diffusion_smpl.py:60-166) and torch.optim.AdamW's step (:177-183).  `cond` is an input: its gradient
// d_cond is returned, and interdiff_mdm_train_full_grads carries it on through MDM._get_embeddings (diffusion_smpl.py:217-221: the shared input embeddings,
// pc_embedding, the positional rows, the eight encoder layers), whose 84 tensors follow the 144 in the flat vectors; pc_embedding is that pass's input seam.
// The sampler's kernels and arena are not touched.
//
// The two stacks, their layouts and workspace plans take a geometry (csrc/mdm_train_stack.h: feed-forward width, token and head widths) and are what the skeleton
// denoiser's trainer (csrc/skeleton_mdm_train.hip) runs too; the SMPL entries at the end of this file run them at SMPL_GEOM.
//
// Stored by the forward, per layer: the layer input, q|k|v and the attention output with its per-row log-sum-exp (layers 0, 7), the three normalised rows + 1/sigma
// and LayerNorm outputs, the cross-attention query, memory k|v and output, the feed-forward pre-activation.  Recomputed by the backward: every softmax probability
// (self-attention, cross-attention, QaN block) and the GELU output.  The encoder stores the same per layer without the cross-attention items, on past_len * B rows.
#include "mdm_train.h"

using namespace mdmtrain;

namespace {

inline bool is_qan(int l) { return l >= 1 && l <= 6; }
inline int64_t n_shared(const Layout &L) { return L.t0_w; }      // bodyEmbedding.* and objEmbedding.*: the first four tensors of the table, back to back

int gemm(hipStream_t st, const float *A, int64_t sam, int64_t sak, const float *Bm, int64_t sbk, int64_t sbn, float *C, int64_t ldc, const float *bias, const float *R,
         int64_t ldr, int M, int N, int K) {
    const Gemm g{A, sam, sak, Bm, sbk, sbn, C, ldc, bias, R, ldr, M, N, K};
    hipLaunchKernelGGL(mt_gemm_kernel, dim3((unsigned)idf_cdiv(N, 32), (unsigned)idf_cdiv(M, 32)), dim3(64), 0, st, g);
    IDF_CHECK_LAUNCH();
    return IDF_OK;
}
// dX[M,K] = dY[M,N] W[N,K] (+ R)
int lin_dx(hipStream_t st, const float *dY, int64_t ldy, const float *W, float *dX, int64_t ldx, const float *R, int64_t ldr, int M, int N, int K) {
    return gemm(st, dY, ldy, 1, W, K, 1, dX, ldx, nullptr, R, ldr, M, K, N);
}
// dW[N,K] = dY[M,N]^T X[M,K]
int lin_dw(hipStream_t st, const float *dY, int64_t ldy, const float *X, int64_t ldx, float *dW, int M, int N, int K) {
    return gemm(st, dY, 1, ldy, X, ldx, 1, dW, K, nullptr, nullptr, 0, N, K, M);
}
// out[N] = column sums of A[M,N] (* Bm), two-stage
int colsum(hipStream_t st, const float *A, int64_t lda, const float *Bm, int64_t ldb, int M, int N, float *partial, float *out) {
    const int slabs = (int)idf_cdiv(M, 64);
    hipLaunchKernelGGL(mt_colsum_partial_kernel, dim3((unsigned)idf_cdiv(N, 64), (unsigned)slabs), dim3(256), 0, st, A, lda, Bm, ldb, M, N, partial);
    IDF_CHECK_LAUNCH();
    hipLaunchKernelGGL(mt_colsum_reduce_kernel, dim3((unsigned)idf_cdiv(N, 256)), dim3(256), 0, st, partial, slabs, N, out);
    IDF_CHECK_LAUNCH();
    return IDF_OK;
}
inline unsigned blocks256(int64_t n) { return (unsigned)idf_cdiv(n, 256); }

// [B][C][T] tokens <-> [B*T][C] rows
int tokens_to_rows(hipStream_t st, const float *x, float *rows, int B, int T, int C) {
    hipLaunchKernelGGL(mt_tokens_to_rows_kernel, dim3(blocks256((int64_t)B * T * C)), dim3(256), 0, st, x, rows, B, T, C);
    IDF_CHECK_LAUNCH();
    return IDF_OK;
}
int rows_to_tokens(hipStream_t st, const float *rows, float *x, int B, int T, int C) {
    hipLaunchKernelGGL(mt_rows_to_tokens_kernel, dim3(blocks256((int64_t)B * T * C)), dim3(256), 0, st, rows, x, B, T, C);
    IDF_CHECK_LAUNCH();
    return IDF_OK;
}

int ln_fwd(hipStream_t st, const float *s, const float *gw, const float *gb, float *xh, float *rs, float *y, int M) {
    hipLaunchKernelGGL(mt_ln_fwd_kernel, dim3((unsigned)idf_cdiv(M, 4)), dim3(256), 0, st, s, gw, gb, xh, rs, y, M);
    IDF_CHECK_LAUNCH();
    return IDF_OK;
}
// LayerNorm backward: d gamma, d beta (two-stage column sums) and dx
int ln_bwd(hipStream_t st, const float *dy, const float *xh, const float *rs, const float *gw, float *dgw, float *dgb, float *dx, float *partial, int M) {
    MT_TRY(colsum(st, dy, D, xh, D, M, D, partial, dgw));
    MT_TRY(colsum(st, dy, D, nullptr, 0, M, D, partial, dgb));
    hipLaunchKernelGGL(mt_ln_bwd_kernel, dim3((unsigned)idf_cdiv(M, 4)), dim3(256), 0, st, dy, xh, rs, gw, dx, M);
    IDF_CHECK_LAUNCH();
    return IDF_OK;
}

Weights16 weights_of(const float *w16) {
    Weights16 W;
    for (int i = 0; i < 16; ++i) W.w[i] = w16[i];
    return W;
}
int loss_grad(hipStream_t st, const float *pred, const float *target, int B, int T, int P, const float *w16, float *dpred) {
    hipLaunchKernelGGL(mt_loss_grad_kernel, dim3(blocks256((int64_t)B * SMPL_GEOM.ctok * T)), dim3(256), 0, st, pred, target, B, T, P, weights_of(w16), dpred);
    IDF_CHECK_LAUNCH();
    return IDF_OK;
}

// ---- the sublayers both stacks are made of; T = tokens per clip ---------------------------------------------------------------------------------------------
// s = x + self_attn(x) (layers 0, 7) | x + QaN block(x) (layers 1..6)
int mix_fwd(hipStream_t st, const float *th, const LayerOff &o, bool qan, const float *xin, float *qkv, float *ao, float *lse, float *G, float *s, int B, int T) {
    const int M = B * T;
    if (qan) {
        hipLaunchKernelGGL(mt_qan_prep_kernel, dim3(NQ), dim3(256), 0, st, th + o.queries, G);
        IDF_CHECK_LAUNCH();
        hipLaunchKernelGGL(mt_qan_fwd_kernel, dim3((unsigned)idf_cdiv(M, 4)), dim3(256), 0, st, xin, G, th + o.wk, s, M, T);
        IDF_CHECK_LAUNCH();
        return IDF_OK;
    }
    MT_TRY(lin_fwd(st, xin, D, th + o.sa_in_w, th + o.sa_in_b, qkv, 3 * D, nullptr, 0, M, 3 * D, D));
    hipLaunchKernelGGL(mt_self_attn_fwd_kernel, dim3((unsigned)(B * HEADS)), dim3(128), (size_t)2 * T * HD * sizeof(float), st, qkv, ao, lse, T);
    IDF_CHECK_LAUNCH();
    return lin_fwd(st, ao, D, th + o.sa_out_w, th + o.sa_out_b, s, D, xin, D, M, D, D);
}
// s = x + linear2(gelu(linear1(x))); leaves the pre-activation z
int ffn_fwd(hipStream_t st, const Ws &w, const float *th, const LayerOff &o, const float *x, float *z, float *s, int M) {
    const int FF = w.geo.ff;
    MT_TRY(lin_fwd(st, x, D, th + o.l1_w, th + o.l1_b, z, FF, nullptr, 0, M, FF, D));
    hipLaunchKernelGGL(mt_gelu_kernel, dim3(blocks256((int64_t)M * FF)), dim3(256), 0, st, z, w.g, (int64_t)M * FF);
    IDF_CHECK_LAUNCH();
    return lin_fwd(st, w.g, FF, th + o.l2_w, th + o.l2_b, s, D, x, D, M, D, FF);
}
// E = d s (the feed-forward output and, through the residual, d x)  ->  F = d x, and the four parameter gradients
int ffn_bwd(hipStream_t st, const Ws &w, const float *th, float *gr, const LayerOff &o, const float *E, const float *x, const float *z, float *F, int M) {
    const int FF = w.geo.ff;
    hipLaunchKernelGGL(mt_gelu_kernel, dim3(blocks256((int64_t)M * FF)), dim3(256), 0, st, z, w.g, (int64_t)M * FF);
    IDF_CHECK_LAUNCH();
    MT_TRY(lin_param_grads(st, w, E, D, w.g, FF, gr + o.l2_w, gr + o.l2_b, M, D, FF));
    MT_TRY(lin_dx(st, E, D, th + o.l2_w, w.dz, FF, nullptr, 0, M, D, FF));
    hipLaunchKernelGGL(mt_gelu_bwd_kernel, dim3(blocks256((int64_t)M * FF)), dim3(256), 0, st, z, w.dz, (int64_t)M * FF);
    IDF_CHECK_LAUNCH();
    MT_TRY(lin_param_grads(st, w, w.dz, FF, x, D, gr + o.l1_w, gr + o.l1_b, M, FF, D));
    return lin_dx(st, w.dz, FF, th + o.l1_w, F, D, E, D, M, FF, D);
}
// E = d s of mix_fwd  ->  Dh = d x (the residual included), and the parameter gradients; F is scratch
int mix_bwd(hipStream_t st, const Ws &w, const float *th, float *gr, const LayerOff &o, bool qan, const float *E, const float *xin, const float *qkv, const float *ao,
            const float *lse, const float *G, float *F, float *Dh, int B, int T) {
    const int M = B * T;
    if (qan) {
        hipLaunchKernelGGL(mt_qan_bwd_token_kernel, dim3((unsigned)idf_cdiv(M, 4)), dim3(256), 0, st, xin, G, th + o.wk, E, w.dsim, w.cj, w.dwk_tok, M, T);
        IDF_CHECK_LAUNCH();
        hipLaunchKernelGGL(mt_qan_bwd_gather_kernel, dim3((unsigned)idf_cdiv(M, 4)), dim3(256), 0, st, E, G, w.dsim, w.cj, Dh, M, T);
        IDF_CHECK_LAUNCH();
        // dG[j][n] = sum_t dsim[t][n][j] x[t-1+j]: slot 0 pairs token t with frame t-1 (rows 1.., a clip's first token is masked: dsim = 0), slot 2 with t+1
        MT_TRY(gemm(st, w.dsim + NQ * SLOTS, SLOTS, NQ * SLOTS, xin, D, 1, w.dG, D, nullptr, nullptr, 0, NQ, D, M - 1));
        MT_TRY(gemm(st, w.dsim + 1, SLOTS, NQ * SLOTS, xin, D, 1, w.dG + (int64_t)NQ * D, D, nullptr, nullptr, 0, NQ, D, M));
        MT_TRY(gemm(st, w.dsim + 2, SLOTS, NQ * SLOTS, xin + D, D, 1, w.dG + (int64_t)2 * NQ * D, D, nullptr, nullptr, 0, NQ, D, M - 1));
        hipLaunchKernelGGL(mt_qan_dqueries_kernel, dim3(NQ), dim3(256), 0, st, th + o.queries, w.dG, gr + o.queries);
        IDF_CHECK_LAUNCH();
        return colsum(st, w.dwk_tok, NQ, nullptr, 0, M, NQ, w.partial, gr + o.wk);
    }
    MT_TRY(lin_param_grads(st, w, E, D, ao, D, gr + o.sa_out_w, gr + o.sa_out_b, M, D, D));
    MT_TRY(lin_dx(st, E, D, th + o.sa_out_w, F, D, nullptr, 0, M, D, D));                                                        // F = d (attention output)
    hipLaunchKernelGGL(mt_self_attn_bwd_kernel, dim3((unsigned)(B * HEADS)), dim3(128), (size_t)2 * T * HD * sizeof(float), st, qkv, ao, lse, F, w.dqkv, w.P, w.dS, T);
    IDF_CHECK_LAUNCH();
    MT_TRY(lin_param_grads(st, w, w.dqkv, 3 * D, xin, D, gr + o.sa_in_w, gr + o.sa_in_b, M, 3 * D, D));
    return lin_dx(st, w.dqkv, 3 * D, th + o.sa_in_w, Dh, D, E, D, M, 3 * D, D);
}

}  // namespace

namespace mdmtrain {

// ---- the flat vectors: tensors packed without padding, in the order of interdiff_amd/mdm_train.py PARAM_NAMES and, behind them, ENCODER_PARAM_NAMES -----------------
struct Packer {
    int64_t at, *off, *size;
    int n;
    void operator()(int64_t &slot, int64_t sz) { slot = at; off[n] = at; size[n] = sz; ++n; at += sz; }
};
// one layer's tensors; cross: a decoder layer (cross-attention, three LayerNorms) -- else an encoder layer (two LayerNorms)
static void layer_layout(Packer &take, LayerOff &y, int l, int64_t FF, bool cross) {
    y.sa_in_w = y.sa_in_b = y.sa_out_w = y.sa_out_b = y.queries = y.wk = y.ca_in_w = y.ca_in_b = y.ca_out_w = y.ca_out_b = y.ln_w[2] = y.ln_b[2] = -1;
    if (is_qan(l)) {
        take(y.queries, (int64_t)NQ * D); take(y.wk, NQ);
    } else {
        take(y.sa_in_w, (int64_t)3 * D * D); take(y.sa_in_b, 3 * D); take(y.sa_out_w, (int64_t)D * D); take(y.sa_out_b, D);
    }
    if (cross) { take(y.ca_in_w, (int64_t)3 * D * D); take(y.ca_in_b, 3 * D); take(y.ca_out_w, (int64_t)D * D); take(y.ca_out_b, D); }
    take(y.l1_w, FF * D); take(y.l1_b, FF); take(y.l2_w, D * FF); take(y.l2_b, D);
    for (int i = 0; i < (cross ? 3 : 2); ++i) { take(y.ln_w[i], D); take(y.ln_b[i], D); }
}

Layout make_layout(const Geom &g) {
    Layout o{};
    Packer take{0, o.off, o.size, 0};
    take(o.body_w, (int64_t)D * g.nbody); take(o.body_b, D); take(o.obj_w, (int64_t)D * g.nobj); take(o.obj_b, D);
    take(o.t0_w, (int64_t)D * D); take(o.t0_b, D); take(o.t2_w, (int64_t)D * D); take(o.t2_b, D);
    for (int l = 0; l < N_LAYERS; ++l) layer_layout(take, o.layer[l], l, g.ff, true);
    take(o.bodyf_w, (int64_t)g.hbody * D); take(o.bodyf_b, g.hbody); take(o.objf_w, (int64_t)g.hobj * D); take(o.objf_b, g.hobj);
    o.total = take.at;
    return o;
}

EncLayout make_enc_layout(const Geom &g, const Layout &L) {
    EncLayout o{};
    Packer take{L.total, o.off, o.size, 0};
    for (int l = 0; l < N_LAYERS; ++l) layer_layout(take, o.layer[l], l, g.ff, false);
    o.total = take.at;
    return o;
}

int table_out(std::initializer_list<TableRun> parts, int64_t total, int64_t *offsets, int64_t *sizes, int32_t *n_tensors, int64_t *n_param) {
    int n = 0;
    for (const TableRun &p : parts)
        for (int i = 0; i < p.n; ++i, ++n) {
            if (offsets) offsets[n] = p.off[i];
            if (sizes) sizes[n] = p.size[i];
        }
    if (n_tensors) *n_tensors = n;
    if (n_param) *n_param = total;
    return IDF_OK;
}

// ---- workspace plan (floats) ---------------------------------------------------------------------------------------------------------------------------
// one layer's saves on M rows of T-token clips; S: the memory's length for a decoder layer, 0 for an encoder layer (no cross-attention, two LayerNorms)
static void layer_plan(Carver &take, LayerWs &y, int l, size_t B, size_t T, size_t FF, size_t S) {
    const size_t M = B * T;
    if (is_qan(l)) y.G = take((size_t)NQ * SLOTS * D);
    else { y.qkv = take(M * 3 * D); y.ao = take(M * D); y.lse = take(B * HEADS * T); }
    for (int i = 0; i < (S ? 3 : 2); ++i) { y.xh[i] = take(M * D); y.rs[i] = take(M); }
    y.x1 = take(M * D);
    if (S) { y.x2 = take(M * D); y.q2 = take(M * D); y.kv = take(S * B * 2 * D); y.o2 = take(M * D); }
    y.z = take(M * FF);
}

Ws plan(float *base, const Geom &g, int B, int T, int S) {
    Ws w{};
    w.geo = g;
    const size_t M = (size_t)B * T, FF = (size_t)g.ff, CTOK = (size_t)g.ctok;
    Carver take{base, 0};
    w.X = take(M * CTOK); w.Y = take(M * CTOK); w.dY = take(M * CTOK);
    w.tin = take((size_t)B * D); w.z0 = take((size_t)B * D); w.sz = take((size_t)B * D); w.temb = take((size_t)B * D);
    for (int l = 0; l <= N_LAYERS; ++l) w.h[l] = take(M * D);
    for (int l = 0; l < N_LAYERS; ++l) layer_plan(take, w.layer[l], l, B, T, FF, S);
    w.g = take(M * FF); w.dz = take(M * FF);
    for (int i = 0; i < 4; ++i) w.t[i] = take(M * D);
    w.dqkv = take(M * 3 * D);
    w.P = take((size_t)B * HEADS * T * T); w.dS = take((size_t)B * HEADS * T * T);
    w.Pc = take(M * HEADS * MAX_MEM); w.dSc = take(M * HEADS * MAX_MEM);
    w.dkv = take((size_t)S * B * 2 * D);
    w.dG = take((size_t)SLOTS * NQ * D); w.dsim = take(M * NQ * SLOTS); w.cj = take(M * SLOTS); w.dwk_tok = take(M * NQ);
    w.partial = take(((M + 63) / 64 + 1) * (FF > (size_t)3 * D ? FF : (size_t)3 * D));      // the widest column sum: a feed-forward bias or the q|k|v bias
    w.dtemb = take((size_t)B * D); w.dsz = take((size_t)B * D);
    w.floats = take.at;
    return w;
}

// The encoder's saves, behind the decoder's plan.  Its scratch (GELU output, d z, the four row buffers, d qkv, P / dS, the QaN items, the column-sum slabs) is the
// decoder's: the encoder's forward ends before the decoder's begins and its backward begins after the decoder's has ended, and S * B < T * B rows.
EncWs enc_plan(float *base, size_t at, const Geom &g, const Layout &L, int B, int S) {
    EncWs w{};
    const size_t M = (size_t)B * S;
    Carver take{base, at};
    w.Xp = take(M * g.ctok);
    for (int l = 0; l <= N_LAYERS; ++l) w.h[l] = take(M * D);
    w.genc = take((size_t)n_shared(L));
    for (int l = 0; l < N_LAYERS; ++l) layer_plan(take, w.layer[l], l, B, S, (size_t)g.ff, 0);
    w.floats = take.at;
    return w;
}

FullWs full_plan(float *base, const Geom &g, const Layout &L, int B, int T, int past_len) {
    const Ws w = plan(base, g, B, T, past_len);
    return {w, enc_plan(base, w.floats, g, L, B, past_len)};
}

int ws_check(const void *ws, size_t ws_bytes, size_t need) {
    if (reinterpret_cast<uintptr_t>(ws) & 255) return IDF_E_INVAL;
    return ws_bytes < need ? IDF_E_NOMEM : IDF_OK;
}

bool shape_ok(const Geom &g, int B, int T, int S, int past_len) {
    return B > 0 && T > 0 && T <= MAX_T && S > 0 && S <= MAX_MEM && past_len >= 2 && T >= past_len + 2 && (int64_t)B * T * (g.ff > 3 * D ? g.ff : 3 * D) < 0x7FFFFFFF;
}

// ---- launchers the model-specific files use too ----------------------------------------------------------------------------------------------------------
int lin_fwd(hipStream_t st, const float *X, int64_t ldx, const float *W, const float *b, float *Y, int64_t ldy, const float *R, int64_t ldr, int M, int N, int K) {
    return gemm(st, X, ldx, 1, W, 1, K, Y, ldy, b, R, ldr, M, N, K);
}
int lin_param_grads(hipStream_t st, const Ws &w, const float *dY, int64_t ldy, const float *X, int64_t ldx, float *dW, float *db, int M, int N, int K) {
    MT_TRY(lin_dw(st, dY, ldy, X, ldx, dW, M, N, K));
    return colsum(st, dY, ldy, nullptr, 0, M, N, w.partial, db);
}

// ---- forward with saves ---------------------------------------------------------------------------------------------------------------------------------
int forward(hipStream_t st, const Layout &L, const Ws &w, const float *th, const float *pe, int pe_rows, const float *x_t, const int64_t *ts, const float *cond, int B, int T,
            int S) {
    const Geom &g = w.geo;
    const int M = B * T, SB = S * B, CTOK = g.ctok, HEAD = g.head();
    MT_TRY(tokens_to_rows(st, x_t, w.X, B, T, CTOK));
    // timestep MLP (layers.py:42-43)
    hipLaunchKernelGGL(mt_gather_pe_kernel, dim3((unsigned)B), dim3(256), 0, st, pe, pe_rows, ts, w.tin);
    IDF_CHECK_LAUNCH();
    MT_TRY(lin_fwd(st, w.tin, D, th + L.t0_w, th + L.t0_b, w.z0, D, nullptr, 0, B, D, D));
    hipLaunchKernelGGL(mt_silu_kernel, dim3(blocks256((int64_t)B * D)), dim3(256), 0, st, w.z0, w.sz, (int64_t)B * D);
    IDF_CHECK_LAUNCH();
    MT_TRY(lin_fwd(st, w.sz, D, th + L.t2_w, th + L.t2_b, w.temb, D, nullptr, 0, B, D, D));
    // embedding: bodyEmbedding(x[:nbody]) + objEmbedding(x[nbody : nbody + nobj]) + temb + pe[t]
    MT_TRY(lin_fwd(st, w.X, CTOK, th + L.body_w, th + L.body_b, w.h[0], D, nullptr, 0, M, D, g.nbody));
    MT_TRY(lin_fwd(st, w.X + g.nbody, CTOK, th + L.obj_w, th + L.obj_b, w.h[0], D, w.h[0], D, M, D, g.nobj));
    hipLaunchKernelGGL(mt_add_temb_pe_kernel, dim3((unsigned)M), dim3(256), 0, st, w.h[0], w.temb, pe, T);
    IDF_CHECK_LAUNCH();
    for (int l = 0; l < N_LAYERS; ++l) {
        const LayerOff &o = L.layer[l];
        const LayerWs &y = w.layer[l];
        const float *xin = w.h[l];
        float *s = w.t[0];                                        // the pre-LayerNorm sums live only until their LayerNorm has run
        MT_TRY(mix_fwd(st, th, o, is_qan(l), xin, y.qkv, y.ao, y.lse, y.G, s, B, T));
        MT_TRY(ln_fwd(st, s, th + o.ln_w[0], th + o.ln_b[0], y.xh[0], y.rs[0], y.x1, M));
        // cross-attention on the memory
        MT_TRY(lin_fwd(st, y.x1, D, th + o.ca_in_w, th + o.ca_in_b, y.q2, D, nullptr, 0, M, D, D));
        MT_TRY(lin_fwd(st, cond, D, th + o.ca_in_w + (int64_t)D * D, th + o.ca_in_b + D, y.kv, 2 * D, nullptr, 0, SB, 2 * D, D));
        hipLaunchKernelGGL(mt_cross_attn_fwd_kernel, dim3(blocks256((int64_t)M * HEADS)), dim3(256), 0, st, y.q2, y.kv, y.o2, B, T, S);
        IDF_CHECK_LAUNCH();
        MT_TRY(lin_fwd(st, y.o2, D, th + o.ca_out_w, th + o.ca_out_b, s, D, y.x1, D, M, D, D));
        MT_TRY(ln_fwd(st, s, th + o.ln_w[1], th + o.ln_b[1], y.xh[1], y.rs[1], y.x2, M));
        // feed-forward
        MT_TRY(ffn_fwd(st, w, th, o, y.x2, y.z, s, M));
        if (is_qan(l)) {
            MT_TRY(ln_fwd(st, s, th + o.ln_w[2], th + o.ln_b[2], y.xh[2], y.rs[2], w.t[1], M));
            hipLaunchKernelGGL(mt_round_trip_kernel, dim3(blocks256((int64_t)M * D)), dim3(256), 0, st, xin, w.t[1], w.h[l + 1], (int64_t)M * D);
            IDF_CHECK_LAUNCH();
        } else {
            MT_TRY(ln_fwd(st, s, th + o.ln_w[2], th + o.ln_b[2], y.xh[2], y.rs[2], w.h[l + 1], M));
        }
    }
    MT_TRY(lin_fwd(st, w.h[N_LAYERS], D, th + L.bodyf_w, th + L.bodyf_b, w.Y, HEAD, nullptr, 0, M, g.hbody, D));
    return lin_fwd(st, w.h[N_LAYERS], D, th + L.objf_w, th + L.objf_b, w.Y + g.hbody, HEAD, nullptr, 0, M, g.hobj, D);
}

// ---- backward: w.dY [B*T][head()] -> grads [n_param], d_cond [S][B][256] ------------------------------------------------------------------------------------
int backward(hipStream_t st, const Layout &L, const Ws &w, const float *th, const float *cond, int B, int T, int S, float *gr, float *d_cond) {
    const Geom &g = w.geo;
    const int M = B * T, SB = S * B, CTOK = g.ctok, HEAD = g.head();
    float *Dh = w.t[0], *E = w.t[1], *F = w.t[2], *Gq = w.t[3];
    // the two output heads
    MT_TRY(lin_param_grads(st, w, w.dY, HEAD, w.h[N_LAYERS], D, gr + L.bodyf_w, gr + L.bodyf_b, M, g.hbody, D));
    MT_TRY(lin_param_grads(st, w, w.dY + g.hbody, HEAD, w.h[N_LAYERS], D, gr + L.objf_w, gr + L.objf_b, M, g.hobj, D));
    MT_TRY(lin_dx(st, w.dY, HEAD, th + L.bodyf_w, Dh, D, nullptr, 0, M, g.hbody, D));
    MT_TRY(lin_dx(st, w.dY + g.hbody, HEAD, th + L.objf_w, Dh, D, Dh, D, M, g.hobj, D));
    bool first_cond = true;
    for (int l = N_LAYERS - 1; l >= 0; --l) {
        const LayerOff &o = L.layer[l];
        const LayerWs &y = w.layer[l];
        const float *xin = w.h[l];
        // Dh = d (LayerNorm3 output): for a QaN layer the backward of tgt + (x - tgt) is the identity on x and nothing on tgt
        MT_TRY(ln_bwd(st, Dh, y.xh[2], y.rs[2], th + o.ln_w[2], gr + o.ln_w[2], gr + o.ln_b[2], E, w.partial, M));            // E = d s3 = d ffn-out = d x2 (residual)
        MT_TRY(ffn_bwd(st, w, th, gr, o, E, y.x2, y.z, F, M));                                                                  // F = d x2
        MT_TRY(ln_bwd(st, F, y.xh[1], y.rs[1], th + o.ln_w[1], gr + o.ln_w[1], gr + o.ln_b[1], E, w.partial, M));              // E = d s2 = d x1 (residual)
        // cross-attention
        MT_TRY(lin_param_grads(st, w, E, D, y.o2, D, gr + o.ca_out_w, gr + o.ca_out_b, M, D, D));
        MT_TRY(lin_dx(st, E, D, th + o.ca_out_w, F, D, nullptr, 0, M, D, D));                                                    // F = d o2
        hipLaunchKernelGGL(mt_cross_attn_bwd_q_kernel, dim3(blocks256((int64_t)M * HEADS)), dim3(256), 0, st, y.q2, y.kv, F, Gq, w.Pc, w.dSc, B, T, S);
        IDF_CHECK_LAUNCH();
        hipLaunchKernelGGL(mt_cross_attn_bwd_kv_kernel, dim3(blocks256((int64_t)SB * 2 * D)), dim3(256), 0, st, y.q2, F, w.Pc, w.dSc, w.dkv, B, T, S);
        IDF_CHECK_LAUNCH();
        MT_TRY(lin_param_grads(st, w, Gq, D, y.x1, D, gr + o.ca_in_w, gr + o.ca_in_b, M, D, D));
        MT_TRY(lin_param_grads(st, w, w.dkv, 2 * D, cond, D, gr + o.ca_in_w + (int64_t)D * D, gr + o.ca_in_b + D, SB, 2 * D, D));
        MT_TRY(lin_dx(st, w.dkv, 2 * D, th + o.ca_in_w + (int64_t)D * D, d_cond, D, first_cond ? nullptr : d_cond, D, SB, 2 * D, D));   // layers 7 .. 0 in this order
        first_cond = false;
        MT_TRY(lin_dx(st, Gq, D, th + o.ca_in_w, F, D, E, D, M, D, D));                                                          // F = d x1
        MT_TRY(ln_bwd(st, F, y.xh[0], y.rs[0], th + o.ln_w[0], gr + o.ln_w[0], gr + o.ln_b[0], E, w.partial, M));              // E = d s1
        MT_TRY(mix_bwd(st, w, th, gr, o, is_qan(l), E, xin, y.qkv, y.ao, y.lse, y.G, F, Dh, B, T));
    }
    // embedding and the timestep MLP: Dh = d h0
    MT_TRY(lin_param_grads(st, w, Dh, D, w.X, CTOK, gr + L.body_w, gr + L.body_b, M, D, g.nbody));
    MT_TRY(lin_param_grads(st, w, Dh, D, w.X + g.nbody, CTOK, gr + L.obj_w, gr + L.obj_b, M, D, g.nobj));
    hipLaunchKernelGGL(mt_sum_frames_kernel, dim3((unsigned)B), dim3(256), 0, st, Dh, w.dtemb, T);
    IDF_CHECK_LAUNCH();
    MT_TRY(lin_param_grads(st, w, w.dtemb, D, w.sz, D, gr + L.t2_w, gr + L.t2_b, B, D, D));
    MT_TRY(lin_dx(st, w.dtemb, D, th + L.t2_w, w.dsz, D, nullptr, 0, B, D, D));
    hipLaunchKernelGGL(mt_silu_bwd_kernel, dim3(blocks256((int64_t)B * D)), dim3(256), 0, st, w.z0, w.dsz, (int64_t)B * D);
    IDF_CHECK_LAUNCH();
    MT_TRY(lin_param_grads(st, w, w.dsz, D, w.tin, D, gr + L.t0_w, gr + L.t0_b, B, D, D));
    return IDF_OK;
}

// ---- the encoder: MDM._get_embeddings from the per-clip row on (diffusion_smpl.py:217-221, diffusion_skeleton.py:208-213), S = past_len tokens per clip -------
// th holds the 228 tensors; target [B][ctok][T] gives the past frames; pc [B][256]; cond [S][B][256] is written in the memory's own order.
int enc_forward(hipStream_t st, const Layout &L, const EncLayout &EL, const Ws &w, const EncWs &e, const float *th, const float *pe, const float *target, const float *pc,
                int B, int T, int S, float *cond) {
    const Geom &g = w.geo;
    const int M = B * S, CTOK = g.ctok;
    hipLaunchKernelGGL(mt_gather_past_kernel, dim3(blocks256((int64_t)M * CTOK)), dim3(256), 0, st, target, e.Xp, B, T, S, CTOK);
    IDF_CHECK_LAUNCH();
    // embedding: (bodyEmbedding(body) + objEmbedding(obj) + pc_embedding) + pe[s] -- the decoder's kernel with pc in the place of the timestep embedding
    MT_TRY(lin_fwd(st, e.Xp, CTOK, th + L.body_w, th + L.body_b, e.h[0], D, nullptr, 0, M, D, g.nbody));
    MT_TRY(lin_fwd(st, e.Xp + g.nbody, CTOK, th + L.obj_w, th + L.obj_b, e.h[0], D, e.h[0], D, M, D, g.nobj));
    hipLaunchKernelGGL(mt_add_temb_pe_kernel, dim3((unsigned)M), dim3(256), 0, st, e.h[0], pc, pe, S);
    IDF_CHECK_LAUNCH();
    for (int l = 0; l < N_LAYERS; ++l) {
        const LayerOff &o = EL.layer[l];
        const LayerWs &y = e.layer[l];
        const float *xin = e.h[l];
        float *s = w.t[0];
        MT_TRY(mix_fwd(st, th, o, is_qan(l), xin, y.qkv, y.ao, y.lse, y.G, s, B, S));
        MT_TRY(ln_fwd(st, s, th + o.ln_w[0], th + o.ln_b[0], y.xh[0], y.rs[0], y.x1, M));
        MT_TRY(ffn_fwd(st, w, th, o, y.x1, y.z, s, M));
        if (is_qan(l)) {
            MT_TRY(ln_fwd(st, s, th + o.ln_w[1], th + o.ln_b[1], y.xh[1], y.rs[1], w.t[1], M));
            hipLaunchKernelGGL(mt_round_trip_kernel, dim3(blocks256((int64_t)M * D)), dim3(256), 0, st, xin, w.t[1], e.h[l + 1], (int64_t)M * D);
            IDF_CHECK_LAUNCH();
        } else {
            MT_TRY(ln_fwd(st, s, th + o.ln_w[1], th + o.ln_b[1], y.xh[1], y.rs[1], e.h[l + 1], M));
        }
    }
    hipLaunchKernelGGL(mt_swap_rows_kernel, dim3((unsigned)M), dim3(256), 0, st, e.h[N_LAYERS], cond, B, S);
    IDF_CHECK_LAUNCH();
    return IDF_OK;
}

// d_cond [S][B][256] -> the 84 encoder gradients, the encoder path's share of the four shared embedding tensors (added to the decoder path's, which gr already
// holds), d_pc [B][256]
int enc_backward(hipStream_t st, const Layout &L, const EncLayout &EL, const Ws &w, const EncWs &e, const float *th, const float *d_cond, int B, int S, float *gr,
                 float *d_pc) {
    const Geom &g = w.geo;
    const int M = B * S, CTOK = g.ctok;
    float *Dh = w.t[0], *E = w.t[1], *F = w.t[2];
    hipLaunchKernelGGL(mt_swap_rows_kernel, dim3((unsigned)M), dim3(256), 0, st, d_cond, Dh, S, B);
    IDF_CHECK_LAUNCH();
    for (int l = N_LAYERS - 1; l >= 0; --l) {
        const LayerOff &o = EL.layer[l];
        const LayerWs &y = e.layer[l];
        MT_TRY(ln_bwd(st, Dh, y.xh[1], y.rs[1], th + o.ln_w[1], gr + o.ln_w[1], gr + o.ln_b[1], E, w.partial, M));              // E = d s2 = d x1 (residual)
        MT_TRY(ffn_bwd(st, w, th, gr, o, E, y.x1, y.z, F, M));                                                                  // F = d x1
        MT_TRY(ln_bwd(st, F, y.xh[0], y.rs[0], th + o.ln_w[0], gr + o.ln_w[0], gr + o.ln_b[0], E, w.partial, M));              // E = d s1
        MT_TRY(mix_bwd(st, w, th, gr, o, is_qan(l), E, e.h[l], y.qkv, y.ao, y.lse, y.G, F, Dh, B, S));
    }
    // Dh = d embedding: pe takes nothing, pc_embedding the sum over a clip's tokens in token order, the two shared linears their encoder-path share
    hipLaunchKernelGGL(mt_sum_frames_kernel, dim3((unsigned)B), dim3(256), 0, st, Dh, d_pc, S);
    IDF_CHECK_LAUNCH();
    MT_TRY(lin_param_grads(st, w, Dh, D, e.Xp, CTOK, e.genc + L.body_w, e.genc + L.body_b, M, D, g.nbody));
    MT_TRY(lin_param_grads(st, w, Dh, D, e.Xp + g.nbody, CTOK, e.genc + L.obj_w, e.genc + L.obj_b, M, D, g.nobj));
    hipLaunchKernelGGL(mt_add_into_kernel, dim3(blocks256(n_shared(L))), dim3(256), 0, st, gr, e.genc, n_shared(L));
    IDF_CHECK_LAUNCH();
    return IDF_OK;
}

}  // namespace mdmtrain

// ---- the SMPL trainer's entries -------------------------------------------------------------------------------------------------------------------------------
namespace {

constexpr Geom GEO = SMPL_GEOM;
const Layout &layout() {
    static const Layout L = make_layout(GEO);
    return L;
}
const EncLayout &enc_layout() {
    static const EncLayout L = make_enc_layout(GEO, layout());
    return L;
}
// w.Y [B*T][144] -> pred [B,1,144,T]
int emit_pred(hipStream_t st, const Ws &w, int B, int T, float *pred) { return rows_to_tokens(st, w.Y, pred, B, T, GEO.ctok); }
// the terms, the loss gradient (or d_pred_in in its place) as rows in w.dY
int terms_and_d_rows(hipStream_t st, const Ws &w, const float *pred, const float *target, int B, int T, int past_len, const float *weights16, const float *d_pred_in,
                     float *terms, void *stream) {
    MT_TRY(interdiff_denoising_losses(pred, target, B, T, past_len, terms, stream));
    const float *dp = d_pred_in;
    if (!dp) {
        float *mine = w.g;                                        // (free between the forward and the backward; M * 1024 >= B * 144 * T floats)
        MT_TRY(loss_grad(st, pred, target, B, T, past_len, weights16, mine));
        dp = mine;
    }
    return tokens_to_rows(st, dp, w.dY, B, T, GEO.ctok);
}

}  // namespace

extern "C" int interdiff_denoising_loss_grad(const float *pred, const float *target, int32_t B, int32_t T, int32_t past_len, const float *weights16, float *d_pred,
                                             void *stream) {
    if (!pred || !target || !weights16 || !d_pred || B <= 0 || past_len < 2 || T < past_len + 2) return IDF_E_INVAL;
    return loss_grad(idf_stream(stream), pred, target, B, T, past_len, weights16, d_pred);
}

extern "C" int interdiff_mdm_train_param_table(int64_t *offsets, int64_t *sizes, int32_t *n_tensors, int64_t *n_param) {
    const Layout &L = layout();
    return table_out({{L.off, L.size, N_TENSORS}}, L.total, offsets, sizes, n_tensors, n_param);
}

extern "C" size_t interdiff_mdm_train_workspace_bytes(int32_t B, int32_t T, int32_t mem_len) {
    if (B <= 0 || T <= 0 || T > MAX_T || mem_len <= 0 || mem_len > MAX_MEM || (int64_t)B * T * GEO.ff >= 0x7FFFFFFF) return 0;
    return plan(nullptr, GEO, B, T, mem_len).floats * sizeof(float);
}

extern "C" int interdiff_mdm_train_grads(const float *params, const float *pe, int32_t pe_rows, const float *x_t, const int64_t *ts, const float *cond, const float *target,
                                         int32_t B, int32_t T, int32_t mem_len, int32_t past_len, const float *weights16, const float *d_pred_in, float *grads,
                                         float *d_cond, float *pred, float *terms, void *ws, size_t ws_bytes, void *stream) {
    if (!params || !pe || !x_t || !ts || !cond || !target || !weights16 || !grads || !d_cond || !pred || !terms || !ws) return IDF_E_INVAL;
    if (!shape_ok(GEO, B, T, mem_len, past_len) || pe_rows < T) return IDF_E_INVAL;
    MT_TRY(ws_check(ws, ws_bytes, interdiff_mdm_train_workspace_bytes(B, T, mem_len)));
    hipStream_t st = idf_stream(stream);
    const Layout &L = layout();
    const Ws w = plan(static_cast<float *>(ws), GEO, B, T, mem_len);
    MT_TRY(forward(st, L, w, params, pe, pe_rows, x_t, ts, cond, B, T, mem_len));
    MT_TRY(emit_pred(st, w, B, T, pred));
    MT_TRY(terms_and_d_rows(st, w, pred, target, B, T, past_len, weights16, d_pred_in, terms, stream));
    return backward(st, L, w, params, cond, B, T, mem_len, grads, d_cond);
}

extern "C" int interdiff_mdm_train_full_param_table(int64_t *offsets, int64_t *sizes, int32_t *n_tensors, int64_t *n_param) {
    const Layout &L = layout();
    const EncLayout &EL = enc_layout();
    return table_out({{L.off, L.size, N_TENSORS}, {EL.off, EL.size, N_ENC_TENSORS}}, EL.total, offsets, sizes, n_tensors, n_param);
}

extern "C" size_t interdiff_mdm_train_full_workspace_bytes(int32_t B, int32_t T, int32_t past_len) {
    if (!shape_ok(GEO, B, T, past_len, past_len)) return 0;
    return full_plan(nullptr, GEO, layout(), B, T, past_len).e.floats * sizeof(float);
}

extern "C" int interdiff_mdm_train_full_grads(const float *params, const float *pe, int32_t pe_rows, const float *x_t, const int64_t *ts, const float *pc,
                                              const float *target, int32_t B, int32_t T, int32_t past_len, const float *weights16, const float *d_pred_in, float *grads,
                                              float *cond, float *d_cond, float *d_pc, float *pred, float *terms, void *ws, size_t ws_bytes, void *stream) {
    if (!params || !pe || !x_t || !ts || !pc || !target || !weights16 || !grads || !cond || !d_cond || !d_pc || !pred || !terms || !ws) return IDF_E_INVAL;
    if (!shape_ok(GEO, B, T, past_len, past_len) || pe_rows < T) return IDF_E_INVAL;
    MT_TRY(ws_check(ws, ws_bytes, interdiff_mdm_train_full_workspace_bytes(B, T, past_len)));
    hipStream_t st = idf_stream(stream);
    const Layout &L = layout();
    const EncLayout &EL = enc_layout();
    const auto [w, e] = full_plan(static_cast<float *>(ws), GEO, L, B, T, past_len);
    MT_TRY(enc_forward(st, L, EL, w, e, params, pe, target, pc, B, T, past_len, cond));
    MT_TRY(forward(st, L, w, params, pe, pe_rows, x_t, ts, cond, B, T, past_len));
    MT_TRY(emit_pred(st, w, B, T, pred));
    MT_TRY(terms_and_d_rows(st, w, pred, target, B, T, past_len, weights16, d_pred_in, terms, stream));
    MT_TRY(backward(st, L, w, params, cond, B, T, past_len, grads, d_cond));
    return enc_backward(st, L, EL, w, e, params, d_cond, B, past_len, grads, d_pc);
}

extern "C" int interdiff_mdm_train_step(float *params, const float *grads, float *exp_avg, float *exp_avg_sq, int64_t n, int32_t step, double lr, double beta1,
                                        double beta2, double eps, double weight_decay, void *stream) {
    if (!params || !grads || !exp_avg || !exp_avg_sq || n <= 0 || step < 1) return IDF_E_INVAL;
    const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
    AdamWK k;
    k.decay = (float)(1.0 - lr * weight_decay);
    k.w1 = (float)(1.0 - beta1);
    k.beta2 = (float)beta2;
    k.w2 = (float)(1.0 - beta2);
    k.step_size = (float)(lr / bc1);
    k.bc2_sqrt = (float)sqrt(bc2);
    k.eps = (float)eps;
    hipLaunchKernelGGL(mt_adamw_kernel, dim3(blocks256(n)), dim3(256), 0, idf_stream(stream), params, grads, exp_avg, exp_avg_sq, n, k);
    IDF_CHECK_LAUNCH();
    return IDF_OK;
}
