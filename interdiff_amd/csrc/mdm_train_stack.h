// The denoiser trainers' shared stacks, host side: what csrc/mdm_train.hip defines for the model-specific trainers (the SMPL trainer in that file, the skeleton
// trainer in csrc/skeleton_mdm_train.hip).  Both reference models (model/diffusion_smpl.py, model/diffusion_skeleton.py) are the same [std, QaN x6, std] decoder
// and encoder around two input embeddings, a timestep MLP and two output linears; they differ in the widths below and in what stands behind the output linears.
// Declarations only: the device code (csrc/mdm_train.h) is compiled once, in mdm_train.hip.
#pragma once
#include "common.h"
#include <initializer_list>

namespace mdmtrain {

constexpr int D = 256, HEADS = 4, HD = 64, NQ = 10, SLOTS = 3, MAX_MEM = 16, MAX_T = 128, N_LAYERS = 8;
constexpr float LN_EPS = 1e-5f;

// ff: feed-forward width.  ctok: channels of a token of x_t.  bodyEmbedding reads columns 0 .. nbody-1 and objEmbedding columns nbody .. nbody+nobj-1 of it.
// bodyFinalLinear gives hbody values and objFinalLinear hobj: a head row is [hbody | hobj], head() wide.
struct Geom {
    int ff, ctok, nbody, nobj, hbody, hobj;
    constexpr int head() const { return hbody + hobj; }
};
constexpr Geom SMPL_GEOM{1024, 144, 135, 9, 135, 9};
constexpr Geom SKELETON_GEOM{256, 106, 63, 36, 63, 7};           // the 7 pose columns of x_t are read by nothing (diffusion_skeleton.py:236-238)

constexpr int N_TENSORS = 144, N_ENC_TENSORS = 84, N_FULL_TENSORS = N_TENSORS + N_ENC_TENSORS;

// One layer of either stack.  An encoder layer has no cross-attention (ca_* = -1) and two LayerNorms (ln_*[2] = -1); a QaN layer has queries / wk in the place of sa_*.
struct LayerOff {
    int64_t sa_in_w, sa_in_b, sa_out_w, sa_out_b, queries, wk, ca_in_w, ca_in_b, ca_out_w, ca_out_b, l1_w, l1_b, l2_w, l2_b, ln_w[3], ln_b[3];
};
struct Layout {
    int64_t body_w, body_b, obj_w, obj_b, t0_w, t0_b, t2_w, t2_b, bodyf_w, bodyf_b, objf_w, objf_b, total;
    LayerOff layer[N_LAYERS];
    int64_t off[N_TENSORS], size[N_TENSORS];
};
struct EncLayout {
    int64_t total;                                                // of the 144 + 84 tensors
    LayerOff layer[N_LAYERS];
    int64_t off[N_ENC_TENSORS], size[N_ENC_TENSORS];
};
// the 144 tensors of a decoder-side flat vector, and the 84 encoder tensors behind them, packed without padding (orders: include/interdiff_hip.h)
Layout make_layout(const Geom &g);
EncLayout make_enc_layout(const Geom &g, const Layout &L);
// A parameter table's entry: the (off, size, n) runs in `parts`, one after the other, copied out; any output may be null.
struct TableRun {
    const int64_t *off, *size;
    int n;
};
int table_out(std::initializer_list<TableRun> parts, int64_t total, int64_t *offsets, int64_t *sizes, int32_t *n_tensors, int64_t *n_param);

// ---- workspace plans (floats) ---------------------------------------------------------------------------------------------------------------------------
// hands out 64-float-aligned slots behind base + at; with a null base it only counts
struct Carver {
    float *base;
    size_t at;
    float *operator()(size_t n) {
        float *p = base ? base + at : nullptr;
        at += (n + 63) / 64 * 64;
        return p;
    }
};
// One layer's saves in either stack.  An encoder layer leaves x2, q2, kv, o2 and xh[2] / rs[2] null.
struct LayerWs {
    float *qkv, *ao, *lse, *xh[3], *rs[3], *x1, *x2, *q2, *kv, *o2, *z, *G;
};
struct Ws {
    Geom geo;
    float *X, *Y, *dY, *tin, *z0, *sz, *temb, *h[N_LAYERS + 1];  // X [M][ctok] the rows of x_t; Y / dY [M][head()] the head rows and their gradient
    LayerWs layer[N_LAYERS];
    float *g, *dz, *t[4], *dqkv, *P, *dS, *Pc, *dSc, *dkv, *dG, *dsim, *cj, *dwk_tok, *partial, *dtemb, *dsz;
    size_t floats;
};
struct EncWs {
    float *Xp, *h[N_LAYERS + 1], *genc;
    LayerWs layer[N_LAYERS];
    size_t floats;                                                // decoder plan included
};
Ws plan(float *base, const Geom &g, int B, int T, int S);
EncWs enc_plan(float *base, size_t at, const Geom &g, const Layout &L, int B, int S);
// the decoder's plan with the encoder's behind it, S = past_len: what a whole-model gradient call works in
struct FullWs {
    Ws w;
    EncWs e;
};
FullWs full_plan(float *base, const Geom &g, const Layout &L, int B, int T, int past_len);
// a *_grads entry's workspace check: 256-byte alignment (IDF_E_INVAL), then room for `need` bytes (IDF_E_NOMEM)
int ws_check(const void *ws, size_t ws_bytes, size_t need);
bool shape_ok(const Geom &g, int B, int T, int S, int past_len);

// ---- launchers: every one returns IDF_OK or IDF_E_LAUNCH ---------------------------------------------------------------------------------------------------
#define MT_TRY(x)                  \
    do {                           \
        const int mt_rc_ = (x);    \
        if (mt_rc_ != IDF_OK) return mt_rc_; \
    } while (0)

// Y[M,N] = X[M,K] W[N,K]^T + b (+ R)
int lin_fwd(hipStream_t st, const float *X, int64_t ldx, const float *W, const float *b, float *Y, int64_t ldy, const float *R, int64_t ldr, int M, int N, int K);
// a linear layer's parameter gradients: dW = dY^T X, db = column sums of dY
int lin_param_grads(hipStream_t st, const Ws &w, const float *dY, int64_t ldy, const float *X, int64_t ldx, float *dW, float *db, int M, int N, int K);

// The decoder with saves: x_t [B][ctok][T] -> w.Y, the head rows [B*T][head()] = bodyFinalLinear | objFinalLinear.
int forward(hipStream_t st, const Layout &L, const Ws &w, const float *th, const float *pe, int pe_rows, const float *x_t, const int64_t *ts, const float *cond, int B, int T,
            int S);
// w.dY (the gradient of the head rows) -> the 144 gradients in gr, d_cond [S][B][256]
int backward(hipStream_t st, const Layout &L, const Ws &w, const float *th, const float *cond, int B, int T, int S, float *gr, float *d_cond);
// The encoder with saves: the past frames of target [B][ctok][T] and a per-clip row `pc` [B][256] added to every token -> cond [S][B][256]
int enc_forward(hipStream_t st, const Layout &L, const EncLayout &EL, const Ws &w, const EncWs &e, const float *th, const float *pe, const float *target, const float *pc,
                int B, int T, int S, float *cond);
// d_cond -> the 84 encoder gradients, the encoder path's share of the four shared embedding tensors added into gr, d_pc [B][256]
int enc_backward(hipStream_t st, const Layout &L, const EncLayout &EL, const Ws &w, const EncWs &e, const float *th, const float *d_cond, int B, int S, float *gr,
                 float *d_pc);

}  // namespace mdmtrain
