/*
 * interdiff_hip.h -- C-ABI of the MI355X-native InterDiff denoising-sampler hot path.
 *
 * The reference (Sirui-Xu/InterDiff) has no FFI: its seams are Python callables on torch
 * tensors.  This library is what a binding for those seams would load:
 * every entry point below names the reference callable it replaces (file:line relative to
 * /root/reference/interdiff).  INTEGRATION.md shows the ctypes stub for each.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer (gfx950 HBM) unless its name starts with h_;
 *  - tensors are dense, row-major, fp32 unless stated; shapes are given in comments;
 *  - `stream` is a hipStream_t passed as void* (NULL = the null stream); all work is
 *    enqueued asynchronously on it, nothing synchronises, nothing allocates: scratch comes
 *    from the caller (`ws`, sized by the matching *_workspace_bytes function);
 *  - return value: 0 on success, a negative code on error (IDF_E_*); no exceptions, no
 *    callbacks, no mutable process state (the only statics are idempotent per-device caches of a
 *    kernel attribute, see csrc/common.h idf_opt_in_lds) => safe to capture in a hipGraph;
 *  - inputs are borrowed; outputs are caller-allocated.
 */
#ifndef INTERDIFF_HIP_H
#define INTERDIFF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IDF_OK            0
#define IDF_E_INVAL      -22   /* bad shape / null pointer / unsupported size            */
#define IDF_E_NOMEM      -12   /* workspace too small                                     */
#define IDF_E_LAUNCH     -5    /* hipGetLastError() != hipSuccess after a launch          */

int         interdiff_abi_version(void);          /* bumped on any signature change       */
const char *interdiff_build_info(void);           /* "gfx950 hipcc ..."                   */

/* ------------------------------------------------------------------------------------
 * Rotation conversions  (pytorch3d.transforms 0.7.2 semantics; eval_smpl_short.py:18,
 * 33,65-66,90-91,157-162; model/diffusion_smpl.py:212-213).  n = number of rotations.
 * quaternions are (w,x,y,z); matrices row-major 3x3; rot6d = first two ROWS.
 * ---------------------------------------------------------------------------------- */
int interdiff_rotation_6d_to_matrix   (const float *d6, float *m,  int64_t n, void *stream);
int interdiff_matrix_to_rotation_6d   (const float *m,  float *d6, int64_t n, void *stream);
int interdiff_matrix_to_axis_angle    (const float *m,  float *aa, int64_t n, void *stream);
int interdiff_axis_angle_to_matrix    (const float *aa, float *m,  int64_t n, void *stream);
int interdiff_axis_angle_to_quaternion(const float *aa, float *q,  int64_t n, void *stream);
int interdiff_rotation_6d_to_axis_angle(const float *d6, float *aa, int64_t n, void *stream);

/* ------------------------------------------------------------------------------------
 * SMPL-H forward kinematics + linear blend skinning
 * replaces SMPL_Layer.forward  (libsmpl/smplpytorch/pytorch/smpl_layer.py:72-175).
 *
 * The model is passed as PACKED constants built once on the host
 * (interdiff_amd/smpl.py: pack_smpl_model):
 *   blend   [3V][KB]   KB = round_up(9(J-1)+n_betas+1, 8): per output coordinate the row
 *                      [posedirs(9(J-1)) | shapedirs(n_betas) | v_template | 0-pad]
 *   jt      [J][3]     J_regressor . v_template
 *   js      [J][3][n_betas]  J_regressor . shapedirs
 *   parents [J] int32  (parents[0] ignored)
 *   skin_idx[V][S] int32, skin_w [V][S]   ELL form of the skinning weights (zeros dropped,
 *                      padded with weight 0 / index 0); S = max non-zeros per vertex
 * ---------------------------------------------------------------------------------- */
typedef struct {
    int32_t V, J, n_betas, KB, S;
    const float   *blend;      /* blend basis [posedirs | shapedirs | template] (KB columns) in the kernel's MFMA fragment order: [ceil(V/64)][4][3][KB/16][64][4], rows past 3V zero (smpl.py pack_smpl_model) */
    const float   *jt;
    const float   *js;
    const int32_t *parents;
    const int32_t *skin_idx;
    const float   *skin_w;
} idf_smpl_model;

size_t interdiff_smpl_workspace_bytes(const idf_smpl_model *m, int64_t N);
/* pose [N,3J] axis-angle, betas [N,n_betas], trans [N,3] -> verts [N,V,3], jtr [N,J,3],
 * v_posed [N,V,3] (may be NULL). */
int interdiff_smpl_forward(const idf_smpl_model *m, const float *pose, const float *betas,
                           const float *trans, int64_t N, float *verts, float *jtr,
                           float *v_posed, void *ws, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------------------------
 * Geometry
 * vertex_normals        replaces data/tools.py:4-40   (faces NOT repeated per frame)
 *   adj_ptr [V+1], adj_face [nnz], adj_corner [nnz] (uint8 as int32): vertex->incident
 *   faces in the reference's accumulation order (corner 1, corner 2, corner 0; ascending
 *   face index inside each) -- built by interdiff_amd/geometry.py: build_vertex_adjacency.
 * nn_argmin / point2point_signed replace tools.py:11-76 + chamfer_distance (brute force,
 *   d2 = (dx*dx+dy*dy)+dz*dz without FMA, lowest index wins ties).
 * ---------------------------------------------------------------------------------- */
int interdiff_vertex_normals(const float *verts, int64_t N, int32_t V, const int32_t *faces,
                             const int32_t *adj_ptr, const int32_t *adj_face,
                             const int32_t *adj_corner, float *normals, void *stream);
/* q [N,Pq,3], r [N,Pr,3] -> idx int32 [N,Pq] : nearest r for every q */
int interdiff_nn_argmin(const float *q, int32_t Pq, const float *r, int32_t Pr, int64_t N,
                        int32_t *idx, void *stream);
/* x [N,P1,3], y [N,P2,3], optional normals (NULL = unsigned).  Outputs as tools.py:73-76:
 * y2x_signed [N,P2], x2y_signed [N,P1], yidx [N,P2], xidx [N,P1], y2x [N,P2,3], x2y [N,P1,3]
 * (vector outputs may be NULL). */
int interdiff_point2point_signed(const float *x, int32_t P1, const float *y, int32_t P2, int64_t N,
                                 const float *x_normals, const float *y_normals,
                                 float *y2x_signed, float *x2y_signed, int32_t *yidx, int32_t *xidx,
                                 float *y2x, float *x2y, void *stream);

/* ------------------------------------------------------------------------------------
 * MDM denoiser, decoder path   replaces MDM.forward / _decode
 * (model/diffusion_smpl.py:226-246; layers [std, QaN x6, std], sublayers.py:206-375).
 *
 * Weights are packed once from a state_dict with the reference's key names
 * (interdiff_amd/mdm.py: pack_mdm_weights) into ONE fp32 arena; idf_mdm_weights holds
 * offsets (in floats) into it.  Token rows are clip-major: row = b*T + t.
 * ---------------------------------------------------------------------------------- */
#define IDF_MDM_LAYERS 8
#define IDF_MDM_D      256
#define IDF_MDM_FF     1024
#define IDF_MDM_HEADS  4
#define IDF_MDM_NQ     10      /* learned queries per QaN layer                          */
#define IDF_MDM_MEM    10      /* memory (past) tokens: the default (every BASELINE config), compact layout of the folded memory */
#define IDF_MDM_MEM_MAX 16     /* longest memory (idf_mdm_weights.mem_len): the reference takes --past_len from the CLI (eval_smpl_short.py:376) */
#define IDF_FFN_SLICES 5       /* hidden-unit slices of the fused FFN = partial output slabs (csrc/ffn.h) */

typedef struct {
    int64_t is_qan;            /* 0: torch TransformerDecoderLayer, 1: QaN               */
    int64_t sa_in_w, sa_in_b, sa_out_w, sa_out_b;   /* std only: [768,256],[768],[256,256],[256] */
    int64_t qc, wk;            /* QaN only: Qc [NQ][3][256] (pre-rotated, pre-scaled) in MFMA fragment order [16][3][4][NQ][4] (mdm.py qan_fragments), wk [NQ] */
    int64_t ca_q_w, ca_q_b;    /* cross-attn query proj [256,256],[256]                  */
    int64_t ca_kv_w, ca_kv_b;  /* cross-attn key|value proj [512,256],[512]              */
    int64_t ca_out_w, ca_out_b;
    int64_t ff1_w, ff1_b, ff2_w, ff2_b;             /* [1024,256],[1024],[256,1024],[256] */
    int64_t ffn_pack;          /* linear1 + linear2 weights in the fused FFN kernel's stream order (5 x 106496 floats, mdm.py pack_ffn) */
    int64_t ffn_b1p;           /* linear1 bias zero-padded to 5 x 208 (+ 256 spare floats)                                      */
    int64_t sa_in_pack;        /* std only: sa_in_w in the LayerNorm+linear kernel's stream order (5 slices x 16 chunks [160][16], rows past 768 zero; mdm.py pack_linear160) */
    int64_t sa_out_frag;       /* std only: sa_out_w in MFMA fragment order [head][4 column quarters][4 k-groups][4 column tiles][64 lanes][4] (mdm.py sa_out_fragments): the attention kernel's out-projection tail */
    int64_t ln_w[3], ln_b[3];
    int64_t ffn_pack_h2;       /* 0, or linear1 + linear2 split into two f16 planes (hi, residual x 2^11) in the split-f16 FFN kernel's stream order
                                  (5 x 110592 floats, mdm.py pack_ffn_h2; csrc/ffn_h2.h).  Only set when the packer has PROVED that no operand of
                                  this layer's feed-forward block can leave the f16 range (mdm.py ffn_h2_range_ok) */
    int64_t sa_in_pack_h2;     /* std only: 0, or sa_in_w as two f16 planes in the split-f16 QKV kernel's stream order (5 slices x 8 K steps
                                  [10 tiles][2 planes][64 lanes][8 halves], rows past 768 zero; mdm.py pack_linear160_h2; csrc/ffn_h2.h
                                  ln_linear_h2_kernel).  The kernel scales every input row by a power of two, so only the weights' range matters */
    int64_t qc_h2;             /* QaN only: 0, or Qc as two f16 planes in the split-f16 row block's fragment order [4 K quarters][2 K steps][3 taps][2 planes][4 kq][NQ][8 halves]
                                  (mdm.py qan_fragments_h2; csrc/rowblock.h rowblock_kernel<.., H2>) */
    int64_t rb_h2_ok;          /* decoder layers: 1 when the packer has proved that the LayerNorm outputs this layer's row block contracts (LN_prev, norm1) stay inside
                                  the f16 range (16 max|gamma| + max|beta| < 65504; mdm.py ln_h2_range_ok) -- with tune[IDF_TUNE_FFN_MATH] == 1 the row block then runs
                                  its three contractions as split-f16 products; 0 = always exact fp32 */
    int64_t sa_out_frag_h2;    /* std only: 0, or sa_out_w as two f16 planes in the split-f16 attention kernel's fragment order [head][16 output column tiles][2 K steps][2 planes]
                                  [64 lanes][8 halves] (mdm.py sa_out_fragments_h2; csrc/attn_h2.h) */
    int64_t qkv_bounds_ok;     /* std only: 1 when eight floats stand right behind the sa_in_pack_h2 stream (arena offset sa_in_pack_h2 + 5 x 40960): max over the q, k, v rows
                                  of sa_in_w of their L1 norm (x 1.001), max |sa_in_b| of the q, k, v rows, two spare (mdm.py qkv_bounds).  With them the QKV kernel may write
                                  its output as the self-attention's f16 plane pairs -- |q_c| <= 2^e_row ||W_c||_1 + |b_c| is the per-row power of two it divides by --
                                  instead of fp32 rows (csrc/ffn_h2.h ln_linear_h2_kernel<.., PLANES>); 0: fp32 rows, the attention splits them itself */
} idf_mdm_layer;

typedef struct {
    int32_t C;                 /* token width (144; 106 for the skeleton tokens of config #1) */
    int32_t n_steps;           /* rows of temb_table                                     */
    const float *arena;
    int64_t in_w, in_b;        /* [256][(C + 3) & ~3] = [bodyEmbedding | objEmbedding | 0], summed bias  */
    int64_t out_w, out_b;      /* [C][256] = [bodyFinalLinear ; objFinalLinear]          */
    int64_t temb_table;        /* [n_steps][256] = time_embed(pe[t]) (weights-only const) */
    int64_t pe;                /* [max_T][256] positional table rows 0..max_T-1          */
    int32_t max_T, has_encoder;
    idf_mdm_layer layer[IDF_MDM_LAYERS];
    /* encoder side ("next" row, MDM._get_embeddings): [std, QaN x6, std] without cross-attention; uses sa_*, qc, wk,
     * ff*, ln_w/ln_b[0..1] (= norm1, norm2); valid when has_encoder != 0 */
    idf_mdm_layer enc_layer[IDF_MDM_LAYERS];
    /* per-handle kernel selection, indexed by IDF_TUNE_*; all zero = exact fp32 arithmetic with the row tile picked per launch.  A field of the
     * handle, not process state: two models in one process never see each other's selection.  Two entries are meaningful; the other six are
     * reserved and must be zero (interdiff_mdm_forward*, interdiff_mdm_encode and interdiff_mdm_ffn return IDF_E_INVAL otherwise).
     * tune[IDF_TUNE_FFN], the row tile of the fused feed-forward block: 0 = by the rows of
     * the launch (16-row tiles up to 800 rows, 64-row tiles from 2800 rows on, 32-row tiles
     * otherwise: csrc/ffn.h ffn_tile_for_rows), 1 = 32-row tiles, 2 = 16-row tiles, 3 = 64-row tiles.  The 32-row kernel agrees with
     * the other two to rounding (7e-7 of the output scale), not bit for bit: a caller that steps ONE batch as several calls on row subsets (the
     * sampler's half-batch chains) sets 1 or 2 from the rows of the whole batch so that every call takes the same kernel
     * (interdiff_amd/mdm.py: MDM._pick_ffn_tile does this before every forward / forward_step / encode / ffn call).
     * tune[IDF_TUNE_FFN_MATH] selects the arithmetic of the feed-forward block, of the QKV projection (layers whose sa_in_pack_h2 is set) AND of the row block's three contractions (layers whose rb_h2_ok -- and, QaN, qc_h2 -- is set): 0 = exact fp32 MFMA (v_mfma_f32_16x16x4_f32, csrc/ffn.h),
     * 1 = split-f16 (every fp32 operand as two f16 planes, three v_mfma_f32_16x16x32_f16 per product, fp32 accumulate: fp32-grade
     * results at 1/43 of the matrix-pipe time, csrc/ffn_h2.h) for every layer whose ffn_pack_h2 is set, exact fp32 for the others.  Its
     * 16-, 32- and 64-row tiles are bit-identical, so with 1 the row tile is a pure performance choice.  2 = like 1 for the feed-forward block and the QKV
     * projection, exact fp32 in the row block. */
    int32_t tune[8];
    /* split-f16 plane fragments of the two token GEMMs at the ends of a step (csrc/tail_h2.h; mdm.py pack_tail_h2), 0 = not packed (token width != 144
     * or a value outside the f16 range): out_w as [9 output tiles][8 K steps][2 planes][64 lanes][8 halves], in_w as [16][5][2][64][8] (K = 144 padded to 160) */
    int64_t out_w_h2, in_w_h2;
    /* 1 when the packer has proved that the heads GEMM's A operand -- LayerNorm norm3 of the LAST decoder layer -- stays inside the f16 range
     * (mdm.py ln_h2_range_ok on its gamma / beta); 0: the step tail keeps the fp32 token GEMMs (and interdiff_mdm_forward_step_ex ignores its flags) */
    int64_t tail_h2_ok;
    /* memory length of the NEXT interdiff_mdm_prepare_memory / forward calls on this handle: rows of cond [mem_len,B,256].  0 = IDF_MDM_MEM (10).  Any 1 ..
     * IDF_MDM_MEM_MAX is served; 10 takes the compact (fast) layout of the folded memory, other lengths a generic one (one more score-column tile in the row
     * block).  A memctx folded at one length must be consumed at the same length (its size differs: interdiff_mdm_memctx_floats_for). */
    int32_t mem_len;
    /* tokens per workgroup of the split-f16 row block (csrc/rowblock.h rowblock8_kernel): 0 = by the launch (8 while B x ceil(T / 8) workgroups fit the chip in one
     * round, else 16), 8 / 16 = forced (A/B runs).  Both forms compute the same bits. */
    int32_t rb_tokens;
} idf_mdm_weights;

/* The token GEMM of the denoiser as a standalone op: C[M,N] = epi(A[M,K] . W[N,K]^T + bias) on the fp32 MFMA
 * (torch.nn.functional.linear semantics; model/diffusion_smpl.py:73-120 linear1/linear2/out_proj).  epi: 0 bias,
 * 1 bias + erf-GELU, 2 bias + resid (leading dimension ldc).  cfg 0 = shipped tile configuration.  K % 64 == 0, N % 16 == 0. */
int interdiff_gemm_f32(const float *A, int32_t lda, const float *W, const float *bias, const float *resid, float *C,
                       int32_t ldc, int32_t M, int32_t N, int32_t K, int32_t epi, int32_t cfg, void *stream);

/* per-sample constants derived from the memory `cond` (constant over all steps): for every
 * layer and clip the folded cross-attention operands
 *   G   [L][B][40][256]  (scores = x . G^T + g0, 40 = heads*MEM, pre-scaled by 1/sqrt(64))
 *   VWT [L][B][256][48]  (out = P . VW + out_bias, stored output-column-major, 40 padded to 48)
 *   g0  [L][B][40]
 * and, behind them, the same G / VW as split-f16 plane fragments for the row block's f16-MFMA form (csrc/denoiser_common.h G_H2, csrc/rowblock.h VW_H2: each (layer,
 * clip) matrix divided by the power of two that puts its largest magnitude in [2^13, 2^14), two f16 planes, fragment order) with the two powers
 * of two per (layer, clip).  Both forms are always folded; which one a forward reads follows tune[IDF_TUNE_FFN_MATH].  The layout is private to
 * the library: `memctx` is an opaque buffer of interdiff_mdm_memctx_floats(B) floats.
 * cond [MEM,B,256] (reference layout). */
/* The feed-forward block of one layer as a standalone op (what bench.py times for its roofline block; the denoiser launches the
 * same kernel): x2 [M,256] -> parts [IDF_FFN_SLICES][M][256] whose sum over the slabs is x2 + linear2(gelu(linear1(x2)))
 * (torch.nn.TransformerDecoderLayer._ff_block + residual; sublayers.py:331-341).  encoder != 0 selects enc_layer[layer].
 * Row tile by w->tune[IDF_TUNE_FFN] (see idf_mdm_weights). */
int interdiff_mdm_ffn(const idf_mdm_weights *w, int32_t layer, int32_t encoder, const float *x2, int32_t M, float *parts, void *stream);
/* floats of a memctx for B clips at memory length mem_len (1 .. IDF_MDM_MEM_MAX; 0 if out of range); interdiff_mdm_memctx_floats(B) is the mem_len = 10 case */
size_t interdiff_mdm_memctx_floats_for(int32_t B, int32_t mem_len);

size_t interdiff_mdm_memctx_floats(int32_t B);
size_t interdiff_mdm_workspace_bytes(int32_t B, int32_t T);
int interdiff_mdm_prepare_memory(const idf_mdm_weights *w, const float *cond, int32_t B,
                                 float *memctx, void *ws, size_t ws_bytes, void *stream);
/* x [B,1,C,T], ts int64 [B] -> x0 [B,1,C,T].
 * Size limits (IDF_E_INVAL beyond them): T <= max_T of the packed positional table (mdm.py pack_mdm_weights(max_T=): up to the 5000 rows of the
 * reference's PositionalEncoding).  Up to T = 208 the temporal self-attention of the two standard layers parks K and V of one (clip, head) in one CU's
 * LDS (2 x T x 68 floats + the score tile = 149 KiB at T = 208: the fast path, every BASELINE shape); longer clips take a K/V-tiled form of the same
 * attention (64-key tiles, running row maximum / sum; csrc/attn.h self_attn_tiled_kernel) -- correct, not tuned.  Memory length: idf_mdm_weights.mem_len;
 * C <= 256 (any width: W_in's rows are packed zero-padded to a multiple of 4 floats, mdm.py; BASELINE config #1 has C = 106).  The reference itself is bounded only by PositionalEncoding(max_len=5000) (model/layers.py:11); its
 * datasets use T = 35 (eval_smpl_short.py:376-377) and BASELINE.json T = 100.  B is unbounded (clips are independent). */
int interdiff_mdm_forward(const idf_mdm_weights *w, const float *memctx, const float *x,
                          const int64_t *ts, int32_t B, int32_t T, float *x0,
                          void *ws, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------------------------
 * Conditioning path ("next" row of SURVEY.md §8(f)): MDM._get_embeddings (model/diffusion_smpl.py:195-223) minus
 * the dataset plumbing.
 *  interdiff_pointnet2_encode   replaces PointNet2Encoder.forward (model/layers.py:141-175) with one key point:
 *      obj_points [B,P,3] (P <= 2048) -> pc [B,256] = [key-point xyz | Linear(SA2 features)]; eval BatchNorm folded
 *      into the shared-MLP convolutions at pack time (weights [cout][cin] + bias per layer).
 *  interdiff_mdm_encode         replaces bodyEmbedding/objEmbedding + PositionalEmbedding + encoder:
 *      x_past [B,1,C,Tp] (the first Tp = past_len frames of the token tensor), pc [B,256] -> cond [Tp,B,256].
 * ---------------------------------------------------------------------------------- */
typedef struct {
    int64_t w[3], b[3];        /* offsets into the arena: folded conv*BN weight [c[l+1]][c[l]], bias [c[l+1]]        */
    int32_t c[4];              /* channel plan (input includes the 3 xyz channels)                                 */
} idf_pn_mlp;

typedef struct {
    const float *arena;
    idf_pn_mlp sa1[2];         /* radii 0.05 / 0.1, 16 / 32 samples: 4-16-16-32, 4-32-32-64                        */
    idf_pn_mlp sa2[2];         /* radii 0.1 / 0.2, 16 / 32 samples: 99-64-64-128, 99-64-96-128                     */
    int64_t lin_w, lin_b;      /* Linear [253][256], [253]                                                         */
} idf_pointnet2;

int interdiff_pointnet2_encode(const idf_pointnet2 *pn, const float *obj_points, int32_t B, int32_t P, float *out,
                               void *stream);
size_t interdiff_mdm_encode_workspace_bytes(int32_t B, int32_t Tp);
int interdiff_mdm_encode(const idf_mdm_weights *w, const float *pc, const float *x_past, int32_t B, int32_t Tp,
                         float *cond, void *ws, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------------------------
 * Sampler step   replaces p_mean_variance's inpainting + q_posterior mean and p_sample's
 * noise add (diffusion/gaussian_diffusion.py:307-311,374,532-547):
 *   x0   = mask ? gt : x0                      (mask [n] uint8, may be NULL)
 *   x    = c1*x0 + c2*x + sigma*eps            (sigma = 0 at t == 0)
 * eps comes from `noise` [n] when non-NULL, else from the counter-based generator
 * (Philox4x32-10 + Box-Muller) keyed by (seed, step_index, element).
 * `inpaint_only` != 0 applies just the first line (used before the correction hook).
 * ---------------------------------------------------------------------------------- */
int interdiff_inpaint(float *x0, const float *gt, const uint8_t *mask, int64_t n, void *stream);
int interdiff_posterior_step(float *x, const float *x0, const float *noise, int64_t n,
                             float c1, float c2, float sigma, uint64_t seed, uint64_t step_index,
                             void *stream);
int interdiff_randn(float *out, int64_t n, uint64_t seed, uint64_t step_index, void *stream);
/* The same two with an element offset: `elem0` (a multiple of 4, else IDF_E_INVAL) is the position of x[0] / out[0] inside the
 * tensor whose noise stream is being drawn.  The reference fills ONE randn_like tensor for the whole batch
 * (gaussian_diffusion.py:532); a rank that holds clips [first, first + B_local) of that batch passes
 * elem0 = first * C * T and draws exactly the elements the unsharded run would ("sliced from one global
 * tensor for parity with a 1-GPU run") -- sharded == unsharded bit for bit.  The un-suffixed entries are elem0 = 0. */
int interdiff_posterior_step_at(float *x, const float *x0, const float *noise, int64_t n,
                                float c1, float c2, float sigma, uint64_t seed, uint64_t step_index,
                                uint64_t elem0, void *stream);
int interdiff_randn_at(float *out, int64_t n, uint64_t seed, uint64_t step_index, uint64_t elem0, void *stream);
/* Graph-replayable form of the same update: all per-step scalars live in HBM, so one captured hipGraph of
 * [interdiff_mdm_forward -> interdiff_posterior_step_dev -> interdiff_sampler_advance] serves every plain step.
 *   state int64[4] = {t (current timestep), loop index (noise counter), seed, arrival counter (zero it once)};
 *   table  f32[steps][4] = {c1[t], c2[t], sigma[t] (0 at t == 0), t/1000};
 *   mask/gt may be NULL (x0 already inpainted).  With ts != NULL the launch also advances the state when its last
 *   workgroup retires: t -= 1, loop index += 1, ts[b] = max(t, 0) for b < B (interdiff_sampler_advance does only that). */
int interdiff_posterior_step_dev(float *x, const float *x0, const float *gt, const uint8_t *mask, int64_t n,
                                 const float *table, int64_t *state, int64_t *ts, int32_t B, void *stream);
int interdiff_sampler_advance(int64_t *state, int64_t *ts, int32_t B, void *stream);
/* Respaced schedules (diffusion/respace.py:64-129: SpacedDiffusion keeps a subset of the base process's timesteps and
 * _WrappedModel.__call__, :124-126, hands the MODEL map_tensor[ts] while everything else -- coefficient tables, denoised_fn, the
 * loop -- counts spaced steps).  tmap int64[steps] = timestep_map: the model's timestep of every loop-side step.  The _map entries are
 * the un-suffixed ones with one change: where those write ts[b] = max(t - 1, 0), these write ts[b] = tmap[max(t - 1, 0)].  state[0],
 * the table row, the parked {t, loop index} (state[4..5]) and the Philox step index stay LOOP-side values; ts holds MODEL timesteps
 * (the caller starts a sample with ts[b] = tmap[t_start]).  tmap == NULL is the identity: the un-suffixed entries call these with
 * NULL and keep their results bit for bit.  A DDIM sampler (gaussian_diffusion.py:738-788, ddim_sample) needs no entry of its own:
 * for an x0-predicting model its update is linear in (x0, x_t, noise), so its rows go into the same table {c1, c2, sigma, t/1000}. */
int interdiff_posterior_step_dev_map(float *x, const float *x0, const float *gt, const uint8_t *mask, int64_t n,
                                     const float *table, const int64_t *tmap, int64_t *state, int64_t *ts, int32_t B, void *stream);
int interdiff_sampler_advance_map(int64_t *state, int64_t *ts, const int64_t *tmap, int32_t B, void *stream);
/* Pseudo linear multistep sampling (plms_sample, diffusion/gaussian_diffusion.py:1001-1083), graph-replayable like
 * interdiff_posterior_step_dev_map: every per-step quantity is read from HBM through state[0] (loop-side t) and state[1] (loop index).
 *   ptable f32[steps][4] = {sqrt(1/ab), sqrt(1/ab - 1), sqrt(ab_prev), sqrt(1 - ab_prev)} of the (spaced) process, each rounded once from fp64;
 *   ring   f32[3][n]: the eps of the last three loop indices, slot = loop index % 3;  order 1..4 (the loops pass 2..4);
 *   gt / mask optional in-kernel inpainting of x0 (x0 itself is not written); tmap as above (NULL = identity); state int64[8] as above.
 * With n % 4 == 0, x / x0 / gt / ring / x_mid 16-byte and mask 4-byte aligned, every access is 16 bytes wide; any other n or alignment
 * takes the scalar form of the same arithmetic (same bits per element).  No float atomics.  The update cancels (a x against r eps', sqrt(ab_prev / ab)
 * times their difference), so every element is evaluated in fp64 from its fp32 operands and rounded once per stored value; the arithmetic is
 * pinned (no contraction, explicit fma).
 *
 * interdiff_plms_step_dev   replaces :1044 (_predict_eps_from_xstart) and :1060-1083:  with t = state[0], it = state[1],
 *     eps  = (a x - x0) / r
 *     eps' = Adams-Bashforth over cur_order = min(order, it + 1) values, newest first: eps; (3, -1)/2; (23, -16, 5)/12; (55, -59, 37, -9)/24
 *     x    = sqrt(ab_prev) (a x - r eps') + sqrt(1 - ab_prev) eps'      (t == 0: x = x0)
 *   ring[it % 3] = eps -- the slot of loop index it - 3, the oldest, which each thread reads before it writes.  The last workgroup to
 *   retire advances: state[0] = t - 1, state[1] = it + 1, ts[b] = tmap[max(t - 1, 0)].
 * interdiff_plms_first_half_dev   replaces :1044 and :1053-1054, the first half of the "pseudo improved Euler" start (x is only read):
 *     ring[it % 3] = eps;  x_mid = x0 sqrt(ab_prev) + sqrt(1 - ab_prev) eps;  then state[0] = t - 1, ts[b] = tmap[t - 1]; the loop index stays.
 *   The caller then runs the denoiser (and inpainting, denoised_fn) on (x_mid, ts): they see t - 1 (:1055).
 * interdiff_plms_second_half_dev  replaces :1055-1058 after that second call: with t - 1 = state[0],
 *     eps2 = (a[t-1] x_mid - x0) / r[t-1];  eps' = (ring[it % 3] + eps2) / 2;  x = sqrt(ab_prev[t]) (a[t] x - r[t] eps') + sqrt(1 - ab_prev[t]) eps'
 *   then state[1] = it + 1; state[0] and ts stay at t - 1, the next step's.  The ring keeps eps, not eps' (:1053). */
int interdiff_plms_step_dev(float *x, const float *x0, const float *gt, const uint8_t *mask, float *ring, int64_t n, int32_t order,
                            const float *ptable, const int64_t *tmap, int64_t *state, int64_t *ts, int32_t B, void *stream);
int interdiff_plms_first_half_dev(const float *x, const float *x0, const float *gt, const uint8_t *mask, float *ring, float *x_mid, int64_t n,
                                  const float *ptable, const int64_t *tmap, int64_t *state, int64_t *ts, int32_t B, void *stream);
int interdiff_plms_second_half_dev(float *x, const float *x0, const float *gt, const uint8_t *mask, const float *ring, const float *x_mid,
                                   int64_t n, const float *ptable, int64_t *state, void *stream);
/* One PLAIN reverse step (no denoised_fn hook) = interdiff_mdm_forward + interdiff_posterior_step_dev(ts != NULL) with the x0
 * prediction consumed inside the denoiser's last GEMM: x [B,1,C,T] is the sampler state, updated in place; ts, table, gt, mask as
 * above; state is int64[8] here: [0..3] as above, [4..5] scratch (this step's {t, loop index}, parked by one thread of layer 0's
 * QKV kernel, which also advances [0..1] and ts -- no arrival counter), [6] = element index of x[0] inside the whole sample's x
 * (a multiple of 4; 0 unless the clips of a sample are stepped as several independent chains, each with its own x slice, ts slice,
 * state, memctx and workspace: the noise of element e is then drawn at counter [6] + e, i.e. what the undivided batch would draw),
 * [7] reserved (0).  Same bits as the two-call form (the update arithmetic and
 * the noise counter are shared), and the two forms can alternate on one state.  Any T: with T % 4 == 0 a lane's four frames are one
 * aligned 16-byte access (x, gt 16-byte aligned, mask 4-byte aligned), other clip lengths (the reference's default T = 35) take a
 * per-row form of the same update.  Layer 0 must be a standard layer (IDF_E_INVAL otherwise: use the two-call form); replaces
 * gaussian_diffusion.py:425-461 (p_sample) for steps without a hook. */
int interdiff_mdm_forward_step(const idf_mdm_weights *w, const float *memctx, float *x, int64_t *ts, int32_t B, int32_t T,
                               const float *gt, const uint8_t *mask, const float *table, int64_t *state,
                               void *ws, size_t ws_bytes, void *stream);
/* interdiff_mdm_forward_step with flags that chain consecutive plain steps of ONE chain on ONE workspace (nothing may touch x, ts or the workspace between
 * the two calls): IDF_STEP_EMBED_NEXT -- this call's last launch also computes the NEXT step's embedding from the token rows it has just updated
 * (csrc/tail_h2.h: LN3 -> heads -> update -> embedding by one workgroup per 16 token rows); IDF_STEP_EMBED_READY -- the previous call was made with
 * IDF_STEP_EMBED_NEXT: this call starts at its QKV projection.  Results are bit-identical to unflagged calls.  Honoured only when
 * interdiff_mdm_step_chaining(w) is 1 (split arithmetic selected in tune[IDF_TUNE_FFN_MATH], token width 144, out_w_h2 / in_w_h2 packed); otherwise the
 * flags are ignored and every call runs its own embedding (same results).  Reference seam: one iteration of p_sample_loop_progressive
 * (gaussian_diffusion.py:640-681) -- the reference runs ~350 launches per iteration. */
#define IDF_STEP_EMBED_READY 1
#define IDF_STEP_EMBED_NEXT 2
int interdiff_mdm_forward_step_ex(const idf_mdm_weights *w, const float *memctx, float *x, int64_t *ts, int32_t B, int32_t T,
                                  const float *gt, const uint8_t *mask, const float *table, int64_t *state, void *ws,
                                  size_t ws_bytes, int32_t flags, void *stream);
/* interdiff_mdm_forward_step_ex under a respaced schedule: tmap as for interdiff_posterior_step_dev_map (NULL = identity = the entry above); layer 0's QKV
 * kernel writes ts[b] = tmap[max(t - 1, 0)], which the next step's embedding -- a chained one (IDF_STEP_EMBED_NEXT) included -- looks up unchanged.
 * Replaces respace.py:124-126 around gaussian_diffusion.py:425-461 (p_sample) / :738-788 (ddim_sample). */
int interdiff_mdm_forward_step_map(const idf_mdm_weights *w, const float *memctx, float *x, int64_t *ts, int32_t B, int32_t T,
                                   const float *gt, const uint8_t *mask, const float *table, const int64_t *tmap, int64_t *state,
                                   void *ws, size_t ws_bytes, int32_t flags, void *stream);
int interdiff_mdm_step_chaining(const idf_mdm_weights *w);
/* Every kernel of the library that issues the f16 MFMA claims its CU for itself (all 160 KiB of LDS, the whole register file: DESIGN.md "exclusive CU");
 * since round 5 each launcher VERIFIES that on the device it launches on -- occupancy query == 1, static + dynamic LDS == 160 KiB, >= 256 registers
 * allocated -- and a kernel that does not pass runs as its fp32-MFMA counterpart instead (same results to rounding; the choice is per device and
 * process-stable, so every route of one process computes the same bits).  This entry forces the check for every such kernel on the current device,
 * writes one text line per kernel into buf (<= cap bytes, NUL-terminated) and returns how many do NOT pass (0 on MI355X), or a negative IDF_E_*. */
int interdiff_exclusive_cu_report(char *buf, int32_t cap);
/* DEBUG, tests only (round 6): from now on every f16-MFMA kernel whose name -- as the report above prints it -- contains one of the comma-separated `patterns` is
 * treated as NOT owning its CU, so its launcher takes the fp32 kernel: the fallbacks can be executed on a device where every claim holds.  NULL / "" clears the
 * list.  Process-wide state (the only such switch in the library; empty unless a test sets it); callers drop captured graphs, which bake the kernel choice in. */
int interdiff_debug_deny_exclusive(const char *patterns);

/* ------------------------------------------------------------------------------------
 * Correction predictor   replaces ObjProjector.sample (model/correction_smpl.py:79-138,
 * eval branch) with BatchNorm folded into the 1x1 convolutions at pack time
 * (interdiff_amd/objprojector.py: pack_objprojector).  arena layout: see that file.
 * obj_angles [T,B,6], obj_trans [T,B,3], markers [T,B,P,3] (P = 67), contact int32 [B,P]
 * -> out [T,B,9].
 * ---------------------------------------------------------------------------------- */
typedef struct {
    int32_t T, past_len, P, n_pre;
    const float *arena;
    int64_t dct_pad;           /* [n_pre][past_len]  DCT with the idx_pad frames folded in */
    int64_t dct;               /* [n_pre][T]                                             */
    int64_t idct;              /* [T][n_pre]                                             */
    int64_t hand_bonus;        /* [P] 0.5 on hand markers                                */
    int64_t layer[12];         /* 3 stacks x 4 layers; each: see pack_objprojector       */
    int32_t cin[12], cout[12];
} idf_objproj;

int interdiff_objprojector_sample(const idf_objproj *op, const float *obj_angles,
                                  const float *obj_trans, const float *markers,
                                  const int32_t *contact, int32_t B, float *out, void *stream);
/* The teacher-forced call of the trainer: replaces the tail of ObjProjector.forward (model/correction_smpl.py:69-77; the axis-angle -> 6D conversion
 * and the contact sum stay with the caller) = sample(..., initialize).  initialize == 0 is interdiff_objprojector_sample itself (same kernel, same
 * bits; ws unused, contact required).  initialize != 0 replaces `results.mean(dim=2)` (:122-123), what validation uses while current_epoch < 10: the
 * three stacks, then the mean over the P + 1 nodes taken in coefficient space (it commutes with the IDCT) and one IDCT; contact is not read (may be
 * NULL); ws >= interdiff_objprojector_forward_workspace_bytes(B).  Additive (the ABI version does not move). */
size_t interdiff_objprojector_forward_workspace_bytes(int32_t B);
int interdiff_objprojector_forward(const idf_objproj *op, const float *obj_angles, const float *obj_trans, const float *markers,
                                   const int32_t *contact, int32_t B, int32_t initialize, float *out, void *ws, size_t ws_bytes, void *stream);

/* ---- FINE-TUNING of the correction predictor under the object-pose loss, with FROZEN normalisation statistics (the reference module in eval() with
 * autograd on: BatchNorm uses its running statistics and never writes them, dropout is off, contact clips take the argmax node; the module in train() -- batch statistics,
 * dropout, drawn nodes -- is the TRAINING block below; the gradient of the contact / penetration terms is interdiff_correction_geometry_grads).  Device code: csrc/objproj_train.h, launchers
 * csrc/objproj_train.hip; the layer backward and the fold / Adam / re-fold kernels are shared with the skeleton fine-tuner (csrc/stgcn_train.h).
 * Additive entries: interdiff_abi_version() stays what it was.
 *
 * PARAMETER TABLE.  `params`, `grads`, `exp_avg`, `exp_avg_sq` are flat fp32 vectors of n_param = 224 174 floats in the order of
 * ObjProjector.named_parameters(): the stacks st_gcnns_relative (67 nodes), st_gcnns (1 node), st_gcnns_all (68 nodes), four layers each, and per layer
 *     [gcn.A [10][68][68]  (st_gcnns_all only)]
 *     gcn.T [10][10]  (st_gcnns_all: [68][10][10])
 *     tcn.0.weight [cout][cin], tcn.0.bias [cout], tcn.1.weight [cout], tcn.1.bias [cout],
 *     residual.0.weight [cout][cin], residual.0.bias [cout], residual.1.weight [cout], residual.1.bias [cout], prelu.weight [1].
 * `bn` is the flat vector of the BatchNorm buffers (n_bn floats, read only -- no entry writes it), per layer
 *     tcn.1.running_mean, tcn.1.running_var, residual.1.running_mean, residual.1.running_var, [cout] each.
 * interdiff_correction_finetune_param_table writes table[12][16] in the column layout of interdiff_skeleton_finetune_param_table (below); only op's
 * cin / cout are read.  interdiff_amd/correction_finetune.py builds the same table from the state_dict and its constructor compares the two.
 *
 * interdiff_correction_finetune_grads   replaces loss.backward() on LitInteraction.calc_loss (train_correction_smpl.py:60-101) of ObjProjector.forward
 *      (model/correction_smpl.py:69-138) -- what _common_step (:187-189) trains on while its annealed geometry weights are zero, epoch 0 at the defaults.
 *      op->arena must be the fold of `params` / `bn` (interdiff_correction_finetune_step keeps it so).  obj_angles [T,B,6], obj_trans [T,B,3],
 *      markers [T,B,67,3], contact int32 [B,67] are what interdiff_objprojector_forward takes (contact may be NULL when initialize != 0); they are the
 *      target as well (obj_gt = obj_angles | obj_trans).  d_obj_pred [T,B,9] or NULL: added to the loss gradient at the prediction before the backward
 *      starts -- the gradient of whatever else the caller's objective reads from obj_pred (the seam for the contact / penetration terms).
 *      weights8: HOST pointer, the 8 loss weights in the order rot_past, nonrot_past, rot_future, nonrot_future, rot_v_past, nonrot_v_past, rot_v_future,
 *      nonrot_v_future (rot = the six rotation channels).  -> out9 (device) = loss, the 8 unweighted terms (of the MSE terms alone, whatever d_obj_pred
 *      is); grads (device) [n_param] in the reference layout.  One 1024-thread workgroup per clip (forward with saves, loss gradient, backward, per-clip
 *      partials by plain stores), then the fold over clips in ascending order and the conversion from the folded convolutions: no atomics, two calls
 *      give the same bits.  Clips whose contact rule selects a node leave EXACT zeros in the columns of st_gcnns_all.3.gcn.A of every other node.
 *      IDF_E_INVAL: null pointer, B < 1, T != op->T, T > 64, past_len >= T, short workspace.
 *      PRECISION: the three stacks run in fp32 on the VALU with compensated sums (not the MFMA forward of interdiff_objprojector_sample); everything
 *      around them -- the DCT (its matrix is formed in the kernel in double; the arena's fp32 dct_pad / dct / idct are not read), the skip connections,
 *      the node selection, the IDCT, the prediction error and the loss gradient -- runs in DOUBLE, a departure from fp32-throughout taken to keep every
 *      gradient tensor within 4x the reference's own fp32 error of the fp64 gradient.  The loss therefore agrees with calc_loss on
 *      interdiff_objprojector_forward's prediction to ~1e-6 relative, not in bits.
 * interdiff_correction_finetune_step    replaces optimizer.step() of torch.optim.Adam(lr, betas, eps, weight_decay) (:51-58), torch's order of
 *      operations, weight decay added to the gradient; `step` = 1 for the first step.  Updates params / exp_avg / exp_avg_sq in place and re-folds
 *      params into `arena` (the float arena op->layer[] indexes: MFMA layout, gcn.A transposed and padded to 80 x 80; folded in double without
 *      contraction, like the host packer).
 * ---------------------------------------------------------------------------------- */
int interdiff_correction_finetune_param_table(const idf_objproj *op, int32_t *table, int32_t *n_param, int32_t *n_bn);
size_t interdiff_correction_finetune_workspace_bytes(const idf_objproj *op, int32_t B);
int interdiff_correction_finetune_grads(const idf_objproj *op, const float *params, const float *bn, const float *obj_angles,
                                        const float *obj_trans, const float *markers, const int32_t *contact, const float *d_obj_pred,
                                        int32_t B, int32_t T, int32_t initialize, const float *weights8, float *out9, float *grads, void *ws,
                                        size_t ws_bytes, void *stream);
int interdiff_correction_finetune_step(const idf_objproj *op, float *arena, float *params, const float *bn, const float *grads,
                                       float *exp_avg, float *exp_avg_sq, int32_t step, double lr, double beta1, double beta2, double eps,
                                       double weight_decay, void *stream);

/* ---- TRAINING of the correction predictor the way the reference trains it (train_correction_smpl.py: the module in train()): every BatchNorm2d
 * normalises with the statistics of the BATCH (biased variance, eps 1e-5) and updates its running buffers; nn.Dropout(p) follows the tcn BatchNorm of
 * every ST_GCNN_layer (model/layers.py:308-318); the contact node of a clip is GIVEN (the caller draws it: torch.multinomial, model/correction_smpl.py:
 * 131-132).  Device code: csrc/objproj_bn_train.h around the fine-tuner's csrc/objproj_train.h, the train-mode layer shared with the skeleton trainer
 * (csrc/stgcn_bn_train.h); launchers csrc/objproj_bn_train.hip.  Additive entries: interdiff_abi_version() stays what it was.  Parameter and buffer
 * layouts: the PARAMETER TABLE above.  The gradient of the contact / penetration terms: interdiff_correction_geometry_grads (d_obj_pred is its seam).
 *
 * interdiff_correction_train_grads   replaces loss.backward() on LitInteraction.calc_loss (train_correction_smpl.py:60-101) of ObjProjector.forward
 *      (model/correction_smpl.py:69-138) with the module in train(), and the buffer updates torch.nn.BatchNorm2d.forward makes there.  Arguments as
 *      interdiff_correction_finetune_grads, and:
 *      nodes int32 [B] or NULL  the node clip b reads when initialize = 0 (replaces :125-136, both branches): 0 = the object node (a clip without
 *                 contact), 1 + marker otherwise; values outside 0 .. 67 are clamped.  NULL: the fine-tuner's rule (node 0 without contact, else
 *                 1 + argmax(contact + hand bonus)); contact may be NULL when nodes is given.  Not read when initialize != 0 (the 68-node mean).
 *      bn [n_bn]  running mean / variance, READ AND WRITTEN IN PLACE when update_running = 1: running <- (1 - momentum) running + momentum {mean,
 *                 variance n / (n - 1)}, n = B * 10 * nodes; untouched (and never read) when update_running = 0.
 *      p_drop in [0, 1); masks: device uint8, one byte per element, the 12 layers in named_parameters() order, each [B][cout][10][nodes] (121 040 bytes
 *                 per clip), keep iff nonzero, kept values times fp32(1 / (1 - p_drop)); NULL: the masks interdiff_correction_train_masks(seed, step)
 *                 writes (p_drop = 0: no dropout, nothing is drawn).
 *      batch_stats [n_bn] or NULL: mean and BIASED variance of this batch in the layout of bn.
 *      op->arena must hold the gcn.T / gcn.A / PReLU values of `params` (interdiff_correction_finetune_step keeps it so); the convolutions and the
 *      BatchNorm affine parameters are read from `params`, unfolded.
 *      17 launches of one 1024-thread workgroup per clip, cut wherever a BatchNorm needs the whole batch (no grid barrier inside a kernel), then the
 *      fold over clips and the statistics kernel, all on `stream`.  Statistics and their gradients are merged over the clips in ascending order in
 *      double (Chan's merge of per-clip (sum, M2)); no atomics: two calls give the same bits.  The gradients of the 24 convolution biases, which cancel
 *      inside the batch normalisation, are written as exact 0.  IDF_E_INVAL: null pointer, B < 1, T != op->T, T > 64, past_len >= T, p_drop outside
 *      [0, 1), momentum outside [0, 1], update_running not 0 / 1, short workspace.
 * interdiff_correction_train_masks   replaces the Bernoulli draw of nn.Dropout in train() (model/layers.py:317): the keep masks of training step `step`
 *      in the layout above, Philox4x32-10 keyed by `seed`, counter (element index / 4, layer, step); an element keeps iff its uniform draw in [0, 1)
 *      is >= p_drop.
 * interdiff_correction_train_workspace_bytes   the workspace interdiff_correction_train_grads needs at batch B (0: bad arguments).
 * optimizer.step() and the re-fold: interdiff_correction_finetune_step above, with the bn vector this entry has just updated.
 * ---------------------------------------------------------------------------------- */
size_t interdiff_correction_train_workspace_bytes(const idf_objproj *op, int32_t B);
int interdiff_correction_train_grads(const idf_objproj *op, const float *params, float *bn, const float *obj_angles, const float *obj_trans,
                                     const float *markers, const int32_t *contact, const int32_t *nodes, const float *d_obj_pred, int32_t B,
                                     int32_t T, int32_t initialize, const float *weights8, double p_drop, const uint8_t *masks, uint64_t seed,
                                     uint64_t step, double momentum, int32_t update_running, float *out9, float *grads, float *batch_stats,
                                     void *ws, size_t ws_bytes, void *stream);
int interdiff_correction_train_masks(const idf_objproj *op, int32_t B, double p_drop, uint64_t seed, uint64_t step, uint8_t *masks_out,
                                     void *stream);

/* ---- THE TRAINERS' OWN PREDICTION: obj_pred [T,B,9] as the backward of the two gradient entries above sees it -- what `self(batch, current_epoch < 10)`
 * returns inside _common_step (train_correction_smpl.py:188) before calc_loss_contact (:189) reads it.  The contact / penetration gradient
 * (interdiff_correction_geometry_grads) is taken AT this prediction and handed to the gradient entry as d_obj_pred.  Additive entries.
 *
 * interdiff_correction_finetune_predict   the forward half of interdiff_correction_finetune_grads alone: the same device functions up to the head
 *      (csrc/objproj_train.h ot_clip_predict), on op->arena -- `params` and `bn` are the vectors that arena is the fold of and are not read.  Arguments
 *      as that entry's; ws >= interdiff_correction_finetune_workspace_bytes(op, B).  -> obj_pred_out f32 [T][B][9], the head's double rounded once.
 * interdiff_correction_train_predict      the forward launches of interdiff_correction_train_grads (phases 0 .. 7) and the head of phase 8 alone:
 *      batch statistics, dropout and given nodes as there -- the same masks / (seed, step) and nodes give the prediction that entry differentiates.
 *      It has no `bn` argument: the train-mode forward never reads the running statistics and this entry never updates them.
 *      ws >= interdiff_correction_train_workspace_bytes(op, B).  9 launches of one workgroup per clip.
 * Both: IDF_E_INVAL as their gradient entries.  A training step with the geometry terms therefore runs the forward twice.
 * ---------------------------------------------------------------------------------- */
int interdiff_correction_finetune_predict(const idf_objproj *op, const float *params, const float *bn, const float *obj_angles,
                                          const float *obj_trans, const float *markers, const int32_t *contact, int32_t B, int32_t T,
                                          int32_t initialize, float *obj_pred_out, void *ws, size_t ws_bytes, void *stream);
int interdiff_correction_train_predict(const idf_objproj *op, const float *params, const float *obj_angles, const float *obj_trans,
                                       const float *markers, const int32_t *contact, const int32_t *nodes, int32_t B, int32_t T,
                                       int32_t initialize, double p_drop, const uint8_t *masks, uint64_t seed, uint64_t step, float *obj_pred_out,
                                       void *ws, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------------------------
 * denoised_fn, fused   replaces eval_smpl_short.py:84-130 for one gated step.
 * x0 [B,1,144,T] is updated in place.  hand_pose [T,B,90] (already idx-padded),
 * beta [T,B,10], obj_points [B,P,3], gt [B,1,144,T], markers_idx int32 [67].
 * Optional debug outputs (may be NULL): condition uint8 [B], contact int32 [B,67],
 * distance [B], loss [B].
 * ---------------------------------------------------------------------------------- */
typedef struct {
    const idf_smpl_model *smpl;
    const idf_objproj    *objproj;
    const int32_t *faces;      /* [F][3] */
    const int32_t *adj_ptr, *adj_face, *adj_corner;
    const int32_t *markers_idx;
    int32_t n_markers, n_points, past_len;
    int32_t tune;              /* A/B only, 0 in the product.  Bit 1 (value 2): the hook launches the one-launch predictor after the contact scan; default: the predictor's three
                                  stacks ride in the scan's launch as leading workgroups and a pick kernel follows the labels (csrc/correction.hip correction_impl, csrc/contact_scan.h launch_contact<false, true>; same bits) */
    /* Scan order of the exact nearest-vertex scans (all four or none; NULL = identity order: same results, no culling benefit).
     * vorder [V]: scan position -> vertex, a permutation that keeps blocks of 16 consecutive positions spatially compact under any
     * pose (the host uses the Morton order of the rest pose, interdiff_amd/correction.py scan_order); faces_scan [F][3] and
     * markers_scan [n_markers] are `faces` / `markers_idx` mapped to scan positions; adj_pair_scan [nnz][2]: for entry e of the
     * adjacency (adj_ptr / adj_face / adj_corner order) the scan positions (a, b) of the incident face's other two vertices such
     * that the face normal at the vertex is (a - v) x (b - v).  Results (indices included) never depend on the order. */
    const int32_t *vorder, *faces_scan, *markers_scan, *adj_pair_scan;
    const int32_t *adj_pair;   /* nullable [nnz][2]: adj_pair_scan's pairs as ORIGINAL vertex ids (kernels that read vertices from HBM) */
    const int32_t *vrank;      /* nullable [V]: vertex -> scan position, the inverse of vorder (round 6): the contact scan then reads a frame's vertices in their own order (coalesced) and scatters them into LDS; NULL = gather through vorder, same results */
} idf_correction_ctx;

size_t interdiff_correction_workspace_bytes(const idf_correction_ctx *c, int32_t B, int32_t T);
int interdiff_correction(const idf_correction_ctx *c, float *x0, const float *gt,
                         const float *hand_pose, const float *beta, const float *obj_points,
                         int32_t B, int32_t T, float blend_t /* t/1000 */,
                         uint8_t *condition, int32_t *contact, float *distance, float *loss,
                         void *ws, size_t ws_bytes, void *stream);
/* The same hook with its one per-call scalar read on the DEVICE: blend weight = table[state[0]][3] (the sampler's coefficient table
 * {c1, c2, sigma, t/1000} and state {t, ...} of interdiff_posterior_step_dev), no debug outputs.  Every launch parameter is then
 * independent of the timestep, so ONE captured hipGraph of a whole hook step -- denoiser forward, inpaint, this, posterior update --
 * serves all eleven corrected steps of a sample (t <= 500, t % 50 == 0: host-known, eval_smpl_short.py:85). */
int interdiff_correction_dev(const idf_correction_ctx *c, float *x0, const float *gt, const float *hand_pose,
                             const float *beta, const float *obj_points, int32_t B, int32_t T, const float *table,
                             const int64_t *state, void *ws, size_t ws_bytes, void *stream);

/* The nearest-vertex scan of the hook / the metrics on its own (tools.point2point_signed's object->human half, tools.py:45-76, fused
 * with the object transform eval_smpl_short.py:107): verts [T*B][V][3] (frame n = t*B + b), obj_points [B][P][3] canonical, objR [T*B][9]
 * row-major, objT [T*B][3] -> o2h [T*B][P] signed distance (nullable), idx int32 [T*B][P] nearest vertex, lowest index on ties
 * (nullable), stats uint64[IDF_CONTACT_STATS] (nullable) = {16-vertex blocks scored, blocks there are, box tests made} summed over
 * waves, the number of workgroups, and thread 0's clock cycles per phase summed over workgroups {records -> LDS, boxes + markers,
 * its wave's tasks, waiting for the other waves, reductions}. */
#define IDF_CONTACT_STATS 12
size_t interdiff_contact_nn_workspace_bytes(const idf_correction_ctx *c, int32_t B, int32_t T);
int interdiff_contact_nn(const idf_correction_ctx *c, const float *verts, const float *obj_points, const float *objR,
                         const float *objT, int32_t B, int32_t T, float *o2h, int32_t *idx, uint64_t *stats,
                         void *ws, size_t ws_bytes, void *stream);

/* Evaluation metrics (eval_smpl_short.py:24-81) over the T frames handed in (the caller slices the future frames,
 * :279); frame-major inputs: obj_pred/obj_gt [T,B,6] (axis-angle | translation), jtr/jtr_gt [T,B,J,3],
 * body_trans(_gt) [T,B,3], verts [T,B,V,3], obj_points [B,P,3] (canonical).  out6 [6][B] rows: global_mpjpe,
 * local_mpjpe, body_translation, obj_translation, obj_rot_error, penetrate. */
size_t interdiff_metrics_workspace_bytes(const idf_correction_ctx *c, int32_t B, int32_t T);
int interdiff_metrics(const idf_correction_ctx *c, const float *obj_pred, const float *jtr,
                      const float *body_trans, const float *obj_gt, const float *jtr_gt,
                      const float *body_trans_gt, const float *verts, const float *obj_points,
                      int32_t B, int32_t T, int32_t J, float *out6 /* [6][B] */,
                      void *ws, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------------------------
 * HO-GCN skeleton mode (eval_skeleton.py; tokens C = 106 = body 21x3 | object keypoints 12x3 |
 * pose [trans 3, quaternion xyzw 4]).  Device code: csrc/skeleton.h, launchers csrc/skeleton.hip.
 * Predictor ObjProjector of model/correction_skeleton.py:7-137 with BatchNorm folded into the 1x1
 * convolutions at pack time (interdiff_amd/skeleton.py: pack_skeleton_objprojector; arena layout
 * there).  Built for n_pre = T = past_len + future_len = 20, 21 joints, channel widths
 * cin, cout <= 64 (IDF_E_INVAL otherwise).
 * ---------------------------------------------------------------------------------- */
typedef struct {
    int32_t T, past_len, J, n_pre;   /* 20, 10, 21, 20                                    */
    const float *arena;
    int64_t dct_pad;           /* [n_pre][past_len]  DCT with the idx_pad frames folded in */
    int64_t dct;               /* [n_pre][T]                                             */
    int64_t idct;              /* [T][n_pre]                                             */
    int64_t layer[12];         /* 3 stacks x 4 layers; each: see pack_skeleton_objprojector */
    int32_t cin[12], cout[12];
} idf_skel_objproj;

/* replaces ObjProjector.sample (model/correction_skeleton.py:84-137): obj_angles [T,B,4] quaternion
 * xyzw, obj_trans [T,B,3], human_points [T,B,J,3] -> quat_out [T,B,4] xyzw, trans_out [T,B,3]. */
int interdiff_skeleton_objprojector_sample(const idf_skel_objproj *op, const float *obj_angles,
                                           const float *obj_trans, const float *human_points, int32_t B,
                                           float *quat_out, float *trans_out, void *stream);
/* replaces eval_skeleton.denoised_fn (eval_skeleton.py:82-111) for one gated step: x [B,1,106,T] (read
 * only), gt = inpainted_motion [B,1,106,T] (only its past pose rows are read), zero_pose_obj [B,12,3]
 * -> out [B,1,106,T] = blend_t * x + (1 - blend_t) * [body, calc_obj_pred(pose'), pose'] with
 * blend_t = t / 1000.  One launch, one workgroup per clip.  The gate (t <= 500, t % 50 == 0) is the
 * caller's. */
int interdiff_skeleton_correction(const idf_skel_objproj *op, const float *x, const float *gt,
                                  const float *zero_pose_obj, int32_t B, int32_t T, float blend_t,
                                  float *out, void *stream);
/* replaces calc_metric_single (eval_skeleton.py:46-68) over frames [from_frame, T): body [T,B,21*3],
 * obj [T,B,12*3], pose [T,B,7] (pred and gt each) -> out4 = {mpjpe_h, mpjpe_o, translation_error,
 * rotation_error}.  One workgroup, fixed reduction order: repeated calls give the same bits. */
int interdiff_skeleton_metrics(const float *body_pred, const float *body_gt, const float *obj_pred,
                               const float *obj_gt, const float *pose_pred, const float *pose_gt,
                               int32_t T, int32_t B, int32_t from_frame, float *out4, void *stream);

/* ---- FINE-TUNING of the skeleton predictor with FROZEN normalisation statistics (the reference module in eval() with autograd on: BatchNorm
 * uses its running statistics and never writes them, dropout is off; train-mode BatchNorm and dropout are NOT built).  Device code:
 * csrc/skeleton_train.h, launchers csrc/skeleton_train.hip.  Additive entries: interdiff_abi_version() stays what it was.
 *
 * PARAMETER TABLE.  `params`, `grads`, `exp_avg`, `exp_avg_sq` are flat fp32 vectors of n_param = 96 110 floats in the order of
 * ObjProjector.named_parameters(): the stacks st_gcnns_relative, st_gcnns, st_gcnns_all, four layers each, and per layer
 *     [gcn.A [20][nodes][nodes]  (st_gcnns_all only, nodes = 22)]
 *     gcn.T [20][20]  (st_gcnns_all: [nodes][20][20])
 *     tcn.0.weight [cout][cin], tcn.0.bias [cout], tcn.1.weight [cout], tcn.1.bias [cout],
 *     residual.0.weight [cout][cin], residual.0.bias [cout], residual.1.weight [cout], residual.1.bias [cout], prelu.weight [1].
 * `bn` is the flat vector of the BatchNorm buffers (n_bn floats, read only -- no entry writes it), per layer
 *     tcn.1.running_mean, tcn.1.running_var, residual.1.running_mean, residual.1.running_var, [cout] each.
 * interdiff_skeleton_finetune_param_table writes table[12][16] = per layer the offsets {A (-1 when absent), T, tcn.0.weight, tcn.0.bias,
 * tcn.1.weight, tcn.1.bias, residual.0.weight, residual.0.bias, residual.1.weight, residual.1.bias, prelu.weight}, then {cin, cout, nodes,
 * joint-stack flag, offset in bn}; only op's cin / cout are read.  interdiff_amd/skeleton_finetune.py builds the same table from the
 * state_dict and the tests compare the two.
 *
 * interdiff_skeleton_finetune_grads   replaces loss.backward() on LitObjInteraction._common_step (train_correction_skeleton.py:128-154:
 *      ObjProjector.forward, model/correction_skeleton.py:68-137, then calc_loss :85-126).  op->arena must be the fold of `params` / `bn`
 *      (interdiff_skeleton_finetune_step keeps it so).  obj_angles [T,B,4], obj_trans [T,B,3], human_points [T,B,21,3] are what
 *      interdiff_skeleton_objprojector_sample takes (ObjProjector.forward's first quaternion conversion is the caller's, as in
 *      SkeletonObjProjector.forward); pose_gt [T,B,7] = translation | quaternion xyzw.  weights8: HOST pointer, the 8 loss weights in the order
 *      rot_past, nonrot_past, rot_future, nonrot_future, rot_v_past, nonrot_v_past, rot_v_future, nonrot_v_future.  -> out9 (device) = loss, the
 *      8 unweighted terms; grads (device) [n_param] in the reference layout.  One 1024-thread workgroup per clip (forward with saves, loss
 *      gradient, backward, per-clip partials by plain stores), then the fold over clips in ascending order and the conversion from the folded
 *      convolutions: no atomics, two calls give the same bits.  IDF_E_INVAL: null pointer, B < 1, T != op->T, short workspace.
 *      PRECISION: the layers run in fp32 on the VALU with compensated sums (not the MFMA forward of interdiff_skeleton_objprojector_sample); the head
 *      of 20 threads per clip (pose from the network output, pose error, loss gradient, backward of matrix_to_quaternion and rotation_6d_to_matrix)
 *      and the input quaternion -> 6D conversion run in DOUBLE, rounded once -- a departure from fp32-throughout taken to keep every gradient tensor
 *      within 4x the reference's own fp32 error of the fp64 gradient.  The loss therefore agrees with the inference kernels' to ~1e-7 relative, not in bits.
 * interdiff_skeleton_finetune_step    replaces optimizer.step() of torch.optim.Adam(lr, betas, eps, weight_decay) (:41-47), torch's order of
 *      operations, weight decay added to the gradient; `step` = 1 for the first step.  Updates params / exp_avg / exp_avg_sq in place and re-folds
 *      params into `arena` (the float arena op->layer[] indexes; folded in double without contraction, like the host packer).
 * ---------------------------------------------------------------------------------- */
int interdiff_skeleton_finetune_param_table(const idf_skel_objproj *op, int32_t *table, int32_t *n_param, int32_t *n_bn);
size_t interdiff_skeleton_finetune_workspace_bytes(const idf_skel_objproj *op, int32_t B);
int interdiff_skeleton_finetune_grads(const idf_skel_objproj *op, const float *params, const float *bn, const float *obj_angles,
                                      const float *obj_trans, const float *human_points, const float *pose_gt, int32_t B, int32_t T,
                                      const float *weights8, float *out9, float *grads, void *ws, size_t ws_bytes, void *stream);
int interdiff_skeleton_finetune_step(const idf_skel_objproj *op, float *arena, float *params, const float *bn, const float *grads,
                                     float *exp_avg, float *exp_avg_sq, int32_t step, double lr, double beta1, double beta2, double eps,
                                     double weight_decay, void *stream);

/* ---- TRAINING of the skeleton predictor the way the reference trains it (train_correction_skeleton.py: the module in train()): every BatchNorm2d
 * normalises with the statistics of the BATCH (biased variance, eps 1e-5) and updates its running buffers; nn.Dropout(p) follows the tcn BatchNorm
 * of every ST_GCNN_layer (model/layers.py:308-318).  Device code: csrc/skeleton_bn_train.h around the fine-tuner's csrc/skeleton_train.h, the train-mode
 * layer in csrc/stgcn_bn_train.h; launchers csrc/skeleton_train.hip.  Additive entries: interdiff_abi_version() stays what it was.  Parameter and buffer layouts: the PARAMETER TABLE above.
 *
 * interdiff_skeleton_train_grads   replaces loss.backward() on LitObjInteraction._common_step (train_correction_skeleton.py:128-154) with the module
 *      in train(), and the buffer updates torch.nn.BatchNorm2d.forward makes there.  Arguments as interdiff_skeleton_finetune_grads, and:
 *      bn [n_bn]  running mean / variance, READ AND WRITTEN IN PLACE when update_running = 1: running <- (1 - momentum) running + momentum {mean,
 *                 variance n / (n - 1)}; untouched (and never read) when update_running = 0.
 *      p_drop in [0, 1); masks: device uint8, one byte per element, the 12 layers in named_parameters() order, each [B][cout][20][nodes], keep iff
 *                 nonzero, kept values times fp32(1 / (1 - p_drop)); NULL: the masks interdiff_skeleton_train_masks(seed, step) writes (p_drop = 0:
 *                 no dropout, nothing is drawn).
 *      batch_stats [n_bn] or NULL: mean and BIASED variance of this batch in the layout of bn.
 *      op->arena must hold the gcn.T / gcn.A / PReLU values of `params` (interdiff_skeleton_finetune_step keeps it so); the convolutions and the
 *      BatchNorm affine parameters are read from `params`, unfolded.
 *      17 launches of one 1024-thread workgroup per clip, cut wherever a BatchNorm needs the whole batch (no grid barrier inside a kernel), then the
 *      fold over clips and the statistics kernel, all on `stream`.  Statistics and their gradients are merged over the clips in ascending order in
 *      double (Chan's merge of per-clip (sum, M2)); no atomics: two calls give the same bits.  The gradients of the 24 convolution biases, which cancel
 *      inside the batch normalisation, are written as exact 0.  IDF_E_INVAL: null pointer, B < 1, T != op->T, p_drop outside [0, 1), momentum outside
 *      [0, 1], update_running not 0 / 1, short workspace.
 * interdiff_skeleton_train_masks   replaces the Bernoulli draw of nn.Dropout in train(): the keep masks of training step `step` in the layout above,
 *      Philox4x32-10 keyed by `seed`, counter (element index / 4, layer, step); an element keeps iff its uniform draw in [0, 1) is >= p_drop.
 * interdiff_skeleton_train_workspace_bytes   the workspace interdiff_skeleton_train_grads needs at batch B (0: bad arguments).
 * ---------------------------------------------------------------------------------- */
size_t interdiff_skeleton_train_workspace_bytes(const idf_skel_objproj *op, int32_t B);
int interdiff_skeleton_train_grads(const idf_skel_objproj *op, const float *params, float *bn, const float *obj_angles, const float *obj_trans,
                                   const float *human_points, const float *pose_gt, int32_t B, int32_t T, const float *weights8, double p_drop,
                                   const uint8_t *masks, uint64_t seed, uint64_t step, double momentum, int32_t update_running, float *out9,
                                   float *grads, float *batch_stats, void *ws, size_t ws_bytes, void *stream);
int interdiff_skeleton_train_masks(const idf_skel_objproj *op, int32_t B, double p_drop, uint64_t seed, uint64_t step, uint8_t *masks_out,
                                   void *stream);

/* ---- the skeleton DENOISER (model/diffusion_skeleton.py MDM): the decoder / encoder of idf_mdm_weights with token width
 * C = n_body + 3 n_points + 7 = 106 (W_in = [bodyEmbedding | objEmbedding | 7 zero columns], feed-forward width <= 1024 zero-padded
 * into the 1024-wide streams) and a KEYPOINT HEAD instead of two plain linears: bodyFinalLinear gives the n_body body channels,
 * objFinalLinear 7 pose values (translation xyz | quaternion xyzw), and the 3 n_points object-keypoint channels of x0 are
 * calc_obj_pred(pose, zero_pose_obj) = R(q) z_k + translation with pytorch3d's un-normalised quaternion_to_matrix
 * (two_s = 2 / (q . q)), formed in the epilogue of the heads GEMM (csrc/skel_head.h).  All offsets in floats into w->arena. */
typedef struct idf_skel_head {
    int32_t n_body, n_points;      /* 63, 12 (3 n_points a multiple of 4, at most 48) */
    int32_t n_tiles, reserved;     /* 32-row column tiles of the packed head: ceil(n_body / 25); reserved = 0 */
    int64_t out_w, out_b;          /* [32 n_tiles][256], [32 n_tiles]: per tile the 7 objFinalLinear rows, then 25 bodyFinalLinear rows (zero past n_body) */
    int64_t shape_w, shape_b;      /* shapeEmbedding [256][3 n_points], [256] (0, 0: no encoder side) */
} idf_skel_head;
/* replaces MDM.forward (diffusion_skeleton.py:250-257): interdiff_mdm_forward for the skeleton model; zero_pose_obj [B,n_points,3]
 * (16-byte aligned), x / x0 [B,1,C,T].  w->C must be n_body + 3 n_points + 7.  Exact-fp32 heads GEMM (the split-f16 step tail serves
 * C = 144 only). */
int interdiff_skeleton_mdm_forward(const idf_mdm_weights *w, const idf_skel_head *head, const float *memctx, const float *x,
                                   const int64_t *ts, const float *zero_pose_obj, int32_t B, int32_t T, float *x0,
                                   void *ws, size_t ws_bytes, void *stream);
/* interdiff_mdm_forward_step for the skeleton model: one plain reverse step, the update over all C channels -- the derived keypoint
 * channels included -- inside the heads GEMM's epilogue.  Same bits as interdiff_skeleton_mdm_forward followed by
 * interdiff_posterior_step_dev(ts != NULL); replaces gaussian_diffusion.py:425-461 (p_sample) around diffusion_skeleton.py:250-257. */
int interdiff_skeleton_mdm_forward_step(const idf_mdm_weights *w, const idf_skel_head *head, const float *memctx, float *x,
                                        int64_t *ts, const float *zero_pose_obj, int32_t B, int32_t T, const float *gt,
                                        const uint8_t *mask, const float *table, int64_t *state, void *ws, size_t ws_bytes,
                                        void *stream);
/* ... under a respaced schedule (tmap as for interdiff_posterior_step_dev_map; NULL = the entry above); replaces respace.py:124-126 around it */
int interdiff_skeleton_mdm_forward_step_map(const idf_mdm_weights *w, const idf_skel_head *head, const float *memctx, float *x,
                                            int64_t *ts, const float *zero_pose_obj, int32_t B, int32_t T, const float *gt,
                                            const uint8_t *mask, const float *table, const int64_t *tmap, int64_t *state, void *ws,
                                            size_t ws_bytes, void *stream);
/* replaces MDM._get_embeddings (diffusion_skeleton.py:194-215): the per-clip additive feature of interdiff_mdm_encode is
 * shapeEmbedding(zero_pose_obj.view(B, 3 n_points)) (one fp32-MFMA GEMM into the workspace), x_past [B,1,C,Tp] holds the past
 * frames (the pose channels meet zero columns of W_in) -> cond [Tp,B,256]. */
size_t interdiff_skeleton_mdm_encode_workspace_bytes(int32_t B, int32_t Tp);
int interdiff_skeleton_mdm_encode(const idf_mdm_weights *w, const idf_skel_head *head, const float *zero_pose_obj,
                                  const float *x_past, int32_t B, int32_t Tp, float *cond, void *ws, size_t ws_bytes,
                                  void *stream);

/* ------------------------------------------------------------------------------------
 * Physics post-optimisation ("next" row N4)   replaces optimization.py:19-173 (optimize):
 * Adam (lr 1e-3) over the rotation MATRICES of the 52 SMPL-H joints and of the object plus the two
 * translations of every frame, loss = penetration + regularisers + temporal smoothness + static-foot
 * term (calc_loss, :54-121), hand-written backward (no autograd).  B clips of T frames are optimised
 * side by side (frame n = b*T + t); the reference does one clip per call.
 *
 * Parameter row of a frame, IDF_OPT_NP floats: R[52][9] (global, 21 body, 30 hand joints; row-major
 * matrices) | body translation [3] | object translation [3] | object rotation [9].
 * Every pointer of idf_opt_state is DEVICE memory owned by the caller (interdiff_amd/optimize.py
 * allocates them as torch tensors): nothing is allocated inside the library.
 * ---------------------------------------------------------------------------------- */
#define IDF_OPT_NP 483
#define IDF_OPT_NLOSS 6      /* per-frame partials: collision, verts_reg, feet, reg (L1), reg_v (smoothness), unused */
typedef struct {
    const idf_correction_ctx *geo;   /* smpl model, faces, vertex->face adjacency (objproj / markers unused) */
    const float   *blendT;           /* [KB][K3P] : transpose of smpl->blend, K3P = 3V rounded up to 1024, zero padded */
    const int32_t *jv_ptr;           /* [J+1]  skinning weights by joint (CSR): entries of joint j are [jv_ptr[j], jv_ptr[j+1]) */
    const int32_t *jv_vtx;           /* [nnz]  vertex of the entry */
    const float   *jv_w;             /* [nnz]  weight of the entry */
    int32_t K3P, _pad;
} idf_opt_ctx;

typedef struct {
    int32_t B, T, P, max_iters;
    /* inputs */
    const float *betas;              /* [N][10] */
    const float *obj_points;         /* [B][P][3] canonical object points */
    /* optimiser state, [N][IDF_OPT_NP] each */
    float *param, *init, *grad, *m, *v, *best;
    /* per-iteration scratch */
    float *pose, *tr;                /* [N][156] axis-angle of param, [N][3] */
    float *verts, *vposed, *verts_gt, *gv;               /* [N][V][3] */
    float *jtr;                      /* [N][J][3] */
    float *pts, *y2x;                /* [N][P][3] */
    float *y2x_signed;               /* [N][P] signed distance of every object point to its nearest vertex */
    int32_t *yidx;                   /* [N][P] that vertex */
    int32_t *near;                   /* [N][V] 1 = some object point within 0.5 m (optimization.py:74-75) */
    float *dvposed;                  /* [N][K3P]  (columns >= 3V stay zero) */
    float *dA;                       /* [N][J][12] */
    float *dfeat;                    /* [K3P/1024][N][KB] split-K partials */
    float *gtr;                      /* [N][3] */
    float *lossf;                    /* [N][IDF_OPT_NLOSS] */
    float *loss;                     /* [B][4] total, collision, reg, reg_v of the last iteration (optimization.py:113-119) */
    float *loss_hist;                /* [max_iters][B][4] */
    float *best_loss;                /* [B] */
    int32_t *flag;                   /* [B] 1 = this iteration is the clip's best so far (after iteration 150, :147) */
    uint8_t *foot_static;            /* [N][2] frame t vs t+1, left / right foot (:47-52) */
    int32_t *foot_cnt;               /* [B][2] */
    int32_t *ctl;                    /* [4]: iteration number ii, Adam steps done, -, - (device side so that steps can be graph-captured) */
    void *smpl_ws; size_t smpl_ws_bytes;     /* interdiff_smpl_workspace_bytes(smpl, N) */
    /* scratch of the culled nearest-neighbour kernels (used when geo->vorder is set and all three are given; NULL = brute force):
     * porder int32 [B][P] (Morton order of every clip's object points), psort float [N][2048][4] (a frame's points in that order),
     * pbox float [N][32][2][4] (boxes of their 64-point patches) */
    int32_t *porder; float *psort, *pbox;
} idf_opt_state;

/* pose [N][156] axis-angle, trans / obj_angles / obj_trans [N][3] (optimization.py:20-32) -> param = init, zeroed moments,
 * verts_gt, static-foot flags; ctl = {first_iter, 0}. */
int interdiff_optimize_init(const idf_opt_ctx *c, const idf_opt_state *st, const float *pose, const float *trans,
                            const float *obj_angles, const float *obj_trans, int32_t first_iter, void *stream);
/* loss + gradient at the current param (grad, loss, lossf are left for inspection); no update. */
int interdiff_optimize_loss_grad(const idf_opt_ctx *c, const idf_opt_state *st, void *stream);
/* one iteration of the loop at optimization.py:139-165: loss_grad, Adam step, best-iterate bookkeeping, ctl advance. */
int interdiff_optimize_step(const idf_opt_ctx *c, const idf_opt_state *st, void *stream);
/* best iterate -> pose [N][156], trans, obj_angles, obj_trans [N][3] (optimization.py:150-172). */
int interdiff_optimize_finish(const idf_opt_ctx *c, const idf_opt_state *st, float *pose, float *trans, float *obj_angles,
                              float *obj_trans, void *stream);
/* HOST-side instance of the device inline that back-propagates through matrix_to_axis_angle + the SMPL Rodrigues for
 * n joints (R [n][9], g_out [n][9] -> g_in [n][9]); lets the CPU test suite check the derivative code without a GPU. */
int interdiff_debug_joint_map_vjp(const float *R, const float *g_out, float *g_in, int32_t n);
/* Diagnostic: n_wg one-wave workgroups each fill 6 KiB of LDS with a pattern and re-read it `spin` times; out[0] counts foreign writes seen,
 * out[4 + 4 k ..] = {workgroup, word, value found, pass} of the first 1000 (tools/lds_sentinel_probe.py; not used by the product path). */
int interdiff_debug_lds_sentinel(uint32_t *out, int32_t n_wg, int32_t spin, void *stream);
/* Diagnostic: the "aggressor" of the co-residency probes (DESIGN.md "exclusive CU"; tools/hook_stage_probe.py, tools/coresidency_repro.hip): `grid` workgroups of 256
 * threads that loop `iters` times over four v_mfma_f32_16x16x32_f16 on register operands and, with_loads != 0, one streaming 16-byte load per lane from
 * src[n_floats] (>= 4096 floats).  Small LDS / register needs on purpose, so that it shares CUs with kernels on other streams.  Never launched by the product path. */
int interdiff_debug_f16_aggressor(const float *src, size_t n_floats, float *sink, int32_t iters, int32_t grid, int32_t with_loads, void *stream);

/* ------------------------------------------------------------------------------------
 * Checkpoint scoring (csrc/losses.hip): the forward, scoring side of interdiff/train_diffusion_smpl.py.  Forward only.
 * Additive entries: no existing signature or struct layout changes, so interdiff_abi_version() stays what it was.
 * Term order everywhere (the reference's dict order): index = 4 * kind + group,
 *   kind  0 past, 1 v_past, 2 future, 3 v_future;   group 0 body_rot, 1 body_nonrot, 2 obj_rot, 3 obj_nonrot.
 *
 *  interdiff_q_sample           replaces GaussianDiffusion.q_sample (diffusion/gaussian_diffusion.py:233-250) with a per-clip timestep,
 *      and the inpainting of x_t in training_losses (:1264-1268).  x_t, x0, noise, gt [B][per_clip], mask uint8 [B][per_clip], ts int64 [B]
 *      (clamped into [0, n_steps)), sqrt_ac / sqrt_1mac f32 [n_steps]: the fp64 tables sqrt(alphas_cumprod), sqrt(1 - alphas_cumprod) cast to
 *      fp32, as `_extract_into_tensor(...).float()` gives them.  x_t = sqrt_ac[t_b] * x0 + sqrt_1mac[t_b] * eps, both products rounded on
 *      their own; then x_t = gt where mask (gt, mask NULL: no inpainting).  eps = noise when given; noise NULL: the library's Philox
 *      generator (csrc/philox.h) at counter elem0 + e under the step index 0xFFFFFFFE, reserved for this entry (the sampler draws at its
 *      loop indices 0 .. steps - 1 and x_T at 0xFFFFFFFF).  elem0 (a multiple of 4) as in interdiff_randn_at: a shard of a batch draws
 *      the whole batch's noise.  x_t 16-byte aligned.
 *  interdiff_denoising_losses   replaces the 16 per-clip terms of LitInteraction.forward_backward (train_diffusion_smpl.py:72-134, l2 :54-58)
 *      on pred / target [B,1,144,T] in rot6d space, as the reference computes them, quirks included: the ground-truth velocity operand of the
 *      first summand of every _v_ term is x_gt[a:b] - x_gt[a:b] (zero), the second summand is a second difference of the prediction alone.
 *      out f32 [16][B].  One launch, one workgroup per clip, sums in a fixed order (no float atomics).  past_len >= 2, T >= past_len + 2.
 *  interdiff_sample_losses      replaces the scoring of validation_step (variant IDF_LOSS_VAL, K = 1: _common_step :396-409 + calc_val_loss
 *      :185-260) and of test_step (IDF_LOSS_TEST: :422-443 + calc_loss :262-379): rot6d -> matrix -> axis-angle per joint (the device
 *      functions interdiff_rotation_6d_to_axis_angle uses), the 30 hand joints spliced in (prediction hand_pose[idx_pad[t]], ground truth
 *      hand_pose[t]; hand_pose [T][B][90], NOT padded), axis-angle -> 3x3 (rotvec_to_rotmat, tools.py:88-90 -- human_body_prior's aa2matrot
 *      is outside the reference tree: RESTATED, parity unpinned -- restatement defines the contract; csrc/rot_math.h), value / velocity
 *      differences and reductions.  samples [K][B,1,144,T], gt [B,1,144,T].  out_terms f32 [32]: the 16 terms over all K samples, then
 *      (TEST) the 16 best-of-K `_min` terms -- per clip the minimum over the samples, then the mean over clips -- (VAL: zeros).
 *      out_per_clip f32 [K][16][B] (nullable: then `ws` holds it, interdiff_sample_losses_workspace_bytes(K, B) bytes): every clip's own
 *      mean of every term.  The future-velocity frames differ between the variants exactly as upstream (VAL past_len .., TEST past_len + 1 ..).
 *      Two launches whatever K is: one workgroup per (clip, sample), then one small workgroup for the means and minima; fixed order.
 *      past_len >= 1, T >= past_len + 2.
 * ---------------------------------------------------------------------------------- */
enum { IDF_LOSS_VAL = 0, IDF_LOSS_TEST = 1 };
int interdiff_q_sample(float *x_t, const float *x0, const float *noise, const int64_t *ts, const float *sqrt_ac, const float *sqrt_1mac,
                       int32_t n_steps, const float *gt, const uint8_t *mask, int32_t B, int64_t per_clip, uint64_t seed, uint64_t elem0,
                       void *stream);
int interdiff_denoising_losses(const float *pred, const float *target, int32_t B, int32_t T, int32_t past_len, float *out, void *stream);
size_t interdiff_sample_losses_workspace_bytes(int32_t K, int32_t B);
int interdiff_sample_losses(const float *samples, const float *gt, const float *hand_pose, int32_t K, int32_t B, int32_t T, int32_t past_len,
                            int32_t variant, float *out_terms, float *out_per_clip, void *ws, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------------------------
 * TRAINING of the SMPL denoiser's decoder (csrc/mdm_train.h, launchers csrc/mdm_train.hip): the backward of MDM.forward(x, timesteps, y)
 * (model/diffusion_smpl.py:226-246) under the loss of LitInteraction.forward_backward (train_diffusion_smpl.py:60-166), and AdamW (:177-183).
 * Additive entries: interdiff_abi_version() stays what it was.  dropout 0, cond_mask_prob 0, stochastic depth at rate 0 (the reference's defaults):
 * train() and eval() compute the same function.  Exact fp32 throughout (v_mfma_f32_16x16x4_f32 and VALU, no f16 MFMA), no float atomics: two
 * calls give the same bits.
 *
 * PARAMETER TABLE.  `params`, `grads`, `exp_avg`, `exp_avg_sq` are flat fp32 vectors of n_param = 7 069 900 floats, the 144 tensors MDM.forward
 * reads, packed without padding in this order (state_dict names, shapes as the reference's):
 *     bodyEmbedding.{weight,bias}, objEmbedding.{weight,bias}, embedTimeStep.time_embed.0.{weight,bias}, embedTimeStep.time_embed.2.{weight,bias},
 *     per decoder layer 0..7:  layers 0, 7: self_attn.in_proj_weight, self_attn.in_proj_bias, self_attn.out_proj.weight, self_attn.out_proj.bias;
 *                              layers 1..6: queries, wk;
 *                              then multihead_attn.in_proj_weight, .in_proj_bias, .out_proj.weight, .out_proj.bias, linear1.{weight,bias},
 *                              linear2.{weight,bias}, norm1.{weight,bias}, norm2.{weight,bias}, norm3.{weight,bias},
 *     bodyFinalLinear.{weight,bias}, objFinalLinear.{weight,bias}.
 * bodyEmbedding / objEmbedding are shared with the encoder; their gradient here is the decoder path's alone (cond is an input of this pass).
 * This table, the FULL, SKELETON and PointNet++ tables below are each built once on the host (csrc/mdm_train.hip make_layout / make_enc_layout,
 * csrc/pointnet2_train.hip) and read once in Python, by interdiff_amd/flat_trainer.py param_table(entry, n), against the names in
 * interdiff_amd/mdm_train.py (PARAM_NAMES, ENCODER_PARAM_NAMES), skeleton_mdm_train.py (PARAM_NAMES) and pointnet2_train.py (POINTNET_PARAM_NAMES).
 *
 *  interdiff_denoising_loss_grad     replaces autograd through the 16 terms of forward_backward (:72-134): d_pred [B,1,144,T] = d/d pred of
 *      mean_b sum_i weights16[i] * term_i[b], the terms of interdiff_denoising_losses (velocity terms as the reference writes them: the
 *      ground-truth operand is zero).  weights16: HOST pointer, term order of interdiff_denoising_losses.  One launch, one thread per element.
 *  interdiff_mdm_train_param_table   offsets / sizes (HOST int64 [144], nullable) of the tensors in the flat vectors, their count and n_param.
 *  interdiff_mdm_train_workspace_bytes   workspace of interdiff_mdm_train_grads; 0 for an unsupported shape (T > 128, mem_len > 16).
 *  interdiff_mdm_train_grads         replaces MDM.forward + loss.backward() of forward_backward for the 144 tensors.  x_t [B,1,144,T] (what
 *      interdiff_q_sample made), ts int64 [B], cond [mem_len][B][256], target [B,1,144,T] (x_start), pe [pe_rows][256] the sinusoidal table
 *      (PositionalEmbedding.pe; pe_rows > every timestep and >= T).  -> pred [B,1,144,T] (the model output), terms [16][B] (as
 *      interdiff_denoising_losses), grads [n_param], d_cond [mem_len][B][256] (summed over the eight layers, 7 .. 0).  d_pred_in NULL: the
 *      gradient of the weighted loss (interdiff_denoising_loss_grad); else [B,1,144,T], the gradient of any other objective with respect to
 *      pred, taken instead.  ws 256-byte aligned.  T <= 128 (one workgroup holds a head's keys), mem_len <= 16, past_len >= 2, T >= past_len + 2.
 *  interdiff_mdm_train_step          replaces optimizer.step() of torch.optim.AdamW (decoupled decay, then Adam with bias correction, torch's
 *      order of operations) on the flat vectors, in place; `step` = 1 for the first step.
 * ---------------------------------------------------------------------------------- */
int interdiff_denoising_loss_grad(const float *pred, const float *target, int32_t B, int32_t T, int32_t past_len, const float *weights16,
                                  float *d_pred, void *stream);
int interdiff_mdm_train_param_table(int64_t *offsets, int64_t *sizes, int32_t *n_tensors, int64_t *n_param);
size_t interdiff_mdm_train_workspace_bytes(int32_t B, int32_t T, int32_t mem_len);
int interdiff_mdm_train_grads(const float *params, const float *pe, int32_t pe_rows, const float *x_t, const int64_t *ts, const float *cond,
                              const float *target, int32_t B, int32_t T, int32_t mem_len, int32_t past_len, const float *weights16,
                              const float *d_pred_in, float *grads, float *d_cond, float *pred, float *terms, void *ws, size_t ws_bytes,
                              void *stream);
int interdiff_mdm_train_step(float *params, const float *grads, float *exp_avg, float *exp_avg_sq, int64_t n, int32_t step, double lr,
                             double beta1, double beta2, double eps, double weight_decay, void *stream);

/* ------------------------------------------------------------------------------------
 * TRAINING of the SMPL denoiser's ENCODER as well (same files): the backward of MDM._get_embeddings from pc_embedding on
 * (model/diffusion_smpl.py:217-221: bodyEmbedding(body[:past]) + objEmbedding(obj[:past]) + pc_embedding, PositionalEmbedding, self.encoder =
 * [std, QaN x6, std] post-norm layers without cross-attention and without a final norm, :20-70, sublayers.py:37-204, layers.py:198-217), chained
 * behind the decoder's through d_cond -- what LitInteraction._common_step (train_diffusion_smpl.py:381-388) gets from calling
 * self.model._get_embeddings(batch) with autograd on.  Additive; same arithmetic contract as above.
 *
 * FULL PARAMETER TABLE.  The flat vectors hold 228 tensors: the 144 above at their offsets, then the 84 encoder tensors, per encoder layer 0..7:
 *     layers 0, 7: self_attn.in_proj_weight, self_attn.in_proj_bias, self_attn.out_proj.weight, self_attn.out_proj.bias;   layers 1..6: queries, wk;
 *     then linear1.{weight,bias}, linear2.{weight,bias}, norm1.{weight,bias}, norm2.{weight,bias}
 * (2 x 789 760 + 6 x 529 162 = 4 754 492 floats; n_param = 11 824 392).  bodyEmbedding / objEmbedding receive the sum of both paths, the decoder
 * path's contribution first and the encoder path's added to it.
 *
 *  interdiff_mdm_train_full_param_table   as interdiff_mdm_train_param_table for the 228 tensors (HOST int64 [228], nullable).
 *  interdiff_mdm_train_full_workspace_bytes   workspace of interdiff_mdm_train_full_grads; 0 for an unsupported shape.
 *  interdiff_mdm_train_full_grads    the arguments of interdiff_mdm_train_grads with pc [B][256] (pc_embedding, the output of
 *      interdiff_pointnet2_encode: the input seam of this pass) in the place of cond, and mem_len = past_len: the encoder's tokens are the past
 *      frames target[..., :past_len].  Encoder forward -> decoder forward -> terms -> decoder backward -> encoder backward.  -> pred, terms,
 *      grads [n_param of the full table], cond [past_len][B][256] (the encoder's output, as MDM._get_embeddings returns it), d_cond (as above),
 *      d_pc [B][256] = d embedding summed over a clip's past_len tokens in token order (the seam a backward of pcEmbedding would take).
 *      pred, terms, d_cond and the gradients of the tensors only the decoder reads have the bits interdiff_mdm_train_grads gives on that cond.
 *      T <= 128, 2 <= past_len <= 16, T >= past_len + 2; IDF_E_INVAL otherwise.
 *  interdiff_mdm_train_step serves the longer vectors as it is (n = the full n_param).
 * ---------------------------------------------------------------------------------- */
int interdiff_mdm_train_full_param_table(int64_t *offsets, int64_t *sizes, int32_t *n_tensors, int64_t *n_param);
size_t interdiff_mdm_train_full_workspace_bytes(int32_t B, int32_t T, int32_t past_len);
int interdiff_mdm_train_full_grads(const float *params, const float *pe, int32_t pe_rows, const float *x_t, const int64_t *ts, const float *pc,
                                   const float *target, int32_t B, int32_t T, int32_t past_len, const float *weights16, const float *d_pred_in,
                                   float *grads, float *cond, float *d_cond, float *d_pc, float *pred, float *terms, void *ws, size_t ws_bytes,
                                   void *stream);

/* ------------------------------------------------------------------------------------
 * Fine-tuning of the SMPL denoiser's PointNet++ (csrc/pointnet2.hip, csrc/pointnet2_train.h / .hip): consumes the d_pc of the entry above.  Additive entries:
 * interdiff_abi_version() stays what it was.  Regime: pcEmbedding in eval() with autograd on (frozen running statistics); the batch-statistic regime is the next block's.
 *
 *  interdiff_pointnet2_encode_saved   replaces PointNet2Encoder.forward (model/layers.py:141-175) as MDM._get_embeddings calls it with autograd on
 *      (model/diffusion_smpl.py:210-211): out [B,256] has the bits of interdiff_pointnet2_encode, and `saves` (interdiff_pointnet2_saves_bytes(B) bytes, 4-byte
 *      aligned) receives per clip what autograd would keep: the 48 SA2 slots as FPS position, point id and duplicate-slot map, the 16 + 32 neighbour point ids
 *      of every centre, the hit counts of all ball queries, the SA1 output of each slot (layout: csrc/pointnet2_train.h).
 *  interdiff_pointnet2_finetune_grads replaces loss.backward() through pcEmbedding (train_diffusion_smpl.py:60-166 with the module of model/layers.py:111-175):
 *      grads [113,917] = d sum(d_pc * pc) / d theta for the 38 raw tensors of the PARAMETER TABLE below.  It runs no sampling and no ball query; activations,
 *      ReLU masks and pool winners are recomputed from `saves` and the folded arena of `pn`, which must be the fold of `theta` / `stats` (interdiff_pointnet2_refold).
 *      d_pc[:, 0:3] (the key point's xyz) reaches no parameter; no gradient with respect to obj_points.  fp32, fixed summation order, clips folded in index
 *      order in double, no atomics.  ws: interdiff_pointnet2_finetune_workspace_bytes(B) bytes, 256-byte aligned.
 *  interdiff_pointnet2_refold         replaces the host fold of eval BatchNorm (mdm.py pack_pointnet2; the reference's BatchNorm2d.forward in eval(), applied by
 *      torch at every call): rewrites pn->arena from theta and stats on the stream, no host round trip; stats are read and never written.
 *  interdiff_pointnet2_finetune_param_table   PARAMETER TABLE: the 38 tensors in the reference's state_dict order -- for SA_modules.{0,1}.mlps.{0,1} and layer
 *      l = 0..2: `.{3l}.weight` [cout,cin,1,1], `.{3l+1}.weight` [cout], `.{3l+1}.bias` [cout]; then Linear.weight [253,256], Linear.bias [253].
 *      stats [1472]: per layer, in the same order, running_mean [cout] then running_var [cout].
 * The optimiser step is interdiff_mdm_train_step on the flat vectors (torch.optim.AdamW.step, train_diffusion_smpl.py:177-183).
 * ---------------------------------------------------------------------------------- */
size_t interdiff_pointnet2_saves_bytes(int32_t B);
int interdiff_pointnet2_encode_saved(const idf_pointnet2 *pn, const float *obj_points, int32_t B, int32_t P, float *out, void *saves, size_t saves_bytes,
                                     void *stream);
int interdiff_pointnet2_finetune_param_table(int64_t *offsets, int64_t *sizes, int32_t *n_tensors, int64_t *n_param);
size_t interdiff_pointnet2_finetune_workspace_bytes(int32_t B);
int interdiff_pointnet2_finetune_grads(const idf_pointnet2 *pn, const float *theta, const float *stats, const float *obj_points, int32_t B, int32_t P,
                                       const void *saves, const float *d_pc, float *grads, void *ws, size_t ws_bytes, void *stream);
int interdiff_pointnet2_refold(const idf_pointnet2 *pn, const float *theta, const float *stats, void *stream);

/* ------------------------------------------------------------------------------------
 * Training of the SMPL denoiser's PointNet++ under BATCH statistics (csrc/pointnet2_bn_train.h / .hip): pcEmbedding in train(), the regime Lightning puts
 * LitInteraction.model in.  Additive entries: interdiff_abi_version() stays what it was.  theta / grads: the 38 raw tensors of
 * interdiff_pointnet2_finetune_param_table (the one table); stats [1472] as there.  Limits: 1 <= B <= 256, 1 <= P <= 2048 (IDF_E_INVAL beyond).
 *
 *  interdiff_pointnet2_train_forward  replaces PointNet2Encoder.forward (model/layers.py:141-175) as MDM._get_embeddings calls it (model/diffusion_smpl.py:210-211)
 *      with the module in train(): each of the twelve BatchNorm2d sites normalises with the mean and biased variance of its own tensor -- in SA1 over all
 *      B * 1024 * nsample rows, padding slots and repeated FPS positions counted as often as they occur; in SA2 over B * 16 and B * 32 rows.  It reads the RAW
 *      tensors (no fold).  pc_out [B,256].  `ws` (interdiff_pointnet2_train_workspace_bytes(B) bytes, 256-byte aligned) keeps the sampling and grouping of every
 *      centre, the batch statistics and what the backward reads.
 *  interdiff_pointnet2_train_grads    replaces loss.backward() through pcEmbedding in train() (train_diffusion_smpl.py:60-166): grads [113,917] =
 *      d sum(d_pc * pc) / d theta, through the batch statistics (BatchNorm2d's train-mode backward), of the forward that left `ws`.  d_pc[:, 0:3] reaches no
 *      parameter; no gradient with respect to obj_points.  fp32 products, fixed summation orders, partial sums folded in index order in double, no atomics.
 *  interdiff_pointnet2_train_stats    replaces the running-statistic update of BatchNorm2d.forward in train() (momentum 0.1 in the reference; the running variance
 *      takes the unbiased batch variance): stats are rewritten in place from the batch statistics in `ws`, in double, rounded once.  num_batches_tracked is the
 *      caller's.  interdiff_pointnet2_refold then rebuilds the eval pack from the new weights and statistics.
 * ---------------------------------------------------------------------------------- */
size_t interdiff_pointnet2_train_workspace_bytes(int32_t B);
int interdiff_pointnet2_train_forward(const float *theta, const float *obj_points, int32_t B, int32_t P, float *pc_out, void *ws, size_t ws_bytes, void *stream);
int interdiff_pointnet2_train_grads(const float *theta, const float *obj_points, int32_t B, int32_t P, const float *d_pc, float *grads, void *ws, size_t ws_bytes,
                                    void *stream);
int interdiff_pointnet2_train_stats(const void *ws, int32_t B, double momentum, float *stats, void *stream);

/* ------------------------------------------------------------------------------------
 * Scoring of a skeleton diffusion checkpoint (csrc/skeleton_losses.hip): the forward, scoring side of interdiff/train_diffusion_skeleton.py.
 * Forward only, additive.  Tokens [B,1,C,T] with C = n_body + 3 * n_points + 7 (63 + 36 + 7 = 106): body | object keypoints | object
 * translation 3 | object quaternion xyzw 4.  The keypoint channels are the prediction's own (the denoiser's keypoint head wrote them): nothing is
 * re-posed.  Term order everywhere (the reference's dict order, :129-143 / :215-229):
 *   0 body_past, 1 body_future, 2 obj_past, 3 obj_future, 4 loss_obj_nonrot_past, 5 loss_obj_nonrot_future, 6 loss_obj_rot_past,
 *   7 loss_obj_rot_future, 8 quaternion_reg_loss, 9 loss_obj_rot_v, 10 loss_obj_nonrot_v, 11 loss_body_v, 12 loss_obj_v
 * -- raw (unweighted) means of squares; the four velocity terms over all T - 1 frame differences, (x[t] - x[t-1]) - (g[t] - g[t-1]);
 * quaternion_reg_loss = mean over frames of (q.q - 1)^2 of the prediction.
 *
 *  interdiff_skeleton_sample_losses     replaces the split of _common_step (:280-283) and calc_val_loss (:190-229).  pred f32 [K][B,1,C,T]: K
 *      samples of one batch (K = 1 is the reference's case; no best-of-K terms, the skeleton trainer has none), gt f32 [B,1,C,T].
 *      out_terms f32 [K][13]: per sample the mean over its B clips.  out_per_clip f32 [K][13][B] (nullable: then `ws` holds it,
 *      interdiff_skeleton_sample_losses_workspace_bytes(K, B) bytes): every clip's own mean of every term -- it depends on that clip's floats
 *      alone, whatever else is in the call.  Two launches whatever K and B are: one workgroup per (sample, clip), then one small workgroup
 *      for the means over clips; fp32, no float atomics, fixed order: two calls give the same bits.
 *      IDF_E_INVAL unless past_len >= 1, T >= past_len + 1 and C == n_body + 3 * n_points + 7; IDF_E_NOMEM for a short workspace; nothing is
 *      launched in either case.
 *  interdiff_skeleton_denoising_losses  replaces the 13 terms of forward_backward (:100-127) in their per-clip form: pred (the model output) and
 *      target f32 [B,1,C,T] with C = n_body + 3 * n_points + 7, out f32 [13][B].  One launch (the first of the two above); the means over the batch
 *      and the weighted sum (:145-161, :168) are the caller's.  Same argument checks.
 * ---------------------------------------------------------------------------------- */
size_t interdiff_skeleton_sample_losses_workspace_bytes(int32_t K, int32_t B);
int interdiff_skeleton_sample_losses(const float *pred, const float *gt, int32_t K, int32_t B, int32_t C, int32_t T, int32_t past_len,
                                     int32_t n_body, int32_t n_points, float *out_terms, float *out_per_clip, void *ws, size_t ws_bytes,
                                     void *stream);
int interdiff_skeleton_denoising_losses(const float *pred, const float *target, int32_t B, int32_t T, int32_t past_len, int32_t n_body,
                                        int32_t n_points, float *out, void *stream);

/* ------------------------------------------------------------------------------------
 * TRAINING of the skeleton denoiser (csrc/skeleton_mdm_train.hip on the stacks of csrc/mdm_train.h / .hip at feed-forward width 256, token width
 * 106): one optimiser step of interdiff/train_diffusion_skeleton.py -- LitInteraction._common_step(mode='train') (:255-262) = MDM._get_embeddings
 * (model/diffusion_skeleton.py:194-215), GaussianDiffusion.q_sample (interdiff_q_sample), MDM.forward(x, timesteps, zero_pose_obj, y) (:231-257:
 * _decode, calc_obj_pred :218-229 with pytorch3d's quaternion_to_matrix, which does not normalise), the loss of forward_backward (:89-168),
 * loss.backward() through all of it, and torch.optim.AdamW (configure_optimizers :181-184).  No seam is left: every one of the model's 230 parameter
 * tensors (5 499 582 floats) gets its gradient.  Additive entries, same arithmetic contract as the SMPL trainer's (exact fp32, no float atomics, two
 * calls give the same bits, linear in d_pred bit for bit); dropout 0, cond_mask_prob 0.  n_body = 63, n_points = 12.
 *
 * SKELETON PARAMETER TABLE.  230 tensors packed without padding: the 144 names of the PARAMETER TABLE above (shapes of the skeleton model:
 * bodyEmbedding [256,63], objEmbedding [256,36], linear1 [256,256], bodyFinalLinear [63,256], objFinalLinear [7,256]), then the 84 encoder tensors in
 * the order of the FULL PARAMETER TABLE, then shapeEmbedding.weight [256,36], shapeEmbedding.bias [256].  bodyEmbedding / objEmbedding receive the
 * decoder path's gradient first and the encoder path's added to it.
 *
 *  interdiff_skeleton_denoising_loss_grad   replaces autograd through the 13 terms (:108-168): d_pred [B,1,106,T] = d/d pred of
 *      mean_b sum_i weights13[i] * term_i[b], the terms and their order of interdiff_skeleton_denoising_losses (the schedule sampler's weights are
 *      all one).  weights13: HOST pointer.  One launch, one thread per element.  past_len >= 1, T >= past_len + 1.
 *  interdiff_skeleton_mdm_train_param_table   offsets / sizes (HOST int64 [230], nullable), their count and n_param.
 *  interdiff_skeleton_mdm_train_workspace_bytes   workspace of the gradient call; 0 for an unsupported shape.
 *  interdiff_skeleton_mdm_train_grads   encoder forward -> decoder forward -> keypoint head -> terms -> head, decoder and encoder backward -> the
 *      shape embedding's gradient.  x_t, target [B,1,106,T] (target = x_start: its past frames are the encoder's tokens), ts int64 [B],
 *      zero_pose_obj [B][12][3] (data: no gradient), pe [pe_rows][256] (pe_rows > every timestep and >= T).  -> grads [n_param],
 *      cond [past_len][B][256] (what _get_embeddings returns), pred [B,1,106,T] = body | R(q) zero_pose_obj + translation | pose, terms [13][B].
 *      d_pred_in NULL: the gradient of the weighted loss; else [B,1,106,T], any other objective's gradient with respect to pred, taken through the
 *      same head backward.  ws 256-byte aligned.  T <= 128, 2 <= past_len <= 16, T >= past_len + 2; IDF_E_INVAL otherwise.
 *  The optimiser step is interdiff_mdm_train_step (elementwise on n floats) as it stands.
 * ---------------------------------------------------------------------------------- */
int interdiff_skeleton_denoising_loss_grad(const float *pred, const float *target, int32_t B, int32_t T, int32_t past_len, const float *weights13,
                                           float *d_pred, void *stream);
int interdiff_skeleton_mdm_train_param_table(int64_t *offsets, int64_t *sizes, int32_t *n_tensors, int64_t *n_param);
size_t interdiff_skeleton_mdm_train_workspace_bytes(int32_t B, int32_t T, int32_t past_len);
int interdiff_skeleton_mdm_train_grads(const float *params, const float *pe, int32_t pe_rows, const float *x_t, const int64_t *ts, const float *target,
                                       const float *zero_pose_obj, int32_t B, int32_t T, int32_t past_len, const float *weights13,
                                       const float *d_pred_in, float *grads, float *cond, float *pred, float *terms, void *ws, size_t ws_bytes,
                                       void *stream);

/* ------------------------------------------------------------------------------------
 * Scoring of a correction-predictor checkpoint (csrc/corr_losses.hip).  Forward only, additive.
 *  interdiff_correction_losses  replaces LitInteraction.calc_loss_contact (interdiff/train_correction_smpl.py:103-185), calc_loss (:60-101) and the
 *      skeleton trainer's calc_loss (train_correction_skeleton.py:85-126).
 *      obj_pred, obj_gt f32 [T][B][rot_width + 3]: rot = the leading rot_width channels, nonrot = the trailing 3 (rot_width 6: rot6d | translation;
 *      4: the skeleton trainer's pose [translation | quaternion xyzw], split as that trainer splits it).
 *      out_terms f32 [10], the reference's dict order: penetration, contact, obj_rot_past, obj_nonrot_past, obj_rot_future, obj_nonrot_future,
 *      obj_rot_v_past, obj_nonrot_v_past, obj_rot_v_future, obj_nonrot_v_future -- raw (unweighted) means.  The future velocity term pairs frame t
 *      with t - 1 from t = past_len on (its first pair straddles the border), as upstream.
 *      Geometry half (obj_points and human_verts given; rot_width must be 6): obj_points f32 [B][P][point_stride] canonical, xyz leading (stride 3, or
 *      6 for the batch's points-with-normals), human_verts f32 [T][B][V][7] = position | normal | contact label, interleaved as the batch has it.
 *      Per frame the points are posed with rotation_6d_to_matrix(obj_pred) and the predicted translation INSIDE the kernel and point2point_signed
 *      (tools.py:11-76) runs in both directions with the contract of interdiff_nn_argmin (d2 = (dx*dx + dy*dy) + dz*dz, no FMA, lowest index wins):
 *        contact      = mean over T*B*V of |h2o| [|h2o| > 0.02 and label > 0.5]
 *        penetration  = mean over T*B*P of 20 |o2h| [o2h < 0], the sign from the body normal of the nearest vertex
 *      (the reference's band 0 < o2h < 0.01 carries weight 0, :141-143: kept).  No per-pair / per-vertex / per-point array is written: only
 *      (sum, count) per workgroup, into ws >= interdiff_correction_losses_workspace_bytes(T, B, V, P).  out_frames (nullable) f32 [T*B][4] =
 *      per frame (penetration sum, contact sum, penetrating points, contact vertices).  T * B <= 65535.
 *      Without the geometry half (both pointers NULL): terms 0 and 1 are 0, ws and out_frames must be NULL.
 *      The per-frame matrices come from interdiff_rotation_6d_to_matrix itself (the rot6d columns are gathered into ws by one strided device copy), so
 *      the entry poses the points from the bits that entry gives.  One copy + three launches (one launch without geometry) whatever T * B is; no float atomics, fixed summation order: two calls give the same bits, and a frame's
 *      partial sums do not depend on which other clips are in the call.  past_len >= 1, T >= past_len + 1.
 * ---------------------------------------------------------------------------------- */
size_t interdiff_correction_losses_workspace_bytes(int32_t T, int32_t B, int32_t V, int32_t P);
int interdiff_correction_losses(const float *obj_pred, const float *obj_gt, const float *obj_points, int32_t point_stride, const float *human_verts,
                                int32_t T, int32_t B, int32_t V, int32_t P, int32_t rot_width, int32_t past_len, float *out_terms, float *out_frames,
                                void *ws, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------------------------
 * Backward pass of the two geometry terms (csrc/corr_geometry_grad.hip).  Additive: interdiff_abi_version() stays what it was.
 *  interdiff_correction_geometry_grads  replaces what loss.backward() sends from the contact and penetration terms of
 *      LitInteraction.calc_loss_contact (interdiff/train_correction_smpl.py:121-153, :159-162) through torch.matmul(obj_points, obj_rot) + trans (:126),
 *      rotation_6d_to_matrix (:121) and tools.point2point_signed (tools.py:11-76) into obj_pred: d (w_penetration * penetration + w_contact * contact)
 *      / d obj_pred, every mask and nearest-neighbour index a constant, as autograd treats them.
 *      obj_pred f32 [T][B][9] (rot6d | translation), obj_points, point_stride, human_verts, T, B, V, P as interdiff_correction_losses takes them.
 *      w_penetration, w_contact >= 0: the ALREADY ANNEALED factors of the weighted dict (:159-162), a^2 * weight_penetration and a^2 * weight_contact.
 *      -> d_obj_pred_out f32 [T][B][9]; terms2_out f32 [2] = (penetration, contact), raw means, the terms 0 and 1 of interdiff_correction_losses (to fp32
 *      rounding); frames_out (nullable) f32 [T*B][4] in that entry's out_frames layout.  With both weights 0 d_obj_pred_out is exact zeros.
 *      A penetrating point j contributes g = 20 (y_j - x_i(j)) / |y_j - x_i(j)| with p = p_j, a contact vertex i contributes g = -(x_i - y_j(i)) /
 *      |x_i - y_j(i)| with p = p_j(i); each adds g to dL/dt and g p^T to dL/dM, and dL/dM goes back through the Gram-Schmidt construction of
 *      rotation_6d_to_matrix (F.normalize's eps 1e-12).  The scan is the forward's (1024 queries of one frame and one direction per workgroup, the
 *      contract of interdiff_nn_argmin) with the argmin index carried on the human side as well; the unit vectors, the 12 sums per frame and the
 *      Gram-Schmidt backward are in double, the result is rounded once.  Nothing per point is scattered: a workgroup writes (sum, count) and 12 doubles
 *      into ws >= interdiff_correction_geometry_grads_workspace_bytes(T, B, V, P), a finishing launch folds them in index order.  One copy + three
 *      launches whatever T * B is; no float atomics: two calls give the same bits, and the output is linear in the weights to the last bit for a
 *      scaling by a power of two.  IDF_E_INVAL: null pointer, a size < 1, point_stride < 3, T * B > 65535, a negative or non-finite weight;
 *      IDF_E_NOMEM: short workspace.
 * ---------------------------------------------------------------------------------- */
size_t interdiff_correction_geometry_grads_workspace_bytes(int32_t T, int32_t B, int32_t V, int32_t P);
int interdiff_correction_geometry_grads(const float *obj_pred, const float *obj_points, int32_t point_stride, const float *human_verts, int32_t T,
                                        int32_t B, int32_t V, int32_t P, double w_penetration, double w_contact, float *d_obj_pred_out,
                                        float *terms2_out, float *frames_out, void *ws, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------------------------
 * Contact-label generation (csrc/contact_labels.hip): the per-frame work of interdiff/data/prepare_behave.py:32-52 (get_contact_labels).  Additive.
 *  interdiff_contact_labels     replaces igl.signed_distance(points, smpl.vertices, smpl.faces) (:42, winding-number sign), `dist < thres` (:45) and
 *      the body vertices within thres of a labelled point (:48-51), for N frames in three launches.  igl is not available: RESTATED, the restatement
 *      defines the contract:
 *        d = min over faces of the exact point-triangle distance (a zero-area face counts through its edges and corners; never NaN),
 *        w = (1 / 4 pi) sum over faces of the signed solid angle (van Oosterom-Strackee atan2 form; a zero-area face contributes 0),
 *        S = (1 - 2 w) d,   obj_label = S < thres,   human_label[v] = exists p: obj_label[p] and |p - v| < thres   (both comparisons strict).
 *      verts f32 [N][V][3]; faces int32 [F][3] in the mesh's own orientation, every index in [0, V) -- validated by the caller, the kernels only clamp;
 *      their order changes no result, only how many (lane, 256-face chunk) pairs the bounding-box test skips (sort them along a space-filling curve).
 *      points f32: point_frame_stride 0 = one cloud [P][3] shared by all frames, 3 * P = per-frame points [N][P][3].  objR f32 [N][9] row-major and
 *      objT f32 [N][3], both or neither: the kernels use p R^T + t (products and sums rounded one by one, left to right); NULL = points as given.
 *      obj_label uint8 [N][P], human_label uint8 [N][V] (all V vertices, unreferenced ones included), signed_dist (nullable) f32 [N][P] = S: w is
 *      computed for every point (the solid angle shares the face loop of the distance), so there is no point that gets +d instead.
 *      ws >= interdiff_contact_labels_workspace_bytes(N, V, F, P): the chunk bounding boxes.  fp32, no float atomics, no reduction across
 *      workgroups: two calls give the same bits.  IDF_E_INVAL: null pointer, non-positive size or thres, a stride that is neither 0 nor 3 * P, one of
 *      objR / objT without the other; IDF_E_NOMEM: short workspace.
 *  interdiff_debug_point_triangle   HOST-side instance of the per-pair device inline: tri [n][9] = a | b | c, p [n][3] -> out [n][2] = squared distance,
 *      signed solid angle; lets the CPU test suite check the region logic without a GPU.
 * ---------------------------------------------------------------------------------- */
size_t interdiff_contact_labels_workspace_bytes(int64_t N, int32_t V, int32_t F, int32_t P);
int interdiff_contact_labels(const float *verts, int64_t N, int32_t V, const int32_t *faces, int32_t F, const float *points, int32_t P,
                             int64_t point_frame_stride, const float *objR, const float *objT, float thres, uint8_t *obj_label /*[N,P]*/,
                             uint8_t *human_label /*[N,V]*/, float *signed_dist /*[N,P] or NULL*/, void *ws, size_t ws_bytes, void *stream);
int interdiff_debug_point_triangle(const float *tri, const float *p, float *out, int32_t n);

/* ------------------------------------------------------------------------------------
 * Mesh rendering (csrc/render.hip, csrc/render.h): the pictures of interdiff/render/mesh_viz.py (visualize_body_obj) without pyrender / EGL -- a tiled
 * software rasteriser whose integer stage is exact by construction.  Additive.  The contract (sub-pixel grid, fill rule, depth key, bit widths) is the
 * head comment of csrc/render.h; tests/render_oracle.py restates it in numpy.
 *  idf_render_scene   off: subtracted after the negation of a moving mesh's coordinates (scene = -p - off); cam_t, cam_cos, cam_sin: camera position and
 *      downward pitch (pose = translate(cam_t) . rotate_x(-pitch)); znear; focal = 1 / tan(yfov / 2); light [3][3]: unit vectors TOWARDS the three
 *      directional lights; shade = min(1, ambient + light_gain * sum max(0, n . L)); bg: background colour in [0, 1].
 *  idf_render_mesh    verts, normals f32 [frames][V][3] (frames = 1: shared by all frames, or N); faces int32 [F][3], every index in [0, V);
 *      rgb f32 [N][3] base colour per frame, or [V][3] per vertex with IDF_RMESH_VERTEX_RGB; R f32 [N][9] row-major and t f32 [N][3], both or
 *      neither: verts and normals are posed per frame inside the setup stage (p R^T + t, rounded left to right as interdiff_contact_labels does).
 *      IDF_RMESH_SCENE_SPACE: the mesh is given in scene coordinates and does not turn with the views (the ground).
 *  interdiff_render_frames   N frames x `views` images (view v turns the moving meshes v quarter turns about +y), H x W pixels each.
 *      out_rgb uint8 [N][views][H][W][3]; out_id (nullable) int32 [N][views][H][W] = the winning slot, -1 background (slot = 2 * source triangle (+ 1),
 *      source triangles numbered through the meshes in the order given); out_depth (nullable) int32, 0x7fffffff background; out_setup (nullable)
 *      int32 [N][views][2 * sum F][20], the setup records.  dropped (HOST, nullable): slots whose snapped coordinates left the guard band -- counted,
 *      never clamped, the rest of the scene is drawn.  stage_ms (HOST, nullable) f32 [3]: setup + count, scan + fill, tile + resolve, hip events
 *      (tile and resolve are ONE kernel -- the resolve reads the tile's keys out of LDS -- so they cannot be timed apart).
 *      ws >= interdiff_render_frames_workspace_bytes(1, ...): images are rendered in as many chunks as the workspace asks for, with identical bits.
 *      Integer atomics only (LDS 64-bit min, global 32-bit add); nothing depends on their order: two calls give the same bits.  The call
 *      synchronises the stream (face check up front, counter at the end).
 *      IDF_E_INVAL: null pointer, a data pointer that is not 4-byte aligned or a ws that is not 256-byte aligned (hipMalloc's and torch's are), N / views / H / W out of range (views 1..4, H, W 1..IDF_RENDER_MAX_DIM), no mesh or more
 *      than IDF_RENDER_MAX_MESHES, V or F non-positive, frames neither 1 nor N, one of R / t without the other, a face index outside [0, V);
 *      IDF_E_NOMEM: a workspace that does not hold one image.  Nothing is written in either case.
 *  interdiff_debug_render_setup_vertex / _pixel   HOST-side instances of the setup stage's per-vertex function and of the per-pixel coverage / depth /
 *      colour function.  vertex: pos, nrm, rgb f32 [n][3] -> out_f f32 [n][6] = xc, yc, d, r, g, b and out_i int32 [n][7] = in front of the near
 *      plane, X, Y, Z, R, G, B (0 when behind).  pixel: rec int32 [n][20], ij int32 [n][2] -> out int32 [n][5] = covered, depth, r, g, b.
 * ---------------------------------------------------------------------------------- */
#define IDF_RENDER_SUBPIX 16
#define IDF_RENDER_GUARD 32768
#define IDF_RENDER_MAX_DIM 2048
#define IDF_RENDER_ZONE (1 << 28)
#define IDF_RENDER_REC_INTS 20
#define IDF_RENDER_TILE 16
#define IDF_RENDER_MAX_MESHES 8
enum { IDF_RMESH_SCENE_SPACE = 1, IDF_RMESH_VERTEX_RGB = 2 };
typedef struct {
    float off[3], cam_t[3];
    float cam_cos, cam_sin, znear, focal;
    float light[9];
    float light_gain, ambient;
    float bg[3];
    float reserved;
} idf_render_scene;
typedef struct {
    const float *verts, *normals;
    const int32_t *faces;
    const float *rgb, *R, *t;
    int32_t V, F, frames, flags;
} idf_render_mesh;
size_t interdiff_render_frames_workspace_bytes(int64_t n_images, int64_t n_triangles, int32_t H, int32_t W);
int interdiff_render_frames(const idf_render_scene *scene, const idf_render_mesh *meshes, int32_t n_meshes, int64_t N, int32_t views, int32_t H,
                            int32_t W, uint8_t *out_rgb, int32_t *out_id, int32_t *out_depth, int32_t *out_setup, int64_t *dropped, float *stage_ms,
                            void *ws, size_t ws_bytes, void *stream);
int interdiff_debug_render_setup_vertex(const idf_render_scene *scene, int32_t view, int32_t scene_space, int32_t H, int32_t W, const float *pos,
                                        const float *nrm, const float *rgb, float *out_f, int32_t *out_i, int32_t n);
int interdiff_debug_render_pixel(const int32_t *rec, const int32_t *ij, int32_t *out, int32_t n);

/* ------------------------------------------------------------------------------------
 * Skeleton-mode clips (csrc/skeleton_render.hip, csrc/skeleton_render.h): the pictures of interdiff/render/viz_helper.py (visualize_skeleton and
 * visualize_skeleton_pred_gt) without matplotlib -- 21 joints, 12 object keypoints, bones / wires as anti-aliased lines with projecting caps, scatter
 * markers as discs, matplotlib's per-frame camera restated.  Additive.  The contract (sub-pixel grid, coverage rule, blend arithmetic, bit widths, draw
 * order) is the head comment of csrc/skeleton_render.h; tests/skeleton_render_oracle.py restates it in numpy.
 *  idf_skel_view   everything of the camera that does not depend on the frame (HOST struct, computed in double by interdiff_amd/skeleton_render.py):
 *      view [3][4]: rows u (screen right), v (screen up), w (out of the screen) of the view rotation in box coordinates, each followed by -(row . eye);
 *      aspect [3]: the box aspect per data axis; margin [3]: the share of the data span added on either side before the 1/48 view margin;
 *      dist: eye distance (10); kx, cx, ky, cy: X = rint(tx kx + cx), Y = rint(ty ky + cy) in 1/16 pixel, origin top-left, y down (ky < 0);
 *      line_wd, disc_wd: FULL line width / disc diameter in 1/16 pixel, 1 .. IDF_SKEL_WD_MAX; style: IDF_SKEL_PLAIN or IDF_SKEL_PREDGT;
 *      pred_from: pred / gt style draws the prediction in frames t >= pred_from; colour [5][4]: RGBA 8-bit -- plain: bones, axis lines, body markers,
 *      object markers, unused; pred / gt: pred bones, axis lines, pred wires, gt bones, gt wires.
 *  interdiff_skeleton_render_frames   B clips x T frames, H x W pixels each, white background.  body f32 [B][T][21][3], obj f32 [B][T][12][3];
 *      body_gt f32 [B][T_gt][21][3], obj_gt f32 [B][T_gt][12][3] (pred / gt style only, both or neither; drawn in frames t < T_gt);
 *      wires int32 [n_wires][2] (DEVICE, pred / gt style, n_wires <= IDF_SKEL_MAX_WIRES; a pair with an index outside [0, 12) draws nothing and is
 *      counted as dropped).  out_rgb uint8 [B][T][H][W][3]; out_setup (nullable) int32 [B][T][IDF_SKEL_MAX_REC][IDF_SKEL_REC_INTS], the frame's
 *      records in draw order; out_count (nullable) int32 [B][T], the number of slots in use.  *dropped (HOST, nullable): primitives left out because
 *      an input is not finite, lies behind the eye or a snapped coordinate leaves the guard band of IDF_RENDER_GUARD -- never clamped, the rest is drawn.
 *      stage_ms (HOST, nullable) f32 [2]: setup, raster (hip events).  ws >= interdiff_skeleton_render_frames_workspace_bytes(1): frames are rendered
 *      in as many chunks as the workspace asks for, with identical bits.  No float atomics; the only atomic is the 32-bit integer add of the dropped
 *      counter: two calls give the same bits.  The call synchronises the stream (the counter is read back).
 *      IDF_E_INVAL: null / misaligned pointer, B, T, H, W out of range (H, W 1..IDF_RENDER_MAX_DIM), a bad style, widths outside 1..IDF_SKEL_WD_MAX,
 *      n_wires outside 0..IDF_SKEL_MAX_WIRES, one of body_gt / obj_gt without the other; IDF_E_NOMEM: a workspace that does not hold one frame.
 *  interdiff_skeleton_raster_records   the raster stage alone on the caller's records: recs (DEVICE) int32 [n_frames][IDF_SKEL_MAX_REC][8], the first
 *      `count` slots of every frame in draw order, each obeying the record contract (|X|, |Y| <= IDF_RENDER_GUARD, wd in 1..IDF_SKEL_WD_MAX; the
 *      arithmetic is only defined inside it, memory safety does not depend on it) -> out_rgb uint8 [n_frames][H][W][3].  n_frames <= 65535.
 *  interdiff_debug_skeleton_setup / _pixel   HOST-side instances of one frame's setup (the per-primitive function the kernel's lanes run, looped) and
 *      of the per-pixel function.  setup: all arrays on the HOST, frame t of clip 0 -> rec int32 [IDF_SKEL_MAX_REC][8], *count, *dropped.
 *      pixel: rec int32 [n_rec][8] in draw order, ij int32 [n][2] -> out int32 [n][3] = r, g, b of pixel (i, j) after folding every record.
 * ---------------------------------------------------------------------------------- */
#define IDF_SKEL_REC_INTS 8
#define IDF_SKEL_MAX_REC 128
#define IDF_SKEL_MAX_WIRES 40
#define IDF_SKEL_WD_MAX 1024
#define IDF_SKEL_TILE 16
enum { IDF_SKEL_PLAIN = 0, IDF_SKEL_PREDGT = 1 };
typedef struct {
    float view[12];
    float aspect[3], margin[3];
    float dist, kx, cx, ky, cy;
    int32_t line_wd, disc_wd, style, pred_from;
    uint8_t colour[5][4];
} idf_skel_view;
size_t interdiff_skeleton_render_frames_workspace_bytes(int64_t n_frames);
int interdiff_skeleton_render_frames(const idf_skel_view *view, const float *body, const float *obj, const float *body_gt, const float *obj_gt,
                                     const int32_t *wires, int32_t n_wires, int64_t B, int32_t T, int32_t T_gt, int32_t H, int32_t W, uint8_t *out_rgb,
                                     int32_t *out_setup, int32_t *out_count, int64_t *dropped, float *stage_ms, void *ws, size_t ws_bytes, void *stream);
int interdiff_skeleton_raster_records(const int32_t *recs, int32_t count, int64_t n_frames, int32_t H, int32_t W, uint8_t *out_rgb, void *stream);
int interdiff_debug_skeleton_setup(const idf_skel_view *view, const float *body, const float *obj, const float *body_gt, const float *obj_gt,
                                   const int32_t *wires, int32_t n_wires, int32_t T, int32_t T_gt, int32_t t, int32_t *rec, int32_t *count,
                                   int32_t *dropped);
int interdiff_debug_skeleton_pixel(const int32_t *rec, int32_t n_rec, const int32_t *ij, int32_t *out, int32_t n);

/* ------------------------------------------------------------------------------------
 * Training batches from a device-resident clip set (csrc/clip_batch.hip, per-clip math csrc/clip_canon.h; interdiff_amd/dataset.py).
 * Additive entries: interdiff_abi_version() stays what it was.
 *
 * idf_clip_set: the sequences of a split, concatenated over their frames (F = sum of the frame counts), all on the DEVICE:
 *      seq_off int64 [n_seq + 1] first global frame of every sequence; pose fp32 [F][156]; betas fp32 [F][10];
 *      fit64 double [F][12] = root axis-angle | body translation | object axis-angle | object translation (the four fields the
 *      canonicalisation computes on, in the files' own precision); joints fp32 [F][9] = pelvis | left foot | right foot (SMPL joints 0, 10, 11);
 *      obj_points6 fp32 [n_seq][P][6] = xyz | normal; first_label int32 [n_seq] the stored foot label of every sequence's frame 0 (10 or 11);
 *      body_ptr int32 [F + 1], body_idx int32 [body_ptr[F]]: the per-frame body contact lists as CSR, every index < V;
 *      markers_idx int32 [n_markers].
 * clips int32 [2][B] (DEVICE) = sequence ids | start frames; clip b holds the sequence frames start + t * sample_rate, t < T <= 128.  The caller
 *      checks that they lie inside the sequence; a clip that does not is skipped (nothing of it is written), never dereferenced.
 *
 *  interdiff_clip_batch   data/dataset_smpl.py:105-152 and :171-179 (Dataset.__getitem__: canonicalisation in the frame of the first pose, foot-ground
 *      labels) plus model/diffusion_smpl.py:212-214 (the ground-truth token) for B clips in ONE launch: body_pose [T,B,66], hand_pose [T,B,90],
 *      body_trans / obj_angles / obj_trans / pelvis [T,B,3], beta [T,B,10], gt [B,1,144,T], ground [T,B,2], centroid [B,3], rotation [B,3,3],
 *      obj_points [B,P,3], obj_points6 [B,P,6]; contact_label uint8 [T,B,V] (:167-168) in a second launch unless the pointer is null (then
 *      interdiff_clip_body_records writes it).  The arithmetic is double, rounded to fp32 once.  A first frame whose heading is undefined (global
 *      orientation entries [0][0] = [2][0] = 0) gives non-finite output, as in the reference.
 *  interdiff_clip_body_records   :134-139, :167-169, :189 in one launch: verts / normals fp32 [n_frames][V][3] (interdiff_smpl_forward on the canonical
 *      pose, interdiff_vertex_normals) + the body CSR -> human_verts fp32 [T,B,V,7] (16-byte aligned) = vertex | normal | label, markers
 *      [T,B,n_markers,7] = its rows markers_idx, contact_label uint8 [T,B,V] (or null).  frame_map int32 [n_frames] (or null: identity): the
 *      destination frame t * B + b of every input frame -- a gender's subset of the clips writes into the batch's slots.
 *  interdiff_debug_clip_canon   HOST instance of the per-clip math for the T gathered frames of one clip: fit double [T][12], pelvis fp32 [T][3],
 *      pose fp32 [T][156] -> root / trans / obj_angle / obj_trans / pelvis_out fp32 [T][3], gt fp32 [144][T], centroid [3], rotation [9].
 *      rotation_override fp32 [9] (or null): a rotation to compose with instead of the one frame 0's heading gives.
 *  Returns: IDF_OK; IDF_E_INVAL (null pointer, B, T, sample_rate <= 0, T > 128, V > 65536, misaligned human_verts); IDF_E_LAUNCH.
 * ---------------------------------------------------------------------------------- */
typedef struct {
    int32_t n_seq, P, V, n_markers;
    const int64_t *seq_off;
    const float *pose, *betas;
    const double *fit64;
    const float *joints, *obj_points6;
    const int32_t *first_label, *body_ptr, *body_idx, *markers_idx;
} idf_clip_set;
typedef struct {
    float *body_pose, *hand_pose, *body_trans, *obj_angles, *obj_trans, *pelvis, *beta, *gt, *ground, *centroid, *rotation, *obj_points, *obj_points6;
    uint8_t *contact_label;
} idf_clip_batch;
int interdiff_clip_batch(const idf_clip_set *cs, const int32_t *clips, int32_t B, int32_t T, int32_t sample_rate, const idf_clip_batch *out, void *stream);
int interdiff_clip_body_records(const idf_clip_set *cs, const int32_t *clips, int32_t B, int32_t T, int32_t sample_rate, const float *verts,
                                const float *normals, const int32_t *frame_map, int64_t n_frames, float *human_verts, float *markers,
                                uint8_t *contact_label, void *stream);
int interdiff_debug_clip_canon(const double *fit, const float *pelvis, const float *pose, int32_t T, const float *rotation_override, float *root,
                               float *trans, float *obj_angle, float *obj_trans, float *pelvis_out, float *gt, float *centroid, float *rotation);

/* ------------------------------------------------------------------------------------
 * The skeleton-mode training set on the device (csrc/skeleton_clip_batch.hip; interdiff_amd/skeleton_dataset.py SkeletonClipSet).
 * Additive entries: interdiff_abi_version() stays what it was.
 *
 *  interdiff_skeleton_video_prepare   data/dataset_skeleton.py:40-65 (recover_init_obj, get_consistent_poses), :85-104 (check_sequences) and the
 *      down-sampling of :148-151 for every video of a set in ONE launch, one workgroup per video.  All pointers DEVICE.  Inputs: the raw float64
 *      arrays of the pickles, concatenated over the videos' frames (F = sum of the frame counts): skel [F][J][3], obj [F][P][3], pose [F][7]
 *      (translation | quaternion xyzw), contact [F]; seq_off int64 [n_video + 1] the first frame of every video, row_off int64 [n_video + 1] its first
 *      row, with rows = ceil(frames / stride) per video (a video whose two table entries disagree is skipped).  Outputs:
 *      table fp32 [rows total][3 J + 3 P + 7] = body | object | pose of the frames stride * r, the quaternion multiplied by the sign s of
 *          get_consistent_poses: s_0 = 1, s_{i+1} = s_i * (q_i . q_{i+1} < 0 ? -1 : 1) on the raw quaternions in double (a tie keeps the sign, as the
 *          reference's strict > does), a prefix parity over ALL frames.  Every value is rounded from float64 once.  Frames that are no multiple of
 *          stride are read for the quaternion and the contact value only;
 *      zero_pose_obj fp32 [n_video][P][3]: recover_init_obj on frame 0 (the quaternion normalised, inverted, as a matrix) in double, rounded once;
 *      report double [n_video][3] = the discrepancy of :98-99 (mean over rows x P of |t + R(q) zero_pose - obj|), the check sum of :93 (the signed sum
 *          of |q| - 1 over the rows), the sum of contact over all frames -- each summed in a fixed order (256 strided partial sums, one tree);
 *      row_contact double [rows total]: contact at the frames stride * r;  signs int8 [F] (or null): s of every frame.
 *      P <= 64.
 *  interdiff_debug_skeleton_video_prepare   HOST instance of the same per-video code for ONE video of F frames (host pointers): the same operations in
 *      the same order, compiled without contraction on both sides, so the outputs are the device's bit for bit.
 *  interdiff_skeleton_window_batch   B windows in ONE launch.  idf_skel_clip_set: what prepare wrote (row_off, table, zero_pose_obj; DEVICE).
 *      clips int32 [2][B] (DEVICE) = video | first row; window b holds the T <= 128 consecutive rows from first row on.  Writes body [B,T,J,3],
 *      obj [B,T,P,3], pose [B,T,7], zero_pose_obj [B,P,3] -- the collated tuple of data/dataset_skeleton.py:157-158 -- and the token
 *      gt [B,1,3J+3P+7,T] of model/diffusion_skeleton.py:206 as train_diffusion_skeleton.py permutes it.  The caller checks that the rows lie inside
 *      the video; a window whose rows do not is skipped (nothing of it is written), never dereferenced.
 *  Returns: IDF_OK; IDF_E_INVAL (null pointer, a count <= 0, P > 64, T > 128, a T x (3J+3P+7) tile beyond 64 KiB of LDS); IDF_E_LAUNCH.
 * ---------------------------------------------------------------------------------- */
typedef struct {
    int32_t n_video, J, P, reserved;
    const int64_t *row_off;
    const float *table, *zero_pose_obj;
} idf_skel_clip_set;
typedef struct {
    float *body, *obj, *pose, *zero_pose_obj, *gt;
} idf_skel_window_batch;
int interdiff_skeleton_video_prepare(const double *skel, const double *obj, const double *pose, const double *contact, const int64_t *seq_off,
                                     const int64_t *row_off, int32_t n_video, int32_t J, int32_t P, int32_t stride, float *table, float *zero_pose_obj,
                                     double *report, double *row_contact, int8_t *signs, void *stream);
int interdiff_debug_skeleton_video_prepare(const double *skel, const double *obj, const double *pose, const double *contact, int64_t F, int32_t J, int32_t P,
                                           int32_t stride, float *table, float *zero_pose_obj, double *report, double *row_contact, int8_t *signs);
int interdiff_skeleton_window_batch(const idf_skel_clip_set *cs, const int32_t *clips, int32_t B, int32_t T, const idf_skel_window_batch *out, void *stream);

/* ------------------------------------------------------------------------------------
 * Live per-kernel timing for bench.py's `roofline` block (not on the product path).
 * Between profile_begin and profile_end every kernel launch of the library is preceded by a
 * hipEventRecord on its stream; profile_end synchronises and attributes the time between
 * consecutive events to the kernel kind of the first (IDF_K_*).  ms/count arrays have
 * IDF_K_COUNT entries.
 * ---------------------------------------------------------------------------------- */
enum {
    IDF_K_EMBED = 0, IDF_K_GEMM_QKV, IDF_K_SELF_ATTN, IDF_K_GEMM_OUTPROJ, IDF_K_ROWBLOCK_QAN,
    IDF_K_ROWBLOCK_STD, IDF_K_FFN_FUSED, IDF_K_RESERVED7, IDF_K_GEMM_HEADS, IDF_K_MEM_PREP,
    IDF_K_INPAINT, IDF_K_POSTERIOR, IDF_K_CORR_PREPARE, IDF_K_SMPL_POSE, IDF_K_SMPL_BLEND_SKIN,
    IDF_K_CORR_CONTACT, IDF_K_CORR_REDUCE, IDF_K_OBJPROJ, IDF_K_CORR_BLEND, IDF_K_OTHER,
    IDF_K_COUNT
};
int interdiff_profile_begin(int32_t capacity);
int interdiff_profile_end(double *ms_per_kind, int64_t *count_per_kind);

/* indices into idf_mdm_weights.tune; indices 0-2 and 5-7 are reserved and must be zero (they held the retired A/B overrides
 * IDF_TUNE_GEMM_EMBED / _QKV / _OUTPROJ / _HEADS, IDF_TUNE_CONTACT and IDF_TUNE_MISC) */
enum {
    IDF_TUNE_FFN = 3, IDF_TUNE_FFN_MATH = 4, IDF_TUNE_COUNT = 8
};

#ifdef __cplusplus
}
#endif
#endif /* INTERDIFF_HIP_H */
