// HO-GCN skeleton mode: the correction predictor ObjProjector.sample (model/correction_skeleton.py:84-137) and the
// correction hook around it (eval_skeleton.py:82-111), device code.  Launchers: csrc/skeleton.hip.
//
// ONE 16-wave workgroup per clip walks the three ST-GCN stacks (model/layers.py:339-345, sublayers.py:415-419,511-516)
// without touching HBM, like the SMPL predictor (csrc/objproj.h), but the skeleton model does not fit that kernel's layout:
// n_pre = 20 DCT coefficients and a joint stack 9->64->32->64->9 over 22 nodes.  Input plus output planes of its 64->32 layer
// would be (64 + 32) x 20 x 22 x 4 B = 168 960 B, more than the 160 KiB of LDS a CU has.  So here every layer runs IN PLACE
// on one LDS buffer of max(cin, cout) planes:
//   1. the residual 1x1 convolution (BN folded) of the layer input goes to REGISTERS: each wave owns a fixed set of 16x16
//      (positions x output channels) tiles, at most SK_MAXT = 7 of them (28 fp32 per lane at the 440 x 64 layers),
//   2. the temporal (and, version 2, spatial) mixing overwrites the input planes in place,
//   3. the tcn 1x1 convolution reads them, adds bias and the residual tile held in registers, applies the PReLU -- still in registers,
//   4. after a barrier (nobody reads the input any more) the waves write their tiles over the buffer: the layer's output.
// LDS: the buffer 64 x 440 fp32 (112 640 B) + the stacks' output keep[9][20][22] (15 840 B) + 2 KiB of small scratch.
// Arithmetic: fp32 throughout; the 1x1 convolutions and the per-coefficient adjacency product on the fp32 MFMA, the 20x20
// temporal mix on the VALU.  The idx_pad repetition of the last past frame is folded into dct_pad [n_pre][past_len] (only the past
// pose rows and the past body frames enter the relative and object branches), and the IDCT is evaluated for node 0 only
// (correction_skeleton.py:130 reads nothing else).
// The ST-GCN layer's arena block and its three products (1x1 convolution tile, temporal mix, adjacency product): csrc/stgcn.h.
#pragma once
#include "stgcn.h"
#include "rot_math.h"

namespace idf_skel_dev {

using namespace idf_stgcn;

constexpr int NP = 20;                     // n_pre = T = past_len + future_len
constexpr int J = 21;                      // body joints
constexpr int NJ = J + 1;                  // joint stack: the object node + 21 joints
constexpr int VP = 32;                     // NJ padded to 2 MFMA tiles (adjacency operand only)
constexpr int CH = 9;                      // 6D rotation | translation
constexpr int MAXC = 64;                   // widest layer
constexpr int C_TOK = 106;                 // token channels: body 63 | object keypoints 36 | pose 7
constexpr int N_OBJ = 12;                  // object keypoints
constexpr int SK_MAXT = 7;                 // 16x16 output tiles per wave: ceil(440 / 16) x 64 / 16 = 112 = 7 x 16
constexpr int BUF = MAXC * NP * NJ;        // the in-place layer buffer
constexpr int KEEP = CH * NP * NJ;         // [9][n_pre][22]: node 0 = object, 1.. = joints
constexpr int SMALL = 512;
constexpr size_t SKEL_LDS = (size_t)(BUF + KEEP + SMALL) * sizeof(float);

// one ST-GCN layer in place on buf = channel-major planes [c][k][node] (plane = NP * nodes floats): cin planes in, cout planes out
template <bool V2>
__device__ inline void st_gcn_layer(float *buf, const LayerP &p, int cin, int cout, int nodes) {
    constexpr bool v2 = V2;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, kq = lane >> 4;
    const int npos = NP * nodes, NT = pad16(cout) >> 4, items = ((npos + 15) >> 4) * NT;
    float r[SK_MAXT][4];
    // 1. residual branch (BN folded) -> registers
#pragma unroll
    for (int j = 0; j < SK_MAXT; ++j) {
        const int item = wave + j * NWAVE;
        if (item < items) {
            const int mt = item / NT, nt = item - mt * NT;
            const f32x4 acc = conv_tile(buf, p.Wr, cin, npos, mt, nt);
            const float bv = p.br[nt * 16 + li];
#pragma unroll
            for (int q = 0; q < 4; ++q) r[j][q] = acc[q] + bv;
        }
    }
    __syncthreads();
    // 2. temporal and (version 2) spatial mixing overwrite the input planes in place
    temporal_mix<NP>(buf, p.Tm, cin, nodes, v2);
    __syncthreads();
    if (v2) {
        spatial_mix<NP, VP>(buf, p.AT, cin, nodes);
        __syncthreads();
    }
    // 3. tcn (BN folded) + bias + residual, PReLU -- in registers
    const float slope = p.prelu;
#pragma unroll
    for (int j = 0; j < SK_MAXT; ++j) {
        const int item = wave + j * NWAVE;
        if (item < items) {
            const int mt = item / NT, nt = item - mt * NT;
            const f32x4 acc = conv_tile(buf, p.Wt, cin, npos, mt, nt);
            const float bv = p.bt[nt * 16 + li];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float v = acc[q] + bv;
                v += r[j][q];
                r[j][q] = v >= 0.f ? v : slope * v;
            }
        }
    }
    __syncthreads();
    // 4. the layer output over the (no longer read) input planes
#pragma unroll
    for (int j = 0; j < SK_MAXT; ++j) {
        const int item = wave + j * NWAVE;
        if (item < items) {
            const int mt = item / NT, nt = item - mt * NT, o = nt * 16 + li;
            if (o < cout) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int pos = mt * 16 + kq * 4 + q;
                    if (pos < npos) buf[o * npos + pos] = r[j][q];
                }
            }
        }
    }
    __syncthreads();
}

// one 4-layer stack on the 9 input planes at buf[0 ..); its 9 output planes end up there
__device__ inline void run_stack(float *buf, const idf_skel_objproj &op, int stack, int nodes) {
#pragma unroll 1
    for (int l = 0; l < 4; ++l) {
        const int li = stack * 4 + l;
        const LayerP p = layer_params<NP, VP>(op.arena + op.layer[li], op.cin[li], op.cout[li], nodes, stack == 2);
        if (stack == 2) st_gcn_layer<true>(buf, p, op.cin[li], op.cout[li], nodes);
        else st_gcn_layer<false>(buf, p, op.cin[li], op.cout[li], nodes);
    }
}

// Where a clip's inputs are.  HOOK: x / gt [B][106][T] token planes (body = x channels 0..62, past pose = gt channels 99..105),
// zero_pose_obj [B][12][3], output [B][106][T].  Otherwise (ObjProjector.sample): angles [T][B][4] xyzw, trans [T][B][3],
// human [T][B][21][3] -> quat_out [T][B][4] xyzw, trans_out [T][B][3].
struct Src {
    const float *x, *gt, *zpo;
    const float *angles, *trans, *human;
    float *out, *quat_out, *trans_out;
    float blend_t;
};

template <bool HOOK>
__device__ __forceinline__ float human_at(const Src &s, int B, int b, int t, int p, int d) {
    if constexpr (HOOK) return s.x[((size_t)b * C_TOK + p * 3 + d) * NP + t];
    else return s.human[(((size_t)t * B + b) * J + p) * 3 + d];
}

// the whole predictor (+ calc_obj_pred and the blend when HOOK) for clip b; all NTHR threads call it together; sm: SKEL_LDS bytes
template <bool HOOK>
__device__ __forceinline__ void skel_body(float *sm, const idf_skel_objproj &op, const Src &s, int B, int b) {
    float *buf = sm, *keep = sm + BUF, *small = keep + KEEP;
    float *og6 = small;                 // [past][9]  past object pose as 6D | translation
    float *og = small + 96;             // [9][NP]    its DCT (idx_pad folded)
    float *res = small + 288;           // [NP][9]    IDCT of node 0
    const int tid = threadIdx.x, past = op.past_len;
    const float *Dp = op.arena + op.dct_pad, *Df = op.arena + op.dct, *Di = op.arena + op.idct;

    // ---- past object pose: quaternion xyzw -> (w,x,y,z) -> matrix -> 6D (correction_skeleton.py:89-90)
    if (tid < past) {
        const int t = tid;
        float q[4], tr[3], m[9];
        if constexpr (HOOK) {
            const float *g = s.gt + (size_t)b * C_TOK * NP + t;
            q[0] = g[105 * NP]; q[1] = g[102 * NP]; q[2] = g[103 * NP]; q[3] = g[104 * NP];
            tr[0] = g[99 * NP]; tr[1] = g[100 * NP]; tr[2] = g[101 * NP];
        } else {
            const float *a = s.angles + ((size_t)t * B + b) * 4, *tt = s.trans + ((size_t)t * B + b) * 3;
            q[0] = a[3]; q[1] = a[0]; q[2] = a[1]; q[3] = a[2];
            tr[0] = tt[0]; tr[1] = tt[1]; tr[2] = tt[2];
        }
        rot::quaternion_to_matrix(q, m);
#pragma unroll
        for (int c = 0; c < 6; ++c) og6[t * CH + c] = m[c];
#pragma unroll
        for (int c = 0; c < 3; ++c) og6[t * CH + 6 + c] = tr[c];
    }
    __syncthreads();
    for (int i = tid; i < CH * NP; i += NTHR) {
        const int c = i / NP, k = i - c * NP;
        float a = 0.f;
        for (int t = 0; t < past; ++t) a += Dp[k * past + t] * og6[t * CH + c];
        og[i] = a;
    }
    __syncthreads();
    // ---- relative branch input rel[c][k][p] -> buf (plane NP*J) and keep[.][.][1+p]
    for (int i = tid; i < CH * NP * J; i += NTHR) {
        const int c = i / (NP * J), r = i - c * NP * J, k = r / J, p = r - k * J;
        float v = og[c * NP + k];
        if (c >= 6) {
            float a = 0.f;
            for (int t = 0; t < past; ++t) a += Dp[k * past + t] * human_at<HOOK>(s, B, b, t, p, c - 6);
            v -= a;
        }
        buf[i] = v;
        keep[c * NP * NJ + k * NJ + 1 + p] = v;
    }
    __syncthreads();
    run_stack(buf, op, 0, J);
    // rel' = rel + stack(rel);  multi = [rel'[:6], rel'[6:] + DCT(body over ALL frames)]
    for (int i = tid; i < CH * NP * J; i += NTHR) {
        const int c = i / (NP * J), r = i - c * NP * J, k = r / J, p = r - k * J;
        float *kp = keep + c * NP * NJ + k * NJ + 1 + p;
        float v = *kp + buf[i];
        if (c >= 6) {
            float a = 0.f;
            for (int t = 0; t < NP; ++t) a += Df[k * NP + t] * human_at<HOOK>(s, B, b, t, p, c - 6);
            v += a;
        }
        *kp = v;
    }
    __syncthreads();
    // ---- object-only branch (1 node)
    for (int i = tid; i < CH * NP; i += NTHR) buf[i] = og[i];
    __syncthreads();
    run_stack(buf, op, 1, 1);
    for (int i = tid; i < CH * NP; i += NTHR) {
        const int c = i / NP, k = i - c * NP;
        keep[c * NP * NJ + k * NJ] = og[i] + buf[i];
    }
    __syncthreads();
    // ---- joint branch over the 22 nodes
    for (int i = tid; i < KEEP; i += NTHR) buf[i] = keep[i];
    __syncthreads();
    run_stack(buf, op, 2, NJ);
    for (int i = tid; i < KEEP; i += NTHR) keep[i] += buf[i];
    __syncthreads();
    // ---- IDCT of node 0 (correction_skeleton.py:129-130)
    for (int i = tid; i < NP * CH; i += NTHR) {
        const int t = i / CH, c = i - t * CH;
        float a = 0.f;
#pragma unroll
        for (int k = 0; k < NP; ++k) a += Di[t * NP + k] * keep[c * NP * NJ + k * NJ];
        res[i] = a;
    }
    __syncthreads();
    // ---- 6D -> matrix -> quaternion (w,x,y,z) -> xyzw (:132-133)
    float *pose = buf;                  // HOOK: [NP][7] = translation | quaternion xyzw (pose_proj, eval_skeleton.py:101)
    float *R = buf + NP * 8;            // HOOK: [NP][9] rotation of pose_proj (calc_obj_pred, :34-44)
    if (tid < NP) {
        const int t = tid;
        float m[9], q[4];
        rot::rot6d_to_matrix(res + t * CH, m);
        rot::matrix_to_quaternion(m, q);
        const float *tr = res + t * CH + 6;
        if constexpr (HOOK) {
            float *pp = pose + t * 8;
            pp[0] = tr[0]; pp[1] = tr[1]; pp[2] = tr[2];
            pp[3] = q[1]; pp[4] = q[2]; pp[5] = q[3]; pp[6] = q[0];
            rot::quaternion_to_matrix(q, R + t * 9);      // calc_obj_pred reads the quaternion back as (w, x, y, z) = (pp[6], pp[3..5]) = q
        } else {
            float *qo = s.quat_out + ((size_t)t * B + b) * 4, *to = s.trans_out + ((size_t)t * B + b) * 3;
            qo[0] = q[1]; qo[1] = q[2]; qo[2] = q[3]; qo[3] = q[0];
            to[0] = tr[0]; to[1] = tr[1]; to[2] = tr[2];
        }
    }
    if constexpr (HOOK) {
        __syncthreads();
        // ---- blend (eval_skeleton.py:111): out = w x + (1 - w) x_,  x_ = [body (x itself), R zero_pose_obj + trans, pose_proj]
        const float w = s.blend_t, w1 = 1.0f - w;
        const float *xb = s.x + (size_t)b * C_TOK * NP, *z = s.zpo + (size_t)b * N_OBJ * 3;
        float *ob = s.out + (size_t)b * C_TOK * NP;
        for (int i = tid; i < C_TOK * NP; i += NTHR) {
            const int c = i / NP, t = i - c * NP;
            const float xv = xb[i];
            float xp;
            if (c < 3 * J) {
                xp = xv;
            } else if (c < 3 * J + 3 * N_OBJ) {
                const int n = (c - 3 * J) / 3, d = (c - 3 * J) - 3 * n;
                const float *Rt = R + t * 9 + d * 3, *zn = z + n * 3;
                xp = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(Rt[0], zn[0]), __fmul_rn(Rt[1], zn[1])), __fmul_rn(Rt[2], zn[2])), pose[t * 8 + d]);
            } else {
                xp = pose[t * 8 + (c - 3 * J - 3 * N_OBJ)];
            }
            ob[i] = __fadd_rn(__fmul_rn(w, xv), __fmul_rn(w1, xp));
        }
    }
}

}  // namespace idf_skel_dev
