// Training of the PointNet++ object encoder under BATCH statistics: PointNet2Encoder.forward (model/layers.py:141-175) as MDM._get_embeddings calls it
// (model/diffusion_smpl.py:210-211) with the module in train() -- the regime Lightning puts LitInteraction.model in -- and its backward.  Each of the twelve BatchNorm2d
// sites normalises with the mean and biased variance of its whole tensor ([B, C, 1024, nsample] in SA1: every centre counts, padding slots and repeated FPS positions
// as often as they occur), back-propagates through them, and moves its running statistics.
//
// Every site is a reduction over the whole batch, so the network is cut at the sites into launches (no grid barrier, as csrc/stgcn_bn_train.h does it):
//   forward   1. pnbt_sample_kernel     one workgroup per clip: FPS (pointnet2_train.h, the eval encoder's), both SA1 ball queries of ALL 1024 positions (one wave per
//                                       centre, ballot + popcount prefix in index order), the SA2 slot lists
//             2. pnbt_dense_kernel<0..2> + pnbt_finish_kernel   one statistic phase per SA1 layer: tiles of 64 rows recompute the layers below from the points and the
//                                       already-final statistics (the 786 k x B rows of activations are never stored); per tile (mean, M2) by a wave reduction, merged
//                                       per workgroup and then over the workgroups in index order by Chan's formula in double; mean and 1 / sigma rounded to fp32 once
//             3. pnbt_live_fwd_kernel   the <= 48 centres per clip the key point groups: their SA1 output, pool winners, x^ at the winner
//             4. pnbt_sa2_fwd_kernel    SA2 for the whole batch, one workgroup per scale (B * 16 and B * 32 rows): its six sites in place
//             5. pnbt_lin_kernel        Linear 256 -> 253 behind the key point's xyz
//   backward  1. pnbt_lin_bwd_kernel, pnbt_sa2_bwd_kernel (batch-statistic terms included), pnbt_slot_bwd_kernel + pnbt_slot_fin_kernel (pool and third-layer step at the
//                                       live slots: sum d, sum d x^ of SA1's third sites)
//             2. pnbt_dense_kernel<3..5> + pnbt_finish_kernel   dz = (gamma / sigma)(d - mean(d) - x^ mean(d x^)) couples every row of a site, so from SA1's third layer
//                                       downwards the gradient is dense: one phase per site recomputes the forward of its tile, carries the gradient down to the site,
//                                       and yields dW of the layer above and (sum d, sum d x^) of the site -- per tile in fp32 in a fixed order, across tiles and
//                                       workgroups in double in index order.  d gamma = sum d x^, d beta = sum d; the gradients are those of the RAW tensors (no fold).
//   statistics  pnbt_stats_kernel       running = (1 - momentum) running + momentum batch (variance unbiased, n / (n - 1)), in double, rounded once
// Form of the hot path: VALU.  Lane = row, wave-uniform output channel: weights and constants come by scalar loads, activations from LDS rows of odd stride; plain fmaf
// chains with channels ascending (pointnet2_bn_train.h).  The v_mfma_f32_16x16x4_f32 form was not built and not measured.
// No float atomics; reductions in fixed orders: two calls give the same bits, the gradient is linear in d_pc bit for bit under a power-of-two factor, and d_pc = 0 (or
// a d_pc confined to columns 0..2, which no parameter reaches) gives exact zeros.  20 launches for a forward + backward, 1 for the statistics.
#include "pointnet2_bn_train.h"

namespace {

using namespace pnbt;

constexpr int SL_POS = 0, SL_DUP = 48, SL_HITS = 96, SLW = 100;       // per-clip slot record, ints: FPS position of each SA2 slot, the first slot with that position, hits
constexpr int SA2_ROW = 99 + 3 * (64 + 96 + 128);                     // floats per SA2 row: xin | x^, a, d of the three layers at their widest
constexpr double BN_EPS = 1e-5;

__device__ __forceinline__ int site_off(const Layer &y) { return y.stat >> 1; }

struct Ws { size_t fpid, nb0, nb1, slot, slotof, bnf, bstat, part, feat1, h3w, win1, dslot, dfeat, lpart, f2, win2, df2, sa2[2], bytes; };
Ws workspace(int B) {
    Ws w;
    size_t at = 0;
    auto take = [&](size_t n) { const size_t o = at; at = idf_align(at + n); return o; };
    const size_t nc = (size_t)B * NP1;
    w.fpid = take(nc * 2); w.nb0 = take(nc * NS0 * 2); w.nb1 = take(nc * NS1 * 2);
    w.slot = take((size_t)B * SLW * 4); w.slotof = take(nc * 2);
    w.bnf = take(4 * NCH * 4); w.bstat = take(2 * NCH * 8);
    w.part = take((size_t)2 * G_MAX * P_STRIDE * 8);
    const size_t nf = (size_t)B * NSLOT * F1;
    w.feat1 = take(nf * 4); w.h3w = take(nf * 4); w.win1 = take(nf); w.dslot = take(nf * 4); w.dfeat = take(nf * 4);
    w.lpart = take((size_t)B * 2 * F1 * 8);
    w.f2 = take((size_t)B * 256 * 4); w.win2 = take((size_t)B * 256 * 4); w.df2 = take((size_t)B * 256 * 4);
    w.sa2[0] = take((size_t)B * NS0 * SA2_ROW * 4); w.sa2[1] = take((size_t)B * NS1 * SA2_ROW * 4);
    w.bytes = at;
    return w;
}

// ---------------------------------------------------------------------------------------------------------------------------------- sampling and grouping
__global__ __launch_bounds__(PT) void pnbt_sample_kernel(const float *__restrict__ obj_points, int P, unsigned short *__restrict__ fpid, unsigned short *__restrict__ nb0,
                                                         unsigned short *__restrict__ nb1, int *__restrict__ slot, short *__restrict__ slotof) {
    __shared__ float4 pts[MAXP];
    __shared__ unsigned short fps[NP1];
    __shared__ float redv[2][NWV];
    __shared__ int redi[2][NWV];
    __shared__ unsigned wcount[NWV];
    __shared__ int list[NSLOT], dup[NSLOT];
    __shared__ short sof[NP1];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = wave_id();
    for (int i = tid; i < MAXP; i += PT) {
        float x = 0.f, y = 0.f, z = 0.f;
        if (i < P) { const float *p = obj_points + ((size_t)b * P + i) * 3; x = p[0]; y = p[1]; z = p[2]; }
        pts[i] = make_float4(x, y, z, 0.f);
    }
    __syncthreads();
    fps_sample(pts, P, fps, redv, redi);
    __syncthreads();
    int tot0, tot1;
    sa2_slots(pts, fps, list, wcount, tot0, tot1);
    fpid[(size_t)b * NP1 + tid] = fps[tid];
    sof[tid] = -1;
    if (tid < NSLOT) {
        int d = tid;
        for (int e = 0; e < tid; ++e)
            if (list[e] == list[tid]) { d = e; break; }
        dup[tid] = d;
        slot[b * SLW + SL_POS + tid] = list[tid];
        slot[b * SLW + SL_DUP + tid] = d;
    }
    if (tid == 0) { slot[b * SLW + SL_HITS] = tot0; slot[b * SLW + SL_HITS + 1] = tot1; }
    __syncthreads();
    if (tid < NSLOT && dup[tid] == tid) sof[list[tid]] = (short)tid;
    __syncthreads();
    slotof[(size_t)b * NP1 + tid] = sof[tid];

    // both SA1 ball queries of every position: one wave per centre, the cloud 64 points at a time in index order (the lists block_rank gives), until both lists are
    // full.  c0 / c1 (wave-uniform) then hold the hits seen so far, exact wherever a list has padding slots; no kernel needs the full counts, so none are kept.
    const float ra = 0.05f, rb = 0.1f;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int k = 0; k < 64; ++k) {
        const int j = wave * 64 + k;
        const size_t ci = (size_t)b * NP1 + j;
        const float4 pc = pts[fps[j]];
        int c0 = 0, c1 = 0, first0 = 0, first1 = 0;
        for (int base = 0; base < P && (c0 < NS0 || c1 < NS1); base += 64) {
            const int i = base + lane;
            const float4 p = pts[i];
            const float d2 = d2_exact(pc.x, pc.y, pc.z, p.x, p.y, p.z);
            const bool h0 = i < P && d2 < ra * ra, h1 = i < P && d2 < rb * rb;
            const unsigned long long m0 = __ballot(h0), m1 = __ballot(h1);
            const int r0 = c0 + __popcll(m0 & below), r1 = c1 + __popcll(m1 & below);
            if (h0 && r0 < NS0) nb0[ci * NS0 + r0] = (unsigned short)i;
            if (h1 && r1 < NS1) nb1[ci * NS1 + r1] = (unsigned short)i;
            if (c0 == 0 && m0) first0 = base + __builtin_ctzll(m0);
            if (c1 == 0 && m1) first1 = base + __builtin_ctzll(m1);
            c0 += __popcll(m0);
            c1 += __popcll(m1);
        }
        if (lane < NS0 && lane >= c0) nb0[ci * NS0 + lane] = (unsigned short)first0;       // padding slots repeat the first hit (0 when there is none)
        if (lane < NS1 && lane >= c1) nb1[ci * NS1 + lane] = (unsigned short)first1;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------- SA1, all rows
// dW[o][c] += sum_n D[n][o] Ain[n][c] over the tile's rows (n ascending, fp32), added to the thread's double accumulators
template <int NT>
__device__ __forceinline__ void grad_w(const float *D, int sd, const float *Ain, int sa, int cin, int cout, double (&acc)[8]) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int idx = threadIdx.x + NT * k;
        if (idx < cin * cout) {
            const int o = idx / cin, c = idx - o * cin;
            float s = 0.f;
            for (int n = 0; n < TR; ++n) s = fmaf(D[n * sd + o], Ain[n * sa + c], s);
            acc[k] += (double)s;
        }
    }
}

struct DenseArgs {
    const float *theta, *obj_points;
    const unsigned short *fpid, *nb0, *nb1;
    const float *bnf;
    const short *slotof;
    const unsigned char *win1;
    const float *feat1, *dfeat;
    double *part;
    int P, B, G;
};

// PH 0..2: the statistics of SA1's layer PH + 1.  PH 3..5: the backward down to layer 6 - PH: its dW, and (sum d, sum d x^) of the site below.
template <int PH>
__global__ __launch_bounds__(256) void pnbt_dense_kernel(const Plan pl, const DenseArgs a) {
    constexpr int NW = 4;
    __shared__ float X[TR * 5], H1[TR * 33], A1[TR * 33], H2[TR * 33], A2[TR * 33], H3[TR * 65], D2[TR * 33];
    __shared__ double accA[64], accB[64];
    const int sc = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = wave_id();
    const int ns = sc ? NS1 : NS0;
    const Layer l1 = pl.ly[3 * sc], l2 = pl.ly[3 * sc + 1], l3 = pl.ly[3 * sc + 2];
    const int c1 = l1.cout, c2 = l2.cout, c3 = l3.cout, s1 = c1 + 1, s2 = c2 + 1, s3 = c3 + 1;
    const float *th = a.theta, *bn = a.bnf;
    const float *W1 = th + l1.raw_w, *W2 = th + l2.raw_w, *W3 = th + l3.raw_w;
    const int o1 = site_off(l1), o2 = site_off(l2), o3 = site_off(l3);
    const int tiles = a.B * NP1 * ns / TR;
    double dw[8] = {0., 0., 0., 0., 0., 0., 0., 0.};
    if (tid < 64) accA[tid] = accB[tid] = 0.0;
    int ntile = 0;

    // the statistic of one layer on this tile: per channel (mean, M2) of the 64 rows by a wave reduction, merged into the workgroup's running pair (Chan, double)
    auto stat = [&](const float *in, int sin, const float *W, int cin, int cout) {
        const double na = 64.0 * ntile, tot = na + 64.0;
        for (int o = wave; o < cout; o += NW) {
            const float z = dotrow(W + (size_t)o * cin, in + lane * sin, cin);
            const float mean = wave_sum(z) * (1.0f / 64.0f), d = z - mean;
            const float m2 = wave_sum(d * d);
            if (lane == 0) {
                const double delta = (double)mean - accA[o];
                accA[o] += delta * 64.0 / tot;
                accB[o] += (double)m2 + delta * delta * na * 64.0 / tot;
            }
        }
    };

    for (int tile = blockIdx.x; tile < tiles; tile += a.G, ++ntile) {
        __syncthreads();
        const int row = tile * TR + lane, ci = row / ns, n = row - ci * ns, b = ci >> 10;
        if (tid < TR) row_input(a.obj_points + (size_t)b * a.P * 3, a.fpid[ci], sc ? a.nb1[(size_t)ci * NS1 + n] : a.nb0[(size_t)ci * NS0 + n], X + lane * 5);
        __syncthreads();
        if (PH == 0) { stat(X, 5, W1, 4, c1); continue; }
        layer_rows<NW>(X, 5, W1, 4, c1, bn + o1, bn + NCH + o1, th + l1.raw_g, th + l1.raw_b, H1, A1, s1);
        __syncthreads();
        if (PH == 1) { stat(A1, s1, W2, c1, c2); continue; }
        layer_rows<NW>(A1, s1, W2, c1, c2, bn + o2, bn + NCH + o2, th + l2.raw_g, th + l2.raw_b, H2, A2, s2);
        __syncthreads();
        if (PH == 2) { stat(A2, s2, W3, c2, c3); continue; }
        layer_rows<NW>(A2, s2, W3, c2, c3, bn + o3, bn + NCH + o3, th + l3.raw_g, th + l3.raw_b, H3, nullptr, s3);
        // d z3 in place (the thread that wrote an element turns it): d y3 lives at the pool winners of the centres the key point groups
        {
            const int slot = a.slotof[ci];
            const size_t at = ((size_t)b * NSLOT + (slot < 0 ? 0 : slot)) * F1 + sc * 32;
            const float *g3 = th + l3.raw_g;
            for (int o = wave; o < c3; o += NW) {
                float d = 0.f;
                if (slot >= 0 && a.win1[at + o] == n && a.feat1[at + o] > 0.f) d = a.dfeat[at + o];
                H3[lane * s3 + o] = bn_back(d, H3[lane * s3 + o], g3[o], bn[NCH + o3 + o], bn[2 * NCH + o3 + o], bn[3 * NCH + o3 + o]);
            }
        }
        __syncthreads();
        if (PH == 3) grad_w<256>(H3, s3, A2, s2, c2, c3, dw);
        {
            const float *g2 = th + l2.raw_g;
            for (int c = wave; c < c2; c += NW) {
                float s = 0.f;
                for (int o = 0; o < c3; ++o) s = fmaf(H3[lane * s3 + o], W3[o * c2 + c], s);
                const float dy = A2[lane * s2 + c] > 0.f ? s : 0.f, h = H2[lane * s2 + c];
                if (PH == 3) {
                    const float S = wave_sum(dy), Q = wave_sum(dy * h);
                    if (lane == 0) { accA[c] += (double)S; accB[c] += (double)Q; }
                } else {
                    D2[lane * s2 + c] = bn_back(dy, h, g2[c], bn[NCH + o2 + c], bn[2 * NCH + o2 + c], bn[3 * NCH + o2 + c]);
                }
            }
        }
        if (PH == 3) continue;
        __syncthreads();
        if (PH == 4) grad_w<256>(D2, s2, A1, s1, c1, c2, dw);
        float *D1 = H3;                                                  // d z3 is spent
        {
            const float *g1 = th + l1.raw_g;
            for (int c = wave; c < c1; c += NW) {
                float s = 0.f;
                for (int o = 0; o < c2; ++o) s = fmaf(D2[lane * s2 + o], W2[o * c1 + c], s);
                const float dy = A1[lane * s1 + c] > 0.f ? s : 0.f, h = H1[lane * s1 + c];
                if (PH == 4) {
                    const float S = wave_sum(dy), Q = wave_sum(dy * h);
                    if (lane == 0) { accA[c] += (double)S; accB[c] += (double)Q; }
                } else {
                    D1[lane * s1 + c] = bn_back(dy, h, g1[c], bn[NCH + o1 + c], bn[2 * NCH + o1 + c], bn[3 * NCH + o1 + c]);
                }
            }
        }
        if (PH == 4) continue;
        __syncthreads();
        grad_w<256>(D1, s1, X, 5, 4, c1, dw);
    }
    __syncthreads();
    double *p = a.part + ((size_t)sc * a.G + blockIdx.x) * P_STRIDE;
    if (PH >= 3) {
        const Layer y = PH == 3 ? l3 : (PH == 4 ? l2 : l1);
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (tid + 256 * k < y.cin * y.cout) p[P_DW + tid + 256 * k] = dw[k];
    }
    if (tid < 64) { p[P_S + tid] = accA[tid]; p[P_Q + tid] = accB[tid]; }
    if (tid == 0) p[P_N] = 64.0 * ntile;
}

// the workgroups' partial records of one phase, merged in index order in double
__global__ __launch_bounds__(256) void pnbt_finish_kernel(int PH, const Plan pl, int B, int G, const double *__restrict__ part, float *__restrict__ bnf,
                                                          double *__restrict__ bstat, float *__restrict__ grads) {
    const int i = blockIdx.x * 256 + threadIdx.x, sc = blockIdx.y;
    const double *p = part + (size_t)sc * G * P_STRIDE;
    if (PH < 3) {
        const Layer y = pl.ly[3 * sc + PH];
        if (i < P_S || i >= P_S + y.cout) return;
        double n = 0.0, mean = 0.0, m2 = 0.0;
        for (int g = 0; g < G; ++g) {
            const double *q = p + (size_t)g * P_STRIDE;
            const double nb = q[P_N], delta = q[i] - mean, tot = n + nb;
            mean += delta * nb / tot;
            m2 += q[i + (P_Q - P_S)] + delta * delta * n * nb / tot;
            n = tot;
        }
        const double var = m2 / n;
        const int off = site_off(y) + (i - P_S);
        bnf[off] = (float)mean;
        bnf[NCH + off] = (float)(1.0 / sqrt(var + BN_EPS));
        bstat[off] = mean;
        bstat[NCH + off] = var;
        return;
    }
    const int l = 5 - PH;
    const Layer y = pl.ly[3 * sc + l];
    const bool is_w = i < y.cin * y.cout;
    int c = -1;
    bool is_q = false;
    if (!is_w) {
        if (l == 0) return;
        const int cb = pl.ly[3 * sc + l - 1].cout;
        if (i >= P_S && i < P_S + cb) c = i - P_S;
        else if (i >= P_Q && i < P_Q + cb) { c = i - P_Q; is_q = true; }
        else return;
    }
    double s = 0.0;
    for (int g = 0; g < G; ++g) s += p[(size_t)g * P_STRIDE + i];
    if (is_w) { grads[y.raw_w + i] = (float)s; return; }
    const Layer yb = pl.ly[3 * sc + l - 1];
    const double N = (double)B * NP1 * (sc ? NS1 : NS0);
    grads[(is_q ? yb.raw_g : yb.raw_b) + c] = (float)s;                  // d gamma = sum d x^, d beta = sum d
    bnf[(is_q ? 3 : 2) * NCH + site_off(yb) + c] = (float)(s / N);
}

// ---------------------------------------------------------------------------------------------------------------------------------- SA1, the live slots
__global__ __launch_bounds__(64) void pnbt_live_fwd_kernel(const Plan pl, const float *__restrict__ theta, const float *__restrict__ obj_points, int P,
                                                           const unsigned short *__restrict__ fpid, const unsigned short *__restrict__ nb0,
                                                           const unsigned short *__restrict__ nb1, const int *__restrict__ slot, const float *__restrict__ bnf,
                                                           float *__restrict__ feat1, float *__restrict__ h3w, unsigned char *__restrict__ win1) {
    __shared__ float X[TR * 5], H1[TR * 33], A1[TR * 33], H2[TR * 33], A2[TR * 33], H3[TR * 65];
    const int s = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    const int *sl = slot + b * SLW;
    if (sl[SL_DUP + s] != s) return;                                     // block-uniform: the slot repeats a position an earlier slot holds
    const size_t ci = (size_t)b * NP1 + sl[SL_POS + s];
    const float *pts = obj_points + (size_t)b * P * 3, *th = theta;
    for (int sc = 0; sc < 2; ++sc) {
        const int ns = sc ? NS1 : NS0, n = lane & (ns - 1);              // lanes beyond the ball evaluate a row again; their rows are never read
        const Layer l1 = pl.ly[3 * sc], l2 = pl.ly[3 * sc + 1], l3 = pl.ly[3 * sc + 2];
        const int c1 = l1.cout, c2 = l2.cout, c3 = l3.cout, s1 = c1 + 1, s2 = c2 + 1, s3 = c3 + 1;
        const int o1 = site_off(l1), o2 = site_off(l2), o3 = site_off(l3);
        __syncthreads();
        row_input(pts, fpid[ci], sc ? nb1[ci * NS1 + n] : nb0[ci * NS0 + n], X + lane * 5);
        __syncthreads();
        layer_rows<1>(X, 5, th + l1.raw_w, 4, c1, bnf + o1, bnf + NCH + o1, th + l1.raw_g, th + l1.raw_b, H1, A1, s1);
        __syncthreads();
        layer_rows<1>(A1, s1, th + l2.raw_w, c1, c2, bnf + o2, bnf + NCH + o2, th + l2.raw_g, th + l2.raw_b, H2, A2, s2);
        __syncthreads();
        layer_rows<1>(A2, s2, th + l3.raw_w, c2, c3, bnf + o3, bnf + NCH + o3, th + l3.raw_g, th + l3.raw_b, H3, nullptr, s3);
        __syncthreads();
        const float *g3 = th + l3.raw_g, *b3 = th + l3.raw_b;
        for (int o = lane; o < c3; o += 64) {                            // max pool over the samples: the first maximum wins
            float best = 0.f;
            int win = 0;
            for (int m = 0; m < ns; ++m) {
                const float v = bn_act(H3[m * s3 + o], g3[o], b3[o]);
                if (m == 0 || v > best) { best = v; win = m; }
            }
            const size_t at = ((size_t)b * NSLOT + s) * F1 + sc * 32 + o;
            feat1[at] = best;
            win1[at] = (unsigned char)win;
            h3w[at] = H3[win * s3 + o];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------- SA2 and the Linear
struct Sa2Buf { float *xin, *H[3], *A[3], *D[3]; };
__device__ __forceinline__ Sa2Buf sa2_buf(float *base, int R) {
    Sa2Buf u;
    float *p = base;
    u.xin = p; p += (size_t)R * CIN2;
    const int w[3] = {64, 96, 128};
    for (int l = 0; l < 3; ++l) { u.H[l] = p; p += (size_t)R * w[l]; u.A[l] = p; p += (size_t)R * w[l]; u.D[l] = p; p += (size_t)R * w[l]; }
    return u;
}

__global__ __launch_bounds__(PT) void pnbt_sa2_fwd_kernel(const Plan pl, const float *__restrict__ theta, const float *__restrict__ obj_points, int P, int B,
                                                          const unsigned short *__restrict__ fpid, const int *__restrict__ slot, const float *__restrict__ feat1,
                                                          float *sa2a, float *sa2b, float *__restrict__ bnf, double *__restrict__ bstat, float *__restrict__ f2,
                                                          int *__restrict__ win2) {
    __shared__ float smu[128], srs[128], Wt[96 * 128];
    __shared__ double red[8][128];
    const int sc = blockIdx.x, tid = threadIdx.x, ch = tid & 127, part = tid >> 7;
    const int ns = sc ? NS1 : NS0, s0 = sc ? NS0 : 0, R = B * ns;
    const Sa2Buf u = sa2_buf(sc ? sa2b : sa2a, R);
    for (int i = tid; i < R * CIN2; i += PT) {
        const int r = i / CIN2, c = i - r * CIN2, b = r / ns, s = s0 + (r - b * ns);
        const int *sl = slot + b * SLW;
        float v;
        if (c < 3) {
            const float *pts = obj_points + (size_t)b * P * 3;
            v = pts[(size_t)fpid[(size_t)b * NP1 + sl[SL_POS + s]] * 3 + c] - pts[c];         // relative to the key point: FPS starts at point 0
        } else {
            v = feat1[((size_t)b * NSLOT + sl[SL_DUP + s]) * F1 + c - 3];
        }
        u.xin[i] = v;
    }
    __syncthreads();
    for (int l = 0; l < 3; ++l) {
        const Layer y = pl.ly[6 + 3 * sc + l];
        const float *in = l ? u.A[l - 1] : u.xin, *W = theta + y.raw_w, *g = theta + y.raw_g, *be = theta + y.raw_b;
        float *H = u.H[l], *A = u.A[l];
        for (int i = tid; i < y.cout * y.cin; i += PT) {                 // the layer's weights, transposed: lanes read consecutive output channels
            const int o = i / y.cin, c = i - o * y.cin;
            Wt[c * y.cout + o] = W[i];
        }
        __syncthreads();
        for (int i = tid; i < R * y.cout; i += PT) {                     // dotrow's chain: c ascending from zero
            const int r = i / y.cout, o = i - r * y.cout;
            const float *x = in + (size_t)r * y.cin;
            float s = 0.f;
            for (int c = 0; c < y.cin; ++c) s = fmaf(Wt[c * y.cout + o], x[c], s);
            H[i] = s;
        }
        __syncthreads();
        // mean and biased variance over the R rows, two passes in double: eight threads per channel take every eighth row, their sums are added in order
        double acc = 0.0;
        if (ch < y.cout)
            for (int r = part; r < R; r += 8) acc += (double)H[(size_t)r * y.cout + ch];
        red[part][ch] = acc;
        __syncthreads();
        double mean = 0.0;
        for (int k = 0; k < 8; ++k) mean += red[k][ch];
        mean /= R;
        __syncthreads();
        acc = 0.0;
        if (ch < y.cout)
            for (int r = part; r < R; r += 8) { const double d = (double)H[(size_t)r * y.cout + ch] - mean; acc += d * d; }
        red[part][ch] = acc;
        __syncthreads();
        if (tid < y.cout) {
            double v = 0.0;
            for (int k = 0; k < 8; ++k) v += red[k][tid];
            const double var = v / R;
            const int off = site_off(y) + tid;
            smu[tid] = bnf[off] = (float)mean;
            srs[tid] = bnf[NCH + off] = (float)(1.0 / sqrt(var + BN_EPS));
            bstat[off] = mean;
            bstat[NCH + off] = var;
        }
        __syncthreads();
        for (int i = tid; i < R * y.cout; i += PT) {
            const int o = i % y.cout;
            const float h = bn_hat(H[i], smu[o], srs[o]);
            H[i] = h;
            A[i] = bn_act(h, g[o], be[o]);
        }
        __syncthreads();
    }
    for (int i = tid; i < B * 128; i += PT) {
        const int b = i >> 7, o = i & 127;
        float best = 0.f;
        int win = 0;
        for (int n = 0; n < ns; ++n) {
            const float v = u.A[2][((size_t)b * ns + n) * 128 + o];
            if (n == 0 || v > best) { best = v; win = n; }
        }
        f2[b * 256 + sc * 128 + o] = best;
        win2[b * 256 + sc * 128 + o] = win;
    }
}

__global__ __launch_bounds__(256) void pnbt_lin_kernel(const Plan pl, const float *__restrict__ theta, const float *__restrict__ obj_points, int P,
                                                       const float *__restrict__ f2, float *__restrict__ out) {
    const int b = blockIdx.x, tid = threadIdx.x;
    float *o = out + (size_t)b * 256;
    if (tid < 3) o[tid] = obj_points[(size_t)b * P * 3 + tid];
    if (tid < 253) {
        const float *w = theta + pl.raw_lin_w + (size_t)tid * 256, *x = f2 + (size_t)b * 256;
        float s = theta[pl.raw_lin_b + tid];
        for (int c = 0; c < 256; ++c) s = fmaf(w[c], x[c], s);
        o[3 + tid] = s;
    }
}

__global__ __launch_bounds__(256) void pnbt_lin_bwd_kernel(const Plan pl, const float *__restrict__ theta, int B, const float *__restrict__ d_pc,
                                                           const float *__restrict__ f2, float *__restrict__ grads, float *__restrict__ df2) {
    int i = blockIdx.x * 256 + threadIdx.x;
    if (i < 253 * 256) {
        const int o = i >> 8, c = i & 255;
        double s = 0.0;
        for (int b = 0; b < B; ++b) s += (double)(d_pc[b * 256 + 3 + o] * f2[b * 256 + c]);
        grads[pl.raw_lin_w + i] = (float)s;
        return;
    }
    i -= 253 * 256;
    if (i < 253) {
        double s = 0.0;
        for (int b = 0; b < B; ++b) s += (double)d_pc[b * 256 + 3 + i];
        grads[pl.raw_lin_b + i] = (float)s;
        return;
    }
    i -= 253;
    if (i < B * 256) {
        const int b = i >> 8, c = i & 255;
        const float *w = theta + pl.raw_lin_w + c;
        float s = 0.f;
        for (int o = 0; o < 253; ++o) s = fmaf(d_pc[b * 256 + 3 + o], w[(size_t)o * 256], s);
        df2[i] = s;
    }
}

__global__ __launch_bounds__(PT) void pnbt_sa2_bwd_kernel(const Plan pl, const float *__restrict__ theta, int B, float *sa2a, float *sa2b, const float *__restrict__ bnf,
                                                          const float *__restrict__ df2, const int *__restrict__ win2, float *__restrict__ grads,
                                                          float *__restrict__ dslot) {
    __shared__ float sm[128], sq[128];
    __shared__ double redS[8][128], redQ[8][128];
    const int sc = blockIdx.x, tid = threadIdx.x, ch = tid & 127, part = tid >> 7;
    const int ns = sc ? NS1 : NS0, s0 = sc ? NS0 : 0, R = B * ns;
    const Sa2Buf u = sa2_buf(sc ? sa2b : sa2a, R);
    for (int i = tid; i < R * 128; i += PT) {                            // the pool: d y3 at the winner, where it is positive
        const int r = i >> 7, o = i & 127, b = r / ns, n = r - b * ns, at = b * 256 + sc * 128 + o;
        u.D[2][i] = (win2[at] == n && u.A[2][i] > 0.f) ? df2[at] : 0.f;
    }
    __syncthreads();
    for (int l = 2; l >= 0; --l) {
        const Layer y = pl.ly[6 + 3 * sc + l];
        const float *in = l ? u.A[l - 1] : u.xin, *W = theta + y.raw_w, *g = theta + y.raw_g, *rs = bnf + NCH + site_off(y);
        float *D = u.D[l];
        const float *H = u.H[l];
        {                                                                // eight threads per channel take every eighth row; their sums are added in order
            double S = 0.0, Q = 0.0;
            if (ch < y.cout)
                for (int r = part; r < R; r += 8) {
                    const float d = D[(size_t)r * y.cout + ch];
                    S += (double)d;
                    Q += (double)(d * H[(size_t)r * y.cout + ch]);
                }
            redS[part][ch] = S;
            redQ[part][ch] = Q;
        }
        __syncthreads();
        if (tid < y.cout) {
            double S = 0.0, Q = 0.0;
            for (int k = 0; k < 8; ++k) { S += redS[k][tid]; Q += redQ[k][tid]; }
            grads[y.raw_b + tid] = (float)S;
            grads[y.raw_g + tid] = (float)Q;
            sm[tid] = (float)(S / R);
            sq[tid] = (float)(Q / R);
        }
        __syncthreads();
        for (int i = tid; i < R * y.cout; i += PT) {
            const int o = i % y.cout;
            D[i] = bn_back(D[i], H[i], g[o], rs[o], sm[o], sq[o]);
        }
        __syncthreads();
        for (int i = tid; i < y.cout * y.cin; i += PT) {
            const int o = i / y.cin, c = i - o * y.cin;
            double s = 0.0;
            for (int r = 0; r < R; ++r) s += (double)(D[(size_t)r * y.cout + o] * in[(size_t)r * y.cin + c]);
            grads[y.raw_w + i] = (float)s;
        }
        if (l > 0) {
            const float *Ab = u.A[l - 1];
            float *Db = u.D[l - 1];
            for (int i = tid; i < R * y.cin; i += PT) {
                const int r = i / y.cin, c = i - r * y.cin;
                float s = 0.f;
                for (int o = 0; o < y.cout; ++o) s = fmaf(D[(size_t)r * y.cout + o], W[(size_t)o * y.cin + c], s);
                Db[i] = Ab[i] > 0.f ? s : 0.f;
            }
        } else {
            for (int i = tid; i < R * F1; i += PT) {                     // d feat1 of the slot; the three relative-xyz channels reach no parameter
                const int r = i / F1, c = i - r * F1, b = r / ns, n = r - b * ns;
                float s = 0.f;
                for (int o = 0; o < y.cout; ++o) s = fmaf(D[(size_t)r * y.cout + o], W[(size_t)o * CIN2 + 3 + c], s);
                dslot[((size_t)b * NSLOT + s0 + n) * F1 + c] = s;
            }
        }
        __syncthreads();
    }
}

// per clip: the slots that repeat a position add into the first slot that holds it (slot order); the pool and third-layer step of SA1 at the live slots
__global__ __launch_bounds__(F1) void pnbt_slot_bwd_kernel(const int *__restrict__ slot, const float *__restrict__ dslot, const float *__restrict__ feat1,
                                                           const float *__restrict__ h3w, float *__restrict__ dfeat, double *__restrict__ lpart) {
    const int b = blockIdx.x, ch = threadIdx.x;
    const int *sl = slot + b * SLW;
    double S = 0.0, Q = 0.0;
    for (int s = 0; s < NSLOT; ++s) {
        if (sl[SL_DUP + s] != s) continue;
        float df = 0.f;
        for (int e = s; e < NSLOT; ++e)
            if (sl[SL_DUP + e] == s) df += dslot[((size_t)b * NSLOT + e) * F1 + ch];
        const size_t at = ((size_t)b * NSLOT + s) * F1 + ch;
        dfeat[at] = df;
        if (feat1[at] > 0.f) { S += (double)df; Q += (double)(df * h3w[at]); }
    }
    lpart[(size_t)b * 2 * F1 + ch] = S;
    lpart[(size_t)b * 2 * F1 + F1 + ch] = Q;
}

__global__ __launch_bounds__(F1) void pnbt_slot_fin_kernel(const Plan pl, int B, const double *__restrict__ lpart, float *__restrict__ bnf, float *__restrict__ grads) {
    const int ch = threadIdx.x, sc = ch < 32 ? 0 : 1, o = ch - sc * 32;
    double S = 0.0, Q = 0.0;
    for (int b = 0; b < B; ++b) { S += lpart[(size_t)b * 2 * F1 + ch]; Q += lpart[(size_t)b * 2 * F1 + F1 + ch]; }
    const Layer y = pl.ly[3 * sc + 2];
    const double N = (double)B * NP1 * (sc ? NS1 : NS0);
    grads[y.raw_b + o] = (float)S;
    grads[y.raw_g + o] = (float)Q;
    bnf[2 * NCH + site_off(y) + o] = (float)(S / N);
    bnf[3 * NCH + site_off(y) + o] = (float)(Q / N);
}

__global__ __launch_bounds__(256) void pnbt_stats_kernel(const Plan pl, int B, double momentum, const double *__restrict__ bstat, float *__restrict__ stats) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= NCH) return;
    int L = 0;
    while (L < 11 && i >= site_off(pl.ly[L + 1])) ++L;
    const Layer y = pl.ly[L];
    const int c = i - site_off(y);
    const double n = (double)B * (L < 6 ? NP1 : 1) * ((L / 3) & 1 ? NS1 : NS0);
    stats[y.stat + c] = (float)((1.0 - momentum) * (double)stats[y.stat + c] + momentum * bstat[i]);
    stats[y.stat + y.cout + c] = (float)((1.0 - momentum) * (double)stats[y.stat + y.cout + c] + momentum * (bstat[NCH + i] * n / (n - 1.0)));
}

const Plan &plan() {
    static const Plan p = make_plan();
    return p;
}

bool args_ok(const void *ws, int B, int P) { return ws && !(reinterpret_cast<uintptr_t>(ws) & 255) && B >= 1 && B <= MAXB && P >= 1 && P <= MAXP; }

DenseArgs dense_args(const Ws &w, char *base, const float *theta, const float *obj_points, int B, int P) {
    DenseArgs a;
    a.theta = theta; a.obj_points = obj_points;
    a.fpid = reinterpret_cast<unsigned short *>(base + w.fpid); a.nb0 = reinterpret_cast<unsigned short *>(base + w.nb0); a.nb1 = reinterpret_cast<unsigned short *>(base + w.nb1);
    a.bnf = reinterpret_cast<float *>(base + w.bnf);
    a.slotof = reinterpret_cast<short *>(base + w.slotof);
    a.win1 = reinterpret_cast<unsigned char *>(base + w.win1);
    a.feat1 = reinterpret_cast<float *>(base + w.feat1); a.dfeat = reinterpret_cast<float *>(base + w.dfeat);
    a.part = reinterpret_cast<double *>(base + w.part);
    a.P = P; a.B = B;
    a.G = B * 256 < G_MAX ? B * 256 : G_MAX;                             // never more workgroups than the smaller scale has tiles
    return a;
}

template <int PH>
void dense_phase(const Plan &pl, const DenseArgs &a, const Ws &w, char *base, float *grads, hipStream_t s) {
    hipLaunchKernelGGL(pnbt_dense_kernel<PH>, dim3(a.G, 2), dim3(256), 0, s, pl, a);
    hipLaunchKernelGGL(pnbt_finish_kernel, dim3((P_N + 255) / 256, 2), dim3(256), 0, s, PH, pl, a.B, a.G, a.part, reinterpret_cast<float *>(base + w.bnf),
                       reinterpret_cast<double *>(base + w.bstat), grads);
}

}  // namespace

extern "C" size_t interdiff_pointnet2_train_workspace_bytes(int32_t B) { return B >= 1 && B <= pnbt::MAXB ? workspace(B).bytes : 0; }

extern "C" int interdiff_pointnet2_train_forward(const float *theta, const float *obj_points, int32_t B, int32_t P, float *pc_out, void *ws, size_t ws_bytes,
                                                 void *stream) {
    if (!theta || !obj_points || !pc_out || !args_ok(ws, B, P)) return IDF_E_INVAL;
    if (ws_bytes < interdiff_pointnet2_train_workspace_bytes(B)) return IDF_E_NOMEM;
    const Plan &pl = plan();
    const Ws w = workspace(B);
    char *base = static_cast<char *>(ws);
    const DenseArgs a = dense_args(w, base, theta, obj_points, B, P);
    float *bnf = reinterpret_cast<float *>(base + w.bnf), *feat1 = reinterpret_cast<float *>(base + w.feat1), *f2 = reinterpret_cast<float *>(base + w.f2);
    double *bstat = reinterpret_cast<double *>(base + w.bstat);
    int *slot = reinterpret_cast<int *>(base + w.slot);
    hipStream_t s = idf_stream(stream);
    idf_prof_mark(IDF_K_OTHER, s);
    hipLaunchKernelGGL(pnbt_sample_kernel, dim3(B), dim3(PT), 0, s, obj_points, P, const_cast<unsigned short *>(a.fpid), const_cast<unsigned short *>(a.nb0),
                       const_cast<unsigned short *>(a.nb1), slot, const_cast<short *>(a.slotof));
    dense_phase<0>(pl, a, w, base, nullptr, s);
    dense_phase<1>(pl, a, w, base, nullptr, s);
    dense_phase<2>(pl, a, w, base, nullptr, s);
    hipLaunchKernelGGL(pnbt_live_fwd_kernel, dim3(NSLOT, B), dim3(64), 0, s, pl, theta, obj_points, P, a.fpid, a.nb0, a.nb1, slot, bnf, feat1,
                       reinterpret_cast<float *>(base + w.h3w), const_cast<unsigned char *>(a.win1));
    hipLaunchKernelGGL(pnbt_sa2_fwd_kernel, dim3(2), dim3(PT), 0, s, pl, theta, obj_points, P, B, a.fpid, slot, feat1, reinterpret_cast<float *>(base + w.sa2[0]),
                       reinterpret_cast<float *>(base + w.sa2[1]), bnf, bstat, f2, reinterpret_cast<int *>(base + w.win2));
    hipLaunchKernelGGL(pnbt_lin_kernel, dim3(B), dim3(256), 0, s, pl, theta, obj_points, P, f2, pc_out);
    idf_prof_mark(-1, s);
    IDF_CHECK_LAUNCH();
    return IDF_OK;
}

extern "C" int interdiff_pointnet2_train_grads(const float *theta, const float *obj_points, int32_t B, int32_t P, const float *d_pc, float *grads, void *ws,
                                               size_t ws_bytes, void *stream) {
    if (!theta || !obj_points || !d_pc || !grads || !args_ok(ws, B, P)) return IDF_E_INVAL;
    if (ws_bytes < interdiff_pointnet2_train_workspace_bytes(B)) return IDF_E_NOMEM;
    const Plan &pl = plan();
    const Ws w = workspace(B);
    char *base = static_cast<char *>(ws);
    const DenseArgs a = dense_args(w, base, theta, obj_points, B, P);
    float *bnf = reinterpret_cast<float *>(base + w.bnf), *f2 = reinterpret_cast<float *>(base + w.f2), *df2 = reinterpret_cast<float *>(base + w.df2);
    float *dslot = reinterpret_cast<float *>(base + w.dslot);
    double *lpart = reinterpret_cast<double *>(base + w.lpart);
    const int *slot = reinterpret_cast<int *>(base + w.slot);
    hipStream_t s = idf_stream(stream);
    idf_prof_mark(IDF_K_OTHER, s);
    hipLaunchKernelGGL(pnbt_lin_bwd_kernel, dim3((253 * 256 + 253 + B * 256 + 255) / 256), dim3(256), 0, s, pl, theta, B, d_pc, f2, grads, df2);
    hipLaunchKernelGGL(pnbt_sa2_bwd_kernel, dim3(2), dim3(PT), 0, s, pl, theta, B, reinterpret_cast<float *>(base + w.sa2[0]), reinterpret_cast<float *>(base + w.sa2[1]),
                       bnf, df2, reinterpret_cast<int *>(base + w.win2), grads, dslot);
    hipLaunchKernelGGL(pnbt_slot_bwd_kernel, dim3(B), dim3(F1), 0, s, slot, dslot, a.feat1, reinterpret_cast<float *>(base + w.h3w), const_cast<float *>(a.dfeat), lpart);
    hipLaunchKernelGGL(pnbt_slot_fin_kernel, dim3(1), dim3(F1), 0, s, pl, B, lpart, bnf, grads);
    dense_phase<3>(pl, a, w, base, grads, s);
    dense_phase<4>(pl, a, w, base, grads, s);
    dense_phase<5>(pl, a, w, base, grads, s);
    idf_prof_mark(-1, s);
    IDF_CHECK_LAUNCH();
    return IDF_OK;
}

extern "C" int interdiff_pointnet2_train_stats(const void *ws, int32_t B, double momentum, float *stats, void *stream) {
    if (!stats || !args_ok(ws, B, 1) || !(momentum >= 0.0 && momentum <= 1.0)) return IDF_E_INVAL;
    const Ws w = workspace(B);
    hipLaunchKernelGGL(pnbt_stats_kernel, dim3((NCH + 255) / 256), dim3(256), 0, idf_stream(stream), plan(), B, momentum,
                       reinterpret_cast<const double *>(static_cast<const char *>(ws) + w.bstat), stats);
    IDF_CHECK_LAUNCH();
    return IDF_OK;
}
