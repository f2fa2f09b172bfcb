// Fine-tuning of the PointNet++ object encoder (frozen normalisation statistics): the backward of PointNet2Encoder.forward (model/layers.py:141-175) as
// MDM._get_embeddings calls it (model/diffusion_smpl.py:210-211) with the module in eval() and autograd on, and the device re-fold of eval BatchNorm.
//
// The forward (csrc/pointnet2.hip, SAVE = true) kept every decision: which 48 SA1 centres the key point groups, which points each centre groups.  The backward
// runs no sampling and no ball query; it recomputes the activations of the live path from those records with the forward's own expression (mlp_layer), so
// ReLU masks and pool winners are the forward's.  It differentiates the FOLDED form (W' = W gamma / sigma, b' = beta - mu gamma / sigma) and unfolds on the device:
//     dW = dW' gamma / sigma (per row),   dgamma = (sum_c dW'[o,c] W[o,c] - db'[o] mu[o]) / sigma[o],   dbeta = db'.
// Launches:  1. pn_sa2_bwd_kernel   one workgroup per clip: Linear, SA2 pools and layers; writes the clip's SA2 / Linear gradient and d feat1 per distinct centre
//            2. pn_sa1_bwd_kernel   one workgroup per (clip, slot); slots that repeat a centre return at once: SA1 pools and layers of one centre
//            3. pn_fold_kernel      per folded parameter: the clips (and centres) added in index order, in double
//            4. pn_unfold_kernel    per raw parameter: the unfold above, in double
// fp32 products and sums in a fixed order, no atomics: two calls give the same bits, the result is linear in d_pc bit for bit under a power-of-two factor.
#include "pointnet2_train.h"

namespace {

using namespace pn2;

constexpr int NT1 = 256;                       // threads of the SA1 workgroup
constexpr double BN_EPS = 1e-5;

// gW[o][c] = sum_n dz[n][o] ain[n][c],  gb[o] = sum_n dz[n][o]   (n ascending)
template <int NT>
__device__ __forceinline__ void grad_weights(const float *dz, int dz_stride, const float *ain, int ain_stride, int cin, int cout, int ns, float *__restrict__ gW,
                                             float *__restrict__ gb) {
    for (int i = threadIdx.x; i < cout * cin; i += NT) {
        const int o = i / cin, c = i - o * cin;
        float s = 0.f;
        for (int n = 0; n < ns; ++n) s += dz[n * dz_stride + o] * ain[n * ain_stride + c];
        gW[i] = s;
    }
    for (int o = threadIdx.x; o < cout; o += NT) {
        float s = 0.f;
        for (int n = 0; n < ns; ++n) s += dz[n * dz_stride + o];
        gb[o] = s;
    }
}

// out[n][c] = [ain[n][c] > 0] sum_o dz[n][o] W[o][c]   (o ascending): the gradient at the previous layer's pre-activation
template <int NT>
__device__ __forceinline__ void grad_input(const float *dz, int dz_stride, const float *__restrict__ W, int cin, int cout, int ns, const float *ain, int ain_stride,
                                           float *out, int out_stride) {
    for (int i = threadIdx.x; i < ns * cin; i += NT) {
        const int n = i / cin, c = i - n * cin;
        float s = 0.f;
        for (int o = 0; o < cout; ++o) s += dz[n * dz_stride + o] * W[(size_t)o * cin + c];
        out[n * out_stride + c] = ain[n * ain_stride + c] > 0.f ? s : 0.f;
    }
}

// a[n][o] (post-ReLU, pooled over n) -> in place the gradient at the last layer's pre-activation: d[o] at the first n that holds the maximum when that maximum
// is positive, zero elsewhere
template <int NT>
__device__ __forceinline__ void pool_backward(float *a, int stride, int ns, int cout, const float *d) {
    for (int o = threadIdx.x; o < cout; o += NT) {
        float m = a[o];
        int win = 0;
        for (int n = 1; n < ns; ++n) {
            const float v = a[n * stride + o];
            if (v > m) { m = v; win = n; }
        }
        for (int n = 0; n < ns; ++n) a[n * stride + o] = (n == win && m > 0.f) ? d[o] : 0.f;
    }
}

__global__ __launch_bounds__(PT) void pn_sa2_bwd_kernel(const idf_pointnet2 pn, const Plan pl, const float *__restrict__ obj_points, int P,
                                                        const int *__restrict__ saves, const float *__restrict__ d_pc, float *__restrict__ gclip,
                                                        float *__restrict__ dfeat) {
    __shared__ float xin[NS1 * 100], a1[NS1 * 64], a2[NS1 * 96], a3[NS1 * 128], tmp[NS1 * 96];
    __shared__ float dxf[NSLOT][F1];
    __shared__ float f2[256], df2[256], dlin[256];
    __shared__ int dupl[NSLOT];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float *ar = pn.arena;
    const int *sv = saves + (size_t)b * SV_WORDS;
    const float *feat = reinterpret_cast<const float *>(sv) + SV_FEAT;
    float *g = gclip + (size_t)b * (pl.n_fold - pl.n_fold_sa1);
    const int base = pl.n_fold_sa1;                                     // the clip buffer starts at SA2's first folded offset
    const float *pts = obj_points + (size_t)b * P * 3;

    if (tid < 256) dlin[tid] = tid < 253 ? d_pc[(size_t)b * 256 + 3 + tid] : 0.f;
    if (tid < NSLOT) dupl[tid] = sv[SV_DUP + tid];
    __syncthreads();
    if (tid < 256) {                                                    // d f2[c] = sum_o d_pc[3 + o] Wlin[o][c]
        float s = 0.f;
        for (int o = 0; o < 253; ++o) s += dlin[o] * ar[pn.lin_w + (size_t)o * 256 + tid];
        df2[tid] = s;
    }
    if (tid < 253) g[pl.fold_lin_b - base + tid] = dlin[tid];
    __syncthreads();

    const float c0x = pts[0], c0y = pts[1], c0z = pts[2];              // the key point: FPS starts at point 0
    for (int sc = 0; sc < 2; ++sc) {
        const int ns = sc ? NS1 : NS0, s0 = sc ? NS0 : 0;
        const idf_pn_mlp &m = pn.sa2[sc];
        const Layer *ly = pl.ly + 6 + 3 * sc;
        const int c1 = ly[0].cout, c2 = ly[1].cout;
        for (int i = tid; i < ns * CIN2; i += PT) {
            const int n = i / CIN2, c = i - n * CIN2;
            float v;
            if (c < 3) {
                const float *q = pts + (size_t)sv[SV_PID + s0 + n] * 3;
                v = (c == 0 ? q[0] - c0x : (c == 1 ? q[1] - c0y : q[2] - c0z));
            } else {
                v = feat[(s0 + n) * F1 + c - 3];
            }
            xin[n * 100 + c] = v;
        }
        __syncthreads();
        mlp_layer(xin, 100, ar + m.w[0], ar + m.b[0], CIN2, c1, ns, a1, c1);
        __syncthreads();
        mlp_layer(a1, c1, ar + m.w[1], ar + m.b[1], c1, c2, ns, a2, c2);
        __syncthreads();
        mlp_layer(a2, c2, ar + m.w[2], ar + m.b[2], c2, 128, ns, a3, 128);
        __syncthreads();
        for (int o = tid; o < 128; o += PT) {                           // the pooled features (the Linear's input)
            float mx = a3[o];
            for (int n = 1; n < ns; ++n) mx = fmaxf(mx, a3[n * 128 + o]);
            f2[sc * 128 + o] = mx;
        }
        pool_backward<PT>(a3, 128, ns, 128, df2 + sc * 128);           // a3 := d z3
        __syncthreads();
        grad_weights<PT>(a3, 128, a2, c2, c2, 128, ns, g + (ly[2].fold_w - base), g + (ly[2].fold_b - base));
        grad_input<PT>(a3, 128, ar + m.w[2], c2, 128, ns, a2, c2, tmp, c2);                 // tmp := d z2
        __syncthreads();
        grad_weights<PT>(tmp, c2, a1, c1, c1, c2, ns, g + (ly[1].fold_w - base), g + (ly[1].fold_b - base));
        grad_input<PT>(tmp, c2, ar + m.w[1], c1, c2, ns, a1, c1, a3, c1);                   // a3 := d z1
        __syncthreads();
        grad_weights<PT>(a3, c1, xin, 100, CIN2, c1, ns, g + (ly[0].fold_w - base), g + (ly[0].fold_b - base));
        for (int i = tid; i < ns * F1; i += PT) {                       // d feat1 of the slot; the three relative-xyz channels reach no parameter
            const int n = i / F1, c = i - n * F1;
            const float *w = ar + m.w[0] + 3 + c;
            float s = 0.f;
            for (int o = 0; o < c1; ++o) s += a3[n * c1 + o] * w[(size_t)o * CIN2];
            dxf[s0 + n][c] = s;
        }
        __syncthreads();
    }
    for (int i = tid; i < 253 * 256; i += PT) g[pl.fold_lin_w - base + i] = dlin[i >> 8] * f2[i & 255];
    // slots that repeat a centre add into the first slot that holds it, in slot order
    for (int i = tid; i < NSLOT * F1; i += PT) {
        const int d = i / F1, c = i - d * F1;
        if (dupl[d] != d) continue;
        float s = 0.f;
        for (int e = d; e < NSLOT; ++e)
            if (dupl[e] == d) s += dxf[e][c];
        dfeat[((size_t)b * NSLOT + d) * F1 + c] = s;
    }
}

__global__ __launch_bounds__(NT1) void pn_sa1_bwd_kernel(const idf_pointnet2 pn, const Plan pl, const float *__restrict__ obj_points, int P,
                                                         const int *__restrict__ saves, const float *__restrict__ dfeat, float *__restrict__ gslot) {
    __shared__ float xin[64 + NS1 * 4], a1[256 + NS1 * 32], a2[256 + NS1 * 32], a3[512 + NS1 * 64], tmp[256 + NS1 * 32];
    __shared__ float df[F1];
    const int s = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int *sv = saves + (size_t)b * SV_WORDS;
    if (sv[SV_DUP + s] != s) return;                                    // block-uniform
    const float *ar = pn.arena;
    const float *pts = obj_points + (size_t)b * P * 3;
    float *g = gslot + ((size_t)b * NSLOT + s) * pl.n_fold_sa1;
    const float *pc = pts + (size_t)sv[SV_PID + s] * 3;
    if (tid < NS0 + NS1) {
        const bool sc1 = tid >= NS0;
        const int n = sc1 ? tid - NS0 : tid;
        const float *p = pts + (size_t)(sc1 ? sv[SV_NB1 + s * NS1 + n] : sv[SV_NB0 + s * NS0 + n]) * 3;
        float *x = xin + (sc1 ? 64 + n * 4 : n * 4);
        const float px = p[0], py = p[1], pz = p[2];
        x[0] = px - pc[0]; x[1] = py - pc[1]; x[2] = pz - pc[2]; x[3] = sqrtf(px * px + py * py + pz * pz);
    }
    if (tid < F1) df[tid] = dfeat[((size_t)b * NSLOT + s) * F1 + tid];
    __syncthreads();
    const idf_pn_mlp &m0 = pn.sa1[0], &m1 = pn.sa1[1];
    mlp_layer<NT1>(xin, 4, ar + m0.w[0], ar + m0.b[0], 4, 16, NS0, a1, 16);
    mlp_layer<NT1>(xin + 64, 4, ar + m1.w[0], ar + m1.b[0], 4, 32, NS1, a1 + 256, 32);
    __syncthreads();
    mlp_layer<NT1>(a1, 16, ar + m0.w[1], ar + m0.b[1], 16, 16, NS0, a2, 16);
    mlp_layer<NT1>(a1 + 256, 32, ar + m1.w[1], ar + m1.b[1], 32, 32, NS1, a2 + 256, 32);
    __syncthreads();
    mlp_layer<NT1>(a2, 16, ar + m0.w[2], ar + m0.b[2], 16, 32, NS0, a3, 32);
    mlp_layer<NT1>(a2 + 256, 32, ar + m1.w[2], ar + m1.b[2], 32, 64, NS1, a3 + 512, 64);
    __syncthreads();
    pool_backward<NT1>(a3, 32, NS0, 32, df);
    pool_backward<NT1>(a3 + 512, 64, NS1, 64, df + 32);
    __syncthreads();
    const Layer *l0 = pl.ly, *l1 = pl.ly + 3;
    grad_weights<NT1>(a3, 32, a2, 16, 16, 32, NS0, g + l0[2].fold_w, g + l0[2].fold_b);
    grad_weights<NT1>(a3 + 512, 64, a2 + 256, 32, 32, 64, NS1, g + l1[2].fold_w, g + l1[2].fold_b);
    grad_input<NT1>(a3, 32, ar + m0.w[2], 16, 32, NS0, a2, 16, tmp, 16);
    grad_input<NT1>(a3 + 512, 64, ar + m1.w[2], 32, 64, NS1, a2 + 256, 32, tmp + 256, 32);
    __syncthreads();
    grad_weights<NT1>(tmp, 16, a1, 16, 16, 16, NS0, g + l0[1].fold_w, g + l0[1].fold_b);
    grad_weights<NT1>(tmp + 256, 32, a1 + 256, 32, 32, 32, NS1, g + l1[1].fold_w, g + l1[1].fold_b);
    grad_input<NT1>(tmp, 16, ar + m0.w[1], 16, 16, NS0, a1, 16, a3, 16);
    grad_input<NT1>(tmp + 256, 32, ar + m1.w[1], 32, 32, NS1, a1 + 256, 32, a3 + 512, 32);
    __syncthreads();
    grad_weights<NT1>(a3, 16, xin, 4, 4, 16, NS0, g + l0[0].fold_w, g + l0[0].fold_b);
    grad_weights<NT1>(a3 + 512, 32, xin + 64, 4, 4, 32, NS1, g + l1[0].fold_w, g + l1[0].fold_b);
}

// gfold[i] = the per-clip (SA1: per clip and distinct centre) gradients added in index order
__global__ __launch_bounds__(256) void pn_fold_kernel(const Plan pl, const int *__restrict__ saves, const float *__restrict__ gslot, const float *__restrict__ gclip,
                                                      int B, float *__restrict__ gfold) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= pl.n_fold) return;
    double s = 0.0;
    if (i < pl.n_fold_sa1) {
        for (int b = 0; b < B; ++b)
            for (int e = 0; e < NSLOT; ++e)
                if (saves[(size_t)b * SV_WORDS + SV_DUP + e] == e) s += (double)gslot[((size_t)b * NSLOT + e) * pl.n_fold_sa1 + i];
    } else {
        const size_t n2 = pl.n_fold - pl.n_fold_sa1;
        for (int b = 0; b < B; ++b) s += (double)gclip[(size_t)b * n2 + (i - pl.n_fold_sa1)];
    }
    gfold[i] = (float)s;
}

__global__ __launch_bounds__(256) void pn_unfold_kernel(const Plan pl, const float *__restrict__ theta, const float *__restrict__ stats,
                                                        const float *__restrict__ gfold, float *__restrict__ grads) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= pl.n_raw) return;
    if (j >= pl.raw_lin_w) { grads[j] = gfold[pl.fold_lin_w + (j - pl.raw_lin_w)]; return; }          // Linear.weight, Linear.bias: contiguous in both
    int L = 0;
    while (L < 11 && j >= pl.ly[L + 1].raw_w) ++L;
    const Layer y = pl.ly[L];
    if (j >= y.raw_b) { grads[j] = gfold[y.fold_b + (j - y.raw_b)]; return; }                           // d beta = d b'
    const int o = j < y.raw_g ? (j - y.raw_w) / y.cin : j - y.raw_g;
    const double sigma = sqrt((double)stats[y.stat + y.cout + o] + BN_EPS);
    if (j < y.raw_g) {
        grads[j] = (float)((double)gfold[y.fold_w + (j - y.raw_w)] * ((double)theta[y.raw_g + o] / sigma));
        return;
    }
    double s = 0.0;
    for (int c = 0; c < y.cin; ++c) s += (double)gfold[y.fold_w + o * y.cin + c] * (double)theta[y.raw_w + o * y.cin + c];
    grads[j] = (float)((s - (double)gfold[y.fold_b + o] * (double)stats[y.stat + o]) / sigma);
}

// the arena of interdiff_pointnet2_encode* from the raw tensors: mdm.py pack_pointnet2's float64 expressions, rounded once
__global__ __launch_bounds__(256) void pn_refold_kernel(const idf_pointnet2 pn, const Plan pl, const float *__restrict__ theta, const float *__restrict__ stats,
                                                        float *__restrict__ arena) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= pl.n_fold) return;
    if (i >= pl.fold_lin_b) { arena[pn.lin_b + (i - pl.fold_lin_b)] = theta[pl.raw_lin_b + (i - pl.fold_lin_b)]; return; }
    if (i >= pl.fold_lin_w) { arena[pn.lin_w + (i - pl.fold_lin_w)] = theta[pl.raw_lin_w + (i - pl.fold_lin_w)]; return; }
    int L = 0;
    while (L < 11 && i >= pl.ly[L + 1].fold_w) ++L;
    const Layer y = pl.ly[L];
    const idf_pn_mlp &m = L < 6 ? pn.sa1[L / 3] : pn.sa2[L / 3 - 2];
    const bool is_w = i < y.fold_b;
    const int o = is_w ? (i - y.fold_w) / y.cin : i - y.fold_b;
    const double sc = (double)theta[y.raw_g + o] / sqrt((double)stats[y.stat + y.cout + o] + BN_EPS);
    if (is_w) {
        arena[m.w[L % 3] + (i - y.fold_w)] = (float)((double)theta[y.raw_w + (i - y.fold_w)] * sc);
    } else {
        const double mean_sc = (double)stats[y.stat + o] * sc;
        arena[m.b[L % 3] + o] = (float)((double)theta[y.raw_b + o] - mean_sc);
    }
}

const Plan &plan() {
    static const Plan p = make_plan();
    return p;
}

bool plan_matches(const idf_pointnet2 *pn) {
    const Plan &pl = plan();
    for (int g = 0; g < 4; ++g) {
        const idf_pn_mlp &m = g < 2 ? pn->sa1[g] : pn->sa2[g - 2];
        for (int l = 0; l < 3; ++l)
            if (m.c[l] != pl.ly[g * 3 + l].cin || m.c[l + 1] != pl.ly[g * 3 + l].cout) return false;
    }
    return true;
}

struct Ws { size_t gclip, gslot, dfeat, gfold, floats; };
Ws workspace(int B) {
    const Plan &pl = plan();
    Ws w;
    size_t at = 0;
    auto take = [&](size_t n) { const size_t o = at; at += (n + 63) / 64 * 64; return o; };
    w.gclip = take((size_t)B * (pl.n_fold - pl.n_fold_sa1));
    w.gslot = take((size_t)B * NSLOT * pl.n_fold_sa1);
    w.dfeat = take((size_t)B * NSLOT * F1);
    w.gfold = take(pl.n_fold);
    w.floats = at;
    return w;
}

}  // namespace

extern "C" int interdiff_pointnet2_finetune_param_table(int64_t *offsets, int64_t *sizes, int32_t *n_tensors, int64_t *n_param) {
    const Plan &pl = plan();
    int k = 0;
    auto put = [&](int off, int size) {
        if (offsets) offsets[k] = off;
        if (sizes) sizes[k] = size;
        ++k;
    };
    for (int L = 0; L < 12; ++L) {
        put(pl.ly[L].raw_w, pl.ly[L].cin * pl.ly[L].cout);
        put(pl.ly[L].raw_g, pl.ly[L].cout);
        put(pl.ly[L].raw_b, pl.ly[L].cout);
    }
    put(pl.raw_lin_w, 253 * 256);
    put(pl.raw_lin_b, 253);
    if (n_tensors) *n_tensors = k;
    if (n_param) *n_param = pl.n_raw;
    return IDF_OK;
}

extern "C" size_t interdiff_pointnet2_finetune_workspace_bytes(int32_t B) { return B > 0 ? workspace(B).floats * sizeof(float) : 0; }

extern "C" int interdiff_pointnet2_finetune_grads(const idf_pointnet2 *pn, const float *theta, const float *stats, const float *obj_points, int32_t B, int32_t P,
                                                  const void *saves, const float *d_pc, float *grads, void *ws, size_t ws_bytes, void *stream) {
    if (!pn || !pn->arena || !theta || !stats || !obj_points || !saves || !d_pc || !grads || !ws || B <= 0 || P < 1 || P > MAXP) return IDF_E_INVAL;
    if (!plan_matches(pn) || (reinterpret_cast<uintptr_t>(ws) & 255)) return IDF_E_INVAL;
    if (ws_bytes < interdiff_pointnet2_finetune_workspace_bytes(B)) return IDF_E_NOMEM;
    const Plan &pl = plan();
    const Ws w = workspace(B);
    float *f = static_cast<float *>(ws);
    const int *sv = static_cast<const int *>(saves);
    hipStream_t s = idf_stream(stream);
    idf_prof_mark(IDF_K_OTHER, s);
    hipLaunchKernelGGL(pn_sa2_bwd_kernel, dim3(B), dim3(PT), 0, s, *pn, pl, obj_points, P, sv, d_pc, f + w.gclip, f + w.dfeat);
    hipLaunchKernelGGL(pn_sa1_bwd_kernel, dim3(NSLOT, B), dim3(NT1), 0, s, *pn, pl, obj_points, P, sv, f + w.dfeat, f + w.gslot);
    hipLaunchKernelGGL(pn_fold_kernel, dim3((pl.n_fold + 255) / 256), dim3(256), 0, s, pl, sv, f + w.gslot, f + w.gclip, B, f + w.gfold);
    hipLaunchKernelGGL(pn_unfold_kernel, dim3((pl.n_raw + 255) / 256), dim3(256), 0, s, pl, theta, stats, f + w.gfold, grads);
    idf_prof_mark(-1, s);
    IDF_CHECK_LAUNCH();
    return IDF_OK;
}

extern "C" int interdiff_pointnet2_refold(const idf_pointnet2 *pn, const float *theta, const float *stats, void *stream) {
    if (!pn || !pn->arena || !theta || !stats || !plan_matches(pn)) return IDF_E_INVAL;
    const Plan &pl = plan();
    hipLaunchKernelGGL(pn_refold_kernel, dim3((pl.n_fold + 255) / 256), dim3(256), 0, idf_stream(stream), *pn, pl, theta, stats, const_cast<float *>(pn->arena));
    IDF_CHECK_LAUNCH();
    return IDF_OK;
}
