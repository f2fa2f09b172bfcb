// Pseudo linear multistep sampler step (plms_sample, diffusion/gaussian_diffusion.py:1001-1083) for an x0-predicting model: the eps of a
// step is re-derived from the (inpainted, hook-corrected) x0, combined with up to three earlier ones held in a ring f32[3][n], and the
// DDIM-like update is applied in place.  Elementwise, one HBM pass, 16 B per lane when the operands allow it.  Device-parameterised like
// posterior_dev_kernel (sampler.hip): t, the loop index and so the ring slot and the number of earlier eps come from the sampler state,
// the four scalars of a step from a table row -- one captured hipGraph serves every plain step, another the two-call first step.
#include "common.h"
#include "philox.h"

namespace {

enum { PLMS_STEP = 0, PLMS_HALF1 = 1, PLMS_HALF2 = 2 };

struct plms_row { double a, r, sp, sq; };            // sqrt(1/ab), sqrt(1/ab - 1), sqrt(ab_prev), sqrt(1 - ab_prev): fp32 table values, widened

__device__ __forceinline__ plms_row plms_load_row(const float *__restrict__ ptable, int64_t t) {
    return plms_row{(double)ptable[t * 4], (double)ptable[t * 4 + 1], (double)ptable[t * 4 + 2], (double)ptable[t * 4 + 3]};
}

// The arithmetic.  The update cancels: a x and r eps' are sqrt(ab_prev / ab) times larger than their difference (3.5e3 at the last step of a
// cosine schedule), and the Adams-Bashforth weights add up to 160/24 in magnitude, so fp32 roundings inside it would surface amplified in x.
// An elementwise kernel has the time: every element is evaluated in fp64 from its fp32 operands and rounded ONCE per stored value.  Pinned
// besides: no contraction by the compiler, the fused operations spelled out, so that the 16-byte and the scalar form -- and any later
// instantiation -- give the same bits.
// eps = (a x - x0) / r                                                                       (:1044, _predict_eps_from_xstart)
__device__ __forceinline__ double plms_eps(const plms_row c, double x, double x0) {
#pragma clang fp contract(off)
    return fma(c.a, x, -x0) / c.r;
}
// Adams-Bashforth over the newest `k` values e1 (newest) .. e4                                  (:1064-1071)
__device__ __forceinline__ double plms_combine(int k, double e1, double e2, double e3, double e4) {
#pragma clang fp contract(off)
    if (k <= 1) return e1;
    if (k == 2) return fma(3.0, e1, -e2) * 0.5;
    if (k == 3) return fma(23.0, e1, fma(-16.0, e2, 5.0 * e3)) / 12.0;
    return fma(55.0, e1, fma(-59.0, e2, fma(37.0, e3, -9.0 * e4))) / 24.0;
}
// x_prev = sqrt(ab_prev) (a x - r eps') + sqrt(1 - ab_prev) eps'                                (:1057-1058, :1074-1075)
__device__ __forceinline__ double plms_update(const plms_row c, double x, double ep) {
#pragma clang fp contract(off)
    const double p = c.r * ep, q = c.sq * ep;
    return fma(c.sp, fma(c.a, x, -p), q);
}
// x_mid = x0 sqrt(ab_prev) + sqrt(1 - ab_prev) eps                                              (:1054)
__device__ __forceinline__ double plms_mid(const plms_row c, double x0, double eps) {
#pragma clang fp contract(off)
    const double q = c.sq * eps;
    return fma(x0, c.sp, q);
}

// one element of a launch; e2..e4: the earlier eps (e4 is what the slot being written held), em: ring eps (HALF2), xm: x_mid (HALF2).
// The eps of THIS step enters its own combination unrounded; the ring keeps its fp32 value for the steps to come.
template <int MODE>
__device__ __forceinline__ void plms_element(const plms_row c, const plms_row cn, int k, bool last, float x, float p, float e2, float e3,
                                             float e4, float em, float xm, float &x_out, float &eps_out) {
    if constexpr (MODE == PLMS_STEP) {
        const double eps = plms_eps(c, x, p);
        eps_out = (float)eps;
        x_out = last ? p : (float)plms_update(c, x, plms_combine(k, eps, e2, e3, e4));
    } else if constexpr (MODE == PLMS_HALF1) {
        const double eps = plms_eps(c, x, p);
        eps_out = (float)eps;
        x_out = (float)plms_mid(c, p, eps);          // (goes to x_mid)
    } else {
        const double eps2 = plms_eps(cn, xm, p);     // the scalars of t - 1 on (x_mid, second x0)
        eps_out = em;
        x_out = (float)plms_update(c, x, ((double)em + eps2) * 0.5);      // the scalars of t on the ORIGINAL x
    }
}

__device__ __forceinline__ float4 ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }

// STEP:  x in/out, ring in/out.   HALF1: x in, ring out, xmid out.   HALF2: x in/out, ring in, xmid in.
template <int MODE, bool VEC>
__global__ __launch_bounds__(256) void plms_kernel(float *__restrict__ x, const float *__restrict__ x0, const float *__restrict__ gt,
                                                   const uint8_t *__restrict__ mask, float *ring, float *xmid, int64_t n, int order,
                                                   const float *__restrict__ ptable, int64_t *__restrict__ state, int64_t *__restrict__ ts,
                                                   int B, const int64_t *__restrict__ tmap) {
    const int64_t s0 = state[0], it = state[1];
    const int64_t t = MODE == PLMS_HALF2 ? s0 + 1 : s0;                  // (half one left state[0] at t - 1)
    const plms_row c = plms_load_row(ptable, t);
    const plms_row cn = MODE == PLMS_HALF2 ? plms_load_row(ptable, s0) : c;
    const int64_t have = it < order - 1 ? it : order - 1;                // earlier eps available = min(order - 1, loop index)
    const int k = (int)have + 1;                                         // cur_order
    const bool last = t == 0;
    float *__restrict__ r1 = ring + (it % 3) * n;                        // written (the oldest: loop index it - 3); HALF2 reads it
    const float *r2 = ring + ((it + 2) % 3) * n, *r3 = ring + ((it + 1) % 3) * n;      // loop indices it - 1, it - 2
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, g0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if constexpr (VEC) {
        for (int64_t g = g0; g < (n >> 2); g += stride) {
            const int64_t i = g * 4;
            const float4 xv = ld4(x + i);
            float4 pv = ld4(x0 + i);
            if (mask) {
                const uchar4 m = *reinterpret_cast<const uchar4 *>(mask + i);
                const float4 gv = ld4(gt + i);
                pv.x = m.x ? gv.x : pv.x; pv.y = m.y ? gv.y : pv.y; pv.z = m.z ? gv.z : pv.z; pv.w = m.w ? gv.w : pv.w;
            }
            float4 a2 = make_float4(0.f, 0.f, 0.f, 0.f), a3 = a2, a4 = a2, em = a2, xm = a2, xo, eo;
            if constexpr (MODE == PLMS_STEP) {
                if (k >= 2) a2 = ld4(r2 + i);
                if (k >= 3) a3 = ld4(r3 + i);
                if (k >= 4) a4 = ld4(r1 + i);
            }
            if constexpr (MODE == PLMS_HALF2) { em = ld4(r1 + i); xm = ld4(xmid + i); }
            plms_element<MODE>(c, cn, k, last, xv.x, pv.x, a2.x, a3.x, a4.x, em.x, xm.x, xo.x, eo.x);
            plms_element<MODE>(c, cn, k, last, xv.y, pv.y, a2.y, a3.y, a4.y, em.y, xm.y, xo.y, eo.y);
            plms_element<MODE>(c, cn, k, last, xv.z, pv.z, a2.z, a3.z, a4.z, em.z, xm.z, xo.z, eo.z);
            plms_element<MODE>(c, cn, k, last, xv.w, pv.w, a2.w, a3.w, a4.w, em.w, xm.w, xo.w, eo.w);
            if constexpr (MODE != PLMS_HALF2) *reinterpret_cast<float4 *>(r1 + i) = eo;
            *reinterpret_cast<float4 *>((MODE == PLMS_HALF1 ? xmid : x) + i) = xo;
        }
    } else {
        for (int64_t i = g0; i < n; i += stride) {
            const float p = (mask && mask[i]) ? gt[i] : x0[i];
            float a2 = 0.f, a3 = 0.f, a4 = 0.f, em = 0.f, xm = 0.f, xo, eo;
            if constexpr (MODE == PLMS_STEP) {
                if (k >= 2) a2 = r2[i];
                if (k >= 3) a3 = r3[i];
                if (k >= 4) a4 = r1[i];
            }
            if constexpr (MODE == PLMS_HALF2) { em = r1[i]; xm = xmid[i]; }
            plms_element<MODE>(c, cn, k, last, x[i], p, a2, a3, a4, em, xm, xo, eo);
            if constexpr (MODE != PLMS_HALF2) r1[i] = eo;
            (MODE == PLMS_HALF1 ? xmid : x)[i] = xo;
        }
    }
    // bookkeeping by the LAST workgroup to arrive (every workgroup has read the state before it adds itself: philox.h)
    if constexpr (MODE == PLMS_STEP) {
        sampler_advance_last(state, ts, B, gridDim.x, t, (uint64_t)it, tmap);
    } else {
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned *arrived = reinterpret_cast<unsigned *>(state + 3);
            if (atomicAdd(arrived, 1u) == gridDim.x - 1) {
                *arrived = 0u;
                if constexpr (MODE == PLMS_HALF1) {                      // t - 1 for the second call; the loop index stays
                    state[0] = t - 1;
                    const int64_t tm = sampler_model_timestep(tmap, t - 1);
                    for (int b = 0; b < B; ++b) ts[b] = tm;
                } else {
                    state[1] = it + 1;                                   // state[0] and ts already are the next step's
                }
            }
        }
    }
}

inline unsigned plms_grid(int64_t work) {
    const int64_t b = idf_cdiv(work, 256);
    return (unsigned)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}

inline bool misaligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

template <int MODE>
int plms_launch(float *x, const float *x0, const float *gt, const uint8_t *mask, float *ring, float *xmid, int64_t n, int order,
                const float *ptable, const int64_t *tmap, int64_t *state, int64_t *ts, int B, void *stream) {
    if (!x || !x0 || !ring || !ptable || !state || n < 0 || (mask && !gt) || order < 1 || order > 4) return IDF_E_INVAL;
    if (MODE != PLMS_STEP && !xmid) return IDF_E_INVAL;
    if (MODE != PLMS_HALF2 && (!ts || B <= 0)) return IDF_E_INVAL;
    if (n == 0) return IDF_OK;
    const bool vec = (n & 3) == 0 && !misaligned16(x) && !misaligned16(x0) && !misaligned16(gt) && !misaligned16(ring) && !misaligned16(xmid) &&
                     (reinterpret_cast<uintptr_t>(mask) & 3) == 0;
    idf_prof_mark(IDF_K_POSTERIOR, idf_stream(stream));
    if (vec)
        hipLaunchKernelGGL((plms_kernel<MODE, true>), dim3(plms_grid(n >> 2)), dim3(256), 0, idf_stream(stream), x, x0, gt, mask, ring, xmid, n,
                           order, ptable, state, ts, B, tmap);
    else
        hipLaunchKernelGGL((plms_kernel<MODE, false>), dim3(plms_grid(n)), dim3(256), 0, idf_stream(stream), x, x0, gt, mask, ring, xmid, n,
                           order, ptable, state, ts, B, tmap);
    idf_prof_mark(-1, idf_stream(stream));
    IDF_CHECK_LAUNCH();
    return IDF_OK;
}

}  // namespace

// plms_sample's multistep branch (gaussian_diffusion.py:1044, :1060-1083)
extern "C" int interdiff_plms_step_dev(float *x, const float *x0, const float *gt, const uint8_t *mask, float *ring, int64_t n, int32_t order,
                                       const float *ptable, const int64_t *tmap, int64_t *state, int64_t *ts, int32_t B, void *stream) {
    return plms_launch<PLMS_STEP>(x, x0, gt, mask, ring, nullptr, n, order, ptable, tmap, state, ts, B, stream);
}

// the first half of plms_sample's "pseudo improved Euler" start (gaussian_diffusion.py:1044, :1053-1054): x is only read
extern "C" int interdiff_plms_first_half_dev(const float *x, const float *x0, const float *gt, const uint8_t *mask, float *ring, float *x_mid,
                                             int64_t n, const float *ptable, const int64_t *tmap, int64_t *state, int64_t *ts, int32_t B,
                                             void *stream) {
    return plms_launch<PLMS_HALF1>(const_cast<float *>(x), x0, gt, mask, ring, x_mid, n, 2, ptable, tmap, state, ts, B, stream);
}

// ... and its second half, after the second denoiser call (gaussian_diffusion.py:1055-1058)
extern "C" int interdiff_plms_second_half_dev(float *x, const float *x0, const float *gt, const uint8_t *mask, const float *ring,
                                              const float *x_mid, int64_t n, const float *ptable, int64_t *state, void *stream) {
    return plms_launch<PLMS_HALF2>(x, x0, gt, mask, const_cast<float *>(ring), const_cast<float *>(x_mid), n, 2, ptable, nullptr, state, nullptr, 0,
                                   stream);
}
