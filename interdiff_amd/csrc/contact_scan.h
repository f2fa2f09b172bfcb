// The exact nearest-vertex scan with block culling: corr_point_order_kernel (K3), corr_contact_kernel<OPT, WITH_PRED> (K4) and their ONE host launcher.
// Three instantiations exist, all launched from correction.hip (this header must stay in that one translation unit: a second one would compile the scan twice,
// and two compilations of this source have differed in the last bit of a frame's loss):
//   <false, true>   the correction hook (correction_impl), with or without predictor workgroups riding along
//   <false, false>  the stand-alone scan and the evaluation metrics (interdiff_contact_nn, interdiff_metrics)
//   <true,  false>  the physics post-optimisation (idf_nn_scan_opt, called from optimize.hip)
//
// CONTRACT of the kernel (the launcher below fills every operand from a ContactArgs; nothing else launches it)
//   frames     !OPT: time-major, n = t*B + b, clip b = n % B; the clip's canonical points obj_points[b] are transformed by (objR[n], objT[n]) on the fly.
//              OPT:  clip-major, n = b*T + t, clip b = n / frames_per_clip; the points pts_frame[n] are taken as they are (objR / objT / obj_points unread),
//                    grid (N, 2): two workgroups share a frame's tasks.
//              WITH_PRED: workgroups blockIdx.x < pred.nclips run the contact-frame predictor of clip blockIdx.x (objproj.h), the rest are frames n = blockIdx.x - nclips.
//   nullable   porder    null = the points are scanned in their own order (task k = points 64k .. 64k+63); else [B][P] scan position -> point, per CLIP in both modes
//              vorder    null = IDENTITY ORDER: records sit in LDS by vertex id and every block is scored (the in-library brute force of the tests)
//              vrank     null = the records are gathered through vorder; else the frame's vertices are read in their own order and scattered
//              adj_pair  null = normals through adj_face / adj_corner / faces; else one (a, b) pair of scan positions per incident face (faces is then unread)
//              markers_out, o2h_out, idx_out, stats: null = not written (OPT writes idx_out only, and needs it)
//              frames below nn_from skip the scan and the signed distance (their loss_sum is 0) and keep the marker distances
//   operands   identity order: vorder = vrank = adj_pair = null, faces = ctx->faces, markers_pos = ctx->markers_idx (vertex ids ARE the scan positions)
//              scan order:     vorder, vrank, adj_pair = ctx->adj_pair_scan, faces = ctx->faces_scan, markers_pos = ctx->markers_scan -- all four of
//                              (vorder, faces_scan, markers_scan, adj_pair_scan) or none; results are the same bits in either order
//              OPT reads no topology and no markers: all of those are null, M = 0
//   limits     P <= MAXP, M <= MAXM (callers check M), ContactLds(V).total float4 of dynamic LDS (V = 6890: 135 KB)
//   DO NOT reformat the kernel bodies casually: which products and sums the compiler contracts into FMAs is decided per expression as written (and per
//   instantiation); the argmin is protected by `fp contract(off)` blocks, the normal / signed-distance expressions are not, and the goldens hold their bits.
#pragma once
#include <float.h>
#include "common.h"
#include "objproj.h"
#include "vec3.h"

namespace {

// ---- K3: scan order of a clip's object points ---------------------------------------------------------------
// porder[b][s] = index of the clip's s-th canonical object point in Morton order (10 bits per axis inside the clip's bounding box).
// The contact scan culls vertex blocks per WAVE; a wave that owns a compact patch of the object (128 consecutive points of this
// order) agrees on which blocks it needs.  A rigid transform keeps the patch compact, so the order is per clip, not per frame.
// One workgroup per clip: bounding box by a block reduction, 41-bit keys (code << 11 | index: unique, so the sort is stable by
// construction), bitonic sort of 2048 keys in LDS.  ~10 us per call for all clips.
constexpr int MAXP = 2048;             // object points per frame handled by one workgroup (CT * QP)
__global__ __launch_bounds__(1024) void corr_point_order_kernel(const float *__restrict__ obj_points, int P, int32_t *__restrict__ porder) {
    __shared__ unsigned long long keys[MAXP];
    __shared__ float red[6][1024];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float *op = obj_points + (size_t)b * P * 3;
    float p[2][3];
    float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int i = tid + 1024 * k;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            p[k][a] = i < P ? op[3 * i + a] : 0.f;
            if (i < P) { lo[a] = fminf(lo[a], p[k][a]); hi[a] = fmaxf(hi[a], p[k][a]); }
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) { red[a][tid] = lo[a]; red[3 + a][tid] = hi[a]; }
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
        if (tid < s) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                red[a][tid] = fminf(red[a][tid], red[a][tid + s]);
                red[3 + a][tid] = fmaxf(red[3 + a][tid], red[3 + a][tid + s]);
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int i = tid + 1024 * k;
        unsigned long long key = ~0ull;                                   // slots past P sort to the end
        if (i < P) {
            unsigned code = 0;
            unsigned q[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float ext = red[3 + a][0] - red[a][0];
                const float u = ext > 0.f ? (p[k][a] - red[a][0]) / ext : 0.f;
                q[a] = (unsigned)fminf(fmaxf(u * 1023.0f, 0.f), 1023.0f);      // NaN -> 0 (fmaxf returns the non-NaN operand)
            }
#pragma unroll
            for (int bit = 0; bit < 10; ++bit)
#pragma unroll
                for (int a = 0; a < 3; ++a) code |= ((q[a] >> bit) & 1u) << (3 * bit + a);
            key = ((unsigned long long)code << 11) | (unsigned)i;
        }
        keys[i] = key;
    }
    __syncthreads();
    for (int k = 2; k <= MAXP; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            const int l = 2 * j * (tid / j) + (tid % j), r = l + j;
            const unsigned long long x = keys[l], y = keys[r];
            const bool up = (l & k) == 0;
            if ((x > y) == up) { keys[l] = y; keys[r] = x; }
            __syncthreads();
        }
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int i = tid + 1024 * k;
        if (i < P) porder[(size_t)b * P + i] = (int32_t)(keys[i] & 2047u);
    }
}

// ---- K4: per-frame contact analysis -------------------------------------------------------------------
// One workgroup (16 waves) per frame.  The frame's 2048 object points are cut into TASKS of 64 consecutive points of the clip's
// Morton order (K3) -- one point per lane -- and the waves pull tasks from an LDS counter: a patch that touches the body needs
// several times the vertex blocks of one that floats free, and a static split of 128 points per wave left the workgroup waiting
// for its slowest wave (tools/contact_probe.py, first version: thread 0 spent 220 k of 450 k cycles at the first barrier).
// Arithmetic is the exact (dx*dx + dy*dy) + dz*dz without FMA contraction, so the argmin is bit-identical to geometry.hip and to
// the oracle.  The fp32 VALU of gfx950 runs plain ops at 16 lanes per clock and PACKED ops (v_pk_add/mul_f32) at twice that, so
// every distance / box instruction works on a PAIR: two consecutive vertices (or two boxes) against the lane's one point --
// records are stored as pairs {x0 x1 y0 y1 | z0 z1 - -}, the point as {q, q}.  (Measured: one point per lane on plain ops cost
// 4.7 cycles per instruction per wave, exactly what a packed instruction costs.)
//
// EXACT block culling (round 3).  The vertex records sit in LDS in SCAN ORDER -- the Morton order of the REST pose, chosen at
// pack time (ctx->vorder): skinning is spatially smooth, so CB consecutive records stay a compact clump under any pose -- and
// each block of CB = 16 records gets its axis-aligned box, built in-kernel from the frame's posed vertices.  Per point:
//   seed    the distance to the FIRST record of every 4th block (108 real distances: a valid upper bound of the minimum), widened by the scan's margin;
//   scan    two levels: super-blocks of SB = 8 blocks (128 records) are tested first, their blocks only if some point needs them.
//           For a box: lower bound lb = |max(lo - q, q - hi, 0)|^2 -- fp32 subtraction is monotone, so each component is at most that of
//           any vertex inside the box.  A box is skipped iff lb > thr (STRICTLY) for every point of the WAVE (one ballot, one uniform
//           branch).  Rounds 3-5 scored with the exact distance E = (dx dx + dy dy) + dz dz and compared lb <= best bit for bit; round 6
//           RANKS with A = fma(dz, dz, fma(dy, dy, dx dx)) (7 instead of 9 instructions per record pair; |A / E - 1| <= 6 ulp-halves, both being
//           three roundings of the same non-negative sum) and carries a margin of 2^-18 (+1e-37) in every comparison that drops something:
//           thr = min(seed, smallest block minimum so far) x (1 + 2^-18).  An executed block is scored with v_min3_f32 over vertex pairs,
//           index bookkeeping once per block; a block whose minimum comes within the margin of the smallest one is remembered as the runner-up.
//   resolve the winning block -- and the runner-up, ~1e-4 of the points -- is re-scored with the EXACT E; among the records at the exact minimum
//           the LOWEST ORIGINAL vertex index wins.  A point with more than one runner-up (~1e-8) is rescanned over all records with E.  Exactly
//           the brute force's lowest-index-wins rule, independent of the scan order and of the ranking distance.  (A rescan costs its
//           workgroup as much as the whole frame: with every near-tie rescanned the kernel was 10 % SLOWER than the exact-ranked scan.)
// Then the normal of the nearest vertex from its incident faces (adjacency as (a, b) record pairs: ONE 8-byte load per face instead
// of face id -> corner -> three vertex ids), the signed distance, the marker distances.  The per-point loss goes to LDS by scan
// position and is reduced in a fixed tree: deterministic whatever wave scored the point.
constexpr int MAXM = 128;
// sqrtf(d2) < 0.02f  <=>  d2 < MARK_D2: the smallest float whose (correctly rounded) square root is >= 0.02f -- 0x39d1b716, one ulp below 0.02f * 0.02f
constexpr float MARK_D2 = 0.00039999996079131961f;
constexpr int CB = 16;                 // vertices per culling / index-bookkeeping block
constexpr int SB = 8;                  // blocks per super-block (128 vertices): its box is tested first, 8 block tests are skipped at once
constexpr int SEED_STRIDE = 4;         // the seed looks at the first record of every 4th block
constexpr int CT = 1024;               // threads per workgroup
constexpr int TASK = 64;               // points per task = one per lane
typedef float v2f __attribute__((ext_vector_type(2)));

// LDS image of the frame (float4 units).  Records: pair p = scan positions 2p, 2p+1 -> {x0 x1 y0 y1}, {z0 z1 - -}.  Boxes: pair j = boxes
// 2j, 2j+1 -> {lox0 lox1 loy0 loy1}, {loz0 loz1 hix0 hix1}, {hiy0 hiy1 hiz0 hiz1}.
struct ContactLds {
    int V4, nCB, nSB, nSeed;
    int rec, mark, box, sbox, seed, flags, red, pl, total;         // offsets in float4 units
    __host__ __device__ explicit ContactLds(int V) {
        V4 = (V + CB - 1) / CB * CB; nCB = V4 / CB; nSB = (nCB + SB - 1) / SB; nSeed = (nCB + SEED_STRIDE - 1) / SEED_STRIDE;
        rec = 0;
        mark = rec + V4;                             // V4 / 2 pairs x 2 float4
        box = mark + MAXM;
        sbox = box + 3 * (nSB * SB / 2);             // block boxes as pairs, padded with dummies to whole super-blocks
        seed = sbox + 3 * ((nSB + 2) / 2);
        flags = seed + 2 * ((nSeed + 1) / 2);        // [MAXM] int, [CT] float, [MAXP] float: in the dynamic region since round 6 (the launch that carries the predictor's
        red = flags + MAXM / 4;                      // workgroups shares ONE LDS size between both roles: statics of one role would sit on top of the other's 152 KB)
        pl = red + CT / 4;
        total = pl + MAXP / 4;
    }
};

__device__ __forceinline__ float3 lds_rec(const float4 *vs, int pos) {                // record at scan position pos
    const float *f = reinterpret_cast<const float *>(vs + 2 * (pos >> 1));
    const int h = pos & 1;
    return make_float3(f[h], f[2 + h], f[4 + h]);
}
__device__ __forceinline__ void lds_rec_store(float4 *vs, int pos, float x, float y, float z) {
    float *f = reinterpret_cast<float *>(vs + 2 * (pos >> 1));
    const int h = pos & 1;
    f[h] = x; f[2 + h] = y; f[4 + h] = z;
}
__device__ __forceinline__ void lds_box_store(float4 *bx, int k, float3 lo, float3 hi) {   // box k of a pair array
    float *f = reinterpret_cast<float *>(bx + 3 * (k >> 1));
    const int h = k & 1;
    f[h] = lo.x; f[2 + h] = lo.y; f[4 + h] = lo.z; f[6 + h] = hi.x; f[8 + h] = hi.y; f[10 + h] = hi.z;
}
__device__ __forceinline__ void lds_box_load(const float4 *bx, int k, float3 &lo, float3 &hi) {
    const float *f = reinterpret_cast<const float *>(bx + 3 * (k >> 1));
    const int h = k & 1;
    lo = make_float3(f[h], f[2 + h], f[4 + h]);
    hi = make_float3(f[6 + h], f[8 + h], f[10 + h]);
}

// OPT = the instantiation of the physics post-optimisation (optimize.hip, optimization.py:64-65): the object points come already
// transformed per frame (pts_frame [N][P][3]), frames are clip-major (clip = n / frames_per_clip) and the only output is the nearest
// vertex of every point -- no normals, markers or loss (the per-vertex contact-radius mask of :74-75 is its own kernel there).
// WITH_PRED (the correction hook, round 6): the launch carries `pred.nclips` extra LEADING workgroups that run the contact-frame predictor's three stacks (csrc/objproj.h PART 1: one
// clip each, 250 us, markers gathered from the posed vertices) beside the scan's N frame workgroups -- the predictor needs the markers only, the contact labels only pick which node's
// IDCT is evaluated afterwards (idf_objproj_pick).  Leading, so they are dispatched first; one launch, so nothing depends on a second queue (a side stream was tried first: its
// blocked barrier packet cost the caller's queue ~1 us per kernel launch for as long as the host ran ahead -- +27 us per step inside the sampler, profiles/r06_hook_overlap.txt).
struct PredArgs {
    idf_objproj op;
    const float *obj_angles, *obj_trans;      // [T][B][6], [T][B][3]
    const int32_t *markers_idx;               // [M] original vertex ids
    float *markers, *keep;                    // [N][M][3] (written here, frames time-major), [B][idf_objproj_keep_floats()]
    int nclips;
};
template <bool OPT, bool WITH_PRED = false>
__global__ __launch_bounds__(CT) void corr_contact_kernel(const float *__restrict__ verts, int V,
                                                          const float *__restrict__ obj_points, int P,
                                                          const int32_t *__restrict__ porder /* nullable [B][P]: scan position -> point */,
                                                          const float *__restrict__ objR, const float *__restrict__ objT,
                                                          const int32_t *__restrict__ faces /* identity order only */,
                                                          const int32_t *__restrict__ adj_ptr,
                                                          const int32_t *__restrict__ adj_face,
                                                          const int32_t *__restrict__ adj_corner,
                                                          const int32_t *__restrict__ adj_pair /* nullable [nnz][2]: per incident face the scan positions (a, b): normal += (a - v) x (b - v) */,
                                                          const int32_t *__restrict__ vorder /* nullable [V]: scan position -> vertex */,
                                                          const int32_t *__restrict__ vrank /* nullable [V]: vertex -> scan position (the inverse): the frame's vertices are then read in their own order */,
                                                          const int32_t *__restrict__ markers_pos /* scan positions */, int M, int B,
                                                          float *__restrict__ markers_out, float *__restrict__ loss_sum,
                                                          float *__restrict__ min_dist, int32_t *__restrict__ label,
                                                          float *__restrict__ o2h_out /* nullable [N][P] */,
                                                          int32_t *__restrict__ idx_out /* nullable [N][P]: nearest vertex */,
                                                          unsigned long long *__restrict__ stats /* nullable [IDF_CONTACT_STATS]: see interdiff_contact_nn */,
                                                          int64_t nn_from /* frames below it skip the NN scan */,
                                                          const float *__restrict__ pts_frame /* OPT: [N][P][3] */, int frames_per_clip /* OPT */,
                                                          const PredArgs pred) {
    extern __shared__ __attribute__((aligned(16))) float4 vs[];
    if constexpr (WITH_PRED) {
        if ((int)blockIdx.x < pred.nclips) {
            // predictor role: this clip's markers out of the posed vertices (what the scan's workgroups also write when asked to), then the three stacks
            const int b = blockIdx.x, Tn = pred.op.T;
            for (int i = threadIdx.x; i < Tn * M; i += CT) {
                const int t = i / M, m = i - t * M;
                const size_t nfr = (size_t)t * B + b;
                const float *v = verts + (nfr * V + pred.markers_idx[m]) * 3;
                float *o = pred.markers + (nfr * M + m) * 3;
                o[0] = v[0]; o[1] = v[1]; o[2] = v[2];
            }
            __threadfence();
            __syncthreads();
            idf_objproj_dev::objproj_body<1>(reinterpret_cast<float *>(vs), pred.op, pred.obj_angles, pred.obj_trans, pred.markers, nullptr, B, b, pred.keep, nullptr);
            return;
        }
    }
    const ContactLds L(V);
    const int nCB = L.nCB, nSB = L.nSB;
    float4 *ms = vs + L.mark, *bb = vs + L.box, *sbb = vs + L.sbox, *sd = vs + L.seed;
    int *flags = reinterpret_cast<int *>(vs + L.flags);
    float *red = reinterpret_cast<float *>(vs + L.red);
    float *pl = reinterpret_cast<float *>(vs + L.pl);                       // per-point loss by scan position
    __shared__ int next_task;
    const int64_t n = WITH_PRED ? (int64_t)blockIdx.x - pred.nclips : (int64_t)blockIdx.x;
    const int b = OPT ? (int)(n / frames_per_clip) : (int)(n % B), tid = threadIdx.x;
    const float *vf = verts + (size_t)n * V * 3;
    const bool do_nn = n >= nn_from;
    // phase clocks of thread 0 (frames that scan only), summed into stats[3 + phase] when the caller asks for statistics
    long long t_prev = 0;
    int n_phase = 0;
    auto phase_done = [&]() {
        if (stats && tid == 0 && do_nn) {
            const long long now = (long long)__builtin_readcyclecounter();
            if (n_phase > 0) atomicAdd(stats + 3 + n_phase, (unsigned long long)(now - t_prev));
            t_prev = now;
        }
        ++n_phase;
    };
    phase_done();
    // (requested first, consumed behind the record gather: the object transform of the frame and this thread's marker position)
    float R[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, tr[3] = {0.f, 0.f, 0.f};
    if constexpr (!OPT) {
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = objR[n * 9 + k];
#pragma unroll
        for (int k = 0; k < 3; ++k) tr[k] = objT[n * 3 + k];
    }
    const int my_marker_pos = (!OPT && tid < M) ? markers_pos[tid] : 0;
    // records -> LDS, four scan positions per thread and trip: all four permutation loads fly together, then all twelve coordinate loads (a gather from the skinning
    // kernel's output through two dependent round trips per TRIP instead of per position: 21 k -> ~8 k cycles of a ~350 k-cycle workgroup, tools/contact_probe.py).  The spare
    // words of a record pair carry the ORIGINAL vertex ids of its two records: the resolve step below reads them from LDS instead of gathering vorder[] per candidate.
    if (vorder && vrank) {
        // with the inverse permutation: vertices in THEIR order (a wave's 12-byte loads cover 768 contiguous bytes instead of 64 cache lines -- the gather below is bound by
        // line requests: 19 k cycles per workgroup), scattered into LDS by scan position
        for (int i0 = tid; i0 < V; i0 += 4 * CT) {
            typedef float f3v __attribute__((ext_vector_type(3), aligned(4)));
            int pos[4];
            f3v pv[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int i = min(i0 + k * CT, V - 1);
                pos[k] = vrank[i];
                pv[k] = *reinterpret_cast<const f3v *>(vf + 3 * i);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (i0 + k * CT < V) {
                    lds_rec_store(vs, pos[k], pv[k].x, pv[k].y, pv[k].z);
                    reinterpret_cast<int *>(vs + 2 * (pos[k] >> 1) + 1)[2 + (pos[k] & 1)] = i0 + k * CT;
                }
            }
        }
        for (int v = V + tid; v < L.V4; v += CT) {                         // past the end: far away, no vertex
            lds_rec_store(vs, v, 3e18f, 3e18f, 3e18f);
            reinterpret_cast<int *>(vs + 2 * (v >> 1) + 1)[2 + (v & 1)] = 0x7fffffff;
        }
    } else
    for (int v0 = tid; v0 < L.V4; v0 += 4 * CT) {
        int o[4];
        float x[4], y[4], z[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int v = v0 + k * CT;
            o[k] = v < V ? (vorder ? vorder[v] : v) : -1;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            x[k] = y[k] = z[k] = 3e18f;                                       // past the end: far away
            if (o[k] >= 0) {                                                  // ONE 12-byte load per vertex (global_load_dwordx3): a scattered gather is bound by instructions x lanes, not bytes
                typedef float f3v __attribute__((ext_vector_type(3), aligned(4)));
                const f3v pv = *reinterpret_cast<const f3v *>(vf + 3 * o[k]);
                x[k] = pv.x; y[k] = pv.y; z[k] = pv.z;
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int v = v0 + k * CT;
            if (v < L.V4) {
                lds_rec_store(vs, v, x[k], y[k], z[k]);
                reinterpret_cast<int *>(vs + 2 * (v >> 1) + 1)[2 + (v & 1)] = o[k] >= 0 ? o[k] : 0x7fffffff;
            }
        }
    }
    if (tid < MAXM) flags[tid] = 0;
    // gridDim.y workgroups share a frame's tasks (OPT: 320 frames on 256 CUs would otherwise take two full rounds)
    const int ntask_all = (P + TASK - 1) / TASK;
    const int task0 = (int)((long long)blockIdx.y * ntask_all / gridDim.y), task1 = (int)((long long)(blockIdx.y + 1) * ntask_all / gridDim.y);
    if (tid == 0) next_task = task0;
    for (int i = tid; i < MAXP; i += CT) pl[i] = 0.f;
    __syncthreads();
    phase_done();                                                          // 1: records in LDS
    if (!OPT && tid < ((M + 1) & ~1)) {                                    // markers as PAIRS, like the vertex records: pair p = markers 2p, 2p + 1 -> {x0 x1 y0 y1}, {z0 z1 - -}; a missing second marker sits far away
        float3 mk = make_float3(3e18f, 3e18f, 3e18f);
        if (tid < M) {
            mk = lds_rec(vs, my_marker_pos);
            if (markers_out) {                                             // (null in the hook's fused route: the predictor role above gathers them, in this same launch)
                float *mo = markers_out + ((size_t)n * M + tid) * 3;
                mo[0] = mk.x; mo[1] = mk.y; mo[2] = mk.z;
            }
        }
        lds_rec_store(ms, tid, mk.x, mk.y, mk.z);
    }
    if (do_nn) {
        // boxes: a wave takes the 64 record pairs of one super-block (8 blocks x 8 pairs), every lane the min / max of its pair; an 8-lane
        // reduction on the DPP path gives the block boxes, the wave reduction the super-block box.  (A first version -- one thread per
        // block reading its 16 records one by one, then one thread per super-block -- took 25 k cycles of a 390 k-cycle workgroup.)
#define IDF_DPP8(v, op, ctrl) v = op(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, v), __builtin_bit_cast(int, v), ctrl, 0xf, 0xf, false)))
        const int lane_ = tid & 63, wave_ = tid >> 6, nsw = 2 * ((nSB + 2) / 2);
        for (int sb = wave_; sb < nsw; sb += CT / 64) {
            const int pr = sb * 64 + lane_;                                  // record pair
            float lx = FLT_MAX, ly = FLT_MAX, lz = FLT_MAX, hx = -FLT_MAX, hy = -FLT_MAX, hz = -FLT_MAX;
            if (2 * pr < V) {
                const float4 xy = vs[2 * pr], zz = vs[2 * pr + 1];
                const bool two = 2 * pr + 1 < V;
                lx = two ? fminf(xy.x, xy.y) : xy.x; hx = two ? fmaxf(xy.x, xy.y) : xy.x;
                ly = two ? fminf(xy.z, xy.w) : xy.z; hy = two ? fmaxf(xy.z, xy.w) : xy.z;
                lz = two ? fminf(zz.x, zz.y) : zz.x; hz = two ? fmaxf(zz.x, zz.y) : zz.x;
            }
            // quad xor 1, quad xor 2, half-row mirror: every lane of an 8-lane group ends with the group's value
            IDF_DPP8(lx, fminf, 0xB1); IDF_DPP8(lx, fminf, 0x4E); IDF_DPP8(lx, fminf, 0x141);
            IDF_DPP8(ly, fminf, 0xB1); IDF_DPP8(ly, fminf, 0x4E); IDF_DPP8(ly, fminf, 0x141);
            IDF_DPP8(lz, fminf, 0xB1); IDF_DPP8(lz, fminf, 0x4E); IDF_DPP8(lz, fminf, 0x141);
            IDF_DPP8(hx, fmaxf, 0xB1); IDF_DPP8(hx, fmaxf, 0x4E); IDF_DPP8(hx, fmaxf, 0x141);
            IDF_DPP8(hy, fmaxf, 0xB1); IDF_DPP8(hy, fmaxf, 0x4E); IDF_DPP8(hy, fmaxf, 0x141);
            IDF_DPP8(hz, fmaxf, 0xB1); IDF_DPP8(hz, fmaxf, 0x4E); IDF_DPP8(hz, fmaxf, 0x141);
            const int cb = sb * SB + (lane_ >> 3);
            if ((lane_ & 7) == 0 && cb < nSB * SB) lds_box_store(bb, cb, make_float3(lx, ly, lz), make_float3(hx, hy, hz));
            const float slx = -wave_max(-lx), sly = -wave_max(-ly), slz = -wave_max(-lz), shx = wave_max(hx), shy = wave_max(hy), shz = wave_max(hz);
            if (lane_ == 0) lds_box_store(sbb, sb, make_float3(slx, sly, slz), make_float3(shx, shy, shz));
        }
#undef IDF_DPP8
        for (int k = tid; k < 2 * ((L.nSeed + 1) / 2); k += CT) {           // seed records: the first record of every SEED_STRIDE-th block, as pairs
            const float3 p = lds_rec(vs, min(k * SEED_STRIDE, nCB - 1) * CB);
            lds_rec_store(sd, k, p.x, p.y, p.z);
        }
    }
    const float *op = OPT ? pts_frame + (size_t)n * P * 3 : obj_points + (size_t)b * P * 3;
    const int ln = tid & 63, ntask = task1;
    __syncthreads();
    phase_done();                                                          // 2: boxes, markers
    float mind2 = FLT_MAX;                                                  // squared distance to the nearest marker over this thread's points
    unsigned n_exec = 0, n_test = 0, n_tasks = 0;
    for (;;) {
        int task = 0;
        if (ln == 0) task = atomicAdd(&next_task, 1);
        task = __builtin_amdgcn_readfirstlane(task);
        if (task >= ntask) break;
        ++n_tasks;
        const int sp = task * TASK + ln;                                   // scan position of this lane's point
        const int i = sp < P ? (porder ? porder[(size_t)b * P + sp] : sp) : -1;
        const bool valid = i >= 0;
        float px = 0.f, py = 0.f, pz = 0.f;
        if (valid) { px = op[3 * i]; py = op[3 * i + 1]; pz = op[3 * i + 2]; }
        // matmul(points, R^T) + t  (eval_smpl_short.py:107); OPT: the caller's transformed points as they are
        const float qx = OPT ? px : (px * R[0] + py * R[1] + pz * R[2]) + tr[0];
        const float qy = OPT ? py : (px * R[3] + py * R[4] + pz * R[5]) + tr[1];
        const float qz = OPT ? pz : (px * R[6] + py * R[7] + pz * R[8]) + tr[2];
        // the signed object->human distance is only consumed on future frames (eval_smpl_short.py:121 slices
        // loss_dist_o[past_len:]); past frames only need the marker distances below
        if (do_nn) {
#pragma clang fp contract(off)
            const v2f QX = v2f{qx, qx}, QY = v2f{qy, qy}, QZ = v2f{qz, qz};
            // exact squared distances of the point to a record pair
            auto pair_d2 = [&](const float4 xy, const float4 zz) {
#pragma clang fp contract(off)
                const v2f dx = QX - v2f{xy.x, xy.y}, dy = QY - v2f{xy.z, xy.w}, dz = QZ - v2f{zz.x, zz.y};
                return (dx * dx + dy * dy) + dz * dz;
            };
            // The SCAN ranks vertices by a cheaper distance (round 6): A = fma(dz, dz, fma(dy, dy, dx * dx)) -- 7 instead of 9 instructions per record pair, 3 roundings like the
            // exact E = (dx * dx + dy * dy) + dz * dz over the same rounded differences, so |A / E - 1| <= 6 u (u = 2^-24; all terms non-negative, no cancellation).  It only FILTERS:
            // every comparison that could drop a vertex carries the margin SCAN_M = 1 + 2^-18 (64 u) plus 1e-37 for the subnormal range, the winning block is re-scored with E, and a
            // point whose runner-up block came within the margin is rescanned over all records with E -- the answer is the brute force's (lowest original index at the exact minimum).
            auto pair_a2 = [&](const float4 xy, const float2 zz) {
                const v2f dx = QX - v2f{xy.x, xy.y}, dy = QY - v2f{xy.z, xy.w}, dz = QZ - v2f{zz.x, zz.y};
                return __builtin_elementwise_fma(dz, dz, __builtin_elementwise_fma(dy, dy, dx * dx));
            };
            constexpr float SCAN_M = 1.000003814697265625f, SCAN_ABS = 1e-37f;
            // ---- seed: an upper bound of the minimum of A, widened by the margin: the cull threshold before any block has been scored
            float seed = FLT_MAX;
            for (int k = 0; k < (L.nSeed + 1) / 2; k += 4) {
                float4 xy[4]; float2 zz[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) { xy[u] = sd[2 * min(k + u, (L.nSeed + 1) / 2 - 1)]; zz[u] = *reinterpret_cast<const float2 *>(&sd[2 * min(k + u, (L.nSeed + 1) / 2 - 1) + 1]); }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const v2f a2 = pair_a2(xy[u], zz[u]);
                    seed = fminf(fminf(seed, a2.x), a2.y);
                }
            }
            float thr = __builtin_fmaf(seed, SCAN_M, SCAN_ABS);      // boxes with lb > thr hold no vertex within the margin of the minimum
            float best = FLT_MAX, bthr = FLT_MAX;                    // smallest block minimum of A so far, and the same widened by the margin
            int tie = 0;                                   // runner-up blocks within the margin of the smallest: 0, 1 (bblk2), 2 = more than one
            int bblk = 0, bblk2 = 0;                                  // first record of the block that last lowered the minimum
            // lower bounds of the point to a PAIR of boxes
            auto pair_lb = [&](const float4 a, const float4 bq, const float4 c) {
#pragma clang fp contract(off)
                const v2f ax = v2f{a.x, a.y} - QX, bx = QX - v2f{bq.z, bq.w};
                const v2f ay = v2f{a.z, a.w} - QY, by = QY - v2f{c.x, c.y};
                const v2f az = v2f{bq.x, bq.y} - QZ, bz = QZ - v2f{c.z, c.w};
                const v2f ex = v2f{fmaxf(fmaxf(ax.x, bx.x), 0.f), fmaxf(fmaxf(ax.y, bx.y), 0.f)};       // v_max3_f32
                const v2f ey = v2f{fmaxf(fmaxf(ay.x, by.x), 0.f), fmaxf(fmaxf(ay.y, by.y), 0.f)};
                const v2f ez = v2f{fmaxf(fmaxf(az.x, bz.x), 0.f), fmaxf(fmaxf(az.y, bz.y), 0.f)};
                // ex <= |dx| of every vertex in the box (subtraction is monotone), so the REAL sum of squares is a lower bound of every vertex's; three roundings here (<= 3 u up)
                // against three in E and A: far inside the margin of thr
                return __builtin_elementwise_fma(ez, ez, __builtin_elementwise_fma(ey, ey, ex * ex));
            };
            auto score_block = [&](int cb) {
                ++n_exec;
                const int v0 = cb * CB;
                float4 xy[CB / 2]; float2 zz[CB / 2];
#pragma unroll
                for (int u = 0; u < CB / 2; ++u) { xy[u] = vs[v0 + 2 * u]; zz[u] = *reinterpret_cast<const float2 *>(&vs[v0 + 2 * u + 1]); }
                float bm = FLT_MAX;
#pragma unroll
                for (int u = 0; u < CB / 2; ++u) {
                    const v2f a2 = pair_a2(xy[u], zz[u]);
                    bm = fminf(fminf(bm, a2.x), a2.y);                          // v_min3_f32
                }
                // a new smallest block: the previous one stays a candidate iff it is within the margin of this one; otherwise a block within the margin of the smallest is one.
                // ONE runner-up block is remembered (bblk2); a second one (tie == 2: ~1e-8 of the points) sends the point to the rescan over all records.
                if (bm < best) {
                    const float w = __builtin_fmaf(bm, SCAN_M, SCAN_ABS);
                    if (best <= w) { tie = tie ? 2 : 1; bblk2 = bblk; } else tie = 0;
                    best = bm; bblk = v0; bthr = w; thr = fminf(thr, w);
                } else if (bm <= bthr) { tie = tie ? 2 : 1; bblk2 = v0; }
            };
            auto scan_super = [&](int sb) {                 // the blocks of super-block sb, two box tests per instruction
                const int cb0 = sb * SB;                    // (fetching 2 or 4 box pairs ahead of their tests: no difference, profiles/r06_contact_bound.txt)
#pragma unroll
                for (int j = 0; j < SB / 2; ++j) {
                    const int cb = cb0 + 2 * j;             // boxes past nCB are dummies (lo = +max: lb = inf, never needed)
                    const float4 *bx = bb + 3 * (cb >> 1);
                    const v2f lb = pair_lb(bx[0], bx[1], bx[2]);
                    n_test += 2;
                    if (__builtin_amdgcn_ballot_w64(valid && lb.x <= thr) != 0ull) score_block(cb);
                    if (__builtin_amdgcn_ballot_w64(valid && lb.y <= thr) != 0ull) score_block(cb + 1);     // thr may just have dropped
                }
            };
            if (!vorder) {
                // identity order: consecutive vertex ids are not neighbours, the boxes cull next to nothing -- score every block (the
                // brute force of rounds 1-2 in task form) instead of paying for the tests as well
                for (int cb = 0; cb < nCB; ++cb) score_block(cb);
            } else
            for (int sb = 0; sb < nSB; sb += 2) {
                const float4 *bx = sbb + 3 * (sb >> 1);
                const v2f lb = pair_lb(bx[0], bx[1], bx[2]);
                n_test += 2;
                if (__builtin_amdgcn_ballot_w64(valid && lb.x <= thr) != 0ull) scan_super(sb);              // wave-uniform branches
                if (__builtin_amdgcn_ballot_w64(valid && lb.y <= thr) != 0ull) scan_super(sb + 1);
            }
            // resolve with the EXACT distance: inside the winning block (no other block came within the margin), else over all records (~1e-5 of the points): the smallest E, and among
            // the records that attain it the lowest ORIGINAL index -- the brute force's rule, whatever the scan order
            int pos = bblk, org = 0x7fffffff;
            float ebest = FLT_MAX;
            auto resolve_pair = [&](int pr) {                 // record pair pr: E = dist2_exact, original ids from the pair's spare words (0x7fffffff past V; those records sit at 3e18)
                const float4 xy = vs[2 * pr], zz = vs[2 * pr + 1];
                const v2f d2 = pair_d2(xy, zz);
                const int o0 = __builtin_bit_cast(int, zz.z), o1 = __builtin_bit_cast(int, zz.w);
                if (d2.x < ebest || (d2.x == ebest && o0 < org)) { ebest = d2.x; org = o0; pos = 2 * pr; }
                if (d2.y < ebest || (d2.y == ebest && o1 < org)) { ebest = d2.y; org = o1; pos = 2 * pr + 1; }
            };
            if (tie < 2) {
#pragma unroll
                for (int u = 0; u < CB / 2; ++u) resolve_pair((bblk >> 1) + u);
                if (tie) {                                // ~1e-4 of the points: the runner-up block as well
#pragma unroll
                    for (int u = 0; u < CB / 2; ++u) resolve_pair((bblk2 >> 1) + u);
                }
            } else {
                for (int pr = 0; pr < (V + 1) / 2; ++pr) resolve_pair(pr);
            }
            pos = min(pos, V - 1);
            if (org == 0x7fffffff) org = vorder ? vorder[pos] : pos;      // NaN input: nothing compared equal
            if constexpr (OPT) {
                if (valid) idx_out[(size_t)n * P + i] = org;
            } else if (valid) {
                // normal of the nearest vertex (data/tools.py:4-40 restricted to one vertex), from LDS, in the reference's accumulation order
                const float3 v3 = lds_rec(vs, pos);
                float3 acc = make_float3(0.f, 0.f, 0.f);
                const int e0 = adj_ptr[org], e1 = adj_ptr[org + 1];
                if (adj_pair) {
                    for (int e = e0; e < e1; e += 4) {               // four incident faces per trip: their (a, b) loads fly together
                        int2 ab[4];
#pragma unroll
                        for (int u = 0; u < 4; ++u) ab[u] = *reinterpret_cast<const int2 *>(adj_pair + 2 * (size_t)min(e + u, e1 - 1));
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            if (e + u < e1) {
                                const float3 nn = cross3(sub3(lds_rec(vs, ab[u].x), v3), sub3(lds_rec(vs, ab[u].y), v3));
                                acc.x += nn.x; acc.y += nn.y; acc.z += nn.z;
                            }
                        }
                    }
                } else {
                    for (int e = e0; e < e1; ++e) {
                        const int f = adj_face[e], c = adj_corner[e];
                        const float3 p0 = lds_rec(vs, faces[3 * f]), p1 = lds_rec(vs, faces[3 * f + 1]), p2 = lds_rec(vs, faces[3 * f + 2]);
                        float3 nn;
                        if (c == 1) nn = cross3(sub3(p2, p1), sub3(p0, p1));
                        else if (c == 2) nn = cross3(sub3(p0, p2), sub3(p1, p2));
                        else nn = cross3(sub3(p1, p0), sub3(p2, p0));
                        acc.x += nn.x; acc.y += nn.y; acc.z += nn.z;
                    }
                }
                const float nl = fmaxf(sqrtf(acc.x * acc.x + acc.y * acc.y + acc.z * acc.z), 1e-6f);
                const float vx = qx - v3.x, vy = qy - v3.y, vz = qz - v3.z;
                const float dt = (acc.x / nl) * vx + (acc.y / nl) * vy + (acc.z / nl) * vz;
                const float d = sqrtf(vx * vx + vy * vy + vz * vz);
                const float o2h = d * (dt > 0.f ? 1.f : (dt < 0.f ? -1.f : 0.f));
                if (o2h_out) o2h_out[(size_t)n * P + i] = o2h;
                if (idx_out) idx_out[(size_t)n * P + i] = org;
                pl[sp] = o2h < 0.f ? fabsf(o2h) * 20.0f : 0.f;                  // eval_smpl_short.py:113-119
            }
        }
        if (!OPT && valid) {
            // Marker distances (eval_smpl_short.py:110-112: contact label = some object point within 2 cm of the marker; min over everything for the clip's condition),
            // two markers per packed instruction, WITHOUT a square root per pair: sqrtf is monotone and correctly rounded, so min_m sqrtf(d2_m) = sqrtf(min_m d2_m)
            // (one root per workgroup, below) and sqrtf(d2) < 0.02f <=> d2 < MARK_D2 -- the smallest float whose root is >= 0.02f (tests/test_abi_and_host.py re-derives it).
            // d2 keeps the roundings the scalar form compiled to: fma(dy, dy, dx * dx) + dz * dz.  (Round 6: the correctly-rounded root, its fix-up and an exec-mask write
            // per marker were 35 instructions x 67 markers per task, a quarter of the kernel.)
#pragma clang fp contract(off)
            const v2f QX = v2f{qx, qx}, QY = v2f{qy, qy}, QZ = v2f{qz, qz};
            for (int p2 = 0; p2 < (M + 1) / 2; ++p2) {
                const float4 xy = ms[2 * p2], zz = ms[2 * p2 + 1];
                const v2f dx = v2f{xy.x, xy.y} - QX, dy = v2f{xy.z, xy.w} - QY, dz = v2f{zz.x, zz.y} - QZ;
                const v2f d2 = __builtin_elementwise_fma(dy, dy, dx * dx) + dz * dz;
                mind2 = fminf(fminf(mind2, d2.x), d2.y);
                if (__builtin_amdgcn_ballot_w64(fminf(d2.x, d2.y) < MARK_D2) != 0ull) {      // wave-uniform, rare
                    if (d2.x < MARK_D2) flags[2 * p2] = 1;                     // benign race: all writers store 1
                    if (d2.y < MARK_D2) flags[2 * p2 + 1] = 1;                 // (the dummy of an odd count is infinitely far: never)
                }
            }
        }
    }
    if (stats && ln == 0 && do_nn) {
        atomicAdd(stats, (unsigned long long)n_exec);
        atomicAdd(stats + 1, (unsigned long long)nCB * n_tasks);
        atomicAdd(stats + 2, (unsigned long long)n_test);
    }
    phase_done();                                                          // 3: this wave's tasks
    if constexpr (OPT) return;                                             // every wave has written its points' indices: nothing to reduce
    __syncthreads();
    phase_done();                                                          // 4: waiting for the other waves
    // deterministic block reductions: the per-point losses by scan position in a fixed tree
    float loss = 0.f;
#pragma unroll
    for (int k = 0; k < MAXP / CT; ++k) loss += pl[tid + CT * k];
    red[tid] = loss;
    __syncthreads();
    for (int s = CT / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    const float loss_total = red[0];
    __syncthreads();
    red[tid] = mind2;
    __syncthreads();
    for (int s = CT / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] = fminf(red[tid], red[tid + s]);
        __syncthreads();
    }
    if (tid == 0) { loss_sum[n] = loss_total; min_dist[n] = red[0] == FLT_MAX ? FLT_MAX : sqrtf(red[0]); }      // the one root of the frame (monotone: = the minimum of the roots)
    if (tid < M) label[(size_t)n * M + tid] = flags[tid];
    phase_done();                                                          // 5: reductions
    if (stats && tid == 0 && do_nn) atomicAdd(stats + 3, 1ull);            // workgroups counted
}

// (An fp32-MFMA "filter" variant of this scan -- g~ = |p|^2 - 2 q.p on v_mfma_f32_16x16x4, exact re-evaluation of
// the vertices inside the error band -- was built, verified bit-identical and measured on MI355X: its two sweeps run
// at 40% of the matrix pipe next to the VALU work that reads every product, 6.1 ms vs 5.0 ms per call for this kernel.
// The fp32 MFMA issues at the fp32 VALU rate on gfx950, so the filter cannot win)
size_t contact_lds_bytes(int V) { return (size_t)ContactLds(V).total * sizeof(float4); }

// Every operand of corr_contact_kernel by name; null / 0 = absent (value-initialise, then set what the call has).
struct ContactArgs {
    const float *verts; int V;                    // posed vertices [N][V][3]
    const float *obj_points; int P;               // canonical points [B][P][3] (!OPT; OPT: only idf_point_order read them)
    int32_t *porder;                              // nullable [B][P]; !OPT: WRITTEN here first (corr_point_order_kernel of obj_points), OPT: read only
    const float *objR, *objT;                     // !OPT: [N][9], [N][3]
    const idf_correction_ctx *ctx;                // topology, markers, scan order
    int B;
    float *markers, *loss_sum, *min_dist;         // !OPT outputs: nullable [N][M][3], [N], [N]
    int32_t *label;                               // !OPT: [N][M]
    float *o2h;                                   // nullable [N][P]
    int32_t *idx;                                 // nullable [N][P] (OPT: required)
    unsigned long long *stats;                    // nullable [IDF_CONTACT_STATS]
    int64_t nn_from;
    const float *pts_frame; int frames_per_clip;  // OPT
    PredArgs pred;                                // WITH_PRED; nclips = 0: no predictor workgroups
};

// The one launch of the scan.  Refusals in the order the three call sites had them: sizes, then the scan-order operand set, then the LDS opt-in.
template <bool OPT, bool WITH_PRED>
int launch_contact(hipStream_t s, int64_t N, const ContactArgs &a) {
    static_assert(!(OPT && WITH_PRED), "the predictor rides with the hook's scan only");
    // the scan's own LDS image stays under 160 KiB - 16384 in every form; the launch that also carries the predictor opts in to 160 KiB - 2048
    constexpr int SCAN_LDS_MAX = 160 * 1024 - 16384, LDS_LIMIT = WITH_PRED ? 160 * 1024 - 2048 : SCAN_LDS_MAX;
    const idf_correction_ctx *c = a.ctx;
    const size_t lds = contact_lds_bytes(a.V);
    if (lds > (size_t)SCAN_LDS_MAX || a.P > MAXP) return IDF_E_INVAL;
    // scan order: either all four of (vorder, faces_scan, markers_scan, adj_pair_scan) or none (identity order: same results, no culling benefit); OPT reads
    // neither faces nor markers and exists for the culled scan only: vorder it is
    const bool ordered = c->vorder != nullptr;
    if (OPT ? !ordered : (ordered != (c->faces_scan != nullptr) || ordered != (c->markers_scan != nullptr) || ordered != (c->adj_pair_scan != nullptr))) return IDF_E_INVAL;
    const int32_t *faces = OPT ? nullptr : ordered ? c->faces_scan : c->faces, *mpos = OPT ? nullptr : ordered ? c->markers_scan : c->markers_idx;
    const int32_t *adj_ptr = OPT ? nullptr : c->adj_ptr, *adj_face = OPT ? nullptr : c->adj_face, *adj_corner = OPT ? nullptr : c->adj_corner;
    const int32_t *adj_pair = OPT ? nullptr : c->adj_pair_scan;
    const int M = OPT ? 0 : c->n_markers;
    if (!OPT && a.porder) hipLaunchKernelGGL(corr_point_order_kernel, dim3((unsigned)a.B), dim3(1024), 0, s, a.obj_points, a.P, a.porder);
    // one LDS size for both roles (the predictor's stacks need 152 KB, the scan less); the predictor's workgroups lead the grid
    const int nclips = WITH_PRED ? a.pred.nclips : 0;
    const size_t lds_launch = (nclips > 0 && lds < idf_objproj_dev::OBJPROJ_LDS) ? idf_objproj_dev::OBJPROJ_LDS : lds;
    if (lds_launch > (size_t)LDS_LIMIT) return IDF_E_INVAL;
    static std::atomic<uint64_t> lds_ok{0};         // one per instantiation
    if (idf_opt_in_lds(reinterpret_cast<const void *>(corr_contact_kernel<OPT, WITH_PRED>), LDS_LIMIT, lds_ok) != IDF_OK) return IDF_E_LAUNCH;
    hipLaunchKernelGGL((corr_contact_kernel<OPT, WITH_PRED>), OPT ? dim3((unsigned)N, 2) : dim3((unsigned)(N + nclips)), dim3(CT), lds_launch, s, a.verts, a.V,
                       a.obj_points, a.P, a.porder, a.objR, a.objT, faces, adj_ptr, adj_face, adj_corner, adj_pair, c->vorder, c->vrank, mpos, M, a.B,
                       a.markers, a.loss_sum, a.min_dist, a.label, a.o2h, a.idx, a.stats, a.nn_from, a.pts_frame, a.frames_per_clip, a.pred);
    return IDF_OK;
}

}  // namespace
