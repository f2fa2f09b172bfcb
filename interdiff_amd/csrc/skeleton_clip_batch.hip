// The skeleton-mode training set on the device (interdiff_amd/skeleton_dataset.py SkeletonClipSet): ingestion of the raw videos in one launch and a batch of
// windows in one launch.
//
// skeleton_video_prepare_kernel   data/dataset_skeleton.py:40-65, 85-104 and the down-sampling of :148-151 for every video of a set: one workgroup per video.
//      1. the quaternion sign of get_consistent_poses (:53-65).  The reference flips frame i+1 iff |s_i q_i - q_{i+1}| > |s_i q_i + q_{i+1}|, and otherwise
//         leaves it AS STORED.  With d_i the dot product of the RAW quaternions in double that is: d_i < 0 -> s_{i+1} = -s_i; d_i > 0 -> s_{i+1} = s_i;
//         a tie (d_i == 0: a zero quaternion, an orthogonal pair) or a NaN -> s_{i+1} = +1 whatever s_i was.  So the sign is a SEGMENTED prefix parity:
//         a tie / NaN transition resets it.  The workgroup scans it in chunks of SKV_THREADS transitions: two ballots per wave (flip, reset); a lane with
//         a reset at or below it counts the flips above the highest such reset and ignores what came before, any other lane counts the flips at or below
//         it and adds the incoming parity; a wave's summary (has a reset, parity after its last reset) goes through LDS, and the waves and the carry
//         between chunks are folded in order by the same composition: integers only, one pass.  Without a tie / NaN it is the plain prefix parity.
//         Frames that are no multiple of `stride` are read for this and for the contact sum, nothing else of them is touched.
//      2. the resident table fp32 [rows][3 J + 3 P + 7] = body | object | pose, row r = frame stride * r, the quaternion times its sign: every float64 is
//         rounded once, so an entry is the reference's batch[i].float() bit for bit.
//      3. zero_pose_obj = recover_init_obj on frame 0 (:40-51) in double, rounded once.
//      4. per video three doubles -- the discrepancy of :98-99, the check sum of :93 (signed), the full-rate contact sum -- each the sum of SKV_THREADS strided
//         partial sums folded by a fixed tree, and the contact value of every row.
//   The per-element math is host + device inline and compiled without contraction (the pragma below), so interdiff_debug_skeleton_video_prepare -- the same
//   order of additions on the CPU -- gives the same bits.
// skeleton_window_batch_kernel   one workgroup per clip: the clip's T rows are ONE contiguous run of the table; it is read once into an LDS tile (leading
//      dimension odd: the transposed read below is conflict-free) and written out five times -- body [B,T,J,3], obj [B,T,P,3], pose [B,T,7] straight,
//      the token gt [B,1,3J+3P+7,T] transposed, zero_pose_obj [B,P,3] -- every global load and store contiguous across the lanes.
#include "common.h"
#include <math.h>

#pragma clang fp contract(off)          // host and device round every product and sum on its own: the two instances agree bit for bit

#define SK_HD __host__ __device__ inline

namespace {

// scipy's Rotation.from_quat(..).as_matrix() on (x, y, z, w), as csrc/clip_canon.h restates it; defined HERE so that they are compiled under the pragma above
struct Quat { double x, y, z, w; };

SK_HD Quat normalized(Quat q) {
    const double n = sqrt(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
    return Quat{q.x / n, q.y / n, q.z / n, q.w / n};
}

SK_HD void as_matrix(const Quat &q, double *m) {
    const double x2 = q.x * q.x, y2 = q.y * q.y, z2 = q.z * q.z, w2 = q.w * q.w;
    const double xy = q.x * q.y, zw = q.z * q.w, xz = q.x * q.z, yw = q.y * q.w, yz = q.y * q.z, xw = q.x * q.w;
    m[0] = x2 - y2 - z2 + w2; m[1] = 2.0 * (xy - zw);     m[2] = 2.0 * (xz + yw);
    m[3] = 2.0 * (xy + zw);   m[4] = -x2 + y2 - z2 + w2;  m[5] = 2.0 * (yz - xw);
    m[6] = 2.0 * (xz - yw);   m[7] = 2.0 * (yz + xw);     m[8] = -x2 - y2 + z2 + w2;
}

SK_HD void mat_vec(const double *m, const double *v, double *o) {
    o[0] = m[0] * v[0] + m[1] * v[1] + m[2] * v[2];
    o[1] = m[3] * v[0] + m[4] * v[1] + m[5] * v[2];
    o[2] = m[6] * v[0] + m[7] * v[1] + m[8] * v[2];
}

constexpr int SKV_THREADS = 256;          // prepare: the workgroup, the scan's chunk and the width of the summation tree
constexpr int SKV_MAX_P = 64;             // object points per video (LDS copy of the double zero pose)
constexpr int SKW_THREADS = 256, SKW_MAX_T = 128, SKW_LDS_BYTES = 64 * 1024;

struct Video {
    const double *skel, *obj, *pose, *contact;      // this video's first frame
    int64_t F, rows;
    int J, P, stride;
};

// what the transition frame i -> i + 1 does to the sign: 0 keeps it, 1 flips it, 2 resets it to + (a tie or a NaN: the reference's `>` is false, and it then
// leaves frame i + 1 as stored -- it does NOT carry frame i's sign over)
SK_HD int flip_bit(const double *pose, int64_t i) {
    const double *a = pose + 7 * i + 3, *b = a + 7;
    const double d = a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3];
    return d < 0.0 ? 1 : (d > 0.0 ? 0 : 2);
}

SK_HD Quat unit_quat(const double *pose) {             // Rot.from_quat normalises
    return normalized(Quat{pose[3], pose[4], pose[5], pose[6]});
}

SK_HD void zero_pose_point(const double *pose0, const double *obj0, int p, double *z) {
    const Quat q = unit_quat(pose0);
    double m[9], v[3];
    as_matrix(Quat{-q.x, -q.y, -q.z, q.w}, m);
    for (int k = 0; k < 3; ++k) v[k] = obj0[3 * p + k] - pose0[k];
    mat_vec(m, v, z);
}

SK_HD double discrep_item(const Video &v, const double *zpo, int64_t item) {      // |t + R(q) z - obj| of (row, point)
    const int64_t r = item / v.P, f = r * v.stride;
    const int p = (int)(item - r * v.P);
    const double *ps = v.pose + 7 * f, *o = v.obj + (f * v.P + p) * 3;
    double m[9], w[3];
    as_matrix(unit_quat(ps), m);
    mat_vec(m, zpo + 3 * p, w);
    const double dx = ps[0] + w[0] - o[0], dy = ps[1] + w[1] - o[1], dz = ps[2] + w[2] - o[2];
    return sqrt(dx * dx + dy * dy + dz * dz);
}

SK_HD double partial_discrep(const Video &v, const double *zpo, int tid) {
    double a = 0.0;
    for (int64_t e = tid; e < v.rows * v.P; e += SKV_THREADS) a += discrep_item(v, zpo, e);
    return a;
}

SK_HD double partial_check(const Video &v, int tid) {         // sum of |q| - 1 over the sampled rows, signed as in the reference's assert
    double a = 0.0;
    for (int64_t r = tid; r < v.rows; r += SKV_THREADS) {
        const double *q = v.pose + 7 * r * v.stride + 3;
        a += sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]) - 1.0;
    }
    return a;
}

SK_HD double partial_contact(const Video &v, int tid) {
    double a = 0.0;
    for (int64_t f = tid; f < v.F; f += SKV_THREADS) a += v.contact[f];
    return a;
}

SK_HD void write_pose_row(const Video &v, float *tab, int W, int64_t r, int neg) {
    const double *ps = v.pose + 7 * r * v.stride;
    float *o = tab + r * W + (W - 7);
    for (int k = 0; k < 3; ++k) o[k] = (float)ps[k];
    for (int k = 3; k < 7; ++k) o[k] = (float)(neg ? -ps[k] : ps[k]);
}

SK_HD void write_table_elem(const Video &v, float *tab, int W, int64_t e) {      // element e of the [rows][3 J + 3 P] body | object part
    const int nb = 3 * v.J, no = 3 * v.P, nc = nb + no;
    const int64_t r = e / nc, f = r * v.stride;
    const int c = (int)(e - r * nc);
    tab[r * W + c] = (float)(c < nb ? v.skel[f * nb + c] : v.obj[f * no + (c - nb)]);
}

__device__ double tree_sum(double *red, double x, int tid) {
    red[tid] = x;
    __syncthreads();
    for (int off = SKV_THREADS / 2; off > 0; off >>= 1) {
        if (tid < off) red[tid] += red[tid + off];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

double tree_sum_host(double *red) {                               // the same additions in the same order
    for (int off = SKV_THREADS / 2; off > 0; off >>= 1)
        for (int tid = 0; tid < off; ++tid) red[tid] += red[tid + off];
    return red[0];
}

__global__ __launch_bounds__(SKV_THREADS) void skeleton_video_prepare_kernel(const double *__restrict__ skel, const double *__restrict__ obj,
                                                                              const double *__restrict__ pose, const double *__restrict__ contact,
                                                                              const int64_t *__restrict__ seq_off, const int64_t *__restrict__ row_off, int J, int P,
                                                                              int stride, float *__restrict__ table, float *__restrict__ zero_pose_obj,
                                                                              double *__restrict__ report, double *__restrict__ row_contact, int8_t *__restrict__ signs) {
    __shared__ double red[SKV_THREADS];
    __shared__ double zpo[3 * SKV_MAX_P];
    __shared__ unsigned wave_par[SKV_THREADS / IDF_WAVE];
    const int vid = blockIdx.x, tid = threadIdx.x;
    const int64_t f0 = seq_off[vid], F = seq_off[vid + 1] - f0, r0 = row_off[vid], rows = row_off[vid + 1] - r0;
    if (f0 < 0 || r0 < 0 || F <= 0 || rows != (F + stride - 1) / stride) return;          // (a bad table never becomes an address; uniform over the workgroup)
    const Video v{skel + f0 * J * 3, obj + f0 * P * 3, pose + f0 * 7, contact + f0, F, rows, J, P, stride};
    const int W = 3 * J + 3 * P + 7;
    float *tab = table + r0 * W;

    // 1. the sign of every frame: segmented prefix parity of the flip bits (a reset starts a new segment), one chunk of SKV_THREADS transitions at a time
    if (tid == 0) {
        write_pose_row(v, tab, W, 0, 0);
        if (signs) signs[f0] = 1;
    }
    unsigned carry = 0;                                           // is the last frame before this chunk negated (the same in every lane)
    const int lane = tid & (IDF_WAVE - 1), wave = tid / IDF_WAVE;
    for (int64_t base = 0; base < F - 1; base += SKV_THREADS) {
        const int64_t i = base + tid;
        const int kind = i < F - 1 ? flip_bit(v.pose, i) : 0;
        const unsigned long long flips = __ballot(kind == 1), resets = __ballot(kind == 2);
        const unsigned long long upto = ~0ull >> (IDF_WAVE - 1 - lane);                   // this lane and the ones below it
        const unsigned long long mine = resets & upto;
        // the flips that count for this lane: those above the highest reset at or below it (all of them without one); ((2 << h) - 1 covers bits 0 .. h, h = 63 too)
        const unsigned long long after = mine ? ~((2ull << (63 - __clzll((long long)mine))) - 1ull) : ~0ull;
        unsigned par = (unsigned)__popcll(flips & upto & after) & 1u;                      // inclusive, inside the wave
        if (lane == 0) {
            const unsigned long long tail = resets ? ~((2ull << (63 - __clzll((long long)resets))) - 1ull) : ~0ull;
            wave_par[wave] = ((unsigned)__popcll(flips & tail) & 1u) | (resets ? 2u : 0u);   // bit 0: parity after the wave's last reset; bit 1: it has a reset
        }
        __syncthreads();
        unsigned before = carry, total = carry;
        for (int w = 0; w < SKV_THREADS / IDF_WAVE; ++w) {
            const unsigned s = wave_par[w];
            total = (s & 2u) ? (s & 1u) : (total ^ s);
            if (w + 1 == wave) before = total;
        }
        if (!mine) par ^= before;                                 // frame i + 1 is negated iff par; a reset at or below the lane cuts the incoming parity off
        if (i < F - 1) {
            if (signs) signs[f0 + i + 1] = par ? -1 : 1;
            if ((i + 1) % stride == 0) write_pose_row(v, tab, W, (i + 1) / stride, (int)par);
        }
        carry = total;
        __syncthreads();                                          // wave_par is rewritten by the next chunk
    }

    // 2. body | object of the sampled rows, the rows' contact values
    for (int64_t e = tid; e < rows * (3 * (J + P)); e += SKV_THREADS) write_table_elem(v, tab, W, e);
    for (int64_t r = tid; r < rows; r += SKV_THREADS) row_contact[r0 + r] = v.contact[r * stride];

    // 3. zero_pose_obj (kept in double for the discrepancy)
    if (tid < P) {
        double z[3];
        zero_pose_point(v.pose, v.obj, tid, z);
        for (int k = 0; k < 3; ++k) {
            zpo[3 * tid + k] = z[k];
            zero_pose_obj[((int64_t)vid * P + tid) * 3 + k] = (float)z[k];
        }
    }
    __syncthreads();

    // 4. the report
    const double disc = tree_sum(red, partial_discrep(v, zpo, tid), tid);
    const double chk = tree_sum(red, partial_check(v, tid), tid);
    const double con = tree_sum(red, partial_contact(v, tid), tid);
    if (tid == 0) {
        report[3 * (int64_t)vid] = disc / (double)(rows * P);
        report[3 * (int64_t)vid + 1] = chk;
        report[3 * (int64_t)vid + 2] = con;
    }
}

__global__ __launch_bounds__(SKW_THREADS) void skeleton_window_batch_kernel(idf_skel_clip_set cs, const int32_t *__restrict__ clips, int B, int T,
                                                                             idf_skel_window_batch out) {
    extern __shared__ float tile[];                               // [T][LD]
    const int b = blockIdx.x, tid = threadIdx.x;
    const int vid = clips[b], first = clips[B + b];
    if (vid < 0 || vid >= cs.n_video || first < 0) return;       // (the host checks before it launches; a bad clip is skipped, never dereferenced)
    const int64_t r0 = cs.row_off[vid], rows = cs.row_off[vid + 1] - r0;
    if (r0 < 0 || (int64_t)first + T > rows) return;
    const int nb = 3 * cs.J, no = 3 * cs.P, W = nb + no + 7, LD = W | 1;
    const float *src = cs.table + (r0 + first) * W;               // the clip's rows: one contiguous run
    for (int e = tid; e < T * W; e += SKW_THREADS) {
        const int t = e / W, c = e - t * W;
        tile[t * LD + c] = src[e];
    }
    __syncthreads();
    float *body = out.body + (size_t)b * T * nb, *obj = out.obj + (size_t)b * T * no, *pose = out.pose + (size_t)b * T * 7, *gt = out.gt + (size_t)b * W * T;
    for (int e = tid; e < T * nb; e += SKW_THREADS) {
        const int t = e / nb, c = e - t * nb;
        body[e] = tile[t * LD + c];
    }
    for (int e = tid; e < T * no; e += SKW_THREADS) {
        const int t = e / no, c = e - t * no;
        obj[e] = tile[t * LD + nb + c];
    }
    for (int e = tid; e < T * 7; e += SKW_THREADS) {
        const int t = e / 7, c = e - t * 7;
        pose[e] = tile[t * LD + nb + no + c];
    }
    for (int e = tid; e < W * T; e += SKW_THREADS) {              // the token: channel-major, frames contiguous
        const int c = e / T, t = e - c * T;
        gt[e] = tile[t * LD + c];
    }
    for (int e = tid; e < no; e += SKW_THREADS) out.zero_pose_obj[(size_t)b * no + e] = cs.zero_pose_obj[(size_t)vid * no + e];
}

}  // namespace

extern "C" int interdiff_skeleton_video_prepare(const double *skel, const double *obj, const double *pose, const double *contact, const int64_t *seq_off,
                                                const int64_t *row_off, int32_t n_video, int32_t J, int32_t P, int32_t stride, float *table, float *zero_pose_obj,
                                                double *report, double *row_contact, int8_t *signs, void *stream) {
    if (!skel || !obj || !pose || !contact || !seq_off || !row_off || n_video <= 0 || J <= 0 || P <= 0 || P > SKV_MAX_P || stride <= 0 || !table || !zero_pose_obj ||
        !report || !row_contact)
        return IDF_E_INVAL;
    hipLaunchKernelGGL(skeleton_video_prepare_kernel, dim3((unsigned)n_video), dim3(SKV_THREADS), 0, idf_stream(stream), skel, obj, pose, contact, seq_off, row_off,
                       J, P, stride, table, zero_pose_obj, report, row_contact, signs);
    IDF_CHECK_LAUNCH();
    return IDF_OK;
}

extern "C" int interdiff_skeleton_window_batch(const idf_skel_clip_set *cs, const int32_t *clips, int32_t B, int32_t T, const idf_skel_window_batch *out, void *stream) {
    if (!cs || cs->n_video <= 0 || cs->J <= 0 || cs->P <= 0 || !cs->row_off || !cs->table || !cs->zero_pose_obj || !clips || B <= 0 || T <= 0 || T > SKW_MAX_T || !out ||
        !out->body || !out->obj || !out->pose || !out->zero_pose_obj || !out->gt)
        return IDF_E_INVAL;
    const int64_t W = 3 * ((int64_t)cs->J + cs->P) + 7, lds = (int64_t)T * (W | 1) * (int64_t)sizeof(float);
    if (lds > SKW_LDS_BYTES) return IDF_E_INVAL;
    hipLaunchKernelGGL(skeleton_window_batch_kernel, dim3((unsigned)B), dim3(SKW_THREADS), (size_t)lds, idf_stream(stream), *cs, clips, B, T, *out);
    IDF_CHECK_LAUNCH();
    return IDF_OK;
}

// HOST instance of the per-video code: ONE video, the arrays of its F frames.  table [rows][3 J + 3 P + 7], zero_pose_obj [P][3], report [3],
// row_contact [rows], signs int8 [F] (or null); rows = ceil(F / stride).
extern "C" int interdiff_debug_skeleton_video_prepare(const double *skel, const double *obj, const double *pose, const double *contact, int64_t F, int32_t J, int32_t P,
                                                      int32_t stride, float *table, float *zero_pose_obj, double *report, double *row_contact, int8_t *signs) {
    if (!skel || !obj || !pose || !contact || F <= 0 || J <= 0 || P <= 0 || P > SKV_MAX_P || stride <= 0 || !table || !zero_pose_obj || !report || !row_contact)
        return IDF_E_INVAL;
    const int64_t rows = (F + stride - 1) / stride;
    const Video v{skel, obj, pose, contact, F, rows, J, P, stride};
    const int W = 3 * J + 3 * P + 7;
    int neg = 0;
    write_pose_row(v, table, W, 0, 0);
    if (signs) signs[0] = 1;
    for (int64_t i = 0; i < F - 1; ++i) {
        const int kind = flip_bit(pose, i);
        neg = kind == 2 ? 0 : neg ^ kind;
        if (signs) signs[i + 1] = neg ? -1 : 1;
        if ((i + 1) % stride == 0) write_pose_row(v, table, W, (i + 1) / stride, neg);
    }
    for (int64_t e = 0; e < rows * (3 * (J + P)); ++e) write_table_elem(v, table, W, e);
    for (int64_t r = 0; r < rows; ++r) row_contact[r] = contact[r * stride];
    double zpo[3 * SKV_MAX_P], red[SKV_THREADS];
    for (int p = 0; p < P; ++p) {
        zero_pose_point(pose, obj, p, zpo + 3 * p);
        for (int k = 0; k < 3; ++k) zero_pose_obj[3 * p + k] = (float)zpo[3 * p + k];
    }
    for (int t = 0; t < SKV_THREADS; ++t) red[t] = partial_discrep(v, zpo, t);
    report[0] = tree_sum_host(red) / (double)(rows * P);
    for (int t = 0; t < SKV_THREADS; ++t) red[t] = partial_check(v, t);
    report[1] = tree_sum_host(red);
    for (int t = 0; t < SKV_THREADS; ++t) red[t] = partial_contact(v, t);
    report[2] = tree_sum_host(red);
    return IDF_OK;
}
