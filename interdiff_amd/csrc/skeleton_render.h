// Skeleton-clip renderer, the inlines shared by the device kernels (skeleton_render.hip) and their host twins (interdiff_debug_skeleton_*).
//
// CONTRACT (restated bit for bit by tests/skeleton_render_oracle.py).
//   record   8 int32 per slot, slots in DRAW order: [0] kind (0 empty: all 8 are 0, 1 segment, 2 disc); [1] X0 [2] Y0 [3] X1 [4] Y1 screen positions in
//     1/16 pixel (IDF_RENDER_SUBPIX), origin = the image's top-left corner, y down, |X|, |Y| <= IDF_RENDER_GUARD (a disc: X1 = X0, Y1 = Y0);
//     [5] wd = FULL line width / disc diameter in 1/16 pixel, 1 .. SK_WD_MAX; [6] R | G << 8 | B << 16; [7] alpha 0 .. 255.
//   draw order   plain: 18 bones, 3 axis lines, then the two scatter collections -- the one whose NEAREST marker is farther first (equal: the body's) --
//     each far to near, equal depths the higher index first.  pred / gt: 3 axis lines, 18 pred bones, pred wires, 18 gt bones, gt wires; a group that is
//     not drawn in a frame keeps its slots, empty.  A dropped primitive leaves its slot empty (a dropped marker: the last slots of its collection).
//   coverage   pixel (i, j) is sampled at the 4 x 4 points S = (16 i + ox, 16 j + oy), ox, oy in {2, 6, 10, 14}; n = the number of covered samples.
//     disc      4 |S - C|^2 <= wd^2.
//     segment   d = B - A, L2 = d . d > 0, e = S - A, cr = d x e, t = d . e, ex = max(-t, t - L2):  covered iff (2 cr)^2 <= wd^2 L2 and
//               (ex <= 0 or (2 ex)^2 <= wd^2 L2) -- the stroke of width wd with PROJECTING caps (extended by wd / 2 beyond either end), edges included.
//     L2 = 0    the cap square alone: |2 (Sx - Ax)| <= wd and |2 (Sy - Ay)| <= wd.
//   blend     per channel a 16-bit accumulator acc in 1/256 of an 8-bit step, white (255 << 8) to begin with; a record with n > 0 folds in as
//     w = alpha n (0 .. 4080);  acc <- floor((acc (4080 - w) + (c8 << 8) w + 2040) / 4080)   ("over", rounded to nearest);  pixel = (acc + 128) >> 8.
//     Records fold in draw order: translucent "over" does not commute.
// BIT WIDTHS.  |X|, |Y| <= 2^15 and 0 <= S < 2^15: |d|, |e| < 2^16 + 1 per component, L2, |cr|, |t| < 2^34, wd <= 2^10 so wd^2 L2 < 2^54.  (2 cr)^2 would
// reach 2^70: a value of |2 cr| or 2 ex above wd << 17 is outside whatever L2 is (L < 2^17, so wd L / 1 < wd 2^17) and is replaced by (wd << 17) + 1
// < 2^28 before it is squared -- a pure early-out, the unbounded-integer restatement of the tests has no such step.  Blend: acc <= 65280, products
// <= 65280 * 4080 < 2^28: 32-bit arithmetic.
// SETUP (fp32, every rounding pinned: contraction off, explicit fmaf), per frame:
//   limits   lo / hi = min / max per axis over every FINITE point drawn in the frame (axis-line ends included); a = lo - (hi - lo) margin,
//            b = hi + (hi - lo) margin; m = (b - a) / 48; lo' = a - m, hi' = b + m; scale = aspect / (hi' - lo').
//   camera   W = (p - lo') scale; vx = view row 0 . (W, 1) as fmaf(r2, Wz, fmaf(r1, Wy, fmaf(r0, Wx, r3))), vy, vw likewise; d = -vw (distance along the
//            view axis, > 0); tx = vx / d, ty = vy / d, tz = -dist / d (larger = farther); X = rint(fmaf(tx, kx, cx)), Y = rint(fmaf(ty, ky, cy)).
//   shade    per scatter collection, over its valid markers: norm = (tz - tzmin) / (tzmax - tzmin) (0 when the range is 0);
//            alpha = rint(fmaf(norm, -178.5, 255)) -- 255 (1 - 0.7 norm); the farthest marker is 76.5 exactly and rounds to 76 in every precision.
#pragma once
#include <math.h>
#include <stdint.h>
#include "../../include/interdiff_hip.h"

#ifndef __HIPCC__
#define __host__
#define __device__
#endif

constexpr int SK_SUB = IDF_RENDER_SUBPIX, SK_GUARD = IDF_RENDER_GUARD, SK_REC = IDF_SKEL_REC_INTS, SK_MAX_REC = IDF_SKEL_MAX_REC;
constexpr int SK_WD_MAX = IDF_SKEL_WD_MAX, SK_TILE = IDF_SKEL_TILE;
constexpr int SK_NB = 21, SK_NO = 12, SK_NBONE = 18;
constexpr int SK_GT0 = SK_NB + SK_NO, SK_AX0 = 2 * SK_GT0, SK_NPT = SK_AX0 + 6;        // point table: body, obj, gt body, gt obj, axis-line ends
constexpr int SK_LANES = 128;                                                          // lanes of one frame's setup: one per slot and one per point
constexpr int SK_WDEN = 255 * 16;
static_assert(SK_NPT <= SK_LANES && SK_MAX_REC <= SK_LANES, "one lane per point and per slot");
static_assert(3 + 2 * (SK_NBONE + IDF_SKEL_MAX_WIRES) <= SK_MAX_REC && SK_NBONE + 3 + SK_NB + SK_NO <= SK_MAX_REC, "every style fits the slot table");
static_assert(IDF_RENDER_MAX_DIM * SK_SUB <= SK_GUARD, "samples stay inside the guard band");
static_assert(((int64_t)SK_WD_MAX << 17) + 1 < (1ll << 31) && (int64_t)SK_WD_MAX * SK_WD_MAX * (1ll << 34) < INT64_MAX, "the squares of the coverage test fit int64");

struct SkFrame {          // one frame's setup state: LDS in the kernel, the stack in the host twin
    float p[SK_NPT][3];
    float X[SK_NPT], Y[SK_NPT], tz[SK_NPT];
    float lim[6];                          // lo x, y, z, hi x, y, z
    float gz[2][2];                        // per scatter collection: tzmin, tzmax over its valid markers
    int32_t gn[2];                         // valid markers per collection
    int32_t rec[SK_MAX_REC][SK_REC];
    int32_t drop[SK_LANES];
    uint8_t drawn[SK_NPT], fin[SK_NPT], ok[SK_NPT];
};

struct SkArgs {
    const float *body, *obj, *body_gt, *obj_gt;       // the CLIP's arrays
    const int32_t *wires;
    int32_t n_wires, T, T_gt, t;
};

__host__ __device__ inline int sk_count(const idf_skel_view &v, int n_wires) {
    return v.style == IDF_SKEL_PLAIN ? SK_NBONE + 3 + SK_NB + SK_NO : 3 + 2 * (SK_NBONE + n_wires);
}

// render/viz_helper.py:11-15 `connections`
__host__ __device__ inline void sk_bone(int k, int &a, int &b) {
    constexpr int8_t tab[SK_NBONE][2] = {{0, 1}, {1, 2}, {2, 3}, {3, 4}, {2, 5}, {5, 6}, {6, 7}, {7, 8}, {2, 9}, {9, 10}, {10, 11}, {11, 12},
                                         {0, 13}, {13, 14}, {14, 15}, {0, 16}, {16, 17}, {17, 18}};
    a = tab[k][0]; b = tab[k][1];
}

// phase 1, lane = point: fetch (float32), note whether the frame draws it and whether it is finite.  Axis lines: viz_helper.py:50-52 / 86-88.
__host__ __device__ inline void sk_phase_load(SkFrame &f, int lane, const idf_skel_view &v, const SkArgs &a) {
    if (lane >= SK_NPT) return;
    const bool pred = v.style == IDF_SKEL_PLAIN || a.t >= v.pred_from;
    const bool gt = v.style == IDF_SKEL_PREDGT && a.body_gt != nullptr && a.t < a.T_gt;
    float x = 0.f, y = 0.f, z = 0.f;
    bool drawn;
    if (lane < SK_GT0) {
        drawn = pred;
        if (drawn) {
            const float *q = lane < SK_NB ? a.body + ((size_t)a.t * SK_NB + lane) * 3 : a.obj + ((size_t)a.t * SK_NO + (lane - SK_NB)) * 3;
            x = q[0]; y = q[1]; z = q[2];
        }
    } else if (lane < SK_AX0) {
        drawn = gt;
        if (drawn) {
            const int l = lane - SK_GT0;
            const float *q = l < SK_NB ? a.body_gt + ((size_t)a.t * SK_NB + l) * 3 : a.obj_gt + ((size_t)a.t * SK_NO + (l - SK_NB)) * 3;
            x = q[0]; y = q[1]; z = q[2];
        }
    } else {
        drawn = true;
        const int l = lane - SK_AX0, line = l >> 1, end = l & 1;
        if (line == 0) y = end ? 1.2f : -0.7f;
        else if (line == 1) x = end ? 1.2f : -1.2f;
        else z = end ? 1.2f : -1.2f;
    }
    f.p[lane][0] = x; f.p[lane][1] = y; f.p[lane][2] = z;
    f.drawn[lane] = drawn;
    f.fin[lane] = drawn && isfinite(x) && isfinite(y) && isfinite(z);
}

// phase 2, lanes 0..5: one bound each, over the finite points drawn
__host__ __device__ inline void sk_phase_limits(SkFrame &f, int lane) {
    if (lane >= 6) return;
    const int k = lane % 3;
    const bool hi = lane >= 3;
    float m = hi ? -INFINITY : INFINITY;
    for (int i = 0; i < SK_NPT; ++i)
        if (f.fin[i]) m = hi ? fmaxf(m, f.p[i][k]) : fminf(m, f.p[i][k]);
    f.lim[lane] = m;
}

// phase 3, lane = point: limits -> world -> view -> perspective -> display, snapped
__host__ __device__ inline void sk_phase_project(SkFrame &f, int lane, const idf_skel_view &v) {
#pragma clang fp contract(off)
    if (lane >= SK_NPT) return;
    float W[3];
    for (int k = 0; k < 3; ++k) {
        const float lo = f.lim[k], hi = f.lim[3 + k];
        const float delta = (hi - lo) * v.margin[k];
        const float a = lo - delta, b = hi + delta;
        const float m = (b - a) / 48.0f;
        const float lo3 = a - m, hi3 = b + m;
        const float sc = v.aspect[k] / (hi3 - lo3);
        W[k] = (f.p[lane][k] - lo3) * sc;
    }
    const float *r = v.view;
    const float vx = fmaf(r[2], W[2], fmaf(r[1], W[1], fmaf(r[0], W[0], r[3])));
    const float vy = fmaf(r[6], W[2], fmaf(r[5], W[1], fmaf(r[4], W[0], r[7])));
    const float d = -fmaf(r[10], W[2], fmaf(r[9], W[1], fmaf(r[8], W[0], r[11])));
    const float tx = vx / d, ty = vy / d;
    const float X = rintf(fmaf(tx, v.kx, v.cx)), Y = rintf(fmaf(ty, v.ky, v.cy));
    f.X[lane] = X; f.Y[lane] = Y; f.tz[lane] = -v.dist / d;
    const float g = (float)SK_GUARD;
    f.ok[lane] = f.fin[lane] && d > 0.f && fabsf(X) <= g && fabsf(Y) <= g;          // NaN fails every comparison
}

// phase 4, lanes 0..1 (plain style): depth range of one scatter collection
__host__ __device__ inline void sk_phase_groups(SkFrame &f, int lane) {
    if (lane >= 2) return;
    const int base = lane ? SK_NB : 0, n = lane ? SK_NO : SK_NB;
    float lo = INFINITY, hi = -INFINITY;
    int cnt = 0;
    for (int i = base; i < base + n; ++i)
        if (f.ok[i]) { lo = fminf(lo, f.tz[i]); hi = fmaxf(hi, f.tz[i]); ++cnt; }
    f.gz[lane][0] = lo; f.gz[lane][1] = hi; f.gn[lane] = cnt;
}

__host__ __device__ inline void sk_write(int32_t *rec, int kind, float X0, float Y0, float X1, float Y1, int wd, const uint8_t *c, int alpha) {
    rec[0] = kind; rec[1] = (int32_t)X0; rec[2] = (int32_t)Y0; rec[3] = (int32_t)X1; rec[4] = (int32_t)Y1; rec[5] = wd;
    rec[6] = (int32_t)c[0] | (int32_t)c[1] << 8 | (int32_t)c[2] << 16; rec[7] = alpha;
}

// phase 5, lane = line slot, and (plain style) lane = marker point: the records.  f.rec and f.drop are zero on entry.
__host__ __device__ inline void sk_phase_emit(SkFrame &f, int lane, const idf_skel_view &v, const SkArgs &a) {
#pragma clang fp contract(off)
    const bool plain = v.style == IDF_SKEL_PLAIN;
    const int n_lines = plain ? SK_NBONE + 3 : 3 + 2 * (SK_NBONE + a.n_wires);
    if (lane < n_lines) {
        int pa = -1, pb = -1, ci = 1, s = lane;
        bool bad = false;
        if (plain) {
            if (s < SK_NBONE) { sk_bone(s, pa, pb); ci = 0; }
            else { pa = SK_AX0 + 2 * (s - SK_NBONE); pb = pa + 1; }
        } else if (s < 3) {
            pa = SK_AX0 + 2 * s; pb = pa + 1;
        } else {
            s -= 3;
            const int per = SK_NBONE + a.n_wires, grp = s / per, k = s % per;          // group 0 pred, 1 gt
            if (k < SK_NBONE) {
                sk_bone(k, pa, pb);
                pa += grp * SK_GT0; pb += grp * SK_GT0;
                ci = grp ? 3 : 0;
            } else {
                const int wa = a.wires[2 * (k - SK_NBONE)], wb = a.wires[2 * (k - SK_NBONE) + 1];
                bad = wa < 0 || wa >= SK_NO || wb < 0 || wb >= SK_NO;
                pa = bad ? SK_AX0 : grp * SK_GT0 + SK_NB + wa; pb = bad ? SK_AX0 : grp * SK_GT0 + SK_NB + wb;
                ci = grp ? 4 : 2;
                if (bad && !f.drawn[grp * SK_GT0]) bad = false;          // a group that is not drawn drops nothing
            }
        }
        if (bad) f.drop[lane] = 1;
        else if (f.drawn[pa] && f.drawn[pb]) {
            if (f.ok[pa] && f.ok[pb]) sk_write(f.rec[lane], 1, f.X[pa], f.Y[pa], f.X[pb], f.Y[pb], v.line_wd, v.colour[ci], v.colour[ci][3]);
            else f.drop[lane] = 1;
        }
    }
    if (plain && lane < SK_GT0) {          // markers: a second duty of the first 33 lanes (their line slots are done)
        const int g = lane < SK_NB ? 0 : 1, base = g ? SK_NB : 0, n = g ? SK_NO : SK_NB;
        const bool obj_first = f.gn[0] > 0 && f.gn[1] > 0 && f.gz[1][0] > f.gz[0][0];
        const int first = SK_NBONE + 3 + ((g == 0) == obj_first ? (g ? SK_NB : SK_NO) : 0);
        if (f.ok[lane]) {
            const float z = f.tz[lane];
            int rank = 0;
            for (int i = base; i < base + n; ++i)
                if (f.ok[i] && (f.tz[i] > z || (f.tz[i] == z && i > lane))) ++rank;
            const float range = f.gz[g][1] - f.gz[g][0];
            const float norm = range > 0.f ? (z - f.gz[g][0]) / range : 0.f;
            const int alpha = (int)rintf(fmaf(norm, -178.5f, 255.0f));
            sk_write(f.rec[first + rank], 2, f.X[lane], f.Y[lane], f.X[lane], f.Y[lane], v.disc_wd, v.colour[2 + g], alpha);
        } else {
            f.drop[SK_NBONE + 3 + lane] = 1;          // (any free cell of the drop table: the slots of the lines end at 21)
        }
    }
}

// ---- integer stage ----
struct SkPrim { int32_t kind, x0, y0, x1, y1, wd, rgb, alpha; };

__host__ __device__ inline SkPrim sk_load(const int32_t *rec) { return SkPrim{rec[0], rec[1], rec[2], rec[3], rec[4], rec[5], rec[6], rec[7]}; }

// conservative pixel box of a record, clipped to the image; false: empty or outside
__host__ __device__ inline bool sk_pixel_box(const SkPrim &p, int H, int W, int &i0, int &i1, int &j0, int &j1) {
    if (p.kind == 0) return false;
    const int m = p.wd + 1;
    i0 = ((p.x0 < p.x1 ? p.x0 : p.x1) - m) >> 4; i1 = ((p.x0 > p.x1 ? p.x0 : p.x1) + m) >> 4;          // arithmetic shifts floor
    j0 = ((p.y0 < p.y1 ? p.y0 : p.y1) - m) >> 4; j1 = ((p.y0 > p.y1 ? p.y0 : p.y1) + m) >> 4;
    i0 = i0 < 0 ? 0 : i0; j0 = j0 < 0 ? 0 : j0;
    i1 = i1 > W - 1 ? W - 1 : i1; j1 = j1 > H - 1 ? H - 1 : j1;
    return i0 <= i1 && j0 <= j1;
}

__host__ __device__ inline bool sk_covered(const SkPrim &p, int32_t sx, int32_t sy) {
    const int64_t ex = sx - p.x0, ey = sy - p.y0, wd = p.wd;
    if (p.kind == 2) return 4 * (ex * ex + ey * ey) <= wd * wd;
    const int64_t dx = p.x1 - p.x0, dy = p.y1 - p.y0, L2 = dx * dx + dy * dy;
    if (L2 == 0) return (ex < 0 ? -2 * ex : 2 * ex) <= wd && (ey < 0 ? -2 * ey : 2 * ey) <= wd;
    const int64_t cr = dx * ey - dy * ex, t = dx * ex + dy * ey, big = wd << 17, lim = wd * wd * L2;
    int64_t c2 = cr < 0 ? -2 * cr : 2 * cr;
    if (c2 > big) return false;
    int64_t e2 = 2 * (-t > t - L2 ? -t : t - L2);
    if (e2 > big) return false;
    if (e2 < 0) e2 = 0;
    return c2 * c2 <= lim && e2 * e2 <= lim;
}

__host__ __device__ inline int sk_samples(const SkPrim &p, int i, int j) {
    int n = 0;
    for (int oy = 2; oy < SK_SUB; oy += 4)
        for (int ox = 2; ox < SK_SUB; ox += 4) n += sk_covered(p, SK_SUB * i + ox, SK_SUB * j + oy) ? 1 : 0;
    return n;
}

__host__ __device__ inline void sk_blend(int32_t acc[3], const SkPrim &p, int n) {
    const int32_t w = p.alpha * n;
    for (int k = 0; k < 3; ++k) {
        const int32_t c = ((p.rgb >> (8 * k)) & 255) << 8;
        acc[k] = (acc[k] * (SK_WDEN - w) + c * w + SK_WDEN / 2) / SK_WDEN;
    }
}
