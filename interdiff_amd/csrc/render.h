// Software rasteriser, the inlines shared by the device kernels (render.hip) and their host twins (interdiff_debug_render_*).
//
// CONTRACT (restated bit for bit by tests/render_oracle.py).
//   setup record   20 int32 per slot: vertex i at [6 i .. 6 i + 5] = X, Y, Z, R, G, B;  [18] = 1 valid / 0 empty (then all 20 are 0);  [19] = 0.
//     X, Y   screen position in 1/16 pixel, origin = the image's top-left corner, y down, |X|, |Y| <= RD_GUARD
//     Z      RD_ZONE - rint(RD_ZONE * near / d), d = distance along the view axis: 0 at the near plane, -> RD_ZONE at infinity (the infinite
//            projection's NDC depth, which is affine in screen space -- integer barycentric interpolation of it is the true depth)
//     R G B  shaded colour in 1/16 of an 8-bit step: 0 .. 4080
//   coverage   pixel (i, j) is sampled at its centre P = (16 i + 8, 16 j + 8).  E(a, b; P) = (bx - ax)(Py - ay) - (by - ay)(Px - ax).  The record is
//     oriented so that A = E(v0, v1; v2) > 0 (v1 and v2 swap when it is negative; A = 0 covers nothing).  w0 = E(v1, v2; P), w1 = E(v2, v0; P),
//     w2 = E(v0, v1; P), w0 + w1 + w2 = A.  P is covered iff every w_k >= 0 and w_k > 0 on an edge that is neither TOP (dy = 0, dx > 0) nor LEFT (dy < 0):
//     two triangles that share an edge cover every pixel of their union exactly once.
//   depth      Zp = floor((w0 Z0 + w1 Z1 + w2 Z2) / A);  key = (Zp << 32) | slot, the smallest key wins: nearer first, then the lower slot.
//   colour     C8 = floor((2 (w0 C0 + w1 C1 + w2 C2) + 16 A) / (32 A)) per channel -- screen-space affine (Gouraud), rounded to nearest.
// BIT WIDTHS.  |X|, |Y| <= 2^15 and 0 <= P <= 2^15, so every difference is below 2^16 + 1 in magnitude, every product below 2^33, an edge function
// (a difference of two products) at most 2^33, and w_k <= A <= 2^33.  Z <= 2^28: the depth sum is <= A * 2^28 <= 2^61.  C <= 4080 < 2^12: the colour
// numerator is <= 2 A 2^12 + 16 A < 2^47.  All inside int64; the static_asserts below derive the same bounds from RD_GUARD, RD_ZONE and RD_CMAX.
#pragma once
#include <math.h>
#include <stdint.h>
#include "../../include/interdiff_hip.h"

#ifndef __HIPCC__
#define __host__
#define __device__
#endif

constexpr int RD_SUB = IDF_RENDER_SUBPIX;           // sub-pixel units per pixel
constexpr int RD_GUARD = IDF_RENDER_GUARD;          // guard band, sub-pixel units
constexpr int RD_ZONE = IDF_RENDER_ZONE;            // depth of a point at infinity
constexpr int RD_REC = IDF_RENDER_REC_INTS;
constexpr int RD_TILE = IDF_RENDER_TILE;
constexpr int RD_CMAX = 255 * 16;
// the overflow bounds of the header comment, derived from the constants
static_assert(IDF_RENDER_MAX_DIM * RD_SUB <= RD_GUARD, "pixel centres stay inside the guard band");
constexpr int64_t RD_DIFF_MAX = 2 * (int64_t)RD_GUARD;                 // |difference of two coordinates, or of a pixel centre and a coordinate|
constexpr int64_t RD_EDGE_MAX = 2 * RD_DIFF_MAX * RD_DIFF_MAX;         // |edge function| = |difference of two products|; also bounds A and every w_k
static_assert(RD_EDGE_MAX <= INT64_MAX / RD_ZONE, "depth sum: w0 Z0 + w1 Z1 + w2 Z2 <= A * RD_ZONE must fit int64");
static_assert(RD_EDGE_MAX <= INT64_MAX / (2 * RD_CMAX + 16), "colour numerator: 2 A C + 16 A must fit int64");

struct RdVert { float xc, yc, d, r, g, b; };       // camera space (x right, y up, d along the view axis) and the shaded colour in [0, 1]
struct RdSnap { float X, Y; int32_t Z, R, G, B; }; // X, Y already integral (rintf) but still float: the guard band is tested before the conversion

// Scene transform + camera + shading of one vertex.  fp32, every rounding pinned (contraction off, explicit fmaf).
//   moving meshes: s = (-p) - off (the reference negates all coordinates, then centres on the body), then `view` quarter turns about +y (exact: sign
//   swaps), normal = the same turns of -n;  scene-space meshes (the ground) skip both.
//   camera: q = s - cam_t;  yc = cos q.y - sin q.z;  d = -(sin q.y + cos q.z)   (the inverse of translate(cam_t) . rotate_x(-pitch))
//   shade = min(1, ambient + gain * sum_k max(0, n . L_k)), colour = base * shade
__host__ __device__ inline RdVert rd_vertex(const idf_render_scene &sc, int view, bool scene_space, float px, float py, float pz, float nx, float ny,
                                            float nz, float br, float bg, float bb) {
#pragma clang fp contract(off)
    float sx = px, sy = py, sz = pz;
    if (!scene_space) {
        sx = (-px) - sc.off[0]; sy = (-py) - sc.off[1]; sz = (-pz) - sc.off[2];
        nx = -nx; ny = -ny; nz = -nz;
        for (int k = 0; k < (view & 3); ++k) {                 // rotate_y(90 deg): x' = z, z' = -x
            float t = sx; sx = sz; sz = -t;
            t = nx; nx = nz; nz = -t;
        }
    }
    const float qx = sx - sc.cam_t[0], qy = sy - sc.cam_t[1], qz = sz - sc.cam_t[2];
    RdVert o;
    o.xc = qx;
    o.yc = fmaf(sc.cam_cos, qy, -(sc.cam_sin * qz));
    o.d = -fmaf(sc.cam_cos, qz, sc.cam_sin * qy);
    float lam = 0.f;
    for (int k = 0; k < 3; ++k) {
        const float c = fmaf(nz, sc.light[3 * k + 2], fmaf(ny, sc.light[3 * k + 1], nx * sc.light[3 * k]));
        lam += fmaxf(c, 0.f);
    }
    const float shade = fminf(fmaf(sc.light_gain, lam, sc.ambient), 1.f);
    o.r = br * shade; o.g = bg * shade; o.b = bb * shade;
    return o;
}

// the point where the edge from a (in front, a.d >= near) to b (behind) meets the near plane; always taken FROM the front vertex, so two triangles
// that share the edge get the same point
__host__ __device__ inline RdVert rd_clip(const idf_render_scene &sc, const RdVert &a, const RdVert &b) {
#pragma clang fp contract(off)
    const float s = (sc.znear - a.d) / (b.d - a.d);
    RdVert o;
    o.xc = fmaf(s, b.xc - a.xc, a.xc); o.yc = fmaf(s, b.yc - a.yc, a.yc); o.d = sc.znear;
    o.r = fmaf(s, b.r - a.r, a.r); o.g = fmaf(s, b.g - a.g, a.g); o.b = fmaf(s, b.b - a.b, a.b);
    return o;
}

__host__ __device__ inline int32_t rd_quant_colour(float c) { return (int32_t)rintf(fminf(fmaxf(c, 0.f), 1.f) * (float)RD_CMAX); }

// projection (yfov through sc.focal = 1 / tan(yfov / 2), square pixels), snap to 1/16 pixel, depth and colour to integers; v.d >= near > 0
__host__ __device__ inline RdSnap rd_project(const idf_render_scene &sc, int H, int W, const RdVert &v) {
#pragma clang fp contract(off)
    const float k = (float)(8 * H) * sc.focal;
    RdSnap o;
    o.X = rintf(fmaf(v.xc / v.d, k, (float)(8 * W)));
    o.Y = rintf(fmaf(v.yc / v.d, -k, (float)(8 * H)));
    const float q = fminf(sc.znear / v.d, 1.f);
    o.Z = RD_ZONE - (int32_t)rintf(q * (float)RD_ZONE);
    o.R = rd_quant_colour(v.r); o.G = rd_quant_colour(v.g); o.B = rd_quant_colour(v.b);
    return o;
}

// One slot's record from three projected vertices.  Returns 1 = written valid, 0 = culled (wholly outside the viewport: empty record), 2 = dropped
// (not outside, but a snapped coordinate leaves the guard band or is not a number: empty record, the caller counts it).
__host__ __device__ inline int rd_emit(int32_t *rec, int H, int W, const RdSnap &a, const RdSnap &b, const RdSnap &c) {
    for (int i = 0; i < RD_REC; ++i) rec[i] = 0;
    const float x1 = (float)(RD_SUB * W), y1 = (float)(RD_SUB * H);
    if ((a.X < 0.f && b.X < 0.f && c.X < 0.f) || (a.X > x1 && b.X > x1 && c.X > x1) || (a.Y < 0.f && b.Y < 0.f && c.Y < 0.f) ||
        (a.Y > y1 && b.Y > y1 && c.Y > y1))
        return 0;
    const float g = (float)RD_GUARD;
    if (!(fabsf(a.X) <= g && fabsf(a.Y) <= g && fabsf(b.X) <= g && fabsf(b.Y) <= g && fabsf(c.X) <= g && fabsf(c.Y) <= g)) return 2;
    const RdSnap *v[3] = {&a, &b, &c};
    for (int i = 0; i < 3; ++i) {
        rec[6 * i] = (int32_t)v[i]->X; rec[6 * i + 1] = (int32_t)v[i]->Y; rec[6 * i + 2] = v[i]->Z;
        rec[6 * i + 3] = v[i]->R; rec[6 * i + 4] = v[i]->G; rec[6 * i + 5] = v[i]->B;
    }
    rec[18] = 1;
    return 1;
}

// Near-plane clip of one source triangle into its two slots (rec0 = slot 2 tri, rec1 = slot 2 tri + 1); returns the number of dropped slots.
//   three in front: slot 0 = (v0, v1, v2).  one in front (a, then b, c in the face's cyclic order): slot 0 = (a, a->b, a->c).
//   two in front (a behind; b, c follow it cyclically): slot 0 = (b, c, c->a), slot 1 = (b, c->a, b->a).   none: both empty.
__host__ __device__ inline int rd_setup_triangle(const idf_render_scene &sc, int H, int W, const RdVert v[3], int32_t *rec0, int32_t *rec1) {
    for (int i = 0; i < RD_REC; ++i) { rec0[i] = 0; rec1[i] = 0; }
    const bool f0 = v[0].d >= sc.znear, f1 = v[1].d >= sc.znear, f2 = v[2].d >= sc.znear;     // a NaN depth counts as behind
    const int nf = (int)f0 + (int)f1 + (int)f2;
    int dropped = 0;
    if (nf == 3) {
        dropped += rd_emit(rec0, H, W, rd_project(sc, H, W, v[0]), rd_project(sc, H, W, v[1]), rd_project(sc, H, W, v[2])) == 2;
    } else if (nf == 1) {
        const int a = f0 ? 0 : (f1 ? 1 : 2), b = (a + 1) % 3, c = (a + 2) % 3;
        dropped += rd_emit(rec0, H, W, rd_project(sc, H, W, v[a]), rd_project(sc, H, W, rd_clip(sc, v[a], v[b])),
                           rd_project(sc, H, W, rd_clip(sc, v[a], v[c]))) == 2;
    } else if (nf == 2) {
        const int a = !f0 ? 0 : (!f1 ? 1 : 2), b = (a + 1) % 3, c = (a + 2) % 3;
        const RdSnap sb = rd_project(sc, H, W, v[b]), sc_ = rd_project(sc, H, W, v[c]);
        const RdSnap ca = rd_project(sc, H, W, rd_clip(sc, v[c], v[a])), ba = rd_project(sc, H, W, rd_clip(sc, v[b], v[a]));
        dropped += rd_emit(rec0, H, W, sb, sc_, ca) == 2;
        dropped += rd_emit(rec1, H, W, sb, ca, ba) == 2;
    }
    return dropped;
}

// ---- integer stage ----
struct RdTri {
    int32_t x[3], y[3], z[3], c[3][3];
    int64_t A;          // twice the area after orientation; 0: covers nothing
};

__host__ __device__ inline int64_t rd_edge(int32_t ax, int32_t ay, int32_t bx, int32_t by, int32_t px, int32_t py) {
    return (int64_t)(bx - ax) * (int64_t)(py - ay) - (int64_t)(by - ay) * (int64_t)(px - ax);
}

// load and orient a record; false when it is empty or has no area
__host__ __device__ inline bool rd_load(const int32_t *rec, RdTri &t) {
    if (rec[18] != 1) { t.A = 0; return false; }
    for (int i = 0; i < 3; ++i) {
        t.x[i] = rec[6 * i]; t.y[i] = rec[6 * i + 1]; t.z[i] = rec[6 * i + 2];
        t.c[i][0] = rec[6 * i + 3]; t.c[i][1] = rec[6 * i + 4]; t.c[i][2] = rec[6 * i + 5];
    }
    t.A = rd_edge(t.x[0], t.y[0], t.x[1], t.y[1], t.x[2], t.y[2]);
    if (t.A < 0) {
        t.A = -t.A;
        int32_t s;
        s = t.x[1]; t.x[1] = t.x[2]; t.x[2] = s;
        s = t.y[1]; t.y[1] = t.y[2]; t.y[2] = s;
        s = t.z[1]; t.z[1] = t.z[2]; t.z[2] = s;
        for (int k = 0; k < 3; ++k) { s = t.c[1][k]; t.c[1][k] = t.c[2][k]; t.c[2][k] = s; }
    }
    return t.A > 0;
}

// the pixels whose centres lie inside the record's bounding box, clipped to the image: [i0, i1] x [j0, j1]; false when there is none
__host__ __device__ inline bool rd_pixel_box(const int32_t *rec, int H, int W, int &i0, int &i1, int &j0, int &j1) {
    if (rec[18] != 1) return false;
    int xmin = rec[0], xmax = rec[0], ymin = rec[1], ymax = rec[1];
    for (int i = 1; i < 3; ++i) {
        xmin = rec[6 * i] < xmin ? rec[6 * i] : xmin; xmax = rec[6 * i] > xmax ? rec[6 * i] : xmax;
        ymin = rec[6 * i + 1] < ymin ? rec[6 * i + 1] : ymin; ymax = rec[6 * i + 1] > ymax ? rec[6 * i + 1] : ymax;
    }
    i0 = (xmin + 7) >> 4; i1 = (xmax - 8) >> 4;           // ceil((xmin - 8) / 16), floor((xmax - 8) / 16): arithmetic shifts floor
    j0 = (ymin + 7) >> 4; j1 = (ymax - 8) >> 4;
    i0 = i0 < 0 ? 0 : i0; j0 = j0 < 0 ? 0 : j0;
    i1 = i1 > W - 1 ? W - 1 : i1; j1 = j1 > H - 1 ? H - 1 : j1;
    return i0 <= i1 && j0 <= j1;
}

// 1 where w = 0 on the edge a -> b does NOT count as inside (the edge is neither top nor left)
__host__ __device__ inline int64_t rd_edge_bias(int32_t ax, int32_t ay, int32_t bx, int32_t by) {
    const int32_t dx = bx - ax, dy = by - ay;
    return (dy < 0 || (dy == 0 && dx > 0)) ? 0 : 1;
}

// coverage of pixel (i, j) and its barycentric weights
__host__ __device__ inline bool rd_cover(const RdTri &t, int i, int j, int64_t w[3]) {
    const int32_t px = RD_SUB * i + RD_SUB / 2, py = RD_SUB * j + RD_SUB / 2;
    w[0] = rd_edge(t.x[1], t.y[1], t.x[2], t.y[2], px, py);
    w[1] = rd_edge(t.x[2], t.y[2], t.x[0], t.y[0], px, py);
    w[2] = rd_edge(t.x[0], t.y[0], t.x[1], t.y[1], px, py);
    return w[0] >= rd_edge_bias(t.x[1], t.y[1], t.x[2], t.y[2]) && w[1] >= rd_edge_bias(t.x[2], t.y[2], t.x[0], t.y[0]) &&
           w[2] >= rd_edge_bias(t.x[0], t.y[0], t.x[1], t.y[1]);
}

__host__ __device__ inline int32_t rd_depth(const RdTri &t, const int64_t w[3]) {
    return (int32_t)((w[0] * t.z[0] + w[1] * t.z[1] + w[2] * t.z[2]) / t.A);
}

__host__ __device__ inline int32_t rd_colour(const RdTri &t, const int64_t w[3], int k) {
    return (int32_t)((2 * (w[0] * t.c[0][k] + w[1] * t.c[1][k] + w[2] * t.c[2][k]) + 16 * t.A) / (32 * t.A));
}
