// Per-clip canonicalisation of a BEHAVE window (data/dataset_smpl.py:105-152) and its column of the denoiser's ground-truth token
// (model/diffusion_smpl.py:212-214), host + device inline: csrc/clip_batch.hip runs one lane per frame, interdiff_debug_clip_canon runs the
// same functions on the CPU.
//
// The arithmetic is DOUBLE and rounded to fp32 once, like the reference (scipy on float64, stored as float32): 2 T B rotation compositions
// per batch are nothing, and near pi an fp32 quaternion -> rotation vector conversion loses the 1e-6 agreement the tests ask for.
// The conversions restate scipy.spatial.transform.Rotation's route (1.15, _rotation.pyx), so that every branch is taken where the host path
// (interdiff_amd/data.py canonicalize_clip) takes it: quaternions are (x, y, z, w);
//   from_rotvec   angle <= 1e-3: scale = 1/2 - angle^2/48 + angle^4/3840, else sin(angle/2)/angle; NOT normalised
//   from_matrix   the largest of the three diagonal entries and the trace picks the formula; normalised
//   p * q         Hamilton product, normalised
//   as_rotvec     w < 0 flips the sign; angle = 2 atan2(|v|, w); angle <= 1e-3: scale = 2 + angle^2/12 + 7 angle^4/2880, else angle/sin(angle/2)
//   as_matrix     the usual nine products
// The 6D rotation of a body joint is pytorch3d's matrix_to_rotation_6d(axis_angle_to_matrix(.)) (csrc/rot_math.h, here in double): first two rows.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define CLIPC_HD __host__ __device__ inline
#else
#define CLIPC_HD inline
#endif

namespace clipc {

struct Quat { double x, y, z, w; };

CLIPC_HD Quat normalized(Quat q) {
    const double n = sqrt(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
    return Quat{q.x / n, q.y / n, q.z / n, q.w / n};
}

CLIPC_HD Quat from_rotvec(const double *r) {
    const double a2 = r[0] * r[0] + r[1] * r[1] + r[2] * r[2], angle = sqrt(a2);
    const double scale = angle <= 1e-3 ? 0.5 - a2 / 48.0 + a2 * a2 / 3840.0 : sin(angle / 2.0) / angle;
    return Quat{scale * r[0], scale * r[1], scale * r[2], cos(angle / 2.0)};
}

CLIPC_HD Quat from_matrix(const double *m) {      // row-major m[9]
    const double tr = m[0] + m[4] + m[8];
    int choice = 0;
    double best = m[0];
    if (m[4] > best) { best = m[4]; choice = 1; }
    if (m[8] > best) { best = m[8]; choice = 2; }
    if (tr > best) choice = 3;
    double q[4];
    if (choice != 3) {
        const int i = choice, j = (i + 1) % 3, k = (j + 1) % 3;
        q[i] = 1.0 - tr + 2.0 * m[3 * i + i];
        q[j] = m[3 * j + i] + m[3 * i + j];
        q[k] = m[3 * k + i] + m[3 * i + k];
        q[3] = m[3 * k + j] - m[3 * j + k];
    } else {
        q[0] = m[7] - m[5];
        q[1] = m[2] - m[6];
        q[2] = m[3] - m[1];
        q[3] = 1.0 + tr;
    }
    return normalized(Quat{q[0], q[1], q[2], q[3]});
}

CLIPC_HD Quat compose(const Quat &p, const Quat &q) {      // p * q: q first, then p
    return normalized(Quat{p.w * q.x + q.w * p.x + (p.y * q.z - p.z * q.y),
                           p.w * q.y + q.w * p.y + (p.z * q.x - p.x * q.z),
                           p.w * q.z + q.w * p.z + (p.x * q.y - p.y * q.x),
                           p.w * q.w - (p.x * q.x + p.y * q.y + p.z * q.z)});
}

CLIPC_HD void as_rotvec(Quat q, double *r) {
    if (q.w < 0) { q.x = -q.x; q.y = -q.y; q.z = -q.z; q.w = -q.w; }
    const double angle = 2.0 * atan2(sqrt(q.x * q.x + q.y * q.y + q.z * q.z), q.w), a2 = angle * angle;
    const double scale = angle <= 1e-3 ? 2.0 + a2 / 12.0 + 7.0 * a2 * a2 / 2880.0 : angle / sin(angle / 2.0);
    r[0] = scale * q.x; r[1] = scale * q.y; r[2] = scale * q.z;
}

CLIPC_HD void as_matrix(const Quat &q, double *m) {
    const double x2 = q.x * q.x, y2 = q.y * q.y, z2 = q.z * q.z, w2 = q.w * q.w;
    const double xy = q.x * q.y, zw = q.z * q.w, xz = q.x * q.z, yw = q.y * q.w, yz = q.y * q.z, xw = q.x * q.w;
    m[0] = x2 - y2 - z2 + w2; m[1] = 2.0 * (xy - zw);     m[2] = 2.0 * (xz + yw);
    m[3] = 2.0 * (xy + zw);   m[4] = -x2 + y2 - z2 + w2;  m[5] = 2.0 * (yz - xw);
    m[6] = 2.0 * (xz - yw);   m[7] = 2.0 * (yz + xw);     m[8] = -x2 - y2 + z2 + w2;
}

CLIPC_HD void mat_vec(const double *m, const double *v, double *o) {
    o[0] = m[0] * v[0] + m[1] * v[1] + m[2] * v[2];
    o[1] = m[3] * v[0] + m[4] * v[1] + m[5] * v[2];
    o[2] = m[6] * v[0] + m[7] * v[1] + m[8] * v[2];
}

// pytorch3d: axis-angle -> quaternion (w first; sin(a/2)/a, series below 1e-6) -> matrix, first two rows
CLIPC_HD void rot6d_of_axis_angle(const double *a, double *d) {
    const double a2 = a[0] * a[0] + a[1] * a[1] + a[2] * a[2], angle = sqrt(a2), half = 0.5 * angle;
    const double s = fabs(angle) < 1e-6 ? 0.5 - a2 / 48.0 : sin(half) / angle;
    const double r = cos(half), i = a[0] * s, j = a[1] * s, k = a[2] * s;
    const double s2 = 2.0 / (r * r + i * i + j * j + k * k);
    d[0] = 1 - s2 * (j * j + k * k); d[1] = s2 * (i * j - k * r); d[2] = s2 * (i * k + j * r);
    d[3] = s2 * (i * j + k * r); d[4] = 1 - s2 * (i * i + k * k); d[5] = s2 * (j * k - i * r);
}

// What the first frame fixes for the whole clip (:119-125): the origin and the rotation that removes the first heading.
struct Frame0 {
    double centroid[3];   // pelvis of frame 0 (an fp32 value)
    double R[9];          // `rotation`: fp32 values, the inverse of rotation_v
    Quat q;               // Rotation.from_matrix(rotation)
};

// rotation_v = [[c, 0, -s], [0, 1, 0], [s, 0, c]] in fp32 with (c, s) = (G00, G20) / sqrt(G00^2 + G20^2) of the first global orientation G;
// rotation = its inverse, evaluated in double on the fp32 entries and rounded to fp32 once (numpy inverts in fp32: equal to an ulp).
// G00 = G20 = 0 (a body lying along the vertical) divides by zero: non-finite output, as in the reference.
CLIPC_HD void frame0_of(const double *root_aa0, const float *pelvis0, Frame0 &f) {
    double G[9];
    as_matrix(from_rotvec(root_aa0), G);
    const double n = sqrt(G[0] * G[0] + G[6] * G[6]);
    const float c = (float)(G[0] / n), s = (float)(G[6] / n);
    const double det = (double)c * c + (double)s * s;
    const float ci = (float)((double)c / det), si = (float)((double)s / det);
    f.R[0] = ci; f.R[1] = 0; f.R[2] = si;
    f.R[3] = 0;  f.R[4] = 1; f.R[5] = 0;
    f.R[6] = -si; f.R[7] = 0; f.R[8] = ci;
    f.q = from_matrix(f.R);
    for (int k = 0; k < 3; ++k) f.centroid[k] = pelvis0[k];
}

CLIPC_HD void frame0_with_rotation(const float *rotation, const float *pelvis0, Frame0 &f) {      // (debug: any rotation matrix)
    for (int k = 0; k < 9; ++k) f.R[k] = rotation[k];
    f.q = from_matrix(f.R);
    for (int k = 0; k < 3; ++k) f.centroid[k] = pelvis0[k];
}

// One frame (:127-152).  fit = root axis-angle | body translation | object axis-angle | object translation (12 doubles), pelvis fp32[3],
// pose fp32[156] (joints 1..21 are read for the token).  Outputs fp32: root / trans / obj_angle / obj_trans / pelvis [3] each and, when gt is
// given, the token column gt[row * gt_stride], rows = 22 x 6 body rotations | body translation | object rotation 6 | object translation.
CLIPC_HD void canon_frame(const Frame0 &f, const double *fit, const float *pelvis, const float *pose, float *root, float *trans, float *obj_angle,
                          float *obj_trans, float *pelvis_out, float *gt, int64_t gt_stride) {
    double t_rel[3], p_rel[3], p0[3], a[3], o[3], rv[3], m[9];
    for (int k = 0; k < 3; ++k) {
        t_rel[k] = fit[3 + k] - f.centroid[k];
        p_rel[k] = (double)pelvis[k] - f.centroid[k];
        p0[k] = p_rel[k] - t_rel[k];
        a[k] = t_rel[k] + p0[k];
    }
    mat_vec(f.R, a, o);
    double tr_out[3], ot_out[3];
    for (int k = 0; k < 3; ++k) trans[k] = (float)(tr_out[k] = o[k] - p0[k]);
    mat_vec(f.R, p_rel, o);
    for (int k = 0; k < 3; ++k) pelvis_out[k] = (float)o[k];
    for (int k = 0; k < 3; ++k) a[k] = fit[9 + k] - f.centroid[k];
    mat_vec(f.R, a, ot_out);
    for (int k = 0; k < 3; ++k) obj_trans[k] = (float)ot_out[k];
    const Quat qb = compose(f.q, from_rotvec(fit)), qo = compose(f.q, from_rotvec(fit + 6));
    as_rotvec(qb, rv);
    for (int k = 0; k < 3; ++k) root[k] = (float)rv[k];
    as_rotvec(qo, rv);
    for (int k = 0; k < 3; ++k) obj_angle[k] = (float)rv[k];
    if (!gt) return;
    as_matrix(qb, m);
    for (int k = 0; k < 6; ++k) gt[k * gt_stride] = (float)m[k];
    for (int j = 1; j < 22; ++j) {
        const double aj[3] = {(double)pose[3 * j], (double)pose[3 * j + 1], (double)pose[3 * j + 2]};
        double d[6];
        rot6d_of_axis_angle(aj, d);
        for (int k = 0; k < 6; ++k) gt[(6 * j + k) * gt_stride] = (float)d[k];
    }
    for (int k = 0; k < 3; ++k) gt[(132 + k) * gt_stride] = (float)tr_out[k];
    as_matrix(qo, m);
    for (int k = 0; k < 6; ++k) gt[(135 + k) * gt_stride] = (float)m[k];
    for (int k = 0; k < 3; ++k) gt[(141 + k) * gt_stride] = (float)ot_out[k];
}

// Foot-ground label (:171-179): moved less than 1 cm since the PREVIOUS SEQUENCE frame.
CLIPC_HD float foot_still(const float *now, const float *before) {
    const double dx = (double)(now[0] - before[0]), dy = (double)(now[1] - before[1]), dz = (double)(now[2] - before[2]);
    return sqrt(dx * dx + dy * dy + dz * dz) < 0.01 ? 1.f : 0.f;
}

}  // namespace clipc
