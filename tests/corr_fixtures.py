"""Seeded inputs of the correction-checkpoint scoring fixture (tests/golden/corr_losses.npz), shared by the generator
(tests/golden/make_golden_corr_losses.py, which feeds them to the reference) and tests/test_correction_losses.py.

``human_verts`` at V = 6890 is 193 KB per frame, so it is NOT stored: it is rebuilt here from a seed with operations that reproduce bit for bit on every machine (the legacy ``numpy.random.RandomState`` streams the
other fixtures rely on, then only IEEE additions, multiplications, divisions and square roots in a written-out order, float64 ->
float32 at the end).  The generator stores a checksum of every rebuilt array and the tests assert it first.

The scene: per clip a "body" of V points on an ellipsoid (normals = the outward unit vectors, contact label 1 on the cap that
faces the object) that drifts and breathes over the frames, and an object of P points in a box placed so that it overlaps that cap:
some object points are inside the body (penetration), some labelled vertices are within 2 cm of an object point and some are not.

Two shapes.  The generator requires that a float64 recomputation agrees with the reference's fp32 run on EVERY nearest-neighbour
index, sign and threshold test, and random clouds produce about one fp32 near-tie per 3e5 queries: the T = 35 clips of the forward /
validation case therefore carry a thinned body and object (V = 701, P = 300: neither a multiple of the kernel's tiles), and the
full-size geometry (V = 6890, P = 2048) runs on FULL_T = 12 frames of two clips.
"""
import zlib
import numpy as np
from interdiff_amd.correction import MARKERS67

T, B, V, P, PAST, SEED = 35, 4, 701, 300, 10, 9704
FULL_T, FULL_B, FULL_V, FULL_P, FULL_SEED = 12, 2, 6890, 2048, 9801
TIE_MARKERS = (5, 20, 10)                  # clip 1: equal counts on two body markers and hand marker 10 -> 10 wins through the +0.5 bonus only
RADII = np.array([0.22, 0.75, 0.16])
HALF = np.array([0.16, 0.30, 0.14])
CAP = 0.35                                 # contact label 1 where the outward unit vector has x > CAP


def checksum(a):
    a = np.ascontiguousarray(a)
    return np.int64(zlib.crc32(a.tobytes()) ^ (a.size << 32))


def scene(seed=SEED, T=T, B=B, V=V, P=P, half=None):
    """-> dict of float32 arrays: human_verts [T,B,V,7], markers [T,B,67,7], obj_points [B,P,6], obj_angle [T,B,3], obj_trans [T,B,3]."""
    rs = np.random.RandomState(seed)
    u = rs.standard_normal((B, V, 3))
    nrm = np.sqrt((u[..., 0] * u[..., 0] + u[..., 1] * u[..., 1]) + u[..., 2] * u[..., 2])
    unit = u / nrm[..., None]                                                   # [B,V,3]
    centre = 0.1 * rs.standard_normal((1, B, 3)) + np.cumsum(0.004 * rs.standard_normal((T, B, 3)), axis=0)
    breathe = 1.0 + 0.02 * rs.standard_normal((T, B, 1, 1))
    verts = centre[:, :, None, :] + breathe * (RADII * unit)[None]              # [T,B,V,3]
    label = (unit[..., 0] > CAP).astype(np.float64)                             # [B,V]
    label = np.repeat(label[None], T, axis=0)                                   # [T,B,V]
    mk = np.asarray(MARKERS67) if V == 6890 else np.arange(67) * (V // 67)      # the marker rows of the body
    label[:, 0, mk] = 0.0                                                       # clip 0: no marker is ever in contact
    if B > 1:
        label[:, 1, mk] = 0.0                                                   # clip 1: three markers with the same count, one of them a hand marker
        label[PAST:, 1, mk[list(TIE_MARKERS)]] = 1.0
    hv = np.concatenate([verts, np.repeat(unit[None], T, axis=0), label[..., None]], axis=3).astype(np.float32)
    pts = rs.uniform(-1.0, 1.0, (B, P, 3)) * (HALF if half is None else np.asarray(half))
    pn = rs.standard_normal((B, P, 3))
    obj_points = np.concatenate([pts, pn], axis=2).astype(np.float32)
    offset = np.array([0.30, 0.0, 0.0]) + 0.03 * rs.standard_normal((1, B, 3))
    obj_trans = centre + offset + np.cumsum(0.003 * rs.standard_normal((T, B, 3)), axis=0)
    obj_angle = 0.3 * rs.standard_normal((1, B, 3)) + np.cumsum(0.01 * rs.standard_normal((T, B, 3)), axis=0)
    return dict(human_verts=hv, markers=np.ascontiguousarray(hv[:, :, mk]), obj_points=obj_points,
                obj_angle=obj_angle.astype(np.float32), obj_trans=obj_trans.astype(np.float32))


def as_batch(sc, torch):
    """The reference's dict-of-lists batch (data/dataset_smpl.py) around the scene's arrays, as torch CPU tensors."""
    t = {k: torch.from_numpy(v) for k, v in sc.items()}
    frames = [dict(objfit_params=dict(angle=t['obj_angle'][i], trans=t['obj_trans'][i]), markers=t['markers'][i], human_verts=t['human_verts'][i])
              for i in range(sc['obj_angle'].shape[0])]
    return dict(frames=frames, obj_points=t['obj_points'])


def full_scene():
    return scene(FULL_SEED, FULL_T, FULL_B, FULL_V, FULL_P)


def composed(pred, gt, pts, hv):
    """The same scoring from the entries the library had before: rotation entry, elementwise posing, interdiff_point2point_signed with
    return_vector, torch masks and means (train_correction_smpl.py:121-153 line by line).  -> (penetration, contact, frames [N,4])."""
    import torch
    from interdiff_amd import transforms
    from interdiff_amd.geometry import point2point_signed
    T, B = pred.shape[:2]
    M = transforms.rotation_6d_to_matrix(pred[..., :6].contiguous())                        # [T,B,3,3]
    p = pts[None, :, :, :3]
    row = lambda i: ((M[:, :, i, 0, None] * p[..., 0] + M[:, :, i, 1, None] * p[..., 1]) + M[:, :, i, 2, None] * p[..., 2]) + pred[:, :, 6 + i, None]
    posed = torch.stack([row(0), row(1), row(2)], dim=-1)                                   # [T,B,P,3]
    x, xn, lab = hv[..., :3], hv[..., 3:6], hv[..., 6]
    o2h_s, h2o_s, _, _, _, _ = point2point_signed(x.reshape(T * B, -1, 3), posed.reshape(T * B, -1, 3), x_normals=xn.reshape(T * B, -1, 3), return_vector=True)
    v_contact = ((h2o_s.abs() > 0.02) & (lab.reshape(T * B, -1) > 0.5)).float()
    w = torch.zeros_like(o2h_s)
    w[(o2h_s < 0.01) & (o2h_s > 0)] = 0
    w[o2h_s < 0] = 20
    frames = torch.stack([(o2h_s.abs() * w).sum(1), (h2o_s.abs() * v_contact).sum(1), (o2h_s < 0).float().sum(1), v_contact.sum(1)], dim=1)
    return (o2h_s.abs() * w).mean(), (h2o_s.abs() * v_contact).mean(), frames
