"""Contact-label generation (interdiff/data/prepare_behave.py): from the raw fits of a BEHAVE sequence and an object mesh to the
``contact.npz`` that ``data.load_behave_sequence`` / ``data.clip_labels`` / ``correction_losses.body_records`` consume.

    contact_labels      ContactLabelGenerator.get_contact_labels :32-52 for N frames on ``interdiff_contact_labels`` (csrc/contact_labels.hip)
    sample_surface      trimesh.Trimesh.sample(n, return_index=True) + face_normals (:91-93), restated on a numpy Generator
    generate_contact    main :59-119 for one sequence: SMPL-H on the HIP ``SMPL_Layer``, the label kernels, the foot label
    write_contact_npz   np.savez(outfile, contact_dict) (:119)

The reference calls ``igl.signed_distance`` (winding-number sign).  igl, trimesh and psbody are not available here, so the contract is the
restatement of SURVEY.md B.6: d = exact distance to the triangle soup, w = generalised winding number, S = (1 - 2 w) d, a point is in
contact when S < thres, a body vertex when a contact point is closer than thres (both strict)."""
import numpy as np
import torch
from . import _lib
from .geometry import MeshTopology, morton_order

_MESH_CACHE = {}


class _LabelMesh:
    """Validated faces of one mesh in the scan order of the label kernels (device int32 [F,3]) + the permutation that made it."""

    def __init__(self, faces, V, rest_vertices, device):
        f = faces.detach().cpu().numpy() if isinstance(faces, torch.Tensor) else np.asarray(faces)
        if f.ndim == 3:
            f = f[0]
        if f.ndim != 2 or f.shape[1] != 3 or len(f) == 0:
            raise ValueError('faces must be [F,3]')
        f = f.astype(np.int64)
        if f.min() < 0 or f.max() >= V:
            raise ValueError('face index out of range: [%d, %d] for %d vertices' % (f.min(), f.max(), V))
        rest = np.asarray(rest_vertices, dtype=np.float64).reshape(V, 3)
        self.order = morton_order(rest[f].mean(1))                      # faces along a Morton curve of their centroids: compact 256-face chunks
        self.faces_host = f
        self.faces = torch.from_numpy(np.ascontiguousarray(f[self.order].astype(np.int32))).to(device)
        self.V, self.F = V, len(f)


def label_mesh(faces, V, rest_vertices, device):
    """The ``_LabelMesh`` of ``faces`` (tensor / array [F,3], or a ``geometry.MeshTopology``): indices validated on the host and faces sorted ONCE
    per mesh -- cached by content like ``geometry._topology``, or on the topology object when one is given.  ``rest_vertices``: [V,3] (or a
    callable that returns them, only called when the mesh is new) -- any pose of the mesh; it decides the scan order, never a result.  A caller
    with many calls on one mesh keeps the returned object and passes it as ``faces``."""
    if isinstance(faces, _LabelMesh):
        return faces
    device = torch.device(device)
    rest = lambda: rest_vertices() if callable(rest_vertices) else rest_vertices
    if isinstance(faces, MeshTopology):
        lm = getattr(faces, '_label_mesh', None)
        if lm is None or lm.V != V or lm.faces.device != device:
            lm = faces._label_mesh = _LabelMesh(faces.faces, V, rest(), device)
        return lm
    f0 = torch.as_tensor(faces).cpu().long()
    f0 = f0[0] if f0.dim() == 3 else f0
    key = (tuple(f0.shape), V, str(device))
    for host, lm in _MESH_CACHE.get(key, []):
        if torch.equal(host, f0):
            return lm
    lm = _LabelMesh(f0, V, rest(), device)
    _MESH_CACHE.setdefault(key, []).append((f0.clone(), lm))
    if len(_MESH_CACHE[key]) > 4:
        _MESH_CACHE[key].pop(0)
    return lm


def contact_labels(verts, faces, points, thres=0.02, objR=None, objT=None, return_signed_dist=False):
    """prepare_behave.py:32-52 for N frames.  ``verts`` [N,V,3] device tensor; ``faces`` [F,3] (tensor / array), a ``geometry.MeshTopology`` or the
    object ``label_mesh`` returned (an out-of-range index raises ValueError before any launch); ``points`` [P,3] -- one cloud for all frames -- or [N,P,3]; ``objR`` [N,3,3] or
    [N,9] and ``objT`` [N,3] (both or neither): the kernels pose the points as ``p @ R.T + t``.
    -> (obj_label bool [N,P], human_label bool [N,V]) and, with ``return_signed_dist``, S = (1 - 2 w) d f32 [N,P].  The winding number is
    computed for EVERY point (it shares the face loop of the distance), so S carries its sign everywhere -- also where d < thres."""
    lib = _lib.load()
    if verts.dim() != 3 or verts.shape[2] != 3:
        raise ValueError('verts must be [N,V,3]')
    N, V, _ = verts.shape
    v = verts.contiguous().float()
    dev = v.device
    mesh = label_mesh(faces, V, lambda: v[0].cpu().numpy(), dev)
    if mesh.V != V:
        raise ValueError('the mesh was validated for %d vertices, verts has %d' % (mesh.V, V))
    pts = torch.as_tensor(points, dtype=torch.float32, device=dev).contiguous()
    if pts.dim() == 2 and pts.shape[1] == 3:
        P, stride = pts.shape[0], 0
    elif pts.dim() == 3 and pts.shape[0] == N and pts.shape[2] == 3:
        P, stride = pts.shape[1], 3 * pts.shape[1]
    else:
        raise ValueError('points must be [P,3] or [N,P,3]')
    if (objR is None) != (objT is None):
        raise ValueError('objR and objT go together')
    R = t = None
    if objR is not None:
        R = torch.as_tensor(objR, dtype=torch.float32, device=dev).reshape(-1, 9).contiguous()
        t = torch.as_tensor(objT, dtype=torch.float32, device=dev).reshape(-1, 3).contiguous()
        if R.shape[0] != N or t.shape[0] != N:
            raise ValueError('objR must be [N,3,3] and objT [N,3]')
    obj = torch.empty(N, P, dtype=torch.uint8, device=dev)
    hum = torch.empty(N, V, dtype=torch.uint8, device=dev)
    sd = torch.empty(N, P, dtype=torch.float32, device=dev) if return_signed_dist else None
    ws = torch.empty(lib.interdiff_contact_labels_workspace_bytes(N, V, mesh.F, P), dtype=torch.uint8, device=dev)
    _lib.check(lib.interdiff_contact_labels(_lib.dptr(v), N, V, _lib.dptr(mesh.faces, torch.int32), mesh.F, _lib.dptr(pts), P, stride,
                                            _lib.dptr(R, allow_none=True), _lib.dptr(t, allow_none=True), float(thres), _lib.dptr(obj), _lib.dptr(hum),
                                            _lib.dptr(sd, allow_none=True), _lib.dptr(ws), ws.numel(), _lib.stream()), 'contact_labels')
    return (obj.bool(), hum.bool(), sd) if return_signed_dist else (obj.bool(), hum.bool())


def face_normals(vertices, faces):
    """Unit normals of the faces (zero for a zero-area face)."""
    v, f = np.asarray(vertices, np.float64), np.asarray(faces, np.int64)
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    l = np.linalg.norm(n, axis=1, keepdims=True)
    return np.where(l > 0, n / np.where(l > 0, l, 1.0), 0.0)


def sample_surface(vertices, faces, n, seed=0):
    """n points spread evenly over the surface -> (points [n,3], face ids [n], face normals [n,3]), float64 / int64.

    Restates ``trimesh.Trimesh.sample(n, return_index=True)``: a face is chosen with probability proportional to its area (a uniform draw
    located in the cumulative areas), then the point is origin + u * edge1 + v * edge2 with (u, v) uniform in the unit square and reflected
    (u, v) -> (1 - u, 1 - v) where u + v > 1.  The draws come from ``numpy.random.Generator(PCG64(seed))``; trimesh draws from numpy's global
    RandomState, so bit parity with a trimesh run is NOT claimed -- only the same distribution."""
    v, f = np.asarray(vertices, np.float64), np.asarray(faces, np.int64)
    rng = np.random.Generator(np.random.PCG64(seed))
    origin, e1, e2 = v[f[:, 0]], v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]
    cum = np.cumsum(0.5 * np.linalg.norm(np.cross(e1, e2), axis=1))
    fid = np.minimum(np.searchsorted(cum, rng.random(n) * cum[-1]), len(f) - 1)
    uv = rng.random((n, 2))
    flip = uv.sum(1) > 1.0
    uv[flip] = 1.0 - uv[flip]
    pts = origin[fid] + uv[:, 0:1] * e1[fid] + uv[:, 1:2] * e2[fid]
    return pts, fid.astype(np.int64), face_normals(v, f)[fid]


def generate_contact(seq, smpl_layer, obj_vertices, obj_faces, num_samples=2048, seed=0, thres=0.02, frame_chunk=256):
    """prepare_behave.py main (:59-119) for one sequence.  ``seq``: the dict of ``data.load_behave_sequence`` (poses [F,156], betas [F,10],
    trans [F,3], obj_angles [F,3], obj_trans [F,3]); ``smpl_layer``: the HIP ``SMPL_Layer`` of the sequence's gender; the object mesh as
    read by ``data.load_obj_mesh`` / ``load_ply_mesh``.  The object is centred at its vertex mean (:89-90) and sampled; per frame the
    rotation matrix comes from scipy in fp64 (:109) and is cast to fp32, the cloud is posed inside the kernel.  Frames run in chunks of
    ``frame_chunk``; a frame's result does not depend on the chunking.
    -> the reference's dict: object_points [P,6] = xyz | face normal, object_contact_vertex_label / human_contact_vertex_label (per frame
    the index arrays, ``np.where`` order), foot_contact_joint_label (10 if jtr[10].y > jtr[11].y else 11)."""
    from scipy.spatial.transform import Rotation
    ov = np.asarray(obj_vertices, np.float64)
    ov = ov - ov.mean(0)
    pts, _, nrm = sample_surface(ov, obj_faces, num_samples, seed)
    dev = smpl_layer.device
    n_frames = min(len(seq['poses']), len(seq['obj_angles']))
    R = Rotation.from_rotvec(np.asarray(seq['obj_angles'][:n_frames], np.float64)).as_matrix().astype(np.float32).reshape(n_frames, 9)
    T = np.asarray(seq['obj_trans'][:n_frames], np.float32)
    cloud = torch.from_numpy(pts.astype(np.float32)).to(dev)
    out = dict(object_points=np.concatenate([pts, nrm], axis=1), object_contact_vertex_label=[], human_contact_vertex_label=[],
               foot_contact_joint_label=[])
    f32 = lambda a, s: torch.from_numpy(np.ascontiguousarray(a[s:s + frame_chunk], dtype=np.float32)).to(dev)
    mesh = label_mesh(smpl_layer.th_faces, smpl_layer.cmodel.V, smpl_layer.v_template, dev)         # sorted by the template's centroids, once
    for s in range(0, n_frames, frame_chunk):
        verts, jtr = smpl_layer(f32(seq['poses'], s), th_betas=f32(seq['betas'], s), th_trans=f32(seq['trans'], s), want_v_posed=False)[:2]
        obj, hum = contact_labels(verts, mesh, cloud, thres, f32(R, s), f32(T, s))
        obj, hum, jt = obj.cpu().numpy(), hum.cpu().numpy(), jtr.cpu().numpy()
        for k in range(len(obj)):
            out['object_contact_vertex_label'].append(np.where(obj[k])[0])
            out['human_contact_vertex_label'].append(np.where(hum[k])[0])
            out['foot_contact_joint_label'].append(10 if jt[k, 10, 1] > jt[k, 11, 1] else 11)
    return out


def write_contact_npz(path, contact):
    """``np.savez(outfile, contact_dict)`` (:119): the dict is pickled into ``arr_0``, which is where ``load_behave_sequence`` looks."""
    np.savez(path, contact)
