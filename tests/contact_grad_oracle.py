"""fp64 numpy restatement of what ``interdiff_correction_geometry_grads`` computes: the two geometry terms of ``LitInteraction.calc_loss_contact``
(train_correction_smpl.py:121-153) and their gradient at the prediction in CLOSED FORM -- no autograd.  With ``y_j = M p_j + t`` the posed object
point, ``x_i`` / ``n_i`` / ``l_i`` a body vertex's position, normal and label, and every mask and index a constant:

    penetration = 1/(N P) sum 20 |y_j - x_i(j)|  over the points with n_i(j) . (y_j - x_i(j)) < 0        i(j): the nearest vertex
    contact     = 1/(N V) sum |x_i - y_j(i)|     over the vertices with l_i > 0.5 and |.| > 0.02         j(i): the nearest posed point

a penetrating point contributes g = 20 (y_j - x_i) / |.| with p = p_j, a contact vertex g = -(x_i - y_j(i)) / |.| with p = p_j(i); each adds g to dL/dt
and g p^T to dL/dM; dL/dM goes back through ``rotation_6d_to_matrix`` (b1 = a1/|a1|, c = a2 - (b1.a2) b1, b2 = c/|c|, b3 = b1 x b2).
Pinned to torch autograd on a line-by-line fp64 restatement of the reference's lines by tests/golden/corr_contact_grad.npz and to a central finite
difference of its own loss (tests/test_contact_grad.py, not on the GPU).
"""
import numpy as np


APART = (0.25, 0.0, 0.0)


def apart(sc, clip=0, shift=APART):
    """A copy of a ``corr_fixtures`` scene with the object of ``clip`` moved out of its body: no point of that clip penetrates in any frame."""
    out = {k: v.copy() for k, v in sc.items()}
    out['obj_trans'][:, clip] += np.asarray(shift, np.float32)
    return out


def rotation_6d_to_matrix(d6):
    """[...,6] -> ([...,3,3] rows b1, b2, b3; the pieces the backward needs)."""
    a1, a2 = d6[..., :3], d6[..., 3:6]
    n1 = np.maximum(np.sqrt((a1 * a1).sum(-1, keepdims=True)), 1e-12)
    b1 = a1 / n1
    s = (b1 * a2).sum(-1, keepdims=True)
    c = a2 - s * b1
    n2 = np.maximum(np.sqrt((c * c).sum(-1, keepdims=True)), 1e-12)
    b2 = c / n2
    return np.stack([b1, b2, np.cross(b1, b2)], axis=-2), (a2, b1, b2, n1, n2, s)


def rotation_6d_backward(dM, parts):
    """dL/dM [...,3,3] -> dL/d(a1 | a2) [...,6]."""
    a2, b1, b2, n1, n2, s = parts
    dot = lambda a, b: (a * b).sum(-1, keepdims=True)
    db1, db2, db3 = dM[..., 0, :], dM[..., 1, :], dM[..., 2, :]
    db1 = db1 + np.cross(b2, db3)
    db2 = db2 + np.cross(db3, b1)
    dc = (db2 - b2 * dot(b2, db2)) / n2
    da2 = dc - b1 * dot(b1, dc)
    db1 = db1 - s * dc - a2 * dot(b1, dc)
    da1 = (db1 - b1 * dot(b1, db1)) / n1
    return np.concatenate([da1, da2], axis=-1)


def nn_index(q, r, chunk=512):
    """[N,Q,3], [N,R,3] -> int64 [N,Q]: exact argmin of d2 = (dx*dx + dy*dy) + dz*dz, lowest index wins."""
    out = np.empty(q.shape[:2], np.int64)
    for n in range(q.shape[0]):
        for s in range(0, q.shape[1], chunk):
            d = [q[n, s:s + chunk, None, k] - r[n, None, :, k] for k in range(3)]
            out[n, s:s + chunk] = np.argmin((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2], axis=1)
    return out


def pose(pred, pts):
    """pred [T,B,9], pts [B,P,3] -> (y [T*B,P,3], the Gram-Schmidt pieces)."""
    M, parts = rotation_6d_to_matrix(pred[..., :6])
    y = np.einsum('tbij,bpj->tbpi', M, pts) + pred[:, :, None, 6:]
    return y.reshape(-1, pts.shape[1], 3), parts


def geometry(pred, obj_points, human_verts, w_pen, w_con, index=None):
    """pred [T,B,9], obj_points [B,P,>=3], human_verts [T,B,V,7], the two annealed weights -> dict: ``loss`` = w_pen * penetration + w_con * contact,
    ``terms`` (penetration, contact), ``grad`` [T,B,9] = d loss / d pred, ``grad_pen`` / ``grad_con`` (the two shares), ``frames`` [T*B,4] = per frame
    (penetration sum, contact sum, penetrating points, contact vertices), ``yidx`` [N,P] / ``xidx`` [N,V], the masks ``pen`` / ``con``.  ``index``: (yidx, xidx) to hold
    fixed (a finite difference must not let them move)."""
    pred = np.asarray(pred, np.float64)
    T, B = pred.shape[:2]
    pts = np.asarray(obj_points, np.float64)[..., :3]
    hv = np.asarray(human_verts, np.float64).reshape(T * B, -1, 7)
    N, V, P = T * B, hv.shape[1], pts.shape[1]
    x, xn, lab = hv[..., :3], hv[..., 3:6], hv[..., 6]
    y, parts = pose(pred, pts)
    yidx, xidx = index if index is not None else (nn_index(y, x), nn_index(x, y))
    take = lambda a, i: np.take_along_axis(a, i[..., None], axis=1)
    p_all = np.broadcast_to(pts[None], (T, B, P, 3)).reshape(N, P, 3)
    # object -> human
    v = y - take(x, yidx)
    d = np.sqrt((v * v).sum(-1))
    dots = (take(xn, yidx) * v).sum(-1)
    pen = (dots < 0) & (d > 0)
    g_pen = np.where(pen[..., None], 20.0 * v / np.where(d > 0, d, 1.0)[..., None], 0.0)           # [N,P,3]
    # human -> object
    u = x - take(y, xidx)
    e = np.sqrt((u * u).sum(-1))
    con = (e > 0.02) & (lab > 0.5)
    g_con = np.where(con[..., None], -u / np.where(e > 0, e, 1.0)[..., None], 0.0)                 # [N,V,3]
    p_con = take(p_all, xidx)

    def back(g, p, scale):
        dM = scale * np.einsum('nqi,nqj->nij', g, p).reshape(T, B, 3, 3)
        dt = scale * g.sum(1).reshape(T, B, 3)
        return np.concatenate([rotation_6d_backward(dM, parts), dt], axis=-1)
    grad_pen, grad_con = back(g_pen, p_all, w_pen / (N * P)), back(g_con, p_con, w_con / (N * V))
    frames = np.stack([(20.0 * d * pen).sum(1), (e * con).sum(1), pen.sum(1).astype(np.float64), con.sum(1).astype(np.float64)], axis=1)
    terms = np.array([frames[:, 0].sum() / (N * P), frames[:, 1].sum() / (N * V)])
    return dict(loss=w_pen * terms[0] + w_con * terms[1], terms=terms, grad=grad_pen + grad_con, grad_pen=grad_pen, grad_con=grad_con, frames=frames,
                yidx=yidx, xidx=xidx, pen=pen, con=con)


def finite_difference(pred, obj_points, human_verts, w_pen, w_con, entries, h=1e-6):
    """Central difference of ``geometry(...)['loss']`` in the listed flat entries of ``pred``, indices and masks held at their values at ``pred``."""
    pred = np.asarray(pred, np.float64)
    base = geometry(pred, obj_points, human_verts, w_pen, w_con)
    index = (base['yidx'], base['xidx'])
    out = []
    for i in entries:
        vals = []
        for sgn in (1.0, -1.0):
            q = pred.copy().reshape(-1)
            q[i] += sgn * h
            r = geometry(q.reshape(pred.shape), obj_points, human_verts, w_pen, w_con, index)
            assert np.array_equal(r['pen'], base['pen']) and np.array_equal(r['con'], base['con']), 'a mask moved inside the difference: smaller h or another entry'
            vals.append(r['loss'])
        out.append((vals[0] - vals[1]) / (2 * h))
    return np.asarray(out), base
