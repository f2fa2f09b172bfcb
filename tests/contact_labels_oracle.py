"""CPU restatement (fp64 numpy, brute force) of the contact-label contract of SURVEY.md B.6 for the tests, and the fixtures they share.

    d[p] = min over faces of the point-triangle distance (face, edge and corner regions of every triangle)
    w[p] = (1 / 4 pi) sum over faces of 2 atan2(A.(B x C), |A||B||C| + A.B |C| + B.C |A| + C.A |B|)  (A, B, C = corners - p);
           a face with a zero normal contributes 0 and counts for d through its three edges
    S = (1 - 2 w) d,  obj_label = S < thres,  human_label[v] = exists labelled p with |p - v| < thres

igl / trimesh / psbody are not available, so nothing here is compared against them: the restatement defines the contract.
The distance is written as "the three edges always, the plane where the projection has non-negative barycentric coordinates" -- not as the
if / else cascade over vertex, edge and face regions that the kernel uses -- and it is pinned by known answers in tests/test_contact_labels.py."""
import numpy as np

THRES = 0.02


def _block(q, m):
    """One block of points against all faces, every quantity as a [Pb,F] plane (no trailing axis of 3: numpy reduces those slowly).  With
    A = a - q and the per-face constants, every other dot product follows from g1 = A.ab, g2 = A.ac and |A|^2 in fp64."""
    Ax, Ay, Az = m['a'][:, 0] - q[:, 0:1], m['a'][:, 1] - q[:, 1:2], m['a'][:, 2] - q[:, 2:3]
    dot = lambda e: Ax * e[:, 0] + Ay * e[:, 1] + Az * e[:, 2]
    g1, g2, num = dot(m['ab']), dot(m['ac']), dot(m['n'])                   # num = A.(B x C) = A.n
    d00, d01, d11, dbc = m['d00'], m['d01'], m['d11'], m['dbc']
    la2 = Ax * Ax + Ay * Ay + Az * Az
    lb2, lc2 = np.maximum(la2 + 2 * g1 + d00, 0.0), np.maximum(la2 + 2 * g2 + d11, 0.0)
    la, lb, lc = np.sqrt(la2), np.sqrt(lb2), np.sqrt(lc2)
    den = la * lb * lc + (la2 + g1) * lc + (la2 + g1 + g2 + d01) * la + (la2 + g2) * lb
    om = 2.0 * np.arctan2(num, den)
    om[:, m['flat']] = 0.0
    w = om.sum(-1) / (4.0 * np.pi)

    def seg(x2, xe, ee):                                                     # |x - s e|^2, s = clip(x.e / e.e), from x.x, x.e, e.e
        s = np.clip(xe / np.where(ee > 0, ee, 1.0), 0.0, 1.0)
        return np.maximum(x2 - 2 * s * xe + s * s * ee, 0.0)
    # the three edges always (x = q - a = -A for ab and ac, x = q - b = -B for bc) ...
    e = np.minimum(np.minimum(seg(la2, -g1, d00), seg(la2, -g2, d11)), seg(lb2, (g1 + d00) - (g2 + d01), dbc))
    # ... and the plane distance where the projection has non-negative barycentric coordinates: (B x C).n, (C x A).n, (A x B).n by Lagrange's identity
    u = (g1 + d00) * (g2 + d11) - (g2 + d01) * (g1 + d01)
    s = (g1 + d01) * g2 - (g2 + d11) * g1
    t = g1 * (g2 + d01) - g2 * (g1 + d00)
    inside = (u >= 0) & (s >= 0) & (t >= 0) & ~m['flat']
    d2 = np.where(inside, num * num / m['nn1'], e)
    return np.sqrt(d2.min(-1)), w


def point_mesh(points, verts, faces, block=64, threads=1):
    """points [P,3], verts [V,3], faces [F,3] -> d [P], w [P] (float64).  ``threads``: blocks of points on a thread pool (numpy releases the GIL)."""
    p = np.asarray(points, np.float64)
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    ab, ac, bc = b - a, c - a, c - b
    n = np.cross(ab, ac)
    nn = (n * n).sum(-1)
    m = dict(a=a, ab=ab, ac=ac, n=n, flat=nn == 0, nn1=np.where(nn == 0, 1.0, nn), d00=(ab * ab).sum(-1), d01=(ab * ac).sum(-1), d11=(ac * ac).sum(-1),
             dbc=(bc * bc).sum(-1))
    blocks = [p[s0:s0 + block] for s0 in range(0, len(p), block)]
    if threads > 1:
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(threads) as ex:
            res = list(ex.map(lambda q: _block(q, m), blocks))
    else:
        res = [_block(q, m) for q in blocks]
    return np.concatenate([r[0] for r in res]), np.concatenate([r[1] for r in res])


def body_labels(points, labelled, verts, thr):
    """human_label [V]: any labelled point strictly closer than thr."""
    q = np.asarray(points, np.float64)[np.asarray(labelled, bool)]
    v = np.asarray(verts, np.float64)
    if len(q) == 0:
        return np.zeros(len(v), bool)
    out = np.zeros(len(v), bool)
    for s0 in range(0, len(v), 1024):
        dv = v[s0:s0 + 1024, None, :] - q[None]
        out[s0:s0 + 1024] = (np.sqrt((dv * dv).sum(-1)) < thr).any(1)
    return out


def frame(points, verts, faces, thres=THRES):
    """Everything the comparison rule needs for one frame: d, w, S, band, lo, hi, the labels, and the two bracketing body-label runs."""
    d, w = point_mesh(points, verts, faces)
    S = (1.0 - 2.0 * w) * d
    band = 1e-5 + 2.0 * d * 1e-4
    lo, hi = S < thres - band, S < thres + band
    return dict(d=d, w=w, S=S, band=band, lo=lo, hi=hi, label=S < thres, human=body_labels(points, S < thres, verts, thres),
                human_lo=body_labels(points, lo, verts, thres - 1e-5), human_hi=body_labels(points, hi, verts, thres + 1e-5))


def pose_points(points, R, t):
    """p R^T + t in fp64 from the fp32 operands the kernel gets."""
    return np.asarray(points, np.float64) @ np.asarray(R, np.float64).reshape(3, 3).T + np.asarray(t, np.float64)


def check_frame(o, obj_label, human_label, signed_dist=None, tag=''):
    """The comparison rule of the issue on one frame.  Prints every figure before it asserts."""
    sure_p, sure_v = o['lo'] == o['hi'], o['human_lo'] == o['human_hi']
    bad_p = int((np.asarray(obj_label, bool) != o['label'])[sure_p].sum())
    bad_v = int((np.asarray(human_label, bool) != o['human_lo'])[sure_v].sum())
    msg = '%s points: %d labelled, %d excluded, %d wrong; vertices: %d labelled, %d excluded, %d wrong' % (
        tag, int(o['label'].sum()), int((~sure_p).sum()), bad_p, int(o['human'].sum()), int((~sure_v).sum()), bad_v)
    if signed_dist is not None:
        err = np.abs(np.asarray(signed_dist, np.float64) - o['S'])
        worst = float((err / o['band']).max())
        msg += '; max |S32 - S64| %.3e (worst err / band %.3f)' % (float(err.max()), worst)
    print(msg)
    assert bad_p == 0 and bad_v == 0, msg
    if signed_dist is not None:
        assert np.isfinite(np.asarray(signed_dist)).all()
        assert worst <= 1.0, msg


# ---------------------------------------------------------------------------------------------------------------- fixtures
def icosphere(subdiv=2):
    """Unit icosphere, outward orientation: (V [n,3] float64, F [m,3] int64); subdiv 2 -> 162 vertices, 320 faces."""
    g = (1.0 + np.sqrt(5.0)) / 2.0
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(x, np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(subdiv):
        mid, nf = {}, []

        def m(i, j):
            k = (min(i, j), max(i, j))
            if k not in mid:
                x = v[i] + v[j]
                v.append(x / np.linalg.norm(x))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v), np.array(f, np.int64)


def bumpy_sphere(radius=0.25):
    """Icosphere subdivided twice with radial bumps (non-convex): V = 162, F = 320."""
    v, f = icosphere(2)
    r = radius * (1.0 + 0.18 * np.sin(5.0 * v[:, 0]) * np.cos(4.0 * v[:, 1]) + 0.1 * np.sin(7.0 * v[:, 2]))
    return v * r[:, None], f


def torus(nu=84, nv=82, R=0.35, r=0.12):
    """nu x nv torus grid, outward orientation, plus two unreferenced vertices: V = nu nv + 2 = 6890, F = 2 nu nv = 13776 at the defaults."""
    u, w = np.meshgrid(np.arange(nu) * 2 * np.pi / nu, np.arange(nv) * 2 * np.pi / nv, indexing='ij')
    v = np.stack([(R + r * np.cos(w)) * np.cos(u), (R + r * np.cos(w)) * np.sin(u), r * np.sin(w)], axis=-1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing='ij')
    idx = lambda a, b: ((a % nu) * nv + (b % nv)).reshape(-1)
    p00, p10, p01, p11 = idx(i, j), idx(i + 1, j), idx(i, j + 1), idx(i + 1, j + 1)
    f = np.concatenate([np.stack([p00, p10, p11], 1), np.stack([p00, p11, p01], 1)])
    v = np.concatenate([v, [[0.0, 0.0, 0.3], [0.0, 0.0, -0.3]]])
    return v, f.astype(np.int64)


def rigid(seed, n, shift=0.5, angle=1.5):
    """n rigid poses (R [n,3,3], t [n,3]) float64 from a seed."""
    from scipy.spatial.transform import Rotation
    rs = np.random.RandomState(seed)
    return Rotation.from_rotvec(rs.uniform(-angle, angle, (n, 3))).as_matrix(), rs.uniform(-shift, shift, (n, 3))


def small_case(kind='closed', seed=11):
    """The small GPU cases: bumpy sphere posed differently in N = 3 frames, a canonical cloud of P = 333 points that straddles the surface and
    its own per-frame pose.  kind: 'closed' (F = 320), 'open' (7 faces removed, F = 313), 'flat' (one collinear zero-area face appended, F = 321).
    -> dict(verts f32 [3,162,3], faces int64, points f32 [333,3], objR f32 [3,9], objT f32 [3,3])."""
    v, f = bumpy_sphere()
    if kind == 'open':
        f = np.delete(f, [3, 50, 51, 52, 120, 200, 319], axis=0)
    elif kind == 'flat':
        v = np.concatenate([v, [0.5 * (v[10] + v[40])]])                  # exactly between two vertices of the mesh: collinear with them
        f = np.concatenate([f, [[10, len(v) - 1, 40]]])
    rs = np.random.RandomState(seed)
    N, P = 3, 333
    dirs = rs.standard_normal((P, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    cloud = dirs * 0.25 * rs.uniform(0.75, 1.3, (P, 1))                     # canonical cloud in the MESH's rest frame
    Rm, tm = rigid(seed + 1, N)                                             # the mesh's pose per frame
    Ro, to = rigid(seed + 2, N, shift=0.02)                                 # a small extra motion of the cloud relative to the mesh
    verts = np.float32(np.einsum('vc,ndc->nvd', v, Rm) + tm[:, None])
    # the cloud's pose: first its own small motion, then the mesh's pose -> it keeps straddling the surface in every frame
    R = np.einsum('nab,nbc->nac', Rm, Ro)
    t = np.einsum('nab,nb->na', Rm, to) + tm
    return dict(verts=verts, faces=f, points=np.float32(cloud), objR=np.float32(R.reshape(N, 9)), objT=np.float32(t))


def torus_case(seed=5):
    """The real-size case: torus V = 6890, F = 13776 under N = 2 rigid poses, P = 2048 points in a ball that cuts through the tube."""
    v, f = torus()
    rs = np.random.RandomState(seed)
    N, P = 2, 2048
    x = rs.standard_normal((P, 3))
    x *= (0.22 * rs.uniform(0, 1, (P, 1)) ** (1.0 / 3.0)) / np.linalg.norm(x, axis=1, keepdims=True)
    cloud = x + np.array([0.35 + 0.12, 0.0, 0.0])                           # centred on the tube's outer equator
    Rm, tm = rigid(seed + 1, N, shift=1.5)
    Ro, to = rigid(seed + 2, N, shift=0.03, angle=0.15)
    verts = np.float32(np.einsum('vc,ndc->nvd', v, Rm) + tm[:, None])
    R = np.einsum('nab,nbc->nac', Rm, Ro)
    t = np.einsum('nab,nb->na', Rm, to) + tm
    return dict(verts=verts, faces=f, points=np.float32(cloud), objR=np.float32(R.reshape(N, 9)), objT=np.float32(t))


def case_oracle(case):
    """Per-frame oracle records of a case (points posed in fp64 from the fp32 operands)."""
    return [frame(pose_points(case['points'], case['objR'][n], case['objT'][n]), case['verts'][n], case['faces']) for n in range(len(case['verts']))]


def box_mesh(size=(0.3, 0.2, 0.25), centre=(0.0, 0.0, 0.0)):
    """12-triangle box, outward orientation."""
    s, c = np.asarray(size, np.float64) / 2, np.asarray(centre, np.float64)
    v = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float64) * s + c
    f = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]], np.int64)
    return v, f
