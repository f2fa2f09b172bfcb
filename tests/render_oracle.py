"""numpy restatement of the mesh renderer's contract (interdiff_amd/csrc/render.h): a floating setup stage (every operation in ``ft``: float64 is
the oracle, float32 the what-a-float32-restatement-gives variant), and an INTEGER raster / resolve stage on setup records (int64, exact).
Also the meshes the tests render.  Nothing here is imported by the product."""
import numpy as np

SUB, GUARD, ZONE, REC, TILE, CMAX = 16, 32768, 1 << 28, 20, 16, 4080
SCENE_SPACE, VERTEX_RGB = 1, 2


# ---------------------------------------------------------------------------------------------------------------------------------------
# scene (the idf_render_scene the kernel receives: every entry a float32 value -- the inputs are the same for both sides)
def raymond_lights():
    th, ph = np.pi * np.array([0, 2.0 / 6.0, 1.0 / 2.0]), np.pi * np.array([1.0 / 3.0, 2.0 / 3.0, 1.0 / 2.0])
    L = np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)], axis=1)
    return L / np.linalg.norm(L, axis=1, keepdims=True)


def make_scene(off=(0, 0, 0), bg=(1, 1, 1)):
    f = lambda x: np.asarray(x, np.float32)
    return dict(off=f(off), cam_t=f([0, 2, 2.5]), cam_cos=f(np.cos(np.pi / 6)), cam_sin=f(np.sin(np.pi / 6)), znear=f(0.05), focal=f(1 / np.tan(np.pi / 6)),
                light=f(raymond_lights()).reshape(9), light_gain=f(5.0 / 3.0 / np.pi), ambient=f(0.3), bg=f(bg))


def bg_bytes(scene):
    return np.rint(np.clip(scene['bg'].astype(np.float64), 0, 1) * 255).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------------------------------
# setup stage
def vertex_stage(scene, view, scene_space, pos, nrm, rgb, ft=np.float64):
    """pos, nrm, rgb [n,3] -> [n,6] = xc, yc, d, r, g, b in dtype ft."""
    s = {k: v.astype(ft) for k, v in scene.items()}
    p, n, c = pos.astype(ft), nrm.astype(ft), rgb.astype(ft)
    if not scene_space:
        p, n = -p - s['off'], -n
        for _ in range(view & 3):
            p = np.stack([p[:, 2], p[:, 1], -p[:, 0]], axis=1)
            n = np.stack([n[:, 2], n[:, 1], -n[:, 0]], axis=1)
    q = p - s['cam_t']
    yc = s['cam_cos'] * q[:, 1] - s['cam_sin'] * q[:, 2]
    d = -(s['cam_cos'] * q[:, 2] + s['cam_sin'] * q[:, 1])
    L = s['light'].reshape(3, 3)
    lam = ft(0)
    for k in range(3):
        lam = lam + np.maximum(n[:, 0] * L[k, 0] + n[:, 1] * L[k, 1] + n[:, 2] * L[k, 2], ft(0))
    shade = np.minimum(s['ambient'] + s['light_gain'] * lam, ft(1))
    return np.stack([q[:, 0], yc, d, c[:, 0] * shade, c[:, 1] * shade, c[:, 2] * shade], axis=1).astype(ft)


def project(scene, H, W, v, ft=np.float64):
    """v [..., 6] camera-space vertices with d >= near -> float X, Y (integral), int Z, R, G, B"""
    k = ft(8 * H) * scene['focal'].astype(ft)
    with np.errstate(all='ignore'):
        X = np.rint(v[..., 0] / v[..., 2] * k + ft(8 * W))
        Y = np.rint(v[..., 1] / v[..., 2] * (-k) + ft(8 * H))
        q = np.minimum(scene['znear'].astype(ft) / v[..., 2], ft(1))
        Z = ZONE - np.rint(np.nan_to_num(q) * ft(ZONE)).astype(np.int64)
        C = np.rint(np.clip(np.nan_to_num(v[..., 3:6]), 0, 1) * ft(CMAX)).astype(np.int64)
    return X, Y, Z, C


def clip_edge(scene, a, b, ft=np.float64):
    """near-plane point of the edge from a (in front) to b (behind)"""
    near = scene['znear'].astype(ft)
    with np.errstate(all='ignore'):
        s = ((near - a[..., 2]) / (b[..., 2] - a[..., 2]))[..., None]
        o = a + s * (b - a)
    o[..., 2] = near
    return o.astype(ft)


def setup_triangles(scene, H, W, tv, ft=np.float64):
    """tv [F,3,6] camera-space triangles -> (records int32 [2F,20], dropped)"""
    F = tv.shape[0]
    near = scene['znear'].astype(ft)
    front = tv[:, :, 2] >= near
    nf = front.sum(1)
    slots = np.zeros((F, 2, 3, 6), ft)
    used = np.zeros((F, 2), bool)
    ar = np.arange(F)
    m = nf == 3
    slots[m, 0], used[m, 0] = tv[m], True
    m = nf == 1
    if m.any():
        a = np.argmax(front[m], axis=1)
        va, vb, vc = tv[ar[m], a], tv[ar[m], (a + 1) % 3], tv[ar[m], (a + 2) % 3]
        slots[m, 0] = np.stack([va, clip_edge(scene, va, vb, ft), clip_edge(scene, va, vc, ft)], axis=1)
        used[m, 0] = True
    m = nf == 2
    if m.any():
        a = np.argmin(front[m], axis=1)
        va, vb, vc = tv[ar[m], a], tv[ar[m], (a + 1) % 3], tv[ar[m], (a + 2) % 3]
        ca, ba = clip_edge(scene, vc, va, ft), clip_edge(scene, vb, va, ft)
        slots[m, 0] = np.stack([vb, vc, ca], axis=1)
        slots[m, 1] = np.stack([vb, ca, ba], axis=1)
        used[m] = True
    sl = slots.reshape(2 * F, 3, 6)
    used = used.reshape(2 * F)
    safe = sl.copy()
    safe[~used] = 1                                   # any finite vertex with d > 0: never read back
    X, Y, Z, C = project(scene, H, W, safe, ft)
    x1, y1 = ft(SUB * W), ft(SUB * H)
    culled = (X < 0).all(1) | (X > x1).all(1) | (Y < 0).all(1) | (Y > y1).all(1)
    with np.errstate(all='ignore'):
        inband = ((np.abs(X) <= GUARD) & (np.abs(Y) <= GUARD)).all(1)
    valid = used & ~culled & inband
    dropped = int((used & ~culled & ~inband).sum())
    rec = np.zeros((2 * F, REC), np.int32)
    Xi, Yi = np.where(valid[:, None], X, 0).astype(np.int64), np.where(valid[:, None], Y, 0).astype(np.int64)
    for i in range(3):
        rec[valid, 6 * i], rec[valid, 6 * i + 1], rec[valid, 6 * i + 2] = Xi[valid, i], Yi[valid, i], Z[valid, i]
        rec[valid, 6 * i + 3:6 * i + 6] = C[valid, i]
    rec[valid, 18] = 1
    return rec, dropped


def pose_mesh(m, n, ft=np.float64):
    """frame n of a mesh dict: positions and normals [V,3] in ft (posed by R, t when given: p R^T + t)"""
    fr = n if m['verts'].shape[0] > 1 else 0
    p, q = m['verts'][fr].astype(ft), m['normals'][fr].astype(ft)
    if m.get('R') is not None:
        R, t = m['R'][n].astype(ft), m['t'][n].astype(ft)
        p, q = ((p[:, 0:1] * R[:, 0] + p[:, 1:2] * R[:, 1]) + p[:, 2:3] * R[:, 2]) + t, (q[:, 0:1] * R[:, 0] + q[:, 1:2] * R[:, 1]) + q[:, 2:3] * R[:, 2]
    return p.astype(ft), q.astype(ft)


def setup_records(scene, meshes, N, views, H, W, ft=np.float64):
    """meshes: list of dicts verts / normals [frames,V,3], faces [F,3], rgb [N,3] or [V,3], flags, optional R [N,3,3], t [N,3].
    -> (records int32 [N, views, 2 sum F, 20], dropped)"""
    out, dropped = [], 0
    for n in range(N):
        for view in range(views):
            tris = []
            for m in meshes:
                p, q = pose_mesh(m, n, ft)
                rgb = m['rgb'] if m['flags'] & VERTEX_RGB else np.broadcast_to(m['rgb'][n], p.shape)
                v = vertex_stage(scene, view, bool(m['flags'] & SCENE_SPACE), p, q, np.asarray(rgb), ft)
                tris.append(v[np.asarray(m['faces'], np.int64)])
            rec, dr = setup_triangles(scene, H, W, np.concatenate(tris), ft)
            out.append(rec)
            dropped += dr
    return np.stack(out).reshape(N, views, -1, REC), dropped


# ---------------------------------------------------------------------------------------------------------------------------------------
# integer stage
def _edge(ax, ay, bx, by, px, py):
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax)


def _bias(ax, ay, bx, by):
    dx, dy = bx - ax, by - ay
    return 0 if (dy < 0 or (dy == 0 and dx > 0)) else 1


def orient(rec):
    """-> (x[3], y[3], z[3], c[3][3], A) python ints / int64 arrays, oriented so that A >= 0"""
    r = np.asarray(rec, np.int64)
    x, y, z, c = r[0:18:6].copy(), r[1:18:6].copy(), r[2:18:6].copy(), np.stack([r[6 * i + 3:6 * i + 6] for i in range(3)])
    A = _edge(x[0], y[0], x[1], y[1], x[2], y[2])
    if A < 0:
        A = -A
        for a in (x, y, z):
            a[1], a[2] = a[2], a[1]
        c = c[[0, 2, 1]]
    return x, y, z, c, A


def pixel_box(rec, H, W):
    xs, ys = rec[..., 0:18:6].astype(np.int64), rec[..., 1:18:6].astype(np.int64)
    i0, i1 = np.maximum((xs.min(-1) + 7) >> 4, 0), np.minimum((xs.max(-1) - 8) >> 4, W - 1)
    j0, j1 = np.maximum((ys.min(-1) + 7) >> 4, 0), np.minimum((ys.max(-1) - 8) >> 4, H - 1)
    return i0, i1, j0, j1, (rec[..., 18] == 1) & (i0 <= i1) & (j0 <= j1)


def cover(rec, I, J):
    """coverage, depth and colour of the record at pixels (I, J) (int arrays): -> covered bool, depth int64, rgb int64 [..., 3]"""
    x, y, z, c, A = orient(rec)
    I, J = np.asarray(I, np.int64), np.asarray(J, np.int64)
    if rec[18] != 1 or A == 0:
        return np.zeros(I.shape, bool), np.zeros(I.shape, np.int64), np.zeros(I.shape + (3,), np.int64)
    px, py = SUB * I + SUB // 2, SUB * J + SUB // 2
    e = ((1, 2), (2, 0), (0, 1))
    w = [_edge(x[a], y[a], x[b], y[b], px, py) for a, b in e]
    cov = np.ones(I.shape, bool)
    for k, (a, b) in enumerate(e):
        cov &= w[k] >= _bias(x[a], y[a], x[b], y[b])
    wz = np.where(cov, w[0] * z[0] + w[1] * z[1] + w[2] * z[2], 0)
    depth = wz // A
    rgb = np.stack([np.where(cov, (2 * (w[0] * c[0, k] + w[1] * c[1, k] + w[2] * c[2, k]) + 16 * A) // (32 * A), 0) for k in range(3)], axis=-1)
    return cov, depth, rgb


def raster(records, H, W, bg=(255, 255, 255), count=False):
    """records int32 [S,20] -> id int32 [H,W] (-1 background), depth int32 (0x7fffffff), rgb uint8 [H,W,3] (+ per-pixel cover count)"""
    EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
    key = np.full((H, W), EMPTY, np.uint64)
    cnt = np.zeros((H, W), np.int32)
    i0, i1, j0, j1, ok = pixel_box(records, H, W)
    for s in np.nonzero(ok)[0]:
        J, I = np.mgrid[j0[s]:j1[s] + 1, i0[s]:i1[s] + 1]
        cov, depth, _ = cover(records[s], I, J)
        if not cov.any():
            continue
        k = (depth.astype(np.uint64) << np.uint64(32)) | np.uint64(s)
        sub = key[j0[s]:j1[s] + 1, i0[s]:i1[s] + 1]
        sub[...] = np.where(cov, np.minimum(sub, k), sub)
        cnt[j0[s]:j1[s] + 1, i0[s]:i1[s] + 1] += cov
    hit = key != EMPTY
    ids = np.where(hit, (key & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    depth = np.where(hit, (key >> np.uint64(32)).astype(np.int64), 0x7fffffff).astype(np.int32)
    rgb = np.empty((H, W, 3), np.uint8)
    rgb[...] = np.asarray(bg, np.uint8)
    for s in np.unique(ids[hit]):
        J, I = np.nonzero(ids == s)
        rgb[J, I] = cover(records[s], I, J)[2].astype(np.uint8)
    return (ids, depth, rgb, cnt) if count else (ids, depth, rgb)


def render(scene, meshes, N, views, H, W, ft=np.float64):
    """-> ids [N,views,H,W], depth, rgb [N,views,H,W,3], records, dropped"""
    rec, dropped = setup_records(scene, meshes, N, views, H, W, ft)
    bg = bg_bytes(scene)
    out = [raster(rec[n, v], H, W, bg) for n in range(N) for v in range(views)]
    st = lambda k: np.stack([o[k] for o in out]).reshape((N, views) + out[0][k].shape)
    return st(0), st(1), st(2), rec, dropped


def near_id_boundary(ids):
    """[H,W] bool: the pixel or one of its 8 neighbours differs in id from one of ITS 8 neighbours, i.e. lies within one pixel of an id boundary"""
    H, W = ids.shape
    p = np.pad(ids, 1, mode='edge')
    edge = np.zeros((H, W), bool)
    for dj in (-1, 0, 1):
        for di in (-1, 0, 1):
            edge |= p[1 + dj:1 + dj + H, 1 + di:1 + di + W] != ids
    pe = np.pad(edge, 1, mode='constant')
    out = np.zeros((H, W), bool)
    for dj in (-1, 0, 1):
        for di in (-1, 0, 1):
            out |= pe[1 + dj:1 + dj + H, 1 + di:1 + di + W]
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# meshes
def vertex_normals(verts, faces):
    """area-weighted smooth normals, [.., V, 3] float64"""
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64)
    fn = np.cross(v[..., f[:, 1], :] - v[..., f[:, 0], :], v[..., f[:, 2], :] - v[..., f[:, 0], :])
    out = np.zeros_like(v)
    for k in range(3):
        np.add.at(out, (Ellipsis, f[:, k], slice(None)), fn)
    return out / np.maximum(np.linalg.norm(out, axis=-1, keepdims=True), 1e-6)


def ellipsoid(radii=(0.22, 0.85, 0.15), rings=84, segs=82):
    """closed lat-long ellipsoid, outward winding: V = rings * segs + 2 = 6890, F = 2 segs (rings - 1) + 2 segs = 13776"""
    th = np.pi * (np.arange(rings) + 1) / (rings + 1)
    ph = 2 * np.pi * np.arange(segs) / segs
    ring = np.stack([np.outer(np.sin(th), np.cos(ph)), np.repeat(np.cos(th)[:, None], segs, 1), np.outer(np.sin(th), np.sin(ph))], axis=-1).reshape(-1, 3)
    v = np.concatenate([ring, [[0, 1, 0]], [[0, -1, 0]]]) * np.asarray(radii)
    idx = lambda r, s: r * segs + (s % segs)
    f = []
    for r in range(rings - 1):
        for s in range(segs):
            f += [[idx(r, s), idx(r, s + 1), idx(r + 1, s)], [idx(r, s + 1), idx(r + 1, s + 1), idx(r + 1, s)]]
    top, bot = rings * segs, rings * segs + 1
    for s in range(segs):
        f += [[top, idx(0, s + 1), idx(0, s)], [bot, idx(rings - 1, s), idx(rings - 1, s + 1)]]
    return v.astype(np.float32), np.asarray(f, np.int32)


def box(extents=(0.3, 0.25, 0.2)):
    e = np.asarray(extents) / 2
    v = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float64) * e
    f = [[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]]
    return v.astype(np.float32), np.asarray(f, np.int32)


def ground_mesh(minx, maxx, minz, maxz):
    """The reference's ground: two thin boxes centred at ((maxx - minx) / 2, (maxz - minz) / 2) with extents x 1 and x 1.6 of the body's range, lying
    in y = [-2e-6, 0]; flat normals (24 vertices per box), the colours of mesh_utils.py (189, 195, 199) and (238, 238, 238).  The outer box is lowered
    by 1 mm (a stated departure: in the reference the two top faces are coplanar and the picture is the GL driver's z-fighting)."""
    ex, ez, cx, cz = maxx - minx, maxz - minz, (maxx - minx) / 2, (maxz - minz) / 2
    V, Nn, C, Fc = [], [], [], []
    for scale, col, drop in ((1.0, (189, 195, 199), 0.0), (1.6, (238, 238, 238), 1e-3)):
        lo = np.array([cx - scale * ex / 2, -2e-6 - drop, cz - scale * ez / 2])
        hi = np.array([cx + scale * ex / 2, 0.0 - drop, cz + scale * ez / 2])
        for axis in range(3):
            for side in (0, 1):
                u, w = (axis + 1) % 3, (axis + 2) % 3
                quad = []
                for a, b in ((0, 0), (1, 0), (1, 1), (0, 1)):
                    p = np.zeros(3)
                    p[axis], p[u], p[w] = (hi if side else lo)[axis], (hi if a else lo)[u], (hi if b else lo)[w]
                    quad.append(p)
                nrm = np.zeros(3)
                nrm[axis] = 1.0 if side else -1.0
                base = len(V)
                V += quad
                Nn += [nrm] * 4
                C += [np.asarray(col) / 255.0] * 4
                Fc += [[base, base + 1, base + 2], [base, base + 2, base + 3]]
    return np.asarray(V, np.float32), np.asarray(Nn, np.float32), np.asarray(C, np.float32), np.asarray(Fc, np.int32)


def mesh(verts, faces, rgb, normals=None, flags=0, R=None, t=None):
    verts = np.asarray(verts, np.float32)
    verts = verts[None] if verts.ndim == 2 else verts
    normals = vertex_normals(verts, faces) if normals is None else np.asarray(normals)
    normals = normals[None] if normals.ndim == 2 else normals
    return dict(verts=np.ascontiguousarray(verts), normals=np.ascontiguousarray(normals, np.float32), faces=np.ascontiguousarray(faces, np.int32),
                rgb=np.ascontiguousarray(rgb, np.float32), flags=flags, R=None if R is None else np.ascontiguousarray(R, np.float32),
                t=None if t is None else np.ascontiguousarray(t, np.float32))


def unproject(scene, H, W, X, Y, d):
    """scene-space point (of a SCENE_SPACE mesh) that the camera sees at sub-pixel (X, Y), depth d: float64"""
    k = 8 * H * float(scene['focal'])
    xc, yc = (np.asarray(X, np.float64) - 8 * W) / k * d, (np.asarray(Y, np.float64) - 8 * H) / (-k) * d
    c, s = float(scene['cam_cos']), float(scene['cam_sin'])
    zc = -np.asarray(d, np.float64) * np.ones_like(xc)
    qy, qz = c * yc + s * zc, -s * yc + c * zc                    # inverse of yc = c qy - s qz, zc = s qy + c qz
    return np.stack([xc + float(scene['cam_t'][0]), qy + float(scene['cam_t'][1]), qz + float(scene['cam_t'][2])], axis=-1)


def adversarial_scene(scene, H, W, seed=0):
    """~40 scene-space triangles with per-vertex colours, placed through the camera so that their SCREEN positions are what is stated: shared edges
    (horizontal, vertical, diagonal), slivers thinner than a pixel, zero-area faces, two interpenetrating triangles, coplanar duplicates, a vertex on a
    pixel centre, one triangle across the near plane, one wholly behind the camera, one wholly off-screen, one covering the whole screen."""
    rs = np.random.RandomState(seed)
    P = lambda x, y, d: unproject(scene, H, W, 16.0 * x, 16.0 * y, d)          # pixel units
    tris = []
    tris.append([P(-40, -40, 6.0), P(3 * W, -40, 6.0), P(-40, 3 * H, 6.0)])                       # covers the whole screen, far
    q = [P(8, 6, 3.0), P(30, 6, 3.0), P(30, 22, 3.0), P(8, 22, 3.0)]                             # quad split by a diagonal shared edge
    tris += [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    tris += [[P(30, 6, 3.0), P(50, 6, 3.0), P(30, 22, 3.0)], [P(50, 6, 3.0), P(50, 22, 3.0), P(30, 22, 3.0)]]       # shares the vertical edge x = 30
    tris += [[P(8, 22, 3.0), P(30, 22, 3.0), P(19, 34, 3.0)]]                                     # shares the horizontal edge y = 22
    c = P(40.5, 30.5, 2.5)                                                                        # fan around a vertex ON a pixel centre
    ring = [P(40.5 + 7 * np.cos(a), 30.5 + 7 * np.sin(a), 2.5) for a in np.linspace(0, 2 * np.pi, 7)[:-1]]
    tris += [[c, ring[i], ring[(i + 1) % 6]] for i in range(6)]
    for i in range(6):                                                                            # slivers thinner than a pixel
        x0, y0 = rs.uniform(5, W - 5), rs.uniform(3, H - 3)
        a = rs.uniform(0, np.pi)
        tris.append([P(x0, y0, 2.0), P(x0 + 25 * np.cos(a), y0 + 25 * np.sin(a), 2.0), P(x0 + 25 * np.cos(a) - 0.4 * np.sin(a), y0 + 25 * np.sin(a) + 0.4 * np.cos(a), 2.0)])
    z = P(20, 10, 1.5)
    tris += [[z, z, z], [P(5, 5, 1.5), P(15, 15, 1.5), P(25, 25, 1.5)]]                           # zero-area: a point, three collinear vertices
    tris += [[P(52, 8, 2.0), P(70, 20, 4.0), P(52, 32, 2.0)], [P(70, 8, 2.0), P(52, 20, 4.0), P(70, 32, 2.0)]]      # interpenetrating pair
    dup = [P(4, 26, 2.2), P(16, 26, 2.2), P(10, 38, 2.2)]
    tris += [dup, dup, dup]                                                                      # coplanar duplicates (colours differ)
    tris.append([P(34, 18, 0.2), P(46, 24, 0.2), P(38, 37, 0.02)])                                # across the near plane: the third vertex is behind it (d < near)
    tris.append([P(60, 30, 0.03), P(66, 31, 0.2), P(62, 38, 0.03)])                               # across it with ONE vertex in front
    tris.append([unproject(scene, H, W, 0, 0, -1.0), unproject(scene, H, W, 500, 0, -2.0), unproject(scene, H, W, 0, 500, -1.5)])     # wholly behind
    tris.append([P(W + 20, 5, 3.0), P(W + 60, 5, 3.0), P(W + 20, 30, 3.0)])                       # wholly off-screen
    for i in range(10):                                                                           # filler: random small and medium triangles
        x0, y0, r = rs.uniform(0, W), rs.uniform(0, H), rs.uniform(0.5, 9)
        tris.append([P(x0 + rs.uniform(-r, r), y0 + rs.uniform(-r, r), rs.uniform(1.5, 5)) for _ in range(3)])
    v = np.asarray(tris, np.float64).reshape(-1, 3)
    faces = np.arange(len(v), dtype=np.int32).reshape(-1, 3)
    nrm = np.tile(np.asarray([[0.0, 0.6, 0.8]]), (len(v), 1))
    rgb = rs.uniform(0.1, 1.0, size=(len(v), 3))
    return mesh(v, faces, rgb, normals=nrm, flags=SCENE_SPACE | VERTEX_RGB)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the clip of the end-to-end test, and visualize_body_obj's scene restated
PALETTE = dict(light_grey=(204, 204, 204), yellow_pale=(226, 215, 132), grey=(110, 110, 110), pink=(255, 182, 193))


def rodrigues(aa):
    aa = np.asarray(aa, np.float64)
    out = []
    for a in aa.reshape(-1, 3):
        th = np.linalg.norm(a)
        k = a / th if th > 0 else np.zeros(3)
        K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        out.append(np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K)
    return np.stack(out)


def e2e_clip(T=3):
    """ellipsoid body (V 6890, F 13776) drifting, a box turning beside it: everything float32, the object also as canonical + per-frame pose"""
    bv, bf = ellipsoid()
    body = np.stack([bv + np.array([0.05 * t, 0.01 * t, 0.03 * t], np.float32) for t in range(T)]).astype(np.float32)
    ov, of = box()
    aa = np.array([[0.2 + 0.1 * t, 0.3, -0.2 * t] for t in range(T)], np.float32)
    tr = np.array([[0.45, 0.15 + 0.02 * t, 0.1] for t in range(T)], np.float32)
    R = rodrigues(aa).astype(np.float32)
    obj = (np.einsum('tij,vj->tvi', R.astype(np.float64), ov.astype(np.float64)) + tr[:, None].astype(np.float64)).astype(np.float32)
    return dict(body=body, body_face=bf, obj_canon=ov, obj_face=of, aa=aa, tr=tr, R=R, obj=obj)


def clip_scene(body, body_face, obj, obj_face, past_len, obj_R=None, obj_t=None):
    """visualize_body_obj's scene: (scene dict, meshes in the product's order: ground, object, body)"""
    body = np.asarray(body, np.float32)
    T = body.shape[0]
    neg = -body
    lo, hi = neg.min(axis=(0, 1)), neg.max(axis=(0, 1))
    minx, maxx, minz, maxz = float(lo[0]), float(hi[0]), float(lo[2]), float(hi[2])
    scene = make_scene(((minx + maxx) / 2, float(lo[1]), (minz + maxz) / 2))
    col = lambda past, fut: np.stack([np.asarray(PALETTE[past if i <= past_len else fut], np.float32) / np.float32(255) for i in range(T)])
    gv, gn, gc, gf = ground_mesh(minx, maxx, minz, maxz)
    meshes = [mesh(gv, gf, gc, normals=gn, flags=SCENE_SPACE | VERTEX_RGB),
              mesh(obj, obj_face, col('grey', 'pink'), R=obj_R, t=obj_t),
              mesh(body, body_face, col('light_grey', 'yellow_pale'))]
    return scene, meshes


def tile_views(rgb):
    """[T,4,H,W,3] -> [T,3,H,4W]: views 0, 1, 3, 2 side by side, channels first"""
    return np.transpose(np.concatenate([rgb[:, 0], rgb[:, 1], rgb[:, 3], rgb[:, 2]], axis=2), (0, 3, 1, 2))
