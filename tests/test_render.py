"""Mesh rendering (interdiff_amd/render.py, csrc/render.hip, csrc/render.h) against the numpy oracle of tests/render_oracle.py.

The integer stage (coverage, depth key, colour) is exact: the GPU tests compare it bit for bit with the oracle's integer raster run on THE KERNEL'S OWN
setup records, no pixel excluded.  The floating setup stage is compared with the float64 setup under SETUP GATES derived here (not from what the code
gives):

  u = 2^-24 (fp32 unit roundoff), M = bound of every coordinate / offset magnitude of the scene, d = depth of the vertex along the view axis.
  X, Y   the fp32 chain carries a relative error of a few u in front of the rounding to the 1/16-pixel grid; at the guard band (2^15 units) that is
         < 0.01 unit, so the snapped values differ by at most ONE unit (a rint flip).
  Z      Z = ZONE - rint(ZONE near / d).  d comes from  s = (-p) - off  (1 rounding, <= u M),  q = s - cam_t  (1 rounding, <= u M),
         sin * q.y  (1 rounding, <= u sin M)  and one fmaf  (<= u d):  |dd| <= (cos + sin) 2 u M + u sin M + u d <= u (3.3 M + d) =: E_d
         (+ `extra`: the error of the INPUT coordinates where they are themselves computed, x (cos + sin)).
         near / d adds one division (relative u);  ZONE * . is exact;  the two rint contribute 1 together:
             |dZ| <= 1 + 1.01 ZONE (near / d) (u + E_d / d)
  colour <= 12 roundings on values <= 3 in front of * 4080: < 0.01 unit, so at most ONE unit (a rint flip).
  flags  identical; the scenes keep every vertex further than 1e-5 (>> E_d) from the near plane.
"""
import ctypes as C
import functools
import os
import re
import subprocess
import numpy as np
import pytest
import torch
from tests import render_oracle as ro
from tests.golden import make_golden_render as mg

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
U = 2.0 ** -24
NEAR = 0.05


def golden():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'render.npz'))


# ------------------------------------------------------------------------------------------------------------------------------------------
# gates
def z_bound(z_ref, M, extra=0.0):
    q = 1.0 - z_ref.astype(np.float64) / ro.ZONE
    d = NEAR / np.maximum(q, 1e-12)
    e_d = U * (3.3 * M + d) + 1.37 * extra
    return 1.0 + 1.01 * ro.ZONE * q * (U + e_d / d)


def check_setup_gates(got, ref, M, extra=0.0, what=''):
    """got, ref int32 [..., 20] setup records -> worst deviations (x/y units, z as a fraction of its bound, colour units)"""
    got, ref = got.reshape(-1, ro.REC).astype(np.int64), ref.reshape(-1, ro.REC).astype(np.int64)
    assert np.array_equal(got[:, 18], ref[:, 18]), what + ': slot layout / invalid flags'
    assert np.array_equal(got[:, 19], ref[:, 19]) and not got[got[:, 18] == 0].any(), what + ': empty records are all zero'
    v = got[:, 18] == 1
    g, r = got[v, :18].reshape(-1, 3, 6), ref[v, :18].reshape(-1, 3, 6)
    dxy = np.abs(g[..., :2] - r[..., :2]).max() if v.any() else 0
    dz = (np.abs(g[..., 2] - r[..., 2]) / z_bound(r[..., 2], M, extra)).max() if v.any() else 0.0
    dc = np.abs(g[..., 3:] - r[..., 3:]).max() if v.any() else 0
    print('%s: setup deviation  x/y %d unit  z %.4f of its bound (%d units at most)  colour %d unit' % (
        what, dxy, dz, np.abs(g[..., 2] - r[..., 2]).max() if v.any() else 0, dc))
    assert dxy <= 1 and dz <= 1.0 and dc <= 1, (what, dxy, dz, dc)
    return dxy, dz, dc


def cover_exact(rec, i, j):
    """the per-pixel function in python integers (unbounded): the overflow check of the int64 restatements"""
    r = [int(x) for x in rec]
    if r[18] != 1:
        return [0, 0, 0, 0, 0]
    v = [r[6 * k:6 * k + 6] for k in range(3)]
    E = lambda a, b, px, py: (b[0] - a[0]) * (py - a[1]) - (b[1] - a[1]) * (px - a[0])
    A = E(v[0], v[1], v[2][0], v[2][1])
    if A == 0:
        return [0, 0, 0, 0, 0]
    if A < 0:
        v[1], v[2], A = v[2], v[1], -A
    px, py = 16 * i + 8, 16 * j + 8
    w, ok = [], True
    for a, b in ((1, 2), (2, 0), (0, 1)):
        e = E(v[a], v[b], px, py)
        dx, dy = v[b][0] - v[a][0], v[b][1] - v[a][1]
        ok &= e >= (0 if (dy < 0 or (dy == 0 and dx > 0)) else 1)
        w.append(e)
    if not ok:
        return [0, 0, 0, 0, 0]
    assert max(abs(x) for x in w) < 2 ** 34 and A < 2 ** 34 and sum(w) == A
    num = sum(w[k] * v[k][2] for k in range(3))
    assert num < 2 ** 62
    return [1, num // A] + [(2 * sum(w[k] * v[k][3 + c] for k in range(3)) + 16 * A) // (32 * A) for c in range(3)]


def tri_rec(v0, v1, v2, z=(100, 100, 100), c=None):
    rec = np.zeros(ro.REC, np.int32)
    for i, v in enumerate((v0, v1, v2)):
        rec[6 * i:6 * i + 2] = v
        rec[6 * i + 2] = z[i]
        rec[6 * i + 3:6 * i + 6] = (1600, 800 * i, 4080) if c is None else c
    rec[18] = 1
    return rec


# ------------------------------------------------------------------------------------------------------------------------------------------
# CPU: the oracle itself
def test_oracle_shared_edges_cover_every_pixel_exactly_once():
    H = W = 24
    px = lambda x, y: (int(round(16 * x)), int(round(16 * y)))
    cases = {
        'horizontal': [(px(2, 10.5), px(20, 10.5), px(9, 3)), (px(2, 10.5), px(11, 21), px(20, 10.5))],
        'vertical': [(px(10.5, 2), px(10.5, 20), px(3, 9)), (px(10.5, 2), px(21, 11), px(10.5, 20))],
        'diagonal': [(px(2, 2), px(20.5, 2), px(20.5, 20.5)), (px(2, 2), px(20.5, 20.5), px(2, 20.5))],
        'diagonal_through_centres': [(px(2.5, 2.5), px(20.5, 2.5), px(20.5, 20.5)), (px(2.5, 2.5), px(20.5, 20.5), px(2.5, 20.5))],
    }
    c = px(10.5, 12.5)                                      # a fan around a vertex that sits exactly on a pixel centre
    ring = [px(10.5 + 8 * np.cos(a), 12.5 + 8 * np.sin(a)) for a in np.linspace(0, 2 * np.pi, 8)[:-1]]
    cases['fan'] = [(c, ring[i], ring[(i + 1) % 7]) for i in range(7)]
    for name, tris in cases.items():
        for flip in (False, True):                          # either orientation of every triangle
            recs = np.stack([tri_rec(*(t[::-1] if flip else t)) for t in tris])
            ids, _, _, cnt = ro.raster(recs, H, W, count=True)
            assert cnt.max() == 1, (name, flip)
            assert ((ids >= 0) == (cnt == 1)).all()
            # every pixel centre strictly inside one of the triangles is covered, and so are the centres ON the shared edges (below)
            J, I = np.mgrid[0:H, 0:W]
            inside = np.zeros((H, W), bool)
            for t in tris:
                x, y = np.array([p[0] for p in t], np.int64), np.array([p[1] for p in t], np.int64)
                e = [ro._edge(x[a], y[a], x[b], y[b], 16 * I + 8, 16 * J + 8) for a, b in ((0, 1), (1, 2), (2, 0))]
                inside |= ((e[0] > 0) & (e[1] > 0) & (e[2] > 0)) | ((e[0] < 0) & (e[1] < 0) & (e[2] < 0))
            assert (cnt[inside] == 1).all(), name           # strictly interior centres of any triangle are covered
            if name == 'horizontal':
                assert (cnt[10, 3:19] == 1).all()           # centres ON the shared edge y = 10.5
            if name == 'vertical':
                assert (cnt[3:19, 10] == 1).all()
            if name == 'fan':
                assert cnt[12, 10] == 1                     # the shared vertex's own pixel: exactly one of the seven
            if name == 'diagonal_through_centres':
                assert all(cnt[k, k] == 1 for k in range(3, 20))      # centres ON the shared diagonal


def test_oracle_known_counts_zero_area_and_coplanar_duplicates():
    # right triangle with legs of 8 pixels on pixel boundaries: centres (i + 1/2, j + 1/2) with i + j + 1 < 8 strictly inside (28), the 8 centres on the
    # hypotenuse (i + j + 1 = 8) lie exactly on it: that edge runs down-left -> not top, not left -> excluded
    rec = tri_rec((0, 0), (128, 0), (0, 128))
    ids, _, _ = ro.raster(rec[None], 16, 16)
    assert (ids >= 0).sum() == 28
    ids, _, _ = ro.raster(tri_rec((0, 128), (128, 0), (128, 128))[None], 16, 16)          # its complement in the square owns the diagonal
    assert (ids >= 0).sum() == 64 - 28
    for z in (tri_rec((40, 40), (40, 40), (40, 40)), tri_rec((8, 8), (72, 72), (136, 136)), tri_rec((8, 8), (8, 8), (136, 136))):
        assert (ro.raster(z[None], 16, 16)[0] == -1).all()
    a = tri_rec((0, 0), (200, 0), (0, 200), c=(4080, 0, 0))
    b = tri_rec((0, 0), (200, 0), (0, 200), c=(0, 4080, 0))
    ids, depth, rgb = ro.raster(np.stack([b, a, b]), 16, 16)
    assert set(np.unique(ids)) == {-1, 0} and (rgb[ids == 0] == (0, 255, 0)).all() and (depth[ids == 0] == 100).all()
    ids, _, rgb = ro.raster(np.stack([b, tri_rec((0, 0), (200, 0), (0, 200), z=(99, 99, 99), c=(4080, 0, 0))]), 16, 16)
    assert set(np.unique(ids)) == {-1, 1} and (rgb[ids == 1] == (255, 0, 0)).all()                       # nearer beats the lower slot
    empty = np.zeros((1, ro.REC), np.int32)
    assert (ro.raster(empty, 8, 8)[0] == -1).all()


# ------------------------------------------------------------------------------------------------------------------------------------------
# CPU: the host twins
def scene_struct(scene):
    from interdiff_amd import _lib
    sc = _lib.RenderScene()
    sc.off[:] = scene['off'].tolist()
    sc.cam_t[:] = scene['cam_t'].tolist()
    sc.cam_cos, sc.cam_sin, sc.znear, sc.focal = float(scene['cam_cos']), float(scene['cam_sin']), float(scene['znear']), float(scene['focal'])
    sc.light[:] = scene['light'].tolist()
    sc.light_gain, sc.ambient = float(scene['light_gain']), float(scene['ambient'])
    sc.bg[:] = scene['bg'].tolist()
    return sc


def test_host_vertex_function_matches_the_float64_setup(lib):
    rs = np.random.RandomState(11)
    H, W = 96, 128
    scene = ro.make_scene(off=(0.3, -0.7, 0.2))
    n = 2500
    worst = [0, 0.0, 0, 0]
    for view, scene_space in ((0, True), (0, False), (1, False), (2, False), (3, False)):
        # points seen at random sub-pixel positions inside the guard band, at depths from far away down to both sides of the near plane
        X, Y = rs.uniform(-ro.GUARD, ro.GUARD, n), rs.uniform(-ro.GUARD, ro.GUARD, n)
        d = np.exp(rs.uniform(np.log(NEAR), np.log(30.0), n))
        d[:200] = NEAR * (1 + rs.choice([-1, 1], 200) * np.exp(rs.uniform(np.log(1e-3), np.log(0.5), 200)))      # just in front of / behind the plane
        d[200:260] = -rs.uniform(0.1, 3, 60)                                                                    # behind the camera
        p = ro.unproject(scene, H, W, X, Y, d)
        p[300:800] = rs.uniform(-2, 2, (500, 3))                                                                # and plain points around the origin
        if not scene_space:                                 # undo the scene transform: s = turn^view(-p - off)
            for _ in range((4 - view) % 4):
                p = np.stack([p[:, 2], p[:, 1], -p[:, 0]], axis=1)
            p = -(p + scene['off'].astype(np.float64))
        pos = np.ascontiguousarray(p, np.float32)
        nrm = rs.standard_normal((n, 3))
        nrm = np.ascontiguousarray(nrm / np.linalg.norm(nrm, axis=1, keepdims=True), np.float32)
        rgb = np.ascontiguousarray(rs.uniform(0, 1, (n, 3)), np.float32)
        out_f, out_i = np.zeros((n, 6), np.float32), np.zeros((n, 7), np.int32)
        sc = scene_struct(scene)
        assert lib.interdiff_debug_render_setup_vertex(C.byref(sc), view, int(scene_space), H, W, pos.ctypes.data, nrm.ctypes.data, rgb.ctypes.data,
                                                       out_f.ctypes.data, out_i.ctypes.data, n) == 0
        v = ro.vertex_stage(scene, view, scene_space, pos, nrm, rgb)
        front = v[:, 2] >= NEAR
        sure = np.abs(v[:, 2] - NEAR) > 1e-5
        assert sure.sum() > n - 5 and np.array_equal(out_i[sure, 0] == 1, front[sure])
        assert (out_i[out_i[:, 0] == 0] == 0).all()
        M = max(np.abs(pos).max(), 2.5) + np.abs(scene['off']).max() + 2.5
        assert np.abs(out_f[:, :3] - v[:, :3]).max() <= 4 * U * M * 3.3 and np.abs(out_f[:, 3:] - v[:, 3:]).max() <= 12 * 3 * U
        k = front & sure & (out_i[:, 0] == 1)
        Xr, Yr, Zr, Cr = ro.project(scene, H, W, v[k])
        band = (np.abs(Xr) < ro.GUARD) & (np.abs(Yr) < ro.GUARD)
        assert band.sum() > 1000
        g = out_i[k][band].astype(np.int64)
        dxy = max(np.abs(g[:, 1] - Xr[band]).max(), np.abs(g[:, 2] - Yr[band]).max())
        dz = (np.abs(g[:, 3] - Zr[band]) / z_bound(Zr[band], M)).max()
        dc = np.abs(g[:, 4:] - Cr[band]).max()
        worst = [max(worst[0], dxy), max(worst[1], dz), max(worst[2], dc), max(worst[3], np.abs(g[:, 3] - Zr[band]).max())]
        assert dxy <= 1 and dz <= 1.0 and dc <= 1, (view, scene_space, dxy, dz, dc)
    print('host vertex twin vs float64: x/y %d unit, z %.4f of its bound (%d units at most), colour %d unit' % (worst[0], worst[1], worst[3], worst[2]))


def test_host_pixel_function_is_the_integer_oracle_bit_for_bit(lib):
    rs = np.random.RandomState(3)
    n = 3000
    rec = np.zeros((n, ro.REC), np.int32)
    xy = rs.randint(-600, 3000, (n, 3, 2))
    xy[:600] = rs.choice([-ro.GUARD, ro.GUARD, ro.GUARD - 1, 0, 16 * 1024 + 8], (600, 3, 2))                # the guard band's extremes: the overflow check
    xy[600:900] = rs.randint(-ro.GUARD, ro.GUARD + 1, (300, 3, 2))
    z = rs.randint(0, ro.ZONE + 1, (n, 3))
    z[:300] = rs.choice([0, ro.ZONE], (300, 3))
    col = rs.randint(0, ro.CMAX + 1, (n, 3, 3))
    col[:300] = rs.choice([0, ro.CMAX], (300, 3, 3))
    for i in range(3):
        rec[:, 6 * i:6 * i + 2], rec[:, 6 * i + 2], rec[:, 6 * i + 3:6 * i + 6] = xy[:, i], z[:, i], col[:, i]
    rec[:, 18] = 1
    rec[-20:, 18] = 0
    rec[-40:-20, 6:8] = rec[-40:-20, 0:2]                                                                       # zero area
    ij = rs.randint(0, 200, (n, 2)).astype(np.int32)
    ij[:900] = rs.randint(0, 2048, (900, 2))
    inside = rs.rand(n) < 0.7                               # most samples at a pixel near the triangle's centroid, so that many are covered
    cen = (xy.mean(1) / 16).astype(np.int64)
    ij[inside] = np.clip(cen[inside] + rs.randint(-1, 2, (inside.sum(), 2)), 0, 2047)
    out = np.zeros((n, 5), np.int32)
    rec, ij = np.ascontiguousarray(rec), np.ascontiguousarray(ij, np.int32)
    assert lib.interdiff_debug_render_pixel(rec.ctypes.data, ij.ctypes.data, out.ctypes.data, n) == 0
    ref = np.zeros((n, 5), np.int64)
    for k in range(n):
        cov, dep, rgb = ro.cover(rec[k], ij[k, 0], ij[k, 1])
        ref[k] = [int(cov), int(dep), *[int(x) for x in rgb]] if cov else 0
        if k < 1000 or k >= n - 40:
            assert list(ref[k]) == cover_exact(rec[k], int(ij[k, 0]), int(ij[k, 1])), k                     # the int64 oracle against unbounded integers
    assert ref[:, 0].sum() > 300 and ref[:900, 0].sum() > 50
    assert np.array_equal(out, ref)


def test_fixture_conditions_and_oracle_regression():
    z = golden()
    scene, meshes = mg.adversarial()
    adv = ro.render(scene, meshes, 1, mg.ADV['views'], mg.ADV['H'], mg.ADV['W'])
    assert adv[4] == 0 and np.array_equal(adv[0][0], z['adv_id']) and np.array_equal(adv[0][0, 0], adv[0][0, 1])
    rec = adv[3][0, 0]
    assert (rec[:, 18] == 0).sum() > 39 and rec[2 * 25 + 1, 18] == 1        # one triangle fills its second slot (two vertices in front of the near plane)
    c, scene, meshes = mg.end_to_end()
    o64 = e2e_oracle()
    assert np.array_equal(o64[0], z['e2e_id']) and np.array_equal(o64[2], z['e2e_rgb'])
    share = mg.e2e_share32(o64, scene, meshes)
    print('end-to-end scene, float32 setup vs float64 setup: differing pixel share per image', share, '(cap / 4 = %g)' % (mg.CAP / 4))
    assert share.max() <= mg.CAP / 4 and np.array_equal(share, z['e2e_share32'])


def test_render_symbols_are_declared_bound_and_exported(lib):
    from interdiff_amd import _lib
    names = ['interdiff_render_frames', 'interdiff_render_frames_workspace_bytes', 'interdiff_debug_render_setup_vertex', 'interdiff_debug_render_pixel']
    hdr = open(os.path.join(ROOT, 'include', 'interdiff_hip.h')).read()
    nm = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for n in names:
        assert re.search(r'\b%s\s*\(' % n, hdr) and n in _lib.exported_symbols() and re.search(r' T %s\b' % n, nm), n
    assert lib.interdiff_abi_version() == _lib.ABI_VERSION == 17
    for k, v in dict(SUBPIX=ro.SUB, GUARD=ro.GUARD, ZONE=ro.ZONE, REC_INTS=ro.REC, TILE=ro.TILE).items():
        assert getattr(_lib, 'RENDER_' + k) == v and re.search(r'#define IDF_RENDER_%s\s+(?:\(1 << 28\)|%d\b)' % (k, v), hdr), k
    assert C.sizeof(_lib.RenderScene) == 4 * 25 and C.sizeof(_lib.RenderMesh) == 6 * 8 + 16
    assert lib.interdiff_render_frames_workspace_bytes(1, 100, 0, 8) == 0 and lib.interdiff_render_frames_workspace_bytes(1, 100, 8, 4096) == 0
    one, four = lib.interdiff_render_frames_workspace_bytes(1, 100, 64, 64), lib.interdiff_render_frames_workspace_bytes(4, 100, 64, 64)
    assert 0 < one < four <= 4 * one


# ------------------------------------------------------------------------------------------------------------------------------------------
# GPU
@functools.lru_cache(maxsize=None)
def e2e_oracle():
    c, scene, meshes = mg.end_to_end()
    return ro.render(scene, meshes, mg.E2E['T'], mg.E2E['views'], mg.E2E['H'], mg.E2E['W'])


def gpu_meshes(meshes):
    from interdiff_amd import render
    return [render.Mesh(m['verts'], m['normals'], m['faces'], m['rgb'], R=m['R'], t=m['t'], scene_space=bool(m['flags'] & ro.SCENE_SPACE),
                        vertex_rgb=bool(m['flags'] & ro.VERTEX_RGB)) for m in meshes]


def gpu_render(scene, meshes, N, views, H, W, workspace_bytes=None):
    from interdiff_amd import render
    out = render.render_frames(scene_struct(scene), gpu_meshes(meshes), N, views, H, W, want_id=True, want_depth=True, want_setup=True,
                               workspace_bytes=workspace_bytes)
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}


def assert_raster_exact(out, scene, what):
    """id, depth and RGB of every image equal the integer oracle run on the kernel's own setup records, no pixel excluded"""
    N, views, H, W = out['id'].shape
    bg = ro.bg_bytes(scene)
    for n in range(N):
        for v in range(views):
            ids, depth, rgb = ro.raster(out['setup'][n, v], H, W, bg)
            assert np.array_equal(out['id'][n, v], ids), (what, n, v, 'id', int((out['id'][n, v] != ids).sum()))
            assert np.array_equal(out['depth'][n, v], depth), (what, n, v, 'depth')
            assert np.array_equal(out['rgb'][n, v], rgb), (what, n, v, 'rgb')


@functools.lru_cache(maxsize=None)
def adversarial_gpu():
    scene, meshes = mg.adversarial()
    return scene, meshes, gpu_render(scene, meshes, 1, mg.ADV['views'], mg.ADV['H'], mg.ADV['W'])


@pytest.mark.gpu
def test_raster_stage_is_bit_exact_on_the_adversarial_scene():
    scene, meshes, out = adversarial_gpu()
    assert out['dropped'] == 0 and out['rgb'].shape == (1, 2, 40, 72, 3) and len(np.unique(out['id'])) > 25
    assert_raster_exact(out, scene, 'adversarial')


@pytest.mark.gpu
def test_setup_stage_against_the_float64_setup():
    scene, meshes, out = adversarial_gpu()
    ref, dropped = ro.setup_records(scene, meshes, 1, mg.ADV['views'], mg.ADV['H'], mg.ADV['W'])
    assert dropped == 0
    M = np.abs(meshes[0]['verts']).max() + 2.5
    check_setup_gates(out['setup'], ref, M, what='adversarial scene')


def capacity_scene(H=64, W=64):
    """4096 one-pixel triangles inside the single tile (1, 1) -- 16 on each of its 256 pixel centres, at 16 depths -- and one triangle covering the
    whole screen behind them"""
    scene = ro.make_scene(bg=(0, 0, 0))
    rs = np.random.RandomState(5)
    P = lambda x, y, d: ro.unproject(scene, H, W, 16.0 * x, 16.0 * y, d)
    tris = []
    for k in range(16):
        for j in range(16, 32):
            for i in range(16, 32):
                d = 2.0 + 0.05 * ((k * 7 + i + 3 * j) % 16)
                tris.append([P(i + 0.1, j + 0.2, d), P(i + 0.9, j + 0.2, d), P(i + 0.5, j + 0.9, d)])
    tris.append([P(-30, -30, 6.0), P(3 * W, -30, 6.0), P(-30, 3 * H, 6.0)])
    v = np.asarray(tris).reshape(-1, 3)
    return scene, [ro.mesh(v, np.arange(len(v), dtype=np.int32).reshape(-1, 3), rs.uniform(0.1, 1, (len(v), 3)), normals=np.tile([[0, 0.6, 0.8]], (len(v), 1)),
                           flags=ro.SCENE_SPACE | ro.VERTEX_RGB)]


@pytest.mark.gpu
def test_binning_has_no_capacity():
    scene, meshes = capacity_scene()
    out = gpu_render(scene, meshes, 1, 1, 64, 64)
    assert_raster_exact(out, scene, 'capacity')
    ids = out['id'][0, 0]
    assert (ids >= 0).all() and (ids[16:32, 16:32] < 2 * 4096).all() and (np.delete(ids, np.s_[16:32], 0) == 2 * 4096).all()
    # every pixel of the tile shows one of the triangles of the NEAREST layer on it (d = 2.0: (7 k + i + 3 j) % 16 == 0)
    tri = ids[16:32, 16:32] // 2
    k, j, i = tri // 256, 16 + (tri % 256) // 16, 16 + tri % 16
    J, I = np.mgrid[16:32, 16:32]
    assert np.array_equal(i, I) and np.array_equal(j, J) and ((7 * k + i + 3 * j) % 16 == 0).all()


def large_list_scene(H=80, W=80, T=2):
    """25 tiles: a scene-space triangle covering the whole screen and one covering about half of it, two MOVING triangles some 80 pixels across (another
    picture in every frame and view) and 300 small moving triangles in front -- every image has slots on more than 16 tiles (the large list) beside binned ones"""
    scene = ro.make_scene(bg=(0.1, 0.1, 0.1))
    rs = np.random.RandomState(21)
    P = lambda x, y, d: ro.unproject(scene, H, W, 16.0 * x, 16.0 * y, d)
    sv = np.asarray([P(-40, -40, 9.0), P(3 * W, -40, 9.0), P(-40, 3 * H, 9.0), P(2, 3, 7.0), P(78, 5, 7.5), P(4, 77, 8.0)])
    static = ro.mesh(sv, [[0, 1, 2], [3, 4, 5]], rs.uniform(0.2, 1, (6, 3)), normals=np.tile([[0, 0.6, 0.8]], (6, 1)), flags=ro.SCENE_SPACE | ro.VERTEX_RGB)
    big = np.array([[-2.0, 0.1, -1.0], [2.0, 0.2, -0.5], [0.0, 2.6, 0.3], [-1.0, 0.1, -2.0], [-0.5, 0.2, 2.0], [0.3, 2.6, 0.0]])
    cen = rs.uniform([-0.8, 0.0, -0.8], [0.8, 1.6, 0.8], (300, 1, 3))
    small = (cen + rs.uniform(-1, 1, (300, 3, 3)) * rs.uniform(0.03, 0.2, (300, 1, 1))).reshape(-1, 3)
    s0 = np.concatenate([big, small])
    frames = np.stack([-(s0 + np.array([0.15 * t, 0.05 * t, -0.1 * t])) for t in range(T)])             # moving meshes are negated by the scene transform
    nrm = rs.standard_normal((len(s0), 3))
    moving = ro.mesh(frames, np.arange(len(s0), dtype=np.int32).reshape(-1, 3), rs.uniform(0.1, 1, (len(s0), 3)),
                     normals=np.tile((nrm / np.linalg.norm(nrm, axis=1, keepdims=True))[None], (T, 1, 1)), flags=ro.VERTEX_RGB)
    return scene, [static, moving]


@pytest.mark.gpu
def test_large_list_slots_on_more_than_sixteen_tiles_chunked_and_not(lib):
    H, W, T, views = 80, 80, 2, 2
    scene, meshes = large_list_scene(H, W, T)
    out = gpu_render(scene, meshes, T, views, H, W)
    assert out['dropped'] == 0
    pics, moving_large = set(), 0
    for n in range(T):
        for v in range(views):
            i0, i1, j0, j1, ok = ro.pixel_box(out['setup'][n, v], H, W)
            tiles = np.where(ok, (i1 // ro.TILE - i0 // ro.TILE + 1) * (j1 // ro.TILE - j0 // ro.TILE + 1), 0)
            assert (tiles > 16).sum() >= 2 and ((tiles > 0) & (tiles <= 16)).sum() >= 100, (n, v, (tiles > 16).sum())      # both kinds of slot in every image
            large = np.nonzero(tiles > 16)[0]
            moving_large += int((large >= 4).sum())         # slots 0..3 are the scene-space mesh's
            assert np.isin(out['id'][n, v], large).mean() > 0.3 and len(np.unique(out['id'][n, v])) > 40                 # and both kinds win pixels
            pics.add(out['id'][n, v].tobytes())
    assert len(pics) == T * views and moving_large >= 4     # four different pictures; the large list's length differs between images
    assert_raster_exact(out, scene, 'large list')
    Ft = sum(len(m['faces']) for m in meshes)
    one = lib.interdiff_render_frames_workspace_bytes(1, Ft, H, W)
    assert lib.interdiff_render_frames_workspace_bytes(2, Ft, H, W) > one
    chunked = gpu_render(scene, meshes, T, views, H, W, workspace_bytes=one)                                             # one image per chunk
    assert all(np.array_equal(out[k], chunked[k]) for k in ('rgb', 'id', 'depth', 'setup'))
    ref, dropped = ro.setup_records(scene, meshes, T, views, H, W)
    check_setup_gates(out['setup'], ref, np.abs(meshes[1]['verts']).max() + np.abs(meshes[0]['verts']).max() + 2.5, what='large-list scene')


@pytest.mark.gpu
def test_end_to_end_video_against_the_float64_oracle():
    from interdiff_amd import render
    c, scene, meshes = mg.end_to_end()
    o64 = e2e_oracle()
    T, views, H, W = mg.E2E['T'], mg.E2E['views'], mg.E2E['H'], mg.E2E['W']
    video = render.visualize_body_obj(c['body'], c['body_face'], c['obj'], c['obj_face'], past_len=mg.E2E['past_len'], h=H, w=W)
    assert video.dtype == np.uint8 and video.shape == (T, 3, H, 4 * W)
    ref = ro.tile_views(o64[2])
    ids = np.concatenate([o64[0][:, 0], o64[0][:, 1], o64[0][:, 3], o64[0][:, 2]], axis=2)               # the same tiling of the oracle's id images
    worst = 0.0
    for t in range(T):
        for s, view in enumerate((0, 1, 3, 2)):
            a, b = video[t, :, :, s * W:(s + 1) * W], ref[t, :, :, s * W:(s + 1) * W]
            diff = (a != b).any(0)
            worst = max(worst, diff.mean())
            assert diff.mean() <= mg.CAP, (t, view, diff.mean())
            assert not (diff & ~ro.near_id_boundary(ids[t, :, s * W:(s + 1) * W])).any(), (t, view, 'a differing pixel away from every id boundary')
    print('end to end: largest share of differing pixels in an image %.5f (cap %g)' % (worst, mg.CAP))
    # the colour switch at i <= past_len is inside the clip: the body's colour differs between frames 1 and 2, not between 0 and 1
    body = o64[0][:, 0] >= 2 * (24 + 12)
    both = body[0] & body[1] & body[2]
    assert both.sum() > 100
    v0 = video[:, :, :, :W].transpose(0, 2, 3, 1)
    assert (v0[1][both].astype(int) - v0[2][both].astype(int)).any(axis=1).mean() > 0.9
    one = render.visualize_body_obj(c['body'], c['body_face'], c['obj'], c['obj_face'], past_len=mg.E2E['past_len'], h=H, w=W, multi_angle=False)
    assert one.shape == (T, 3, H, W) and np.array_equal(one, video[:, :, :, :W])


@pytest.mark.gpu
def test_overdraw_stress_random_face_soup():
    from interdiff_amd import synthetic as syn
    m = syn.smplh_model(seed=7)
    v = np.asarray(m['v_template'], np.float32)
    neg = -v
    scene = ro.make_scene(off=((neg[:, 0].min() + neg[:, 0].max()) / 2, neg[:, 1].min(), (neg[:, 2].min() + neg[:, 2].max()) / 2))
    faces = np.asarray(m['faces'], np.int32)
    assert faces.shape == (13776, 3)
    meshes = [ro.mesh(v, faces, np.array([[0.9, 0.8, 0.5]]))]
    out = gpu_render(scene, meshes, 1, 1, 48, 64)
    assert out['dropped'] == 0 and (out['id'] >= 0).mean() > 0.05
    assert_raster_exact(out, scene, 'soup')


@pytest.mark.gpu
def test_determinism_permutation_and_chunking(lib):
    scene, meshes, out = adversarial_gpu()
    again = gpu_render(scene, meshes, 1, mg.ADV['views'], mg.ADV['H'], mg.ADV['W'])
    assert all(np.array_equal(out[k], again[k]) for k in ('rgb', 'id', 'depth', 'setup'))
    # a scene without coplanar duplicates: the same RGB after a permutation of its faces
    c, e2e_scene, e2e_meshes = mg.end_to_end()
    T, H, W = 2, 48, 64
    sub = [dict(m, verts=m['verts'][:T] if m['verts'].shape[0] > 1 else m['verts'], normals=m['normals'][:T] if m['normals'].shape[0] > 1 else m['normals'],
                rgb=m['rgb'] if m['flags'] & ro.VERTEX_RGB else m['rgb'][:T]) for m in e2e_meshes]
    base = gpu_render(e2e_scene, sub, T, 2, H, W)
    perm = [dict(m, faces=np.ascontiguousarray(m['faces'][np.random.RandomState(i).permutation(len(m['faces']))])) for i, m in enumerate(sub)]
    assert np.array_equal(gpu_render(e2e_scene, perm, T, 2, H, W)['rgb'], base['rgb'])
    # a workspace that holds ONE image: four chunks, the bits of the unchunked call
    Ft = sum(len(m['faces']) for m in sub)
    one = lib.interdiff_render_frames_workspace_bytes(1, Ft, H, W)
    assert lib.interdiff_render_frames_workspace_bytes(2, Ft, H, W) > one
    chunked = gpu_render(e2e_scene, sub, T, 2, H, W, workspace_bytes=one)
    assert all(np.array_equal(base[k], chunked[k]) for k in ('rgb', 'id', 'depth', 'setup'))


@pytest.mark.gpu
def test_object_posed_in_the_kernel():
    c = ro.e2e_clip(mg.E2E['T'])
    T, H, W = mg.E2E['T'], mg.E2E['H'], mg.E2E['W']
    scene, posed = ro.clip_scene(c['body'], c['body_face'], c['obj'], c['obj_face'], 1)
    _, inkernel = ro.clip_scene(c['body'], c['body_face'], c['obj_canon'], c['obj_face'], 1, obj_R=c['R'], obj_t=c['tr'])
    # host side: normals of the posed mesh = the canonical normals turned (float64), so both calls shade the same surface
    n0 = ro.vertex_normals(c['obj_canon'], c['obj_face'])
    posed[1] = ro.mesh(c['obj'], c['obj_face'], posed[1]['rgb'], normals=np.einsum('tij,vj->tvi', c['R'].astype(np.float64), n0))
    a = gpu_render(scene, [posed[1]], T, 4, H, W)
    b = gpu_render(scene, [inkernel[1]], T, 4, H, W)
    assert (a['setup'][..., 18] == 1).sum() >= 12 * 12
    M = np.abs(c['obj']).max() + np.abs(scene['off']).max() + 2.5
    check_setup_gates(b['setup'], a['setup'], M, extra=7 * U * M, what='object posed in the kernel vs on the host')
    ref, _ = ro.setup_records(scene, [inkernel[1]], T, 4, H, W)
    check_setup_gates(b['setup'], ref, M, extra=7 * U * M, what='object posed in the kernel vs float64 oracle')
    assert_raster_exact(b, scene, 'posed in kernel')


def raw_call(lib, scene, gm, N, views, H, W, rgb, ws, ws_bytes, mesh_edit=None, dropped=None):
    from interdiff_amd import _lib
    structs = [m.struct() for m in gm]
    if mesh_edit:
        mesh_edit(structs)
    arr = (_lib.RenderMesh * len(structs))(*structs)
    sc = scene_struct(scene) if scene is not None else None
    rc = lib.interdiff_render_frames(C.byref(sc) if sc is not None else None, arr, len(structs), N, views, H, W, rgb.data_ptr() if rgb is not None else None,
                                     None, None, None, C.byref(dropped) if dropped is not None else None, None, ws.data_ptr() if ws is not None else None,
                                     ws_bytes, _lib.stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.gpu
def test_error_codes_and_the_guard_band(lib):
    INVAL, NOMEM = -22, -12
    scene, meshes = mg.adversarial()
    H, W = mg.ADV['H'], mg.ADV['W']
    gm = gpu_meshes(meshes)
    F = len(meshes[0]['faces'])
    nbytes = lib.interdiff_render_frames_workspace_bytes(1, F, H, W)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device='cuda')
    rgb = torch.full((1, 1, H, W, 3), 7, dtype=torch.uint8, device='cuda')
    call = lambda **kw: raw_call(lib, kw.pop('scene', scene), gm, kw.pop('N', 1), kw.pop('views', 1), kw.pop('H', H), kw.pop('W', W), kw.pop('rgb', rgb),
                                 kw.pop('ws', ws), kw.pop('ws_bytes', nbytes), **kw)

    def edit(field, value):
        def f(structs):
            setattr(structs[0], field, value)
        return f
    bad_faces = torch.as_tensor(meshes[0]['faces']).cuda().clone()
    bad_faces[5, 1] = len(meshes[0]['verts'][0])
    neg_faces = torch.as_tensor(meshes[0]['faces']).cuda().clone()
    neg_faces[0, 0] = -1
    cases = dict(null_scene=(dict(scene=None), INVAL), null_rgb=(dict(rgb=None), INVAL), null_ws=(dict(ws=None), INVAL),
                 null_verts=(dict(mesh_edit=edit('verts', None)), INVAL), misaligned_verts=(dict(mesh_edit=edit('verts', gm[0].verts.data_ptr() + 2)), INVAL),
                 misaligned_faces=(dict(mesh_edit=edit('faces', gm[0].faces.data_ptr() + 1)), INVAL),
                 rotation_without_translation=(dict(mesh_edit=edit('R', gm[0].verts.data_ptr())), INVAL),
                 h_zero=(dict(H=0), INVAL), w_zero=(dict(W=0), INVAL), w_beyond_the_guard_band=(dict(W=2049), INVAL), h_beyond=(dict(H=4096), INVAL),
                 no_frames=(dict(N=0), INVAL), five_views=(dict(views=5), INVAL), frames_mismatch=(dict(mesh_edit=edit('frames', 3)), INVAL),
                 no_faces=(dict(mesh_edit=edit('F', 0)), INVAL), face_index_too_large=(dict(mesh_edit=edit('faces', bad_faces.data_ptr())), INVAL),
                 face_index_negative=(dict(mesh_edit=edit('faces', neg_faces.data_ptr())), INVAL),
                 workspace_too_small=(dict(ws_bytes=nbytes - 256), NOMEM), no_workspace_bytes=(dict(ws_bytes=0), NOMEM))
    for name, (kw, want) in cases.items():
        assert call(**kw) == want, name
        assert (rgb == 7).all(), name + ': wrote to the output'
    assert call() == 0 and not (rgb == 7).all()
    # guard band: one triangle reaches far below the screen -- counted, not clamped; the others are drawn
    P = lambda x, y, d: ro.unproject(scene, H, W, 16.0 * x, 16.0 * y, d)
    v = np.concatenate([meshes[0]['verts'][0], [P(10, 10, 3.0), P(30, 10, 3.0), P(20, 5000, 3.0)]]).astype(np.float32)
    m2 = ro.mesh(v, np.concatenate([meshes[0]['faces'], [[len(v) - 3, len(v) - 2, len(v) - 1]]]), np.concatenate([meshes[0]['rgb'], np.ones((3, 3))]),
                 normals=np.concatenate([meshes[0]['normals'][0], np.tile([[0, 0.6, 0.8]], (3, 1))]), flags=meshes[0]['flags'])
    out = gpu_render(scene, [m2], 1, 1, H, W)
    assert out['dropped'] == 1 and ro.setup_records(scene, [m2], 1, 1, H, W)[1] == 1
    assert not out['setup'][0, 0, -2:].any() and np.array_equal(out['id'][0, 0], adversarial_gpu()[2]['id'][0, 0])
    assert_raster_exact(out, scene, 'guard band')


@pytest.mark.gpu
def test_visualize_writes_the_gif_and_eval_visualize(tmp_path):
    from PIL import Image
    from interdiff_amd import render, eval as ev
    c = ro.e2e_clip(3)
    T, H, W = 3, 48, 64
    plain = render.visualize_body_obj(c['body'], c['body_face'], c['obj'], c['obj_face'], past_len=1, h=H, w=W)
    path = str(tmp_path / 'clip.gif')
    saved = render.visualize_body_obj(c['body'], c['body_face'], c['obj'], c['obj_face'], past_len=1, h=H, w=W, save_path=path, sample_rate=2)
    assert np.array_equal(saved, plain) and os.path.exists(path)

    def read_gif(p):
        im = Image.open(p)
        frames = []
        for k in range(im.n_frames):
            im.seek(k)
            frames.append((im.size, im.info['duration']))
        return frames
    assert render.frame_duration_ms(2) == 70 and render.frame_duration_ms(1) == 30             # 15 and 30 fps on the GIF's 10 ms grid
    assert read_gif(path) == [((4 * W, H), 70)] * T
    dev = lambda a: torch.as_tensor(a).cuda()
    on_device = render.visualize_body_obj(dev(c['body']), dev(c['body_face']), dev(c['obj']), dev(c['obj_face']), past_len=1, h=H, w=W)
    assert np.array_equal(on_device, plain)
    pngs = str(tmp_path / 'frames')
    render.visualize_body_obj(c['body'], c['body_face'], c['obj'], c['obj_face'], past_len=1, h=H, w=W, save_path=pngs)
    assert sorted(os.listdir(pngs)) == ['%05d.png' % i for i in range(T)]
    assert np.array_equal(np.asarray(Image.open(os.path.join(pngs, '00002.png'))), plain[2].transpose(1, 2, 0))
    # eval.visualize: the object centred on its vertex mean and posed per frame in the kernel; the reference's file name
    obj = torch.cat([dev(c['aa']), dev(c['tr'])], dim=1)
    shifted = c['obj_canon'] + np.float32([0.5, -0.25, 1.0])
    gif, video = ev.visualize(dict(start_frame=[35]), 4, obj, dev(c['body']), dev(c['body_face']), (shifted, c['obj_face']), 'pred', tmp_path, past_len=1, h=H, w=W)
    assert gif == os.path.join(str(tmp_path), 'render', 's35_l3_r1_4_pred.gif') and read_gif(gif) == [((4 * W, H), 30)] * T
    assert video.shape == (T, 3, H, 4 * W)
    diff = (video != plain).any(1).reshape(T, -1).mean(1)
    assert diff.max() <= mg.CAP, diff                   # the same clip through the other object route: equal up to the setup stage's rounding
    # a clip that walks 3 m towards the camera: its ground crosses the near plane and leaves the guard band -- counted and REPORTED, the rest is drawn
    far = c['body'].copy()
    far[1] += np.float32([-1.0, 0, -1.5])
    far[2] += np.float32([-2.0, 0, -3.0])
    scene, meshes = ro.clip_scene(far, c['body_face'], c['obj'], c['obj_face'], 1)
    assert ro.setup_records(scene, meshes[:1], T, 4, H, W)[1] > 0
    with pytest.warns(RuntimeWarning, match='guard band'):
        walked = render.visualize_body_obj(far, c['body_face'], c['obj'], c['obj_face'], past_len=1, h=H, w=W)
    assert walked.shape == plain.shape and (walked != 255).any()
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('error')                  # the ordinary clip is silent
        render.visualize_body_obj(c['body'], c['body_face'], c['obj'], c['obj_face'], past_len=1, h=H, w=W, multi_angle=False)
    marked = render.visualize_body_obj(c['body'], c['body_face'], c['obj'], c['obj_face'], past_len=1, h=H, w=W, pcd=c['body'][:, ::700])
    assert marked.shape == plain.shape and (marked != plain).any()
