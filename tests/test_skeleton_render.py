"""Skeleton-clip rendering (interdiff_amd/skeleton_render.py, csrc/skeleton_render.hip, csrc/skeleton_render.h) against the numpy oracle of
tests/skeleton_render_oracle.py and against what matplotlib and the reference's render/viz_helper.py did (tests/golden/skel_render.npz, recorded by
tests/golden/make_golden_skeleton_render.py -- no test imports matplotlib or the reference).

GATES, derived here and not from what the code gives.
  float64 camera vs matplotlib (CPU).  Both evaluate the same rational function of the data in float64, in different operation orders (matplotlib
    composes three 4 x 4 matrices first).  Every intermediate is bounded by 12 (eye offsets ~ 10 + box coordinates < 2), the chains are < 40 operations
    long, the quotient by d ~ 10 and the display scale k = box / 0.185 px per unit follow:  |dpx| <= 40 * 2^-53 * 12 / 10 * 2 k * 2 (both sides)
    =: CAM_GATE(k) -- 4.3e-11 px at 640 x 480.  Limits: 8 roundings of values <= 3: 8 * 2^-53 * 3.  Alpha: the recorded float alpha x 255 lies within
    0.5 + 1e-9 of the integer.  Draw order: equal.
  fp32 setup vs the float64 setup (GPU).  u = 2^-24.  World coordinates: p - lo' (the limits carry <= 4 u |lim|), x scale (2 u): <= 8 u * 2.  Three
    fmaf rows on values <= 12: <= 4 u * 12 each.  tx = vx / d: relative (4 * 12 / |vx| ...) -- absolute <= (48 u + 48 u |tx|) / 10 + u |tx| < 6 u.
    X = fmaf(tx, kx, cx): <= 6 u kx + u |X|; at the largest supported size (2048 px: kx = 1.4e5 units, |X| <= 2^15) that is 0.05 + 0.002 unit,
    at 640 x 480 0.012 unit: far below 1/2, so the snapped values differ by at most ONE unit (a rint flip).  Alpha: norm = (tz - tzmin) / range carries
    <= 3 u |tz| / range; the fixture keeps neighbouring depths > 1e-5 apart and ranges > 1e-3, so norm is good to 2e-4 and 178.5 norm to 0.04: at most
    ONE unit, and the counting ranks are identical.  Kinds, colours, widths, order, dropped count: identical.
  end to end (GPU).  CAP = 0.005 of an image's pixels (make_golden_skeleton_render.py): one flipped coordinate moves one end of one stroke by 1/16 px; the
    sliver it sweeps along the stroke's two long edges has area <= 2 * L / 32 px^2 and holds <= L samples at 16 samples per px^2, so <= L pixels change,
    L <= 60 px for the longest stroke of a 96 x 128 image (its box is 74 px): 60 / 12288 = 0.0049.  With the flip probabilities above (~150 coordinates x
    2 * 0.002) fewer than one image in a hundred has a flip at all; the generator asserts that the float32 restatement stays within CAP / 4.
"""
import ctypes as C
import os
import numpy as np
import pytest
import torch
from tests import skeleton_render_oracle as so
from tests.golden import make_golden_skeleton_render as mg

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
ADV = dict(H=40, W=72)
STYLES = (('plain', 0, {}), ('predgt', 1, dict(vertical_axis='y')), ('turned', 1, dict(vertical_axis='y', **mg.TURNED)))


@pytest.fixture(scope='module')
def z():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'skel_render.npz'))


def clip_args(z, style):
    """keyword tail of so.setup / so.render_clip for a style"""
    if style == 0:
        return dict(body_gt=None, obj_gt=None, T_gt=0, pred_from=mg.PRED_FROM, bones=z['bones'], wires=())
    return dict(body_gt=z['gt_body'], obj_gt=z['gt_obj'], T_gt=mg.T_GT, pred_from=mg.PRED_FROM, bones=z['bones'], wires=z['wires_chair4'])


def cam_gate(k_px):
    return 40 * 2.0 ** -53 * 12 / 10 * 2 * k_px * 2


# ------------------------------------------------------------------------------------------------------------------------------------------
# CPU: the camera
def test_float64_camera_is_matplotlibs(z):
    h, w = 480, 640
    k_px = so.figure_box(h, w)[2] / so.VIEW_SPAN
    worst = 0.0
    for name, style, kw in STYLES:
        vp = so.view_params(style=style, h=h, w=w, **kw)
        for n, t in enumerate(mg.KEEP[name]):
            o = so.setup(vp, t, z['body'], z['obj'], **clip_args(z, style))
            key = lambda k: z['%s_plain' % k][n] if name == 'plain' else z['%s_%s_%d' % (k, name, t)]
            lim, M, disp, segpt, rgba = (key(k) for k in ('lim', 'M', 'disp', 'segpt', 'rgba'))
            assert np.abs(o['lo'] - lim[:, 0]).max() <= 8 * 2.0 ** -53 * 3 and np.abs(o['hi'] - lim[:, 1]).max() <= 8 * 2.0 ** -53 * 3, (name, t)
            # get_proj() rebuilt from the oracle's pieces: perspective(focal 1, dist 10) . view . world
            world, view = np.eye(4), np.eye(4)
            world[[0, 1, 2], [0, 1, 2]], world[:3, 3] = o['scale'], -o['lo'] * o['scale']
            view[:3] = vp['view'].reshape(3, 4)
            proj = np.array([[1.0, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, -so.DIST], [0, 0, -1, 0]])
            assert np.abs(proj @ view @ world - M).max() <= 1e-13 * np.abs(M).max() * 40, (name, t)
            # the lines matplotlib drew, in its order, are the oracle's slots that hold a record, in theirs
            slots = [s for s, r in zip(so.slot_table(vp, z['bones'], clip_args(z, style)['wires']), o['rec']) if r[0] == so.KIND_SEG]
            assert len(slots) == len(disp), (name, t, len(slots), len(disp))
            P, _ = so.frame_points(vp, t, z['body'], z['obj'], clip_args(z, style)['body_gt'], clip_args(z, style)['obj_gt'], clip_args(z, style)['T_gt'], mg.PRED_FROM)
            for (pa, pb, ci), d2, p3, c in zip(slots, disp, segpt, rgba):
                assert np.array_equal(P[[pa, pb]].astype(np.float32), p3.astype(np.float32)), (name, t, pa, pb)          # the same 3D ends: the same line
                mine = np.stack([o['disp'][[pa, pb], 0] / so.SUB, h - o['disp'][[pa, pb], 1] / so.SUB], 1)
                worst = max(worst, np.abs(mine - d2).max())
                assert np.array_equal(np.rint(c * 255).astype(np.int64), vp['colours'][ci]), (name, t, ci, c)
            if name == 'plain':
                groups = o['marker_groups']
                for j, ci in enumerate(groups):
                    idx, md, mc = z['mark_idx_%d_%d' % (t, j)], z['mark_disp_%d_%d' % (t, j)], z['mark_rgba_%d_%d' % (t, j)]
                    base, cnt = (0, so.NB) if ci == so.C_BODY_MARK else (so.NB, so.NO)
                    assert len(idx) == cnt, 'the collections are drawn in the same order'
                    assert np.array_equal(np.rint(mc[0, :3] * 255).astype(np.int64), vp['colours'][ci][:3])
                    order = np.argsort(o['marker_rank'][ci])
                    assert np.array_equal(order, idx), (name, t, j)
                    mine = np.stack([o['disp'][base + order, 0] / so.SUB, h - o['disp'][base + order, 1] / so.SUB], 1)
                    worst = max(worst, np.abs(mine - md).max())
                    assert np.abs(o['marker_alpha'][ci][order] - mc[:, 3] * 255).max() <= 0.5 + 1e-9
    print('float64 camera vs matplotlib: worst display deviation %.3g px (gate %.3g)' % (worst, cam_gate(k_px)))
    assert worst <= cam_gate(k_px)
    for c, rgb in (('b', (0, 0, 255)), ('r', (255, 0, 0)), ('g', (0, 128, 0)), ('w', (255, 255, 255)), ('seagreen', (46, 139, 87)), ('salmon', (250, 128, 114)),
                   ('lightgrey', (211, 211, 211)), ('dimgrey', (105, 105, 105))):
        assert tuple(np.rint(z['colour_' + c] * 255).astype(int)) == rgb, c          # 'g' is 127.5: half to even


def test_product_tables_and_view_are_the_recorded_ones(z):
    from interdiff_amd import skeleton_render as sr
    assert np.array_equal(np.array(sr.BONES), z['bones']) and len(sr.BONES) == 18
    names = sorted(k[6:] for k in z.files if k.startswith('wires_'))
    assert names == sorted(sr.OBJ_WIRES) and len(names) == 9
    for k in names:
        assert np.array_equal(np.array(sr.OBJ_WIRES[k]), z['wires_' + k]), k
    assert sr.PLAIN_COLOURS == so.PLAIN_COLOURS and sr.PREDGT_COLOURS == so.PREDGT_COLOURS
    for name, style, kw in STYLES:
        for h, w in ((480, 640), (96, 128), (50, 70)):
            v = sr.make_view('plain' if style == 0 else 'predgt', vertical_axis=kw.get('vertical_axis', 'z'), h=h, w=w,
                             **{k: kw[k] for k in ('elev', 'azim', 'roll') if k in kw})
            vp = so.view_params(style=style, h=h, w=w, **kw)
            f32 = lambda x: np.asarray(x, np.float64).astype(np.float32)
            assert np.abs(np.array(v.view[:]) - vp['view']).max() <= 2.0 ** -24 * 12 + 1e-12
            for a, b in ((v.aspect[:], vp['aspect']), (v.margin[:], vp['margin']), ([v.dist, v.kx, v.cx, v.ky, v.cy], [vp[k] for k in ('dist', 'kx', 'cx', 'ky', 'cy')])):
                assert np.array_equal(np.array(a, np.float32), f32(b)), (name, h, w)
            assert (v.line_wd, v.disc_wd, v.style, v.pred_from) == (vp['line_wd'], vp['disc_wd'], style, mg.PRED_FROM)
            assert np.array_equal(np.array([list(c) for c in v.colour]), vp['colours'])


# ------------------------------------------------------------------------------------------------------------------------------------------
# CPU: the integer stage
def covered_exact(rec, sx, sy):
    """the coverage rule in python integers (unbounded), with no early-out"""
    kind, x0, y0, x1, y1, wd = (int(v) for v in rec[:6])
    ex, ey = sx - x0, sy - y0
    if kind == so.KIND_DISC:
        return 4 * (ex * ex + ey * ey) <= wd * wd
    dx, dy = x1 - x0, y1 - y0
    L2 = dx * dx + dy * dy
    if L2 == 0:
        return abs(2 * ex) <= wd and abs(2 * ey) <= wd
    cr, t = dx * ey - dy * ex, dx * ex + dy * ey
    e = max(-t, t - L2)
    return (2 * cr) ** 2 <= wd * wd * L2 and (e <= 0 or (2 * e) ** 2 <= wd * wd * L2)


def pixel_exact(recs, i, j):
    acc = [255 << 8] * 3
    for rec in recs:
        if rec[0] == so.KIND_EMPTY:
            continue
        n = sum(covered_exact(rec, so.SUB * i + ox, so.SUB * j + oy) for oy in so.OFFS for ox in so.OFFS)
        w = int(rec[7]) * n
        acc = [(a * (so.WDEN - w) + ((int(rec[6]) >> s & 255) << 8) * w + so.WDEN // 2) // so.WDEN for a, s in zip(acc, (0, 8, 16))]
    return [(a + 128) >> 8 for a in acc]


@pytest.fixture(scope='module')
def adv():
    recs = so.adversarial_records()
    return recs, [so.raster(r, ADV['H'], ADV['W']) for r in recs]


def test_integer_stage_in_unbounded_integers(adv):
    recs, pics = adv
    H, W = ADV['H'], ADV['W']
    exact = np.array([[pixel_exact(recs[0], i, j) for i in range(W)] for j in range(H)], np.uint8)
    assert np.array_equal(exact, pics[0]), 'the int64 restatement (with its early-out) equals the unbounded one on every pixel'
    # frame 1: the two translucent discs in the other order, where they overlap
    box = (slice(8, 33), slice(22, 57))
    exact1 = np.array([[pixel_exact(recs[1], i, j) for i in range(box[1].start, box[1].stop)] for j in range(box[0].start, box[0].stop)], np.uint8)
    assert np.array_equal(exact1, pics[1][box])
    assert (pics[0] != pics[1]).any() and np.array_equal(pics[0][:8], pics[1][:8]), 'translucent "over" does not commute; nothing else changed'
    # the int64 path: the largest values it squares stay below 2^63
    for rec in recs[0]:
        wd = int(rec[5])
        assert ((wd << 17) + 1) ** 2 < 2 ** 63 and wd * wd * (2 * (4 * so.GUARD) ** 2) < 2 ** 63
    # known pictures: the zero-length segment is its 33 / 16 px cap square around (5, 5) px; the radius-3 disc covers one sample of one pixel
    p0 = so.raster([recs[0][0]], H, W)
    assert (p0 != 255).any(-1).sum() == 4 and (p0[4:6, 4:6] == (0, 0, 255)).all()          # samples up to 80 +- 16.5: all 16 of four pixels, none of the next
    one = [recs[0][12]]
    p1 = so.raster(one, H, W)
    assert (p1 != 255).any(-1).sum() == 1 and tuple(p1[30, 30]) == (239, 239, 239)          # 255 * (1 - 1 / 16) = 239.06
    # the two records outside the image change nothing, empty or not
    without = [r for k, r in enumerate(recs[0]) if k not in (9, 10)]
    assert np.array_equal(so.raster(without, H, W), pics[0])


def host_pixels(lib, recs, H, W):
    r = np.ascontiguousarray(np.array(recs, np.int64).astype(np.int32))
    jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    ij = np.ascontiguousarray(np.stack([ii, jj], -1).reshape(-1, 2).astype(np.int32))
    out = np.zeros((H * W, 3), np.int32)
    assert lib.interdiff_debug_skeleton_pixel(r.ctypes.data, len(r), ij.ctypes.data, out.ctypes.data, len(ij)) == 0
    return out.reshape(H, W, 3).astype(np.uint8)


def test_host_pixel_function_is_the_integer_oracle_bit_for_bit(lib, adv):
    recs, pics = adv
    for r, p in zip(recs, pics):
        assert np.array_equal(host_pixels(lib, r, ADV['H'], ADV['W']), p)


def host_setup(lib, view, t, body, obj, body_gt=None, obj_gt=None, wires=()):
    from interdiff_amd import _lib
    rec, cnt, dr = np.zeros((_lib.SKEL_MAX_REC, _lib.SKEL_REC_INTS), np.int32), C.c_int32(), C.c_int32()
    f = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)
    body, obj, body_gt, obj_gt = f(body), f(obj), f(body_gt), f(obj_gt)
    w = np.ascontiguousarray(wires, np.int32) if len(wires) else None
    p = lambda a: None if a is None else a.ctypes.data
    rc = lib.interdiff_debug_skeleton_setup(C.byref(view), p(body), p(obj), p(body_gt), p(obj_gt), p(w), 0 if w is None else len(w), len(body),
                                            0 if body_gt is None else len(body_gt), t, rec.ctypes.data, C.byref(cnt), C.byref(dr))
    assert rc == 0, rc
    return rec, cnt.value, dr.value


def product_view(name, style, kw, h, w):
    from interdiff_amd import skeleton_render as sr
    return sr.make_view('plain' if style == 0 else 'predgt', vertical_axis=kw.get('vertical_axis', 'z'), h=h, w=w, **{k: kw[k] for k in ('elev', 'azim', 'roll') if k in kw})


def check_setup(got, ref, what):
    """records within one sub-pixel unit and one alpha unit of the float64 oracle's; kinds, widths, colours and order identical"""
    got, ref = np.asarray(got, np.int64), np.asarray(ref, np.int64)
    assert got.shape == ref.shape, what
    assert np.array_equal(got[:, [0, 5, 6]], ref[:, [0, 5, 6]]), what + ': kinds, widths, colours, draw order'
    dxy, da = np.abs(got[:, 1:5] - ref[:, 1:5]).max(), np.abs(got[:, 7] - ref[:, 7]).max()
    assert dxy <= 1 and da <= 1, (what, dxy, da)
    return dxy, da


def test_host_setup_function_matches_the_oracle(lib, z):
    """the host instance of the per-frame setup: bit for bit the float32 restatement, within the gates of the float64 one"""
    for name, style, kw in STYLES:
        for h, w in ((480, 640), (96, 128)):
            v, vp = product_view(name, style, kw, h, w), so.view_params(style=style, h=h, w=w, **kw)
            ca = clip_args(z, style)
            for t in range(mg.T):
                rec, cnt, dr = host_setup(lib, v, t, z['body'], z['obj'], ca['body_gt'], ca['obj_gt'], ca['wires'])
                o64, o32 = so.setup(vp, t, z['body'], z['obj'], **ca), so.setup(vp, t, z['body'], z['obj'], dtype=np.float32, **ca)
                assert cnt == o64['count'] == o32['count'] and dr == o64['dropped'] == 0
                assert not rec[cnt:].any()
                assert np.array_equal(rec[:cnt], o32['rec']), (name, h, t)
                check_setup(rec[:cnt], o64['rec'], '%s %dx%d frame %d' % (name, h, w, t))


def test_switches_ties_and_dropped_primitives(lib, z):
    v1, vp1 = product_view('predgt', 1, dict(vertical_axis='y'), 96, 128), so.view_params(style=1, vertical_axis='y', h=96, w=128)
    ca = clip_args(z, 1)
    n_w, per = len(ca['wires']), so.NBONE + len(ca['wires'])
    for t, pred, gt in ((10, False, True), (11, True, True), (mg.T_GT - 1, True, True), (mg.T_GT, True, False)):
        rec, cnt, dr = host_setup(lib, v1, t, z['body'], z['obj'], ca['body_gt'], ca['obj_gt'], ca['wires'])
        assert cnt == 3 + 2 * per and dr == 0
        assert (rec[:3, 0] == 1).all(), 'the axis lines come first'
        assert (rec[3:3 + per, 0] == 1).all() == pred and rec[3:3 + per].any() == pred, (t, 'prediction: frames > 10')
        assert (rec[3 + per:cnt, 0] == 1).all() == gt and rec[3 + per:cnt].any() == gt, (t, 'ground truth: frames < len(gt)')
        assert np.array_equal(rec[:cnt], so.setup(vp1, t, z['body'], z['obj'], dtype=np.float32, **ca)['rec'])
    # an unknown object name draws no wires
    from interdiff_amd import skeleton_render as sr
    assert len(sr._wire_table('no such object', None)) == 0 and len(sr._wire_table('chair4', None)) == 18 and len(sr._wire_table('x', [(0, 1)])) == 1
    rec, cnt, dr = host_setup(lib, v1, 12, z['body'], z['obj'], ca['body_gt'], ca['obj_gt'], ())
    assert cnt == 3 + 2 * so.NBONE and (rec[:cnt, 0] == 1).all()
    # plain: the white axis lines come last among the lines; an exact depth tie draws the higher index first; a joint that is not finite
    v0, vp0 = product_view('plain', 0, {}, 96, 128), so.view_params(style=0, h=96, w=128)
    body = z['body'].copy()
    body[0, 15] = body[0, 7] = body[0, 2]
    rec, cnt, dr = host_setup(lib, v0, 0, body, z['obj'])
    o = so.setup(vp0, 0, body, z['obj'], dtype=np.float32, **clip_args(z, 0))
    assert np.array_equal(rec[:cnt], o['rec']) and dr == 0
    assert (rec[so.NBONE:so.NBONE + 3, 6] == 0xFFFFFF).all() and (rec[:so.NBONE, 6] == 0xFF0000).all()
    order = np.argsort(o['marker_rank'][so.C_BODY_MARK])
    tied = [int(i) for i in order if i in (2, 7, 15)]
    assert tied == [15, 7, 2]            # (matplotlib's own order here is z['tie_order'] = 7, 15, 2: its argsort is not stable; markers of one depth share colour and alpha)
    assert sorted(z['tie_order'].tolist()) == [2, 7, 15]
    body = z['body'].copy()
    body[0, 2, 1] = np.nan               # joint 2: bones (1,2) (2,3) (2,5) (2,9) and its marker
    rec, cnt, dr = host_setup(lib, v0, 0, body, z['obj'])
    o = so.setup(vp0, 0, body, z['obj'], dtype=np.float32, **clip_args(z, 0))
    assert dr == o['dropped'] == 5 and np.array_equal(rec[:cnt], o['rec'])
    assert (rec[:cnt, 0] != 0).sum() == cnt - 5, 'dropped and counted, the rest is drawn'
    body[0, 2, 1] = np.inf
    assert host_setup(lib, v0, 0, body, z['obj'])[2] == 5
    # the guard band: with per-frame limits no point of a real view gets near it, so the display scale is blown up 200 times;
    # what then lands beyond +-2048 px of the image's corner is dropped and counted, never clamped, and the rest keeps its coordinates
    v0.kx, v0.ky = v0.kx * 200, v0.ky * 200
    vpg = dict(vp0, kx=float(v0.kx), ky=float(v0.ky))
    rec, cnt, dr = host_setup(lib, v0, 0, z['body'], z['obj'])
    o = so.setup(vpg, 0, z['body'], z['obj'], dtype=np.float32, **clip_args(z, 0))
    kept = (rec[:cnt, 0] != 0).sum()
    assert dr == o['dropped'] and 0 < dr < cnt and kept == cnt - dr and kept > 0 and np.array_equal(rec[:cnt], o['rec'])
    assert np.abs(rec[:cnt, 1:5]).max() <= so.GUARD


# ------------------------------------------------------------------------------------------------------------------------------------------
# CPU: the oracle's pictures against the reference's frames
@pytest.fixture(scope='module')
def oracle_480(z):
    out = {}
    for name, style, kw in STYLES:
        vp = so.view_params(style=style, **kw)
        out[name] = so.render_clip(vp, z['body'], z['obj'], frames=mg.KEEP[name], **clip_args(z, style))
    return out


def ink_check(ref, pics, what):
    for n, (a, b) in enumerate(zip(ref, pics)):
        ea, eb = so.ink_exceptions(a, b)
        print('%s frame %d: ink of the reference without ours within 2 px %.4f, ours without the reference %.4f (cap %.2f)' % (what, n, ea, eb, mg.INK_CAP))
        assert so.ink(a).sum() > 200 and so.ink(b).sum() > 200, what
        assert ea <= mg.INK_CAP and eb <= mg.INK_CAP, (what, n, ea, eb)


def test_oracle_pictures_put_their_ink_where_the_reference_does(z, oracle_480):
    for name, _, _ in STYLES:
        ink_check(z['ref_' + name], oracle_480[name], name)
        mad = [np.abs(a.astype(np.int64) - b.astype(np.int64))[so.ink(a) | so.ink(b)].mean() for a, b in zip(z['ref_' + name], oracle_480[name])]
        print(name, 'mean absolute colour difference on the union of ink (measured, not gated):', mad)
        assert np.allclose(mad, z['colour_mad_' + name]), 'the golden file holds the measurement'


def test_fixture_conditions_and_oracle_regression(z):
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'skel_render.npz')) < 1000000
    for name, style, kw in STYLES:
        assert z['e2e_share32_' + name].max() <= mg.CAP / 4
        vs = so.view_params(style=style, h=mg.E2E['H'], w=mg.E2E['W'], **kw)
        pics = so.render_clip(vs, z['body'], z['obj'], frames=mg.E2E['frames'], **clip_args(z, style))
        assert np.array_equal(pics, z['e2e_rgb_' + name])
    vp = so.view_params(style=0)
    for t in mg.KEEP['plain']:                        # depth gaps inside each scatter far above fp32 resolution; the limits of frame 5 are the data's
        o = so.setup(vp, t, z['body'], z['obj'], **clip_args(z, 0))
        for base, n in ((0, so.NB), (so.NB, so.NO)):
            tz = np.sort(o['tz'][base:base + n])
            assert np.diff(tz).min() > mg.MIN_DEPTH_GAP and tz[-1] - tz[0] > 1e-3
    assert so.setup(vp, 5, z['body'], z['obj'], **clip_args(z, 0))['hi'][1] > 1.5 > so.setup(vp, 0, z['body'], z['obj'], **clip_args(z, 0))['hi'][1]


# ------------------------------------------------------------------------------------------------------------------------------------------
# CPU: host glue
def test_gif_writer_and_argument_errors(tmp_path):
    from PIL import Image
    from interdiff_amd import skeleton_render as sr
    rs = np.random.RandomState(0)
    few = rs.randint(0, 6, (3, 20, 30, 1)).astype(np.uint8) * np.array([40, 30, 50], np.uint8)          # 6 colours per frame: stored exactly
    many = rs.randint(0, 256, (2, 20, 30, 3)).astype(np.uint8)
    for name, frames in (('few', few), ('many', many)):
        path = str(tmp_path / (name + '.gif'))
        sr.save_gif(frames, path)
        im = Image.open(path)
        assert im.n_frames == len(frames) and im.info['duration'] == 50 and im.info['loop'] == 0
        for i, f in enumerate(frames):
            im.seek(i)
            back = np.array(im.convert('RGB'))
            want = f if name == 'few' else np.array(Image.fromarray(f).quantize(256).convert('RGB'))
            assert np.array_equal(back, want), (name, i)
    body, obj = np.zeros((4, 21, 3), np.float32), np.zeros((4, 12, 3), np.float32)
    for bad in (lambda: sr.visualize_skeleton(body[:, :20], obj, None), lambda: sr.visualize_skeleton(body, obj.reshape(4, 12 * 3)[:, :35], None),
                lambda: sr.visualize_skeleton(body.reshape(1, 4, 21, 3), obj, None), lambda: sr.visualize_skeleton(body.astype(str), obj, None),
                lambda: sr.visualize_skeleton(body[:0], obj[:0], None), lambda: sr.visualize_skeleton(body, obj[:3], None),
                lambda: sr.visualize_skeleton_pred_gt(body, obj, body[:, :3], obj, None), lambda: sr.visualize_skeleton_pred_gt(body, obj, body, obj, None, obj_connections=[(0, 12)]),
                lambda: sr.render_skeleton_clips(body, obj, body, obj), lambda: sr.render_skeleton_clips(body, obj, style='predgt', body_gt=body),
                lambda: sr.render_skeleton_clips(body, obj, h=0), lambda: sr.render_skeleton_clips(body, obj, style='sketch')):
        with pytest.raises(ValueError):
            bad()


def test_visualize_file_names_and_the_sample_idx_skip(tmp_path, monkeypatch):
    """the trainers' ``visualize``: clip 0 of a [T,B,...] batch, file names, the gt file skipped for sample_idx > 0 (the renderer itself replaced by a stub)"""
    from interdiff_amd import skeleton_render as sr
    seen = []

    def stub(body, obj, *a, **kw):
        seen.append((np.asarray(body).copy(), np.asarray(obj).copy(), kw.get('style')))
        return dict(rgb=torch.full((1, len(body), 8, 8, 3), 255, dtype=torch.uint8), dropped=0)
    monkeypatch.setattr(sr, 'render_skeleton_clips', stub)
    T, B = 5, 3
    rs = np.random.RandomState(1)
    bp, op, bg, og = (torch.from_numpy(rs.standard_normal(s).astype(np.float32)) for s in ((T, B, 63), (T, B, 36), (T, B, 21, 3), (T, B, 12, 3)))
    w = sr.visualize(bp, op, bg, og, tmp_path, 'val', 7, 3)
    assert [os.path.relpath(p, tmp_path) for p in w] == [os.path.join('render', 'val_7_3_p.gif'), os.path.join('render', 'val_7_3_gt.gif')]
    assert all(os.path.exists(p) for p in w)
    assert np.array_equal(seen[0][0], bp[:, 0].reshape(T, 21, 3).numpy()) and np.array_equal(seen[1][1], og[:, 0].numpy()) and seen[0][2] == 'plain'
    w = sr.visualize(bp, op, bg, og, tmp_path, 'test', 0, 2, sample_idx=0)
    assert [os.path.basename(p) for p in w] == ['test_0_2_0_p.gif', 'test_0_2_0_gt.gif']
    w = sr.visualize(bp, op, bg, og, tmp_path, 'test', 0, 2, sample_idx=4)
    assert [os.path.basename(p) for p in w] == ['test_0_2_4_p.gif'] and not os.path.exists(os.path.join(tmp_path, 'render', 'test_0_2_4_gt.gif'))


def test_skeleton_render_symbols_are_declared_bound_and_exported(lib):
    from interdiff_amd import _lib
    names = ['interdiff_skeleton_render_frames', 'interdiff_skeleton_render_frames_workspace_bytes', 'interdiff_skeleton_raster_records',
             'interdiff_debug_skeleton_setup', 'interdiff_debug_skeleton_pixel']
    hdr = open(os.path.join(ROOT, 'include', 'interdiff_hip.h')).read()
    for n in names:
        assert n in _lib.exported_symbols() and n + '(' in hdr and hasattr(lib, n)
    assert lib.interdiff_abi_version() == _lib.ABI_VERSION                     # additive entries: the ABI version does not move
    for k, v in (('IDF_SKEL_REC_INTS', _lib.SKEL_REC_INTS), ('IDF_SKEL_MAX_REC', _lib.SKEL_MAX_REC), ('IDF_SKEL_MAX_WIRES', _lib.SKEL_MAX_WIRES),
                 ('IDF_SKEL_WD_MAX', _lib.SKEL_WD_MAX), ('IDF_SKEL_TILE', _lib.SKEL_TILE)):
        assert '#define %s %d\n' % (k, v) in hdr
    assert (so.REC, so.MAX_REC, so.MAX_WIRES) == (_lib.SKEL_REC_INTS, _lib.SKEL_MAX_REC, _lib.SKEL_MAX_WIRES)
    assert C.sizeof(_lib.SkelView) == 12 * 4 + 6 * 4 + 5 * 4 + 4 * 4 + 20
    assert lib.interdiff_skeleton_render_frames_workspace_bytes(0) == 0 and lib.interdiff_skeleton_render_frames_workspace_bytes(3) >= 3 * 128 * 8 * 4


# ------------------------------------------------------------------------------------------------------------------------------------------
# GPU
def gpu_clip(z, style, h, w, kw, B=1, **extra):
    from interdiff_amd import skeleton_render as sr
    ca = clip_args(z, style)
    rep = lambda a: None if a is None else np.stack([a + 0.03 * b for b in range(B)])
    return sr.render_skeleton_clips(rep(z['body']), rep(z['obj']), rep(ca['body_gt']), rep(ca['obj_gt']), style='plain' if style == 0 else 'predgt',
                                    obj_connections=ca['wires'] if style else None, h=h, w=w, want_setup=True,
                                    **{k: kw[k] for k in ('elev', 'azim', 'roll') if k in kw}, **extra)


def assert_raster_exact(out, h, w, what, frames=None):
    """every picture equals the integer oracle run on the kernel's own setup records, no pixel excluded"""
    rgb, setup, count = out['rgb'].cpu().numpy(), out['setup'].cpu().numpy(), out['count'].cpu().numpy()
    for b in range(rgb.shape[0]):
        for t in (range(rgb.shape[1]) if frames is None else frames):
            assert np.array_equal(rgb[b, t], so.raster(setup[b, t, :count[b, t]], h, w)), (what, b, t)


@pytest.mark.gpu
def test_raster_stage_is_bit_exact_on_the_adversarial_scene(adv):
    from interdiff_amd import _lib, skeleton_render as sr
    recs, pics = adv
    dev = torch.zeros(len(recs), _lib.SKEL_MAX_REC, _lib.SKEL_REC_INTS, dtype=torch.int32)
    for f, r in enumerate(recs):
        dev[f, :len(r)] = torch.tensor(r, dtype=torch.int64).to(torch.int32)
    got = sr.raster_records(dev.cuda(), len(recs[0]), ADV['H'], ADV['W']).cpu().numpy()
    assert np.array_equal(got, np.stack(pics))


@pytest.mark.gpu
@pytest.mark.parametrize('name,style,kw', STYLES, ids=[s[0] for s in STYLES])
def test_end_to_end_clip_setup_raster_and_picture(z, name, style, kw):
    """96 x 128, the whole clip: setup records against the float64 setup (module docstring), the raster bit for bit on the kernel's own records, and the
    share of pixels that differ from the float64 oracle's picture"""
    h, w = mg.E2E['H'], mg.E2E['W']
    out = gpu_clip(z, style, h, w, kw)
    assert out['dropped'] == 0
    vp, ca = so.view_params(style=style, h=h, w=w, **kw), clip_args(z, style)
    setup, count = out['setup'].cpu().numpy()[0], out['count'].cpu().numpy()[0]
    worst = (0, 0)
    for t in range(mg.T):
        o = so.setup(vp, t, z['body'], z['obj'], **ca)
        assert count[t] == o['count'] and not setup[t, count[t]:].any()
        worst = max(worst, check_setup(setup[t, :count[t]], o['rec'], '%s frame %d' % (name, t)))
    print('%s: setup deviation from the float64 setup: %d unit, alpha %d unit' % ((name,) + worst))
    assert_raster_exact(out, h, w, name, frames=mg.E2E['frames'])
    rgb = out['rgb'].cpu().numpy()[0][list(mg.E2E['frames'])]
    share = (rgb != z['e2e_rgb_' + name]).any(-1).reshape(len(rgb), -1).mean(1)
    print('%s: share of pixels that differ from the float64 oracle picture per image: %s (cap %.4f)' % (name, share, mg.CAP))
    assert share.max() <= mg.CAP


@pytest.mark.gpu
def test_odd_size_repeatability_chunking_and_batching(lib, z):
    """50 x 70 (no multiple of the tile): raster exact; two calls give equal bits; a workspace that holds 7 frames (9 chunks for 3 x 20) gives the
    bits of one chunk; three clips batched equal three single calls"""
    from interdiff_amd import skeleton_render as sr
    h, w = 50, 70
    for name, style, kw in STYLES[:2]:
        a = gpu_clip(z, style, h, w, kw, B=3)
        assert_raster_exact(a, h, w, name, frames=(0, 5, 12, 19))
        b = gpu_clip(z, style, h, w, kw, B=3)
        small = lib.interdiff_skeleton_render_frames_workspace_bytes(7)
        c = gpu_clip(z, style, h, w, kw, B=3, workspace_bytes=small)
        d = gpu_clip(z, style, h, w, kw, B=3, workspace_bytes=lib.interdiff_skeleton_render_frames_workspace_bytes(1))
        for o in (b, c, d):
            assert torch.equal(a['rgb'], o['rgb']) and torch.equal(a['setup'], o['setup']) and torch.equal(a['count'], o['count'])
        ca = clip_args(z, style)
        for i in range(3):
            sh = lambda x: None if x is None else x + 0.03 * i
            one = sr.render_skeleton_clips(sh(z['body']), sh(z['obj']), sh(ca['body_gt']), sh(ca['obj_gt']), style='plain' if style == 0 else 'predgt',
                                           obj_connections=ca['wires'] if style else None, h=h, w=w, want_setup=True)
            assert torch.equal(one['rgb'][0], a['rgb'][i]) and torch.equal(one['setup'][0], a['setup'][i])
    # a joint that is not finite: dropped and counted, the rest drawn
    body = z['body'].copy()
    body[3, 2, 0] = np.nan
    out = sr.render_skeleton_clips(body, z['obj'], h=h, w=w, want_setup=True)
    assert out['dropped'] == 5
    assert_raster_exact(out, h, w, 'nan joint', frames=(3,))
    o = so.setup(so.view_params(style=0, h=h, w=w), 3, body, z['obj'], **clip_args(z, 0))
    check_setup(out['setup'].cpu().numpy()[0, 3, :o['count']], o['rec'], 'nan joint')


@pytest.mark.gpu
def test_public_functions_against_the_reference_frames(z, tmp_path):
    """visualize_skeleton and visualize_skeleton_pred_gt at 640 x 480, once each, under the ink condition of the CPU test; the GIFs they write"""
    from PIL import Image
    from interdiff_amd import skeleton_render as sr
    p1, p2 = str(tmp_path / 'plain.gif'), str(tmp_path / 'predgt.xyz')
    f1 = sr.visualize_skeleton(z['body'], z['obj'].reshape(mg.T, 36), p1)
    f2 = sr.visualize_skeleton_pred_gt(torch.from_numpy(z['body']), z['obj'], z['gt_body'], z['gt_obj'], p2, tmp_dir=str(tmp_path / 'never_made'))
    assert f1.shape == f2.shape == (mg.T, 480, 640, 3) and f1.dtype == np.uint8
    assert os.path.exists(str(tmp_path / 'predgt.gif')) and not os.path.exists(str(tmp_path / 'never_made'))
    ink_check(z['ref_plain'], f1[list(mg.KEEP['plain'])], 'visualize_skeleton')
    ink_check(z['ref_predgt'], f2[list(mg.KEEP['predgt'])], 'visualize_skeleton_pred_gt')
    f3 = sr.visualize_skeleton_pred_gt(z['body'], z['obj'], z['gt_body'], z['gt_obj'], None, **mg.TURNED)
    ink_check(z['ref_turned'], f3[list(mg.KEEP['turned'])], 'visualize_skeleton_pred_gt, turned')
    f4 = sr.visualize_skeleton_pred_gt(z['body'], z['obj'], z['gt_body'], z['gt_obj'], None, obj_name='no such object')
    assert so.ink(f4[12]).sum() < so.ink(f2[12]).sum()
    for path, frames in ((p1, f1), (str(tmp_path / 'predgt.gif'), f2)):
        im = Image.open(path)
        assert im.n_frames == mg.T and im.info['duration'] == 50 and im.info['loop'] == 0
        for i in (0, 12, 19):
            im.seek(i)
            f = frames[i]
            exact = len(np.unique(f.reshape(-1, 3), axis=0)) <= 256
            want = f if exact else np.array(Image.fromarray(f).quantize(256).convert('RGB'))
            assert np.array_equal(np.array(im.convert('RGB')), want), (path, i, exact)


@pytest.mark.gpu
def test_trainer_visualize_writes_both_gifs(z, tmp_path):
    from PIL import Image
    from interdiff_amd import skeleton_render as sr
    T, B = 6, 2
    bp = torch.from_numpy(np.stack([z['body'][:T], z['body'][:T] + 1], 1)).cuda()
    op = torch.from_numpy(np.stack([z['obj'][:T], z['obj'][:T] + 1], 1)).reshape(T, B, 36).cuda()
    bg = torch.from_numpy(np.stack([z['gt_body'][:T]] * 2, 1)).cuda()
    og = torch.from_numpy(np.stack([z['gt_obj'][:T]] * 2, 1)).cuda()
    w = sr.visualize(bp, op, bg, og, tmp_path, 'val', 2, 9, h=96, w=128)
    assert [os.path.basename(p) for p in w] == ['val_2_9_p.gif', 'val_2_9_gt.gif']
    for path, (b, o) in zip(w, ((z['body'][:T], z['obj'][:T]), (z['gt_body'][:T], z['gt_obj'][:T]))):
        frames = sr.visualize_skeleton(b, o, None, h=96, w=128)
        im = Image.open(path)
        assert im.n_frames == T
        for i in range(T):
            im.seek(i)
            f = frames[i]
            exact = len(np.unique(f.reshape(-1, 3), axis=0)) <= 256
            want = f if exact else np.array(Image.fromarray(f).quantize(256).convert('RGB'))
            assert np.array_equal(np.array(im.convert('RGB')), want), (path, i)
