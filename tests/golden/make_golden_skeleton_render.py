"""tests/golden/skel_render.npz: what the reference's render/viz_helper.py and matplotlib did for a seeded synthetic skeleton clip, and what the numpy
oracle (tests/skeleton_render_oracle.py) gives for the fixed scenes of tests/test_skeleton_render.py.

    python -m tests.golden.make_golden_skeleton_render /path/to/reference/interdiff

Needs matplotlib (the version asserted below) and the reference tree; viz_helper.py is loaded by file path (its package's __init__ needs trimesh).
Recorded, per kept frame of ``visualize_skeleton`` (plain) and ``visualize_skeleton_pred_gt`` (default view and a turned one):
  ref_*        the reference's own GIF frames, read back from the files it wrote (uint8 [n, 480, 640, 3])
  lim_*        matplotlib's 3D limits [n, 3, 2];  M_* = get_proj() [n, 4, 4]
  disp_*       display coordinates (x right, y UP, pixels) of both ends of every line, in draw order [n, lines, 2, 2];  segpt_* the 3D ends [n, lines, 2, 3]
  mark_*       plain only, per scatter collection in DRAW order: source index, display xy, depth-shaded alpha of the markers in draw order
  bones, wires_<name>, colour_<name>   the reference's topology tables and matplotlib's RGB of the named colours
  tie_order    the order in which matplotlib drew three markers of exactly equal depth (indices 2, 7, 15 of one scatter)
  e2e_*        oracle pictures of the 96 x 128 end-to-end clip and the float32-vs-float64 setup share; colour_mad_* the measured colour difference
The conditions the tests rely on are asserted here and again by the tests."""
import importlib.util
import os
import sys
import tempfile
import numpy as np
from tests import skeleton_render_oracle as so

HERE = os.path.dirname(os.path.abspath(__file__))
MPL_VERSION = '3.10.8'
T, T_GT, PRED_FROM = 20, 16, 11
KEEP = dict(plain=(0, 5, 19), predgt=(3, 12, 18), turned=(12,))
TURNED = dict(elev=30.0, azim=45.0, roll=10.0)
E2E = dict(H=96, W=128, frames=(5, 12, 18))
CAP = 0.005                        # differing pixels per image allowed between the kernel and the float64 oracle
INK_CAP = 0.01
MIN_DEPTH_GAP = 1e-5               # between two markers of a collection, in projected depth (|tz| ~ 1): far above float32 resolution (6e-8)
SEED = 4                           # the first seed whose kept frames meet MIN_DEPTH_GAP and the float32 condition below


def synthetic_clip(seed=None, n=T):
    """a body of 21 joints and 12 object keypoints drifting through a room-sized box; frame 5 reaches beyond the axis lines' range"""
    rs = np.random.RandomState(SEED if seed is None else seed)
    b0 = rs.uniform([-0.35, -0.6, -0.35], [0.35, 0.9, 0.35], (21, 3))
    o0 = rs.uniform([0.3, -0.3, 0.1], [0.8, 0.3, 0.6], (12, 3))
    tt = np.arange(n)[:, None, None]
    body = b0 + 0.01 * tt * rs.standard_normal((1, 1, 3)) + 0.02 * np.cumsum(rs.standard_normal((n, 21, 3)), 0) / 4
    obj = o0 + 0.015 * tt * rs.standard_normal((1, 1, 3))
    body[5] *= 2.3                                                            # y up to ~2: the limits of this frame are the data's
    gt_b = body + 0.05 * rs.standard_normal(body.shape)
    gt_o = obj + 0.05 * rs.standard_normal(obj.shape)
    return body.astype(np.float32), obj.astype(np.float32), gt_b[:T_GT].astype(np.float32), gt_o[:T_GT].astype(np.float32)


def record_reference(ref_root, out):
    import matplotlib
    assert matplotlib.__version__ == MPL_VERSION, matplotlib.__version__
    matplotlib.use('Agg')
    from mpl_toolkits.mplot3d import axes3d, art3d
    from matplotlib.colors import to_rgba
    from PIL import Image
    spec = importlib.util.spec_from_file_location('viz_helper', os.path.join(ref_root, 'render', 'viz_helper.py'))
    vh = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(vh)
    out['bones'] = np.array(vh.connections, np.int32)
    for k, v in vh.obj_connects.items():
        out['wires_' + k] = np.array(v, np.int32)
    for c in ('b', 'r', 'g', 'w', 'seagreen', 'salmon', 'lightgrey', 'dimgrey'):
        out['colour_' + c] = np.array(to_rgba(c)[:3])
    log, cur = {}, [None]
    orig = axes3d.Axes3D.draw
    from matplotlib import animation
    orig_frame = animation.FuncAnimation._draw_frame

    def draw_frame(self, framedata):
        cur[0] = int(framedata)
        return orig_frame(self, framedata)

    def draw(self, renderer):
        orig(self, renderer)
        lines = [l for l in self.get_children() if isinstance(l, art3d.Line3D)]
        cols = sorted((c for c in self.get_children() if isinstance(c, art3d.Path3DCollection)), key=lambda c: c.zorder)
        assert all(l.get_zorder() == 2 and abs(l.get_linewidth() - 1.5) < 1e-12 and l.get_solid_capstyle() == 'projecting' and l.get_antialiased() for l in lines)
        assert all(c.zorder > 2 for c in cols)
        rec = dict(lim=np.array([self.get_xlim3d(), self.get_ylim3d(), self.get_zlim3d()]), M=np.array(self.M), box=np.array(self.bbox.bounds),
                   view=np.array([self.viewLim.x0, self.viewLim.y0, self.viewLim.width, self.viewLim.height]),
                   disp=np.array([self.transData.transform(np.asarray(l.get_xydata(), float)) for l in lines]),
                   segpt=np.array([np.stack([np.asarray(a, float) for a in l._verts3d], 1) for l in lines]),
                   rgba=np.array([to_rgba(l.get_color()) for l in lines]), marks=[])
        for c in cols:
            assert np.allclose(c.get_sizes(), 20.0) and np.allclose(c.get_linewidths(), 1.0), (c.get_sizes(), c.get_linewidths())
            fc = c.get_facecolor()
            assert np.array_equal(fc, c.get_edgecolor())
            rec['marks'].append(dict(idx=np.array(c._z_markers_idx), disp=self.transData.transform(np.asarray(c._offset_zordered, float)), rgba=fc,
                                     pts=np.stack([np.asarray(a, float) for a in c._offsets3d], 1), vz=np.asarray(c._vzs, float)))
        log[cur[0]] = rec                                                     # a frame is drawn more than once while it is saved: the last draw stands
    axes3d.Axes3D.draw = draw
    animation.FuncAnimation._draw_frame = draw_frame
    body, obj, gt_b, gt_o = synthetic_clip()
    out.update(body=body, obj=obj, gt_body=gt_b, gt_obj=gt_o)
    tmp = tempfile.mkdtemp()

    def frames_of(path):
        im = Image.open(path)
        assert im.n_frames == T and im.info['duration'] == 50 and im.info['loop'] == 0, (im.n_frames, im.info)
        fr = []
        for i in range(im.n_frames):
            im.seek(i)
            fr.append(np.array(im.convert('RGB')))
        return np.stack(fr)
    try:
        runs = (('plain', lambda p: vh.visualize_skeleton(body, obj, p)),
                ('predgt', lambda p: vh.visualize_skeleton_pred_gt(body, obj, gt_b, gt_o, p, tmp_dir=os.path.join(tmp, 'tmp'))),
                ('turned', lambda p: vh.visualize_skeleton_pred_gt(body, obj, gt_b, gt_o, p, tmp_dir=os.path.join(tmp, 'tmp'), **TURNED)))
        for name, run in runs:
            log.clear()
            path = os.path.join(tmp, name + '.gif')
            run(path)
            fr = frames_of(path)
            assert fr.shape == (T, 480, 640, 3)
            assert sorted(log) == list(range(T))
            recs = log
            keep = KEEP[name]
            out['ref_' + name] = fr[list(keep)]
            for k in ('lim', 'M', 'disp', 'segpt', 'rgba'):
                if name == 'plain':
                    out[k + '_' + name] = np.stack([recs[t][k] for t in keep])
                else:                                                         # the number of lines changes with the frame
                    for t in keep:
                        out['%s_%s_%d' % (k, name, t)] = recs[t][k]
            assert all(np.allclose(recs[t]['box'], so.figure_box(480, 640), atol=1e-9) for t in keep)
            assert all(np.allclose(recs[t]['view'], [-so.VIEW_HALF, -so.VIEW_HALF, so.VIEW_SPAN, so.VIEW_SPAN], atol=1e-12) for t in keep)
            if name == 'plain':
                for t in keep:
                    assert len(recs[t]['marks']) == 2
                    for j, mk in enumerate(recs[t]['marks']):
                        gaps = np.diff(np.sort(mk['vz']))
                        assert gaps.min() > MIN_DEPTH_GAP, gaps.min()
                        out['mark_idx_%d_%d' % (t, j)], out['mark_disp_%d_%d' % (t, j)], out['mark_rgba_%d_%d' % (t, j)] = mk['idx'], mk['disp'], mk['rgba']
                        out['mark_n_%d_%d' % (t, j)] = np.array(len(mk['idx']))
        # what matplotlib does with markers of EQUAL depth: two coincident points appended to a collection
        out['tie_order'] = tie_probe()
    finally:
        axes3d.Axes3D.draw = orig
        animation.FuncAnimation._draw_frame = orig_frame
    return out


def tie_probe():
    """draw order of exactly equal depths in one scatter (duplicated points), as matplotlib sorts them: indices of the duplicates in draw order"""
    import matplotlib.pyplot as plt
    fig = plt.figure()
    ax = fig.add_subplot(111, projection='3d')
    rs = np.random.RandomState(3)
    p = rs.uniform(-1, 1, (21, 3))
    p[7] = p[15] = p[2]
    c = ax.scatter3D(p[:, 0], p[:, 1], p[:, 2], color='r')
    fig.canvas.draw()
    idx = np.array(c._z_markers_idx)
    plt.close(fig)
    return np.array([i for i in idx if i in (2, 7, 15)], np.int32)


def oracle_part(out):
    body, obj, gt_b, gt_o = out['body'], out['obj'], out['gt_body'], out['gt_obj']
    bones, wires = out['bones'], out['wires_chair4']
    for name, style, kw in (('plain', 0, {}), ('predgt', 1, dict(vertical_axis='y')), ('turned', 1, dict(vertical_axis='y', **TURNED))):
        vp = so.view_params(style=style, **kw)
        pics = so.render_clip(vp, body, obj, gt_b, gt_o, T_GT, PRED_FROM, bones, wires, frames=KEEP[name])
        ref = out['ref_' + name]
        exc, mad = [], []
        for a, b in zip(ref, pics):
            exc.append(so.ink_exceptions(a, b))
            u = so.ink(a) | so.ink(b)
            mad.append(np.abs(a.astype(np.int64) - b.astype(np.int64))[u].mean() if u.any() else 0.0)
        print(name, 'ink exceptions (reference not met, oracle not met) per frame:', exc, 'colour MAD on the union of ink:', mad)
        assert max(max(e) for e in exc) <= INK_CAP, exc
        out['ink_exc_' + name], out['colour_mad_' + name] = np.array(exc), np.array(mad)
        vs = so.view_params(style=style, h=E2E['H'], w=E2E['W'], **kw)
        o64 = so.render_clip(vs, body, obj, gt_b, gt_o, T_GT, PRED_FROM, bones, wires, frames=E2E['frames'])
        o32 = so.render_clip(vs, body, obj, gt_b, gt_o, T_GT, PRED_FROM, bones, wires, frames=E2E['frames'], dtype=np.float32)
        share = (o64 != o32).any(-1).reshape(len(o64), -1).mean(1)
        print(name, 'float32 setup vs float64 setup, differing pixel share per image:', share)
        assert share.max() <= CAP / 4
        out['e2e_rgb_' + name], out['e2e_share32_' + name] = o64, share


def main():
    out = {}
    record_reference(sys.argv[1], out)
    oracle_part(out)
    path = os.path.join(HERE, 'skel_render.npz')
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 1000000, os.path.getsize(path)
    print(path, os.path.getsize(path))


if __name__ == '__main__':
    main()
