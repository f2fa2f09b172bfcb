"""Pictures of a skeleton-mode clip: ``visualize_skeleton`` and ``visualize_skeleton_pred_gt`` of the reference's render/viz_helper.py, and the
``visualize`` method of its skeleton trainers, on the HIP line / disc rasteriser of csrc/skeleton_render.hip.

The reference draws with matplotlib's 3D axes.  The CAMERA here is matplotlib's, restated (``make_view``; per-frame limits inside the kernel): figure
of w x h pixels at ``dpi``, subplot box (.125, .9, .11, .88) shrunk to a centred square, 2D view limits +-0.095, perspective of focal length 1 from
distance 10, box aspect (4, 4, 3), limits recomputed for every frame from what the frame draws.  The PICTURE is this package's own rasterisation
(4 x 4 sub-samples, integer "over"): it agrees with Agg's in where the ink is, not in its anti-aliasing.  Not drawn: axes, ticks, text (the reference
turns them off).
"""
import ctypes as C
import math
import os
import numpy as np
import torch
from . import _lib

# render/viz_helper.py:11-15 `connections`: the 18 bones of the 21-joint body (joints 19, 20 carry no bone)
BONES = ((0, 1), (1, 2), (2, 3), (3, 4), (2, 5), (5, 6), (6, 7), (7, 8), (2, 9), (9, 10), (10, 11), (11, 12), (0, 13), (13, 14), (14, 15), (0, 16), (16, 17),
         (17, 18))
# render/viz_helper.py:17-28 `obj_connects`: wires between the 12 object keypoints, per object name
_CHAIR = ((4, 9), (2, 11), (1, 8), (0, 10), (0, 1), (1, 4), (2, 4), (2, 3), (3, 5), (0, 2), (0, 5), (7, 3), (7, 5), (7, 0), (7, 2), (0, 6), (6, 1), (6, 2), (6, 4))
_BOX = ((4, 5), (5, 9), (5, 11), (2, 5), (2, 6), (2, 0), (2, 11), (9, 4), (9, 11), (9, 1), (9, 10), (1, 0), (1, 7), (0, 6), (3, 4), (3, 5), (3, 10), (3, 8), (8, 6),
        (8, 7), (8, 10), (3, 6), (0, 7), (1, 11), (4, 10), (10, 7))
OBJ_WIRES = {
    'chair4': ((1, 2), (1, 4), (2, 4), (1, 0), (0, 2), (0, 5), (5, 7), (0, 10), (2, 11), (4, 9), (1, 8), (2, 3), (5, 3), (4, 6), (0, 6), (0, 7), (2, 7), (3, 7)),
    'box2': ((2, 11), (2, 5), (9, 11), (1, 0), (1, 7), (8, 10), (3, 4), (4, 9), (3, 8), (7, 8), (1, 11), (3, 5), (6, 2), (3, 6), (2, 0), (4, 10), (6, 8), (1, 2),
             (7, 10), (7, 0), (4, 5), (5, 11), (0, 6), (6, 7), (1, 9), (9, 10), (5, 9), (7, 9)),
    'board': ((3, 6), (6, 5), (3, 9), (5, 9), (5, 1), (1, 4), (2, 4), (1, 7), (0, 7), (0, 11), (11, 10), (8, 10), (2, 8), (2, 9)),
    'chair2': _CHAIR,
    'box3': _BOX,
    'table': ((0, 2), (2, 3), (3, 4), (4, 0), (0, 1), (2, 1), (1, 10), (3, 5), (2, 5), (5, 8), (4, 6), (3, 6), (6, 7), (0, 11), (4, 11), (11, 9)),
    'chair': _CHAIR,
    'box': _BOX,
    'tripod': ((3, 5), (4, 6), (0, 1), (7, 10), (7, 11), (9, 7), (1, 8), (4, 8), (5, 8), (8, 2), (8, 7), (7, 10)),
}
NB, NO = 21, 12
# RGBA 8 bit, in the slots of idf_skel_view.colour.  matplotlib's 'b', 'w', 'r', 'g' (g = (0, 0.5, 0) -> 128) / seagreen, salmon, lightgrey at 0.8, dimgrey at 0.5
PLAIN_COLOURS = ((0, 0, 255, 255), (255, 255, 255, 255), (255, 0, 0, 255), (0, 128, 0, 255), (0, 0, 0, 0))
PREDGT_COLOURS = ((46, 139, 87, 204), (255, 255, 255, 255), (250, 128, 114, 204), (211, 211, 211, 204), (105, 105, 105, 128))
PRED_FROM = 11                           # viz_helper.py:95 `if frame>10`
GIF_FRAME_MS = 50                        # FuncAnimation(interval=50).save with the Pillow writer: 50 ms per frame, loop 0
DEFAULT_WORKSPACE = 64 << 20
DIST, VIEW_HALF, VIEW_SPAN = 10.0, 0.095, 0.185          # eye distance; 2D view limits +-0.95 / dist, width 0.9 / dist + 2 * 0.05 / dist


def figure_box(h, w):
    """the axes box in display pixels (x0, y0 from the BOTTOM, width, height): the default subplot box shrunk to a centred square"""
    x0, x1, y0, y1 = 0.125 * w, 0.9 * w, 0.11 * h, 0.88 * h
    s = min(x1 - x0, y1 - y0)
    return x0 + (x1 - x0 - s) / 2, y0 + (y1 - y0 - s) / 2, s, s


def _norm_angle(a):
    a = (a + 180.0) % 360.0 - 180.0                      # art3d._norm_angle: into (-180, 180]
    return 180.0 if a == -180.0 else a


def make_view(style='plain', elev=117.0, azim=-88.0, roll=0.0, vertical_axis='z', h=480, w=640, dpi=100.0, pred_from=PRED_FROM):
    """idf_skel_view: the part of matplotlib's camera that does not depend on the frame, computed in double.
    get_proj(): box aspect (4, 4, 3) * 1.8294640721620434 * 25 / 24 / |(4, 4, 3)| rolled to the vertical axis; eye = aspect / 2 + dist * (cos e cos a,
    cos e sin a, sin e) rolled likewise; w = unit(eye - centre), u = unit(V x w) with V = -+ the vertical axis (- when |elev| > 90 deg), v = w x u;
    a roll turns u, v about w by -roll."""
    if style not in ('plain', 'predgt') or vertical_axis not in ('x', 'y', 'z'):
        raise ValueError("make_view: style 'plain' or 'predgt', vertical_axis 'x', 'y' or 'z'")
    if not (1 <= h <= _lib.RENDER_MAX_DIM and 1 <= w <= _lib.RENDER_MAX_DIM and dpi > 0):
        raise ValueError('make_view: h, w must be in 1..%d and dpi positive' % _lib.RENDER_MAX_DIM)
    va = 'xyz'.index(vertical_axis)
    ba = np.array([4.0, 4.0, 3.0])
    aspect = np.roll(ba * (1.8294640721620434 * 25 / 24 / np.linalg.norm(ba)), va - 2)
    centre = 0.5 * aspect
    er, ar = np.deg2rad(elev), np.deg2rad(azim)
    eye = centre + DIST * np.roll([np.cos(er) * np.cos(ar), np.cos(er) * np.sin(ar), np.sin(er)], va - 2)
    V = np.zeros(3)
    V[va] = -1.0 if abs(np.deg2rad(_norm_angle(elev))) > np.pi / 2 else 1.0
    wv = (eye - centre) / np.linalg.norm(eye - centre)
    u = np.cross(V, wv)
    u /= np.linalg.norm(u)
    v = np.cross(wv, u)
    rr = np.deg2rad(_norm_angle(roll))
    if rr != 0:                                          # Rodrigues about w by -roll (proj3d._rotation_about_vector)
        turn = lambda x: x * np.cos(-rr) + np.cross(wv, x) * np.sin(-rr) + wv * np.dot(wv, x) * (1 - np.cos(-rr))
        u, v = turn(u), turn(v)
    sv = _lib.SkelView()
    for i, a in enumerate((u, v, wv)):
        sv.view[4 * i:4 * i + 3] = [float(x) for x in a]
        sv.view[4 * i + 3] = float(-np.dot(a, eye))
    sv.aspect[:] = [float(x) for x in aspect]
    # the z margin of a perspective axes is 0 until a scatter raises it to 0.05 (Axes3D.clear / scatter): the pred / gt style has no scatter
    sv.margin[:] = [0.05, 0.05, 0.05 if style == 'plain' else 0.0]
    bx, by, bw, bh = figure_box(h, w)
    sub = _lib.RENDER_SUBPIX
    sv.dist = DIST
    sv.kx, sv.cx = bw / VIEW_SPAN * sub, (bx + VIEW_HALF / VIEW_SPAN * bw) * sub
    sv.ky, sv.cy = -bh / VIEW_SPAN * sub, (h - by - VIEW_HALF / VIEW_SPAN * bh) * sub
    sv.line_wd = int(np.rint(1.5 * dpi / 72.0 * sub))                               # lines.linewidth 1.5 pt
    sv.disc_wd = int(np.rint((math.sqrt(20.0) + 1.0) * dpi / 72.0 * sub))           # s = 20 pt^2 disc and the outer half of its 1 pt edge, both sides
    if not (1 <= sv.line_wd <= _lib.SKEL_WD_MAX and 1 <= sv.disc_wd <= _lib.SKEL_WD_MAX):
        raise ValueError('make_view: dpi %r gives a line or marker wider than %d / 16 pixels' % (dpi, _lib.SKEL_WD_MAX))
    sv.style = _lib.SKEL_PLAIN if style == 'plain' else _lib.SKEL_PREDGT
    sv.pred_from = int(pred_from)
    for i, c in enumerate(PLAIN_COLOURS if style == 'plain' else PREDGT_COLOURS):
        sv.colour[i][:] = c
    return sv


def _clips(x, n, name):
    """numpy array or tensor, [..., n, 3] or [..., 3 n] with 1 or 2 leading axes -> the tensor as [B, T, n, 3], still where and what it was (nothing is
    moved to the device before every argument has been checked)"""
    if isinstance(x, np.ndarray):
        if x.dtype.kind not in 'fiu':
            raise ValueError('%s: a numeric array expected, got dtype %s' % (name, x.dtype))
        x = torch.from_numpy(np.ascontiguousarray(x))
    if not isinstance(x, torch.Tensor) or x.is_complex() or x.dtype == torch.bool:
        raise ValueError('%s: a numeric numpy array or tensor expected' % name)
    sh = tuple(x.shape)
    if len(sh) >= 2 and sh[-1] == 3 and sh[-2] == n:
        lead = sh[:-2]
    elif len(sh) >= 1 and sh[-1] == 3 * n:
        lead = sh[:-1]
    else:
        raise ValueError('%s: [..., %d, 3] or [..., %d] expected, got %s' % (name, n, 3 * n, sh))
    if len(lead) not in (1, 2) or 0 in lead:
        raise ValueError('%s: one (T) or two (B, T) non-empty leading axes expected, got %s' % (name, sh))
    return x.reshape((lead if len(lead) == 2 else (1,) + lead) + (n, 3))


def _wire_table(obj_name, obj_connections):
    w = OBJ_WIRES.get(obj_name, ()) if obj_connections is None else obj_connections           # obj_connects.get(obj_name, [])
    w = np.asarray(w, np.int64).reshape(-1, 2) if len(w) else np.zeros((0, 2), np.int64)
    if len(w) > _lib.SKEL_MAX_WIRES or (w < 0).any() or (w >= NO).any():
        raise ValueError('object wires: at most %d pairs of keypoint indices in 0..%d' % (_lib.SKEL_MAX_WIRES, NO - 1))
    return w.astype(np.int32)


def render_skeleton_clips(body, obj, body_gt=None, obj_gt=None, *, style='plain', elev=117.0, azim=-88.0, roll=0.0, vertical_axis=None, obj_name='chair4',
                          obj_connections=None, pred_from=PRED_FROM, h=480, w=640, dpi=100, device='cuda', want_setup=False, workspace_bytes=None,
                          stage_ms=False):
    """interdiff_skeleton_render_frames on [B,T,...] (or [T,...]) clips -> dict(rgb uint8 [B,T,h,w,3] on the device, dropped, and setup / count / stage_ms
    when asked for).  style 'plain': visualize_skeleton's picture (vertical axis z); 'predgt': visualize_skeleton_pred_gt's (vertical axis y), the
    prediction drawn in frames >= pred_from, the ground truth [B,T_gt,...] in frames < T_gt.  ``workspace_bytes`` caps the workspace: the frames are
    then rendered in chunks, with identical bits."""
    lib = _lib.load()
    vertical_axis = vertical_axis or ('z' if style == 'plain' else 'y')
    view = make_view(style, elev, azim, roll, vertical_axis, h, w, dpi, pred_from)
    b, o = _clips(body, NB, 'body'), _clips(obj, NO, 'obj')
    if o.shape[:2] != b.shape[:2]:
        raise ValueError('body and obj: the same clips and frames expected, got %s and %s' % (tuple(b.shape), tuple(o.shape)))
    B, T = b.shape[:2]
    bg = og = wires = None
    T_gt, n_wires = 0, 0
    if style == 'predgt':
        wt = _wire_table(obj_name, obj_connections)
        n_wires = len(wt)
        if (body_gt is None) != (obj_gt is None):
            raise ValueError('body_gt and obj_gt come together')
        if body_gt is not None:
            bg, og = _clips(body_gt, NB, 'body_gt'), _clips(obj_gt, NO, 'obj_gt')
            if bg.shape[0] != B or og.shape[:2] != bg.shape[:2]:
                raise ValueError('body_gt / obj_gt: %d clips of the same length expected, got %s and %s' % (B, tuple(bg.shape), tuple(og.shape)))
            T_gt = bg.shape[1]
    elif body_gt is not None or obj_gt is not None:
        raise ValueError("the 'plain' style draws one skeleton: no ground truth")
    put = lambda x: None if x is None else x.to(device=device, dtype=torch.float32).contiguous()       # a device tensor stays where it is
    b, o, bg, og = put(b), put(o), put(bg), put(og)
    dev = b.device
    wires = torch.from_numpy(wt).to(dev).contiguous() if n_wires else None
    one, full = lib.interdiff_skeleton_render_frames_workspace_bytes(1), lib.interdiff_skeleton_render_frames_workspace_bytes(B * T)
    nbytes = min(full, max(one, DEFAULT_WORKSPACE if workspace_bytes is None else int(workspace_bytes)))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    rgb = torch.empty(B, T, h, w, 3, dtype=torch.uint8, device=dev)
    setup = torch.empty(B, T, _lib.SKEL_MAX_REC, _lib.SKEL_REC_INTS, dtype=torch.int32, device=dev) if want_setup else None
    count = torch.empty(B, T, dtype=torch.int32, device=dev) if want_setup else None
    dropped, ms = C.c_int64(0), (C.c_float * 2)()
    _lib.check(lib.interdiff_skeleton_render_frames(C.byref(view), _lib.dptr(b), _lib.dptr(o), _lib.dptr(bg, allow_none=True), _lib.dptr(og, allow_none=True),
                                                    _lib.dptr(wires, allow_none=True), n_wires, B, T, T_gt, h, w, _lib.dptr(rgb),
                                                    _lib.dptr(setup, allow_none=True), _lib.dptr(count, allow_none=True), C.byref(dropped),
                                                    ms if stage_ms else None, _lib.dptr(ws), nbytes, _lib.stream()), 'skeleton_render_frames')
    out = dict(rgb=rgb, dropped=int(dropped.value))
    if want_setup:
        out['setup'], out['count'] = setup, count
    if stage_ms:
        out['stage_ms'] = dict(setup=ms[0], raster=ms[1])
    return out


def raster_records(recs, count, h, w):
    """interdiff_skeleton_raster_records: the raster stage alone.  recs int32 device tensor [n, SKEL_MAX_REC, 8], the first ``count`` slots of every
    frame in draw order -> uint8 [n,h,w,3] on the device"""
    lib = _lib.load()
    if recs.dim() != 3 or tuple(recs.shape[1:]) != (_lib.SKEL_MAX_REC, _lib.SKEL_REC_INTS) or recs.dtype != torch.int32:
        raise ValueError('raster_records: int32 [n, %d, %d] expected' % (_lib.SKEL_MAX_REC, _lib.SKEL_REC_INTS))
    rgb = torch.empty(recs.shape[0], h, w, 3, dtype=torch.uint8, device=recs.device)
    _lib.check(lib.interdiff_skeleton_raster_records(_lib.dptr(recs), int(count), recs.shape[0], h, w, _lib.dptr(rgb), _lib.stream()), 'skeleton_raster_records')
    return rgb


def save_gif(frames, path, duration_ms=GIF_FRAME_MS):
    """uint8 [T,h,w,3] -> an animated GIF through PIL, ``duration_ms`` per frame, looping for ever.  A frame of at most 256 colours gets a palette that
    holds exactly its colours (the file then reproduces it bit for bit); any other frame is quantised by PIL."""
    from PIL import Image
    ims = []
    for f in np.asarray(frames):
        flat = f.reshape(-1, 3)
        cols, inv = np.unique(flat, axis=0, return_inverse=True)
        if len(cols) <= 256:
            im = Image.fromarray(inv.reshape(f.shape[:2]).astype(np.uint8), 'P')
            pal = np.zeros((256, 3), np.uint8)
            pal[:len(cols)] = cols
            im.putpalette(pal.reshape(-1).tolist())
        else:
            im = Image.fromarray(f).quantize(256)
        ims.append(im)
    ims[0].save(path, save_all=True, append_images=ims[1:], duration=duration_ms, loop=0, optimize=False, disposal=1)


def _gif_path(save_dir):
    return None if save_dir is None else os.fspath(save_dir)


def visualize_skeleton(skeledonData, objPoint, save_dir='./test.gif', *, h=480, w=640, dpi=100, device='cuda'):
    """render/viz_helper.py:29 visualize_skeleton: blue bones, red joint markers, green object keypoints, view elev 117 azim -88, limits per frame; the three
    white axis lines are drawn after the bones and overpaint what they cross.  skeledonData [T,21,3] or [T,63], objPoint [T,12,3] or [T,36] (numpy arrays
    or tensors) -> uint8 frames [T,h,w,3]; the GIF (50 ms per frame) is written unless ``save_dir`` is None."""
    out = render_skeleton_clips(_one_clip(skeledonData, NB, 'skeledonData'), _one_clip(objPoint, NO, 'objPoint'), style='plain', h=h, w=w, dpi=dpi, device=device)
    frames = out['rgb'][0].cpu().numpy()
    if save_dir is not None:
        save_gif(frames, _gif_path(save_dir))
    return frames


def _one_clip(x, n, name):
    sh = tuple(getattr(x, 'shape', ()))
    if not (len(sh) == 3 and sh[1:] == (n, 3)) and not (len(sh) == 2 and sh[1] == 3 * n):
        raise ValueError('%s: [T, %d, 3] or [T, %d] expected, got %s' % (name, n, 3 * n, sh))
    return x


def visualize_skeleton_pred_gt(skeledonData, objPoint, skeledonData_gt, objPoint_gt, save_dir='./test.gif', elev=117., azim=-88., roll=0.0, obj_name='chair4',
                               tmp_dir='./tmp', *, obj_connections=None, h=480, w=640, dpi=100, device='cuda'):
    """render/viz_helper.py:77 visualize_skeleton_pred_gt as shipped (its GIF branch): vertical axis y, the view (elev, azim, roll); the white axis lines
    first; the prediction (seagreen bones, salmon object wires, alpha 0.8) in frames > 10; the ground truth (lightgrey 0.8, dimgrey 0.5) while
    frame < len(objPoint_gt).  ``obj_name`` picks the object's wires (OBJ_WIRES; an unknown name draws none), ``obj_connections`` overrides the lookup;
    ``tmp_dir`` is accepted and unused (it serves the reference's PNG strip, which is not built).  The file is ``save_dir[:-4] + '.gif'`` as in the
    reference.  -> uint8 frames [T,h,w,3]."""
    out = render_skeleton_clips(_one_clip(skeledonData, NB, 'skeledonData'), _one_clip(objPoint, NO, 'objPoint'), _one_clip(skeledonData_gt, NB, 'skeledonData_gt'),
                                _one_clip(objPoint_gt, NO, 'objPoint_gt'), style='predgt', elev=elev, azim=azim, roll=roll, obj_name=obj_name,
                                obj_connections=obj_connections, h=h, w=w, dpi=dpi, device=device)
    frames = out['rgb'][0].cpu().numpy()
    if save_dir is not None:
        save_gif(frames, _gif_path(save_dir)[:-4] + '.gif')
    return frames


def visualize(body_pred, obj_pred, body_gt, obj_gt, save_dir, mode, epoch, batch_idx, sample_idx=None, **kw):
    """The ``visualize`` method of the skeleton trainers (train_correction_skeleton.py:156-180, train_diffusion_skeleton.py:298-322): clip 0 of a [T,B,...]
    batch, prediction and ground truth each through ``visualize_skeleton``, written to ``save_dir/render/{mode}_{epoch}_{batch_idx}[_{sample_idx}]_p.gif``
    and ``..._gt.gif``; the gt file is skipped when sample_idx > 0.  -> the list of files written."""
    T = body_pred.shape[0]
    pick = lambda x, n: (x.detach() if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x)))[:, 0].reshape(T, n, 3)
    folder = os.path.join(os.fspath(save_dir), 'render')
    os.makedirs(folder, exist_ok=True)
    stem = '%s_%s_%s' % (mode, epoch, batch_idx) + ('' if sample_idx is None else '_%s' % sample_idx)
    written = [os.path.join(folder, stem + '_p.gif')]
    visualize_skeleton(pick(body_pred, NB), pick(obj_pred, NO), written[0], **kw)
    if sample_idx is not None and sample_idx > 0:        # no need to render gt many times
        return written
    written.append(os.path.join(folder, stem + '_gt.gif'))
    visualize_skeleton(pick(body_gt, NB), pick(obj_gt, NO), written[1], **kw)
    return written
