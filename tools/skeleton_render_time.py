"""Time the skeleton-clip renderer (interdiff_amd/skeleton_render.py) per stage and per 640 x 480 frame.

    python tools/skeleton_render_time.py [--out profiles/skeleton_render_time.json] [--repeats 20]
    python tools/skeleton_render_time.py --reference-cpu /path/to/reference/interdiff [--out ...]

The GPU part: one clip (T = 20) and 64 clips batched, both styles; a warm-up, then the median over ``--repeats`` calls of the library's own hip-event
stage times (setup, raster) and of the call's wall time with the frames left on the device.  ``--reference-cpu`` re-measures what the reference's
matplotlib functions take per clip on this host's CPU and MERGES the figures into the output file; it needs matplotlib and the reference tree, runs
no GPU code and is meant for a machine that has both.
"""
import argparse
import json
import os
import sys
import time
import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)
T, H, W = 20, 480, 640


def clip(B, seed=0):
    rs = np.random.RandomState(seed)
    body = rs.uniform([-0.35, -0.6, -0.35], [0.35, 0.9, 0.35], (B, 1, 21, 3)) + 0.01 * np.cumsum(rs.standard_normal((B, T, 21, 3)), 1)
    obj = rs.uniform([0.3, -0.3, 0.1], [0.8, 0.3, 0.6], (B, 1, 12, 3)) + 0.01 * np.cumsum(rs.standard_normal((B, T, 1, 3)), 1)
    return body.astype(np.float32), obj.astype(np.float32)


def gpu_part(repeats):
    import torch
    from interdiff_amd import skeleton_render as sr
    out = {}
    for B in (1, 64):
        body, obj = (torch.from_numpy(a).cuda() for a in clip(B))
        gb, go = (torch.from_numpy(a).cuda() for a in clip(B, seed=1))
        for style, args in (('plain', (body, obj)), ('predgt', (body, obj, gb, go))):
            run = lambda: sr.render_skeleton_clips(*args, style=style, h=H, w=W, stage_ms=True)
            for _ in range(3):
                run()
            torch.cuda.synchronize()
            setup, raster, wall = [], [], []
            for _ in range(repeats):
                t0 = time.perf_counter()
                r = run()                                   # the call synchronises (it reads the dropped counter back)
                wall.append((time.perf_counter() - t0) * 1e3)
                setup.append(r['stage_ms']['setup'])
                raster.append(r['stage_ms']['raster'])
            med = lambda x: float(np.median(x))
            out['%s_B%d' % (style, B)] = dict(clips=B, frames=B * T, setup_ms=med(setup), raster_ms=med(raster), wall_ms=med(wall),
                                              raster_us_per_frame=med(raster) * 1e3 / (B * T), wall_ms_per_clip=med(wall) / B,
                                              raster_ms_min=float(np.min(raster)), raster_ms_max=float(np.max(raster)), repeats=repeats)
            print(style, B, out['%s_B%d' % (style, B)], flush=True)
    out['device'] = torch.cuda.get_device_name(0)
    return out


def reference_cpu(ref_root):
    import importlib.util
    import tempfile
    import matplotlib
    matplotlib.use('Agg')
    spec = importlib.util.spec_from_file_location('viz_helper', os.path.join(ref_root, 'render', 'viz_helper.py'))
    vh = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(vh)
    (body, obj), (gb, go) = clip(1), clip(1, seed=1)
    tmp = tempfile.mkdtemp()
    out = dict(matplotlib=matplotlib.__version__)
    for name, run in (('visualize_skeleton', lambda p: vh.visualize_skeleton(body[0], obj[0], p)),
                      ('visualize_skeleton_pred_gt', lambda p: vh.visualize_skeleton_pred_gt(body[0], obj[0], gb[0], go[0], p, tmp_dir=os.path.join(tmp, 't')))):
        run(os.path.join(tmp, 'warm.gif'))
        ts = []
        for i in range(3):
            t0 = time.perf_counter()
            run(os.path.join(tmp, '%d.gif' % i))
            ts.append(time.perf_counter() - t0)
        out[name + '_s_per_clip'] = float(np.median(ts))
        print(name, ts, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'skeleton_render_time.json'))
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--reference-cpu', default=None, metavar='REFERENCE_ROOT')
    a = ap.parse_args()
    res = json.load(open(a.out)) if os.path.exists(a.out) else {}
    if a.reference_cpu:
        res['reference_cpu'] = reference_cpu(a.reference_cpu)
    else:
        res['gpu'] = gpu_part(a.repeats)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, 'w'), indent=1, sort_keys=True)
    print(a.out)


if __name__ == '__main__':
    main()
