"""hip-event timing of the mesh renderer (interdiff_amd/render.py, csrc/render.hip); not on the product path.

    python tools/render_time.py [--reps 5] [--json profiles/render_time.json]

Body: the closed ellipsoid of tests/render_oracle.py (V = 6890, F = 13776); object: a 2048-face ellipsoid turning beside it; the reference's ground.
4 views at 512 x 512, the default workspace cap of render.py (the images go through in chunks).  Warmed medians of ``--reps`` calls of
``render_frames`` (scene building and vertex normals are outside: they are the existing kernels) for
  * one clip at T = 35 and at T = 100,
  * 16 clips of T = 35 one after the other (16 scenes; one call each),
and the per-stage split of one call (setup + bin count | scan + fill | tile + resolve: the launcher's own hip events, a separate call because
they synchronise per chunk; tile and resolve are ONE kernel, so the JSON's ``tile_resolve`` cannot be split further).  Per image = per view of a frame."""
import argparse
import json
import os
import sys
import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)
from interdiff_amd import render                                      # noqa: E402
from tests import render_oracle as ro                                 # noqa: E402

DEV = 'cuda'
H = W = 512
VIEWS = 4


def clip(T, seed):
    rs = np.random.RandomState(seed)
    bv, bf = ro.ellipsoid()
    ov, of = ro.ellipsoid(radii=(0.2, 0.15, 0.12), rings=32, segs=32)
    walk = np.cumsum(rs.uniform(-0.01, 0.02, (T, 3)) * np.array([1, 0.1, 1]), axis=0).astype(np.float32)
    body = bv[None] + walk[:, None]
    aa = np.stack([np.linspace(0, 1.5, T), np.full(T, 0.3), np.linspace(0, -0.7, T)], axis=1)
    R = ro.rodrigues(aa).astype(np.float32)
    tr = (walk + np.array([0.45, 0.1, 0.1], np.float32)).astype(np.float32)
    return body, bf, ov, of, R, tr


def median_ms(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--json', default=os.path.join(ROOT, 'profiles', 'render_time.json'))
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    res = dict(H=H, W=W, views=VIEWS, reps=a.reps, pixels_per_image=H * W, workspace_cap_bytes=render.DEFAULT_WORKSPACE)
    for T, seed in ((35, 0), (100, 1)):
        body, bf, ov, of, R, tr = clip(T, seed)
        scene, meshes, _ = render.build_clip(body, bf, ov, of, past_len=10, obj_R=R, obj_t=tr, device=DEV)
        res['triangles_per_image'] = int(sum(m.faces.shape[0] for m in meshes))
        n_img = T * VIEWS
        ms = median_ms(lambda: render.render_frames(scene, meshes, T, VIEWS, H, W), a.reps)
        st = render.render_frames(scene, meshes, T, VIEWS, H, W, stage_ms=True)['stage_ms']
        res['clip_T%d' % T] = dict(images=n_img, total_ms=ms, per_image_ms=ms / n_img, stage_ms_per_image={k: v / n_img for k, v in st.items()})
        print('T = %3d: %8.2f ms per call, %.3f ms per image; stages per image %s' % (T, ms, ms / n_img, res['clip_T%d' % T]['stage_ms_per_image']))
    clips = []
    for k in range(16):
        body, bf, ov, of, R, tr = clip(35, 10 + k)
        clips.append(render.build_clip(body, bf, ov, of, past_len=10, obj_R=R, obj_t=tr, device=DEV)[:2])

    def sixteen():
        for scene, meshes in clips:
            render.render_frames(scene, meshes, 35, VIEWS, H, W)
    ms = median_ms(sixteen, max(1, a.reps // 2), warm=1)
    res['sixteen_clips_T35'] = dict(images=16 * 35 * VIEWS, total_ms=ms, per_image_ms=ms / (16 * 35 * VIEWS))
    print('16 clips of T = 35: %8.2f ms, %.3f ms per image' % (ms, res['sixteen_clips_T35']['per_image_ms']))
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    json.dump(res, open(a.json, 'w'), indent=1, sort_keys=True)
    print('wrote', a.json)


if __name__ == '__main__':
    main()
