"""hip-event timing of the contact-label kernels (interdiff_amd/contact_labels.py, csrc/contact_labels.hip); not on the product path.

    python tools/contact_labels_time.py [--reps 20] [--json profiles/contact_labels_time.json] [--no-oracle] [--no-resources]

At the real shape -- N = 64 frames, V = 6890, F = 13776, P = 2048, the torus fixture of tests/contact_labels_oracle.py under 64 rigid poses --
the warmed median of ``--reps`` calls of ``contact_labels`` (the three launches of ``interdiff_contact_labels``; faces sorted beforehand), per call
and per frame, with the faces in Morton order (what the Python side does), in the mesh's own order and shuffled (no compact chunk: the
with / without-culling A/B).  Beside it:
  * the fp64 numpy oracle's time for one frame on 16 threads (the CPU restatement; igl itself is not installed and cannot be timed here),
  * the fp32 error of the winding number and of S against that oracle on the timed frame,
  * the share of (lane, 256-face chunk) pairs whose distance half the bounding-box test skips, recomputed on the host from the oracle's
    per-chunk distances for frame 0 (lane = point; a wave skips the instructions only when all 64 of its lanes skip: that share is given too).
The kernels' registers / LDS / scratch come from a device-only compile (``--no-resources`` skips that)."""
import argparse
import json
import os
import re
import subprocess
import sys
import time
import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)
from interdiff_amd import contact_labels as clab                      # noqa: E402
from tests import contact_labels_oracle as co                         # noqa: E402

DEV = 'cuda'


def median_us(fn, reps, warm=3):
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
        out.append(a.elapsed_time(b) * 1e3)
    return float(np.median(out))


def kernel_resources():
    from interdiff_amd.csrc import build
    src = os.path.join(ROOT, 'interdiff_amd', 'csrc', 'contact_labels.hip')
    try:
        asm = subprocess.run([build.HIPCC] + build.FLAGS + ['--cuda-device-only', '-S', '-o', '-', src], capture_output=True, text=True, check=True).stdout
    except Exception as e:                                            # pragma: no cover
        print('kernel resources unavailable: %r' % e)
        return None
    out = {}
    for blk in asm.split('- .agpr_count')[1:]:
        get = lambda k: int(re.search(r'\.%s:\s+(\d+)' % k, blk).group(1))
        name = re.search(r'\.name:\s+(\S+)', blk).group(1)
        short = next((k for k in ('ct_boxes_kernel', 'ct_points_kernel', 'ct_body_kernel') if k in name), name)
        out[short] = dict(vgprs=get('vgpr_count'), sgprs=get('sgpr_count'), lds_bytes=get('group_segment_fixed_size'),
                          scratch_bytes=get('private_segment_fixed_size'), vgpr_spills=get('vgpr_spill_count'))
    return out


def cull_share(points, verts, faces_sorted, chunk=256, wave=64):
    """Share of (point, chunk) pairs with box distance >= the running minimum, and of (wave, chunk) pairs where all lanes skip -- the kernel's
    test replayed in fp64 on the host."""
    p, v = np.asarray(points, np.float64), np.asarray(verts, np.float64)
    nch = -(-len(faces_sorted) // chunk)
    best = np.full(len(p), np.inf)
    skip = np.zeros((len(p), nch), bool)
    for c in range(nch):
        f = faces_sorted[c * chunk:(c + 1) * chunk]
        tri = v[f]
        lo, hi = tri.reshape(-1, 3).min(0), tri.reshape(-1, 3).max(0)
        e = np.maximum(np.maximum(lo - p, p - hi), 0.0)
        skip[:, c] = (e * e).sum(1) >= best
        d, _ = co.point_mesh(p, v, f, block=256, threads=16)
        best = np.minimum(best, d * d)
    waves = skip[:len(p) // wave * wave].reshape(-1, wave, nch).all(1)
    return float(skip.mean()), float(waves.mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--json', default=os.path.join(ROOT, 'profiles', 'contact_labels_time.json'))
    ap.add_argument('--no-resources', action='store_true')
    ap.add_argument('--no-oracle', action='store_true')
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    N, P = 64, 2048
    tv, tf = co.torus()
    case = co.torus_case()
    Rm, tm = co.rigid(77, N, shift=1.5)
    Ro, to = co.rigid(78, N, shift=0.03, angle=0.15)
    verts = torch.from_numpy(np.float32(np.einsum('vc,ndc->nvd', tv, Rm) + tm[:, None])).to(DEV)
    R = torch.from_numpy(np.float32(np.einsum('nab,nbc->nac', Rm, Ro).reshape(N, 9))).to(DEV)
    T = torch.from_numpy(np.float32(np.einsum('nab,nb->na', Rm, to) + tm)).to(DEV)
    cloud = torch.from_numpy(case['points']).to(DEV)
    V, F = tv.shape[0], tf.shape[0]
    res = dict(N=N, V=V, F=F, P=P, reps=a.reps)
    mesh = clab.label_mesh(tf, V, tv, DEV)                            # Morton order of the rest pose
    plain = type(mesh).__new__(type(mesh))
    plain.__dict__.update(mesh.__dict__)
    plain.faces = torch.from_numpy(tf.astype(np.int32)).to(DEV)       # the mesh's own order (grid rows: already fairly compact)
    shuffled = type(mesh).__new__(type(mesh))
    shuffled.__dict__.update(mesh.__dict__)
    shuffled.faces = torch.from_numpy(tf[np.random.RandomState(0).permutation(F)].astype(np.int32)).to(DEV)      # no compact chunk: nothing to cull
    outs = {}
    for tag, m in (('morton', mesh), ('mesh_order', plain), ('shuffled', shuffled)):
        fn = lambda: clab.contact_labels(verts, m, cloud, 0.02, R, T, return_signed_dist=True)
        outs[tag] = [o.cpu().numpy() for o in fn()]
        us = median_us(fn, a.reps)
        res['call_%s_us' % tag], res['per_frame_%s_us' % tag] = us, us / N
        print('%-11s %10.1f us per call of %d frames, %8.2f us per frame' % (tag, us, N, us / N))
    for tag in ('mesh_order', 'shuffled'):
        res['labels_differ_%s' % tag] = int((outs[tag][0] != outs['morton'][0]).sum() + (outs[tag][1] != outs['morton'][1]).sum())
    res['labelled_points_share'] = float(outs['morton'][0].mean())
    if not a.no_oracle:
        pts0 = co.pose_points(case['points'], R[0].cpu().numpy(), T[0].cpu().numpy())
        v0 = verts[0].cpu().numpy()
        t0 = time.time()
        d, w = co.point_mesh(pts0, v0, tf, threads=16)
        res['oracle_fp64_frame_s_16_threads'] = time.time() - t0
        S = (1.0 - 2.0 * w) * d
        S32 = outs['morton'][2][0].astype(np.float64)
        far = d >= 0.02
        res['max_abs_S_err'] = float(np.abs(S32 - S).max())
        res['max_S_err_over_band'] = float((np.abs(S32 - S) / (1e-5 + 2e-4 * d)).max())
        res['max_abs_w_err_where_d_ge_thres'] = float(np.abs((1.0 - S32 / d) / 2.0 - w)[far].max())
        res['labels_wrong_vs_oracle'] = int((outs['morton'][0][0] != (S < 0.02)).sum())
        print('oracle: %.2f s per frame (fp64 numpy, 16 threads); max |S32 - S64| %.3e (%.3f of the band), max |w32 - w64| %.3e' % (
            res['oracle_fp64_frame_s_16_threads'], res['max_abs_S_err'], res['max_S_err_over_band'], res['max_abs_w_err_where_d_ge_thres']))
        for tag, m in (('morton', mesh), ('mesh_order', plain), ('shuffled', shuffled)):
            lane, wave = cull_share(pts0, v0, m.faces.cpu().numpy().astype(np.int64))
            res['cull_lane_share_%s' % tag], res['cull_wave_share_%s' % tag] = lane, wave
            print('%-11s box test skips %.3f of (lane, chunk) pairs, %.3f of (wave, chunk) pairs' % (tag, lane, wave))
    if not a.no_resources:
        res['kernel_resources'] = kernel_resources()
        print(res['kernel_resources'])
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    json.dump(res, open(a.json, 'w'), indent=1, sort_keys=True)
    print('wrote', a.json)


if __name__ == '__main__':
    main()
