"""Timing of the skeleton dataset on the device (``skeleton_dataset.SkeletonClipSet``, csrc/skeleton_clip_batch.hip) beside the host routes it replaces and beside
the trainer steps a batch feeds.  One process, the sides alternating block by block (``--blocks`` blocks of ``--calls`` calls each, after a warm-up block that is
dropped), per side the median of the block medians and their range, milliseconds.  Every call is a host clock around work that ends in a device synchronise, so
host arithmetic, uploads and kernels all count.  Not on the product path.

    python tools/skeleton_dataset_time.py [--blocks 7] [--calls 10] [--videos 500] [--frames 2400] [--host-videos 20] [--json profiles/skeleton_dataset_time.json]

1. A batch: B = 32 and 64, T = 20, windows drawn from 40 synthetic videos of 1500 frames.  Sides:
     assemble_ms          ``assemble(ids, rows)``: the index upload and ONE launch -- the tuple and the token
     host_route_ms        what a DataLoader over the reference's window list does: stack B float64 windows (already materialised), ``.float()``, copy to the device
     finetune_step_ms / trainer_step_ms / denoiser_step_ms   one ``training_step`` of ``SkeletonFineTuner`` / ``SkeletonTrainer`` / ``SkeletonDenoiserTrainer``
2. Ingestion of a set of the reference's size: ``--videos`` videos of ``--frames`` frames (8 distinct synthetic videos, repeated).
     set_build_ms         ``SkeletonClipSet(videos)``: host concatenation, upload of the float64 arrays, the prepare launch, the report download (median of 3 after one)
     prepare_kernel_ms    the prepare launch alone on arrays already uploaded (median of 5 after one)
     host_ingest_ms_per_video   the reference's ingestion restated in numpy / scipy the way it is written -- a Python loop over every frame for the quaternion
                          signs, recover_init_obj, the discrepancy, then every window sliced and copied -- on ``--host-videos`` videos; host_ingest_ms_all_videos is that
                          figure times ``--videos``: an EXTRAPOLATION, said so wherever it is quoted
"""
import argparse
import json
import os
import sys
import time
import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)
from interdiff_amd import _lib, synthetic as syn, skeleton_train as st                # noqa: E402
from interdiff_amd.skeleton_dataset import SkeletonClipSet                            # noqa: E402
from interdiff_amd.skeleton_finetune import SkeletonFineTuner                         # noqa: E402
from interdiff_amd.skeleton_mdm_train import SkeletonDenoiserTrainer                  # noqa: E402

DEV, STRIDE, WINDOW, T = 'cuda', 12, 240, 20


def make_video(rs, F, name):
    from scipy.spatial.transform import Rotation
    q = np.cumsum(0.02 * rs.standard_normal((F, 4)), axis=0) + rs.standard_normal(4)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    q *= np.where(rs.uniform(size=(F, 1)) < 0.3, -1.0, 1.0)                           # sign flips, as the raw data has them
    trans = np.cumsum(0.004 * rs.standard_normal((F, 3)), axis=0)
    zero = 0.3 * rs.standard_normal((12, 3))
    obj = np.einsum('fij,kj->fki', Rotation.from_quat(q).as_matrix(), zero) + trans[:, None]
    skeleton = 0.4 * rs.standard_normal((1, 21, 3)) + np.cumsum(0.004 * rs.standard_normal((F, 21, 3)), axis=0)
    return dict(skeleton=skeleton, obj=obj, pose=np.concatenate([trans, q], axis=1), contact=np.ones((F, 1)), filename=name, obj_name=name.split('_')[1])


def host_ingest(video):
    """data/dataset_skeleton.py get_sequences as it is written, in this tool's own words: -> the list of windows (float64 copies)."""
    from scipy.spatial.transform import Rotation
    skel, obj, pose = video['skeleton'], video['obj'], video['pose']
    F = len(pose)
    p0, o0 = pose[0], obj[0]
    zero = (Rotation.from_quat(p0[3:]).inv().as_matrix()[None] @ (o0 - p0[None, :3])[:, :, None])[:, :, 0]
    rows = pose[::STRIDE]
    pred = rows[:, None, :3, None] + Rotation.from_quat(rows[:, 3:]).as_matrix()[:, None] @ zero[None, :, :, None]
    discrepancy = np.linalg.norm(pred[..., 0] - obj[::STRIDE], axis=-1).mean()
    fixed = pose.copy()
    for i in range(F - 1):                                                            # one Python iteration per full-rate frame
        if np.linalg.norm(fixed[i, 3:] - fixed[i + 1, 3:]) > np.linalg.norm(fixed[i, 3:] + fixed[i + 1, 3:]):
            fixed[i + 1, 3:] = -fixed[i + 1, 3:]
    windows, start = [], 0
    while start + WINDOW < F:
        sl = slice(start, start + WINDOW, STRIDE)
        windows.append((skel[sl].copy(), obj[sl].copy(), fixed[sl].copy(), zero))
        start += STRIDE
    return windows, discrepancy


def block_ms(fn, calls):
    out = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(out))


def alternate(sides, blocks, calls):
    meds = {k: [] for k in sides}
    for blk in range(blocks + 1):                                       # block 0 warms every side up and is dropped
        for k, fn in sides.items():
            m = block_ms(fn, calls)
            if blk:
                meds[k].append(m)
    return {k: dict(median=float(np.median(v)), lo=float(min(v)), hi=float(max(v))) for k, v in meds.items()}


def spread(v):
    return dict(median=float(np.median(v)), lo=float(min(v)), hi=float(max(v)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--blocks', type=int, default=7)
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--videos', type=int, default=500)
    ap.add_argument('--frames', type=int, default=2400)
    ap.add_argument('--host-videos', type=int, default=20)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    rs = np.random.RandomState(2025)
    res = dict(device=torch.cuda.get_device_name(0), blocks=a.blocks, calls=a.calls, T=T, stride=STRIDE, window=WINDOW, row_bytes=106 * 4, shapes=[])

    # 1. a batch
    n_vid, F = 40, 1500
    videos = [make_video(rs, F, 'sub%d_box_%03d' % (i, i)) for i in range(n_vid)]
    cs = SkeletonClipSet(videos, device=DEV)
    idx = cs.index()
    held = {}                                                                         # (video, row) -> the reference's materialised float64 window
    fixed = [host_ingest(v)[0] for v in videos]
    for k, row, _ in idx.entries:
        held[(k, row)] = fixed[k][row]
    msd = {k: torch.from_numpy(v) for k, v in syn.skeleton_mdm_state_dict(1106).items()}
    ck = dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'skel_ckpt.npz')))
    res.update(batch_videos=n_vid, batch_frames_per_video=F, windows=len(idx), resident_table_mb=cs.t['table'].numel() * 4 / 1e6)
    for B in (32, 64):
        pick = [idx[int(i)] for i in rs.choice(len(idx), B, replace=False)]
        ids, rows = [k for k, _, _ in pick], [r for _, r, _ in pick]
        batch = cs.assemble(ids, rows)
        ft, tr, den = SkeletonFineTuner(ck, device=DEV), st.SkeletonTrainer(st.init_state_dict(11), seed=5, device=DEV), SkeletonDenoiserTrainer(msd, device=DEV)

        def host_route():
            wins = [held[(k, r)] for k, r in zip(ids, rows)]
            return [torch.stack([torch.from_numpy(w[i]) for w in wins]).float().to(DEV) for i in range(4)]
        got = host_route()
        assert all(torch.equal(got[i], batch[i]) for i in range(3)), 'the two routes must give the same batch'
        sides = dict(assemble_ms=lambda: cs.assemble(ids, rows), host_route_ms=host_route, finetune_step_ms=lambda: ft.training_step(batch),
                     trainer_step_ms=lambda: tr.training_step(batch), denoiser_step_ms=lambda: den.training_step(batch, seed=1))
        row = dict(B=B, **alternate(sides, a.blocks, a.calls))
        med = lambda k: row[k]['median']
        row['shortest_step_ms'] = min(med('finetune_step_ms'), med('trainer_step_ms'), med('denoiser_step_ms'))
        row['assemble_below_shortest_step'] = bool(med('assemble_ms') < row['shortest_step_ms'])
        row['batch_kb'] = (B * T * 106 * 2 + B * 36) * 4 / 1e3                        # the tuple and the token
        res['shapes'].append(row)
        print('B = %d, T = %d on %s' % (B, T, res['device']))
        for k in sides:
            print('  %-22s %9.3f  [%.3f, %.3f]' % (k, row[k]['median'], row[k]['lo'], row[k]['hi']))
        print('  shortest trainer step %.3f   assemble below it: %s' % (row['shortest_step_ms'], row['assemble_below_shortest_step']))
    del cs, held, fixed, videos

    # 2. ingestion at the reference's size
    base = [make_video(rs, a.frames, 'sub%d_box_%03d' % (i, i)) for i in range(8)]
    videos = [base[i % 8] for i in range(a.videos)]
    build = []
    for rep in range(4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        big = SkeletonClipSet(videos, device=DEV)
        torch.cuda.synchronize()
        if rep:
            build.append(1e3 * (time.perf_counter() - t0))
        if rep < 3:
            del big
    n, J, P = a.videos, 21, 12
    cat = lambda k, w: torch.from_numpy(np.concatenate([v[k].reshape(a.frames, w) for v in videos])).to(DEV)
    raw = [cat('skeleton', 63), cat('obj', 36), cat('pose', 7), cat('contact', 1)]
    seq_off = torch.arange(n + 1, dtype=torch.int64, device=DEV) * a.frames
    table, zpo = torch.empty_like(big.t['table']), torch.empty_like(big.t['zero_pose_obj'])
    report, rc = torch.empty(n, 3, dtype=torch.float64, device=DEV), torch.empty(table.shape[0], dtype=torch.float64, device=DEV)
    lib = _lib.load()

    def prepare():
        _lib.check(lib.interdiff_skeleton_video_prepare(*[_lib.dptr(x) for x in raw], _lib.dptr(seq_off), _lib.dptr(big.t['row_off']), n, J, P, STRIDE, _lib.dptr(table),
                                                        _lib.dptr(zpo), _lib.dptr(report), _lib.dptr(rc), None, _lib.stream()), 'prepare')
    kern = [block_ms(prepare, 1) for _ in range(6)][1:]
    assert torch.equal(table, big.t['table']) and torch.equal(zpo, big.t['zero_pose_obj'])
    host = []
    for v in videos[:a.host_videos]:
        t0 = time.perf_counter()
        host_ingest(v)
        host.append(1e3 * (time.perf_counter() - t0))
    res['ingest'] = dict(videos=a.videos, frames_per_video=a.frames, rows=int(table.shape[0]), resident_table_mb=table.numel() * 4 / 1e6,
                         upload_mb=sum(x.numel() for x in raw) * 8 / 1e6, set_build_ms=spread(build), prepare_kernel_ms=spread(kern), host_videos=a.host_videos,
                         host_ingest_ms_per_video=spread(host), host_ingest_ms_all_videos_extrapolated=float(np.median(host)) * a.videos)
    g = res['ingest']
    print('ingestion: %d videos x %d frames: set build %.1f ms [%.1f, %.1f], prepare kernel alone %.3f ms [%.3f, %.3f]; host ingestion %.1f ms per video '
          '(%d timed) = %.0f ms for all, extrapolated' % (a.videos, a.frames, g['set_build_ms']['median'], g['set_build_ms']['lo'], g['set_build_ms']['hi'],
                                                          g['prepare_kernel_ms']['median'], g['prepare_kernel_ms']['lo'], g['prepare_kernel_ms']['hi'],
                                                          g['host_ingest_ms_per_video']['median'], a.host_videos, g['host_ingest_ms_all_videos_extrapolated']))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(res, open(a.json, 'w'), indent=1, sort_keys=True)


if __name__ == '__main__':
    main()
