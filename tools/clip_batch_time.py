"""Timing of a training batch from the device-resident clip set (``dataset.DeviceClipSet.assemble``, csrc/clip_batch.hip) beside the host route the package offered
before it and beside the trainer steps the batch feeds.  One process, the sides alternating block by block (``--blocks`` blocks of ``--calls`` calls each, after a
warm-up block that is dropped), per side the median of the block medians and their range, milliseconds.  Every call is a host clock around work that ends in a
device synchronise, so host arithmetic, uploads and kernels all count.  Not on the product path.

    python tools/clip_batch_time.py [--blocks 7] [--calls 10] [--json profiles/clip_batch_time.json]

Shapes: B = 16 and 32, T = 35 (past 10 + future 25), P = 2048, V = 6890; 4 synthetic sequences of 300 frames on the synthetic body model, ~200 body contacts a frame.  Sides:
  assemble_ms / assemble_body_ms            ``assemble(body=False)`` / ``assemble(body=True)`` (the latter includes the SMPL forward and the vertex normals of T B frames)
  host_canonicalize_ms, host_labels_ms,     ``data.canonicalize_clip`` x B, ``data.clip_labels`` x B, ``data.collate_raw`` (with the upload),
  host_collate_ms, host_body_records_ms     ``correction_losses.body_records`` (label upload, SMPL forward, normals, 7-way cat, marker gather)
  finetune_step_ms / denoiser_step_ms       ``CorrectionFineTuner.training_step(batch, 0)`` / ``DenoiserTrainer(train_encoder=True).training_step(batch)`` on the assembled batch
Reported per shape: host_route_ms = the four host sides added (host_route_nobody_ms: the first three), and whether ``assemble`` is below the shortest trainer step."""
import argparse
import json
import os
import sys
import time
import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)
from interdiff_amd import synthetic as syn, data as D, correction_losses as cl      # noqa: E402
from interdiff_amd.dataset import DeviceClipSet                                      # noqa: E402
from interdiff_amd.smpl import SMPL_Layer                                            # noqa: E402
from interdiff_amd.mdm_train import DenoiserTrainer                                  # noqa: E402
from interdiff_amd.correction_finetune import CorrectionFineTuner                   # noqa: E402

DEV, PAST, FUT, P, F, N_SEQ = 'cuda', 10, 25, 2048, 300, 4


def sequences(rs):
    out = []
    for i in range(N_SEQ):
        poses = np.float32(rs.uniform(-0.3, 0.3, (F, 156)))
        poses[:, :3] = np.float32(rs.uniform(-1.5, 1.5, (F, 3)))
        trans = np.float32(np.cumsum(rs.uniform(-0.01, 0.01, (F, 3)), axis=0))
        out.append(dict(poses=poses, betas=np.float32(rs.uniform(-1, 1, (1, 10)).repeat(F, 0)), trans=trans, obj_angles=rs.uniform(-1.5, 1.5, (F, 3)),
                        obj_trans=trans.astype(np.float64) + rs.uniform(-0.5, 0.5, (F, 3)), obj_points=np.float32(rs.standard_normal((P, 6)) * 0.2),
                        obj_contact_label=[rs.choice(P, rs.randint(0, 60), replace=False) for _ in range(F)],
                        contact_label=[rs.choice(6890, rs.randint(100, 300), replace=False) for _ in range(F)],
                        ground_joint_label=np.full(F, 10, np.int64), gender='male', obj_name='box', seq_name='Date01_Sub01_box_%d' % i))
    return out


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--blocks', type=int, default=7)
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    rs = np.random.RandomState(2024)
    seqs = sequences(rs)
    layer = SMPL_Layer({k: (torch.from_numpy(v) if isinstance(v, np.ndarray) else v) for k, v in syn.smplh_model(7).items()}, device=DEV)
    cs = DeviceClipSet(seqs, layer, PAST, FUT, device=DEV)
    jt = cs.t['joints'].cpu().numpy().reshape(N_SEQ, F, 3, 3)
    msd = {k: torch.from_numpy(v) for k, v in syn.mdm_state_dict(seed=233).items()}
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'correction_ckpt.npz'))
    osd = {k: torch.from_numpy(z[k]) for k in z.files}
    T = PAST + FUT
    res = dict(device=torch.cuda.get_device_name(0), blocks=a.blocks, calls=a.calls, T=T, P=P, V=cs.V, frames_per_sequence=F, sequences=N_SEQ, shapes=[])
    for B in (16, 32):
        ids = [int(i) for i in rs.randint(0, N_SEQ, B)]
        starts = [int(s) for s in rs.randint(0, F - T + 1, B)]
        batch = cs.assemble(ids, starts)
        ft, den = CorrectionFineTuner(osd, T=T, past_len=PAST, device=DEV), DenoiserTrainer(msd, device=DEV, past_len=PAST, train_encoder=True)
        pts = np.stack([seqs[k]['obj_points'][:, :3] for k in ids])
        host = {}

        def canon():
            host['clips'] = [D.canonicalize_clip(seqs[k], jt[k, :, 0], s, PAST, FUT) for k, s in zip(ids, starts)]

        def labels():
            host['labels'] = [D.clip_labels(seqs[k], c, jt[k, :, 1], jt[k, :, 2], s, PAST, FUT) for k, s, c in zip(ids, starts, host['clips'])]

        def collate():
            host['raw'] = D.collate_raw(host['clips'], pts, device=DEV)

        def records():
            raw = host['raw']
            lab = torch.from_numpy(np.stack([l['contact_label'] for l in host['labels']], axis=1))
            cl.body_records(layer, torch.cat([raw['body_pose'], raw['hand_pose']], dim=2), raw['beta'], raw['body_trans'], lab)
        sides = dict(assemble_ms=lambda: cs.assemble(ids, starts, body=False), assemble_body_ms=lambda: cs.assemble(ids, starts, body=True),
                     host_canonicalize_ms=canon, host_labels_ms=labels, host_collate_ms=collate, host_body_records_ms=records,
                     finetune_step_ms=lambda: ft.training_step(batch, 0), denoiser_step_ms=lambda: den.training_step(batch, seed=1))
        row = dict(B=B, **alternate(sides, a.blocks, a.calls))
        med = lambda k: row[k]['median']
        row['host_route_nobody_ms'] = med('host_canonicalize_ms') + med('host_labels_ms') + med('host_collate_ms')
        row['host_route_ms'] = row['host_route_nobody_ms'] + med('host_body_records_ms')
        row['shortest_step_ms'] = min(med('finetune_step_ms'), med('denoiser_step_ms'))
        row['assemble_below_shortest_step'] = bool(med('assemble_ms') < row['shortest_step_ms'])
        row['assemble_body_below_shortest_step'] = bool(med('assemble_body_ms') < row['shortest_step_ms'])
        row['human_verts_mb'] = T * B * cs.V * 7 * 4 / 1e6
        res['shapes'].append(row)
        print('B = %d, T = %d, P = %d, V = %d on %s' % (B, T, P, cs.V, res['device']))
        for k in sides:
            print('  %-28s %9.3f  [%.3f, %.3f]' % (k, row[k]['median'], row[k]['lo'], row[k]['hi']))
        print('  host route (no body / body)  %9.3f / %.3f   shortest trainer step %.3f   assemble below it: %s (with body: %s)'
              % (row['host_route_nobody_ms'], row['host_route_ms'], row['shortest_step_ms'], row['assemble_below_shortest_step'], row['assemble_body_below_shortest_step']))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(res, open(a.json, 'w'), indent=1, sort_keys=True)


if __name__ == '__main__':
    main()
