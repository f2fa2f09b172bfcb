"""hip-event timing of the denoiser trainer WITH the PointNet++ object encoder in the pass (``DenoiserTrainer(train_encoder=True, train_pointnet=True)``,
csrc/pointnet2_train.hip), by the method of tools/mdm_train_time.py: one process, the sides alternating block by block (``--blocks`` blocks of ``--calls`` calls
each, after a warm-up block), per side the median of the block medians and their range, milliseconds.  Not on the product path.

    python tools/pointnet2_finetune_time.py [--blocks 7] [--calls 10] [--json profiles/pointnet2_finetune_time.json]

Shapes: B = 16 and 32 at T = 35, past_len 10, P = 2048 (the box-shell clouds of synthetic.make_embedding_inputs), seeded inputs, the synthetic weights.  Sides:
  hip_pointnet_step_ms      encode with saves + the full pass + the PointNet++ backward + AdamW on 266 tensors + the re-fold
  hip_encoder_step_ms       the parent-equivalent step: train_encoder=True on the same raw-obj_points batch (it already pays the encode), AdamW on 228 tensors
  encode_ms / encode_saved_ms / backward_ms / refold_ms     interdiff_pointnet2_encode, _encode_saved, _finetune_grads, _refold alone
Reported: the milliseconds the feature adds to the parent's step, and the backward as a fraction of the encode."""
import argparse
import json
import os
import sys
import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mdm_train_time as mtt                                             # noqa: E402
from interdiff_amd import synthetic as syn                               # noqa: E402
from interdiff_amd.mdm_train import DenoiserTrainer                     # noqa: E402

DEV, PAST, T, P = mtt.DEV, mtt.PAST, 35, 2048


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--blocks', type=int, default=7)
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    sd = {k: torch.from_numpy(v) for k, v in syn.mdm_state_dict(seed=233).items()}
    res = dict(device=torch.cuda.get_device_name(0), blocks=a.blocks, calls=a.calls, past_len=PAST, P=P, shapes=[])
    for B in (16, 32):
        bt = syn.make_clip_batch(seed=500 + B + T, B=B, T=T, past_len=PAST, n_points=8)
        gt = torch.from_numpy(bt['gt']).to(DEV)
        pts = torch.from_numpy(syn.make_embedding_inputs(seed=600 + B, B=B, T=1, n_points=P)['obj_points']).to(DEV)
        t = torch.from_numpy(np.random.RandomState(B * T).randint(0, 1000, size=B).astype(np.int64)).to(DEV)
        eps = torch.randn(gt.shape, device=DEV, generator=torch.Generator(DEV).manual_seed(1))
        d_pc = torch.randn(B, 256, device=DEV, generator=torch.Generator(DEV).manual_seed(2))
        new, old = DenoiserTrainer(sd, device=DEV, train_encoder=True, train_pointnet=True), DenoiserTrainer(sd, device=DEV, train_encoder=True)
        batch = dict(gt=gt, obj_points=pts)
        first = float(new.training_step(batch, t=t, noise=eps)[0].mean()), float(old.training_step(batch, t=t, noise=eps)[0].mean())
        ft = new.pointnet
        sides = dict(hip_pointnet_step_ms=lambda: new.training_step(batch, t=t, noise=eps),
                     hip_encoder_step_ms=lambda: old.training_step(batch, t=t, noise=eps),
                     encode_ms=lambda: old.encode_points(pts), encode_saved_ms=lambda: ft.encode_saved(pts),
                     backward_ms=lambda: ft.grads(d_pc, flat=True), refold_ms=ft.refold)
        row = dict(B=B, T=T, first_loss_pointnet=first[0], first_loss_encoder=first[1], **mtt.alternate(sides, a.blocks, a.calls))
        row['pointnet_adds_ms'] = row['hip_pointnet_step_ms']['median'] - row['hip_encoder_step_ms']['median']
        row['backward_over_encode'] = row['backward_ms']['median'] / row['encode_ms']['median']
        res['shapes'].append(row)
        print('B = %d, T = %d, P = %d on %s: first-step loss with the PointNet++ in the pass %.6f, without %.6f' % (B, T, P, res['device'], first[0], first[1]))
        mtt.print_sides(row, sides)
        print('  the feature adds (ms)            %9.3f' % row['pointnet_adds_ms'])
        print('  backward / encode                %9.3f' % row['backward_over_encode'])
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(res, open(a.json, 'w'), indent=1, sort_keys=True)


if __name__ == '__main__':
    main()
