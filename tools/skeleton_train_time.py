"""Device-event timing of one train-mode training step of the skeleton correction predictor (interdiff_amd/skeleton_train.py: batch statistics,
dropout from the in-kernel generator, running-buffer update, Adam, re-fold) next to one frozen-statistics step of
``SkeletonFineTuner.training_step`` (the yardstick: one launch per clip for the whole network, no seams), on the same GPU in the same process;
not on the product path.

    python tools/skeleton_train_time.py [--blocks 9] [--steps 50] [--json profiles/skeleton_train_time.json]

At B = 32 (the reference trainer's default batch) and B = 3, T = 20, past_len 10; the seeded synthetic batch of interdiff_amd.synthetic and the
checkpoint stand-in of tools/skeleton_finetune_time.py (the timing does not depend on the weights' values).  Both shapes are warmed up; a timed
block is ``steps`` consecutive steps between two device events; the two sides alternate block by block; reported: the median over the blocks
of microseconds per step, and the spread (min, max).  The train-mode step is 17 phase launches + masks + fold + statistics + Adam + re-fold =
22 launches against the fine-tuner's 5, so what this measures is mostly the cost of the seams."""
import argparse
import json
import os
import sys
import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from interdiff_amd import skeleton_finetune as sf, skeleton_train as st, synthetic as syn      # noqa: E402
from skeleton_finetune_time import synthetic_state_dict                                        # noqa: E402

DEV = 'cuda'
T = 20


def block_us(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--blocks', type=int, default=9)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X'
    sd = synthetic_state_dict()
    res = {'blocks': a.blocks, 'steps_per_block': a.steps, 'device': torch.cuda.get_device_name(0)}
    for B in (32, 3):
        bt = {k: torch.from_numpy(v).to(DEV) for k, v in syn.make_skeleton_batch(81, B=B, T=T).items()}
        batch = (bt['body'], bt['obj'], bt['pose'], bt['zero_pose_obj'])
        ft, tr = sf.SkeletonFineTuner(sd, device=DEV), st.SkeletonTrainer(sd, dropout=0.1, seed=82, device=DEV)
        sides = {'finetune': lambda: ft.training_step(batch), 'train': lambda: tr.training_step(batch), 'train_grads_only': lambda: tr._train_grads(batch)}
        res['first_loss_finetune_B%d' % B], res['first_loss_train_B%d' % B] = float(ft.training_step(batch)), float(tr.training_step(batch))
        for fn in sides.values():                       # warm-up of every shape and side
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in sides}
        for _ in range(a.blocks):                       # alternate the sides block by block
            for k, fn in sides.items():
                times[k].append(block_us(fn, a.steps))
        for k, v in times.items():
            res['%s_step_B%d_us' % (k, B)] = {'median': float(np.median(v)), 'min': float(np.min(v)), 'max': float(np.max(v))}
            print('B = %2d  %-18s median %10.1f us per step (min %.1f, max %.1f over %d blocks of %d steps)' % (B, k, np.median(v), np.min(v), np.max(v), a.blocks, a.steps))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(res, open(a.json, 'w'), indent=1, sort_keys=True)


if __name__ == '__main__':
    main()
