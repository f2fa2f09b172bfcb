"""hip-event timing of the checkpoint-scoring path (interdiff_amd/losses.py, csrc/losses.hip); not on the product path.

    python tools/loss_time.py [--reps 50] [--json PATH]

Times ``calc_loss`` at K = 10 samples for B = 32, T = 35 (the reference's default shape) and B = 16, T = 100, the same scoring done
with the torch-op composition of tests/losses_oracle.py on the same GPU (fp32, what the reference's calc_loss amounts to), and one
``denoising_losses`` call (q_sample + one denoiser forward + the 16 per-clip terms) at both shapes.  Medians in microseconds."""
import argparse
import json
import os
import sys
import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)
from interdiff_amd import losses as L, synthetic as syn                 # noqa: E402
from interdiff_amd.diffusion import create_gaussian_diffusion           # noqa: E402
from interdiff_amd.mdm import MDM                                       # noqa: E402
from tests import losses_oracle as lo                                   # noqa: E402

DEV = 'cuda'


def median_us(fn, reps, warm=5):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    model = MDM({k: torch.from_numpy(v) for k, v in syn.mdm_state_dict(233).items()}, device=DEV)
    diff = create_gaussian_diffusion('cosine', 1000)
    res = {}
    for B, T, K in ((32, 35, 10), (16, 100, 10)):
        bt = {k: torch.from_numpy(v).to(DEV) for k, v in syn.make_clip_batch(seed=77, B=B, T=T, n_points=8).items() if isinstance(v, np.ndarray)}
        g = torch.Generator(device=DEV).manual_seed(1)
        samples = bt['gt'][None] + 0.03 * torch.randn(K, *bt['gt'].shape, device=DEV, generator=g)
        tag = 'B%d_T%d' % (B, T)
        res['calc_loss_K%d_%s_us' % (K, tag)] = median_us(lambda: L.calc_loss(samples, bt), a.reps)
        res['calc_val_loss_%s_us' % tag] = median_us(lambda: L.calc_val_loss(samples[0], bt), a.reps)
        res['torch_ops_calc_loss_K%d_%s_us' % (K, tag)] = median_us(lambda: lo.sample_terms(samples, bt['gt'], bt['hand_pose'], 10, 'test'), max(3, a.reps // 10), warm=2)
        t = torch.randint(0, 1000, (B,), device=DEV, generator=g)
        model(bt['gt'], t, y={'cond': bt['cond']})
        res['denoising_losses_%s_us' % tag] = median_us(lambda: L.denoising_losses(model, diff, bt, t=t, seed=3), a.reps)
        pred = model(bt['gt'], t, y={'cond': bt['cond']}).clone()
        out = torch.empty(16, B, device=DEV)
        from interdiff_amd import _lib
        res['denoising_losses_kernel_only_%s_us' % tag] = median_us(lambda: _lib.check(model.lib.interdiff_denoising_losses(
            _lib.dptr(pred), _lib.dptr(bt['gt']), B, T, 10, _lib.dptr(out), _lib.stream())), a.reps)
    for k, v in res.items():
        print('%-44s %10.1f' % (k, v))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(res, open(a.json, 'w'), indent=1, sort_keys=True)


if __name__ == '__main__':
    main()
