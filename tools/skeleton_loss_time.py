"""hip-event timing of the skeleton checkpoint-scoring path (interdiff_amd/skeleton_losses.py, csrc/skeleton_losses.hip); not on the
product path.

    python tools/skeleton_loss_time.py [--reps 50] [--json PATH]

At B = 64, T = 20 (past_len 10): ``calc_val_loss`` (two launches + the two torch elementwise ops of the weights), the two-launch entry
alone, the one-launch per-clip entry alone, the two-launch entry at K = 10 samples, and one ``denoising_losses`` call (q_sample + one eager
``SkeletonMDM.forward`` + the 13 per-clip terms).  Medians of warmed calls in microseconds."""
import argparse
import json
import os
import sys
import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)
from interdiff_amd import _lib, skeleton as sk, skeleton_losses as SL, synthetic as syn      # noqa: E402
from interdiff_amd.diffusion import create_gaussian_diffusion                                # noqa: E402

DEV = 'cuda'
B, T, P, K = 64, 20, 10, 10


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
    model = sk.SkeletonMDM({k: torch.from_numpy(v) for k, v in syn.skeleton_mdm_state_dict(1106).items()}, device=DEV)
    diff = create_gaussian_diffusion('cosine', 1000)
    bt = {k: torch.from_numpy(v) for k, v in syn.make_skeleton_batch(77, B=B, T=T).items()}
    gt, kw = SL.sample_kwargs(model, (bt['body'], bt['obj'], bt['pose'], bt['zero_pose_obj']), P)
    g = torch.Generator(device=DEV).manual_seed(1)
    samples = gt[None] + 0.03 * torch.randn(K, *gt.shape, device=DEV, generator=g)
    lib = model.lib
    tag = 'B%d_T%d' % (B, T)
    res = {}
    res['calc_val_loss_%s_us' % tag] = median_us(lambda: SL.calc_val_loss(samples[0], gt, P), a.reps)
    for k in (1, K):
        s = samples[:k].contiguous()
        terms, per = torch.empty(k, 13, device=DEV), torch.empty(k, 13, B, device=DEV)
        res['skeleton_sample_losses_kernels_only_K%d_%s_us' % (k, tag)] = median_us(lambda: _lib.check(lib.interdiff_skeleton_sample_losses(
            _lib.dptr(s), _lib.dptr(gt), k, B, 106, T, P, 63, 12, _lib.dptr(terms), _lib.dptr(per), None, 0, _lib.stream())), a.reps)
    out = torch.empty(13, B, device=DEV)
    res['skeleton_denoising_losses_kernel_only_%s_us' % tag] = median_us(lambda: _lib.check(lib.interdiff_skeleton_denoising_losses(
        _lib.dptr(samples[0]), _lib.dptr(gt), B, T, P, 63, 12, _lib.dptr(out), _lib.stream())), a.reps)
    t = torch.randint(0, 1000, (B,), device=DEV, generator=g)
    cond, z = kw['y']['cond'], kw['zero_pose_obj']
    res['denoising_losses_%s_us' % tag] = median_us(lambda: SL.denoising_losses(model, diff, gt, z, cond, t=t, seed=3, past_len=P), a.reps)
    for k, v in res.items():
        print('%-56s %10.1f' % (k, v))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(res, open(a.json, 'w'), indent=1, sort_keys=True)


if __name__ == '__main__':
    main()
