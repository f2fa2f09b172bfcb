"""Time the HO-GCN skeleton correction hook (interdiff_amd.skeleton.HipSkeletonCorrection, one fused launch) at B = 1 and 64:
a warmed call, median of N, measured with hip events around each call.  With --cpu, also the CPU time of the restated reference
hook (tests/skeleton_oracle.py, fp32 torch on the host, median of N wall-clock calls) on the same inputs.

    python tools/skeleton_hook_time.py [--n 50] [--cpu] [--json out.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=50)
    ap.add_argument('--cpu', action='store_true')
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    from interdiff_amd import skeleton as sk
    torch.set_grad_enabled(False)
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'skel_ckpt.npz'))
    sd = {k: torch.from_numpy(z[k]) for k in z.files}
    dev = 'cuda'
    hook = sk.HipSkeletonCorrection(sk.SkeletonObjProjector(sd, device=dev), device=dev)
    res = {}
    for B in (1, 64):
        g = torch.Generator().manual_seed(B)
        x, gt = 0.5 * torch.randn(B, 1, 106, 20, generator=g), 0.5 * torch.randn(B, 1, 106, 20, generator=g)
        zp = 0.3 * torch.randn(B, 12, 3, generator=g)
        xd, yd, zd = x.to(dev), {'inpainted_motion': gt.to(dev)}, zp.to(dev)
        t = torch.full((B,), 250, dtype=torch.int64, device=dev)
        t.host_value = 250
        kw = {'y': yd, 'zero_pose_obj': zd}
        for _ in range(5):
            hook(xd, t, kw)
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            hook(xd, t, kw)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        res['hip_B%d_ms' % B] = float(np.median(ms))
        if a.cpu:
            from tests import skeleton_oracle as so
            layers = so.state_dict_layers(sd, dtype=torch.float32)
            so.denoised_fn(layers, x, 250, {'inpainted_motion': gt}, zp)
            wall = []
            for _ in range(max(3, a.n // 5)):
                c0 = time.perf_counter()
                so.denoised_fn(layers, x, 250, {'inpainted_motion': gt}, zp)
                wall.append((time.perf_counter() - c0) * 1e3)
            res['cpu_restatement_B%d_ms' % B] = float(np.median(wall))
    res['n'] = a.n
    print(json.dumps(res))
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
