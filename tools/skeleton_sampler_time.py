"""ms per step of whole 1000-step samples at the skeleton pipeline's default shape (eval_skeleton.py: B = 64, T = 20), hip events, one warm-up
sample then the median of 3 (not product code):

  (a) the skeleton denoiser (interdiff_amd.skeleton.SkeletonMDM: FF = 256 zero-padded, keypoint head), plain
  (b) the same with the HO-GCN correction hook at its eleven steps
  (c) the C = 106, FF = 1024, plain-linear-heads stand-in of test_config1_skeleton_tokens_through_the_denoiser_kernels, plain

Leg (c) needs nothing of the skeleton denoiser: on a commit that has no SkeletonMDM the script prints (c) alone -- the baseline the other two are
compared with (one box, one session).

    python tools/skeleton_sampler_time.py [--out profiles/NAME.json] [--legs abc] [--steps 1000] [--commit LABEL]
"""
import argparse, json, os, statistics, subprocess, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from interdiff_amd import synthetic as syn                                        # noqa: E402
from interdiff_amd import skeleton as sk                                          # noqa: E402
from interdiff_amd.mdm import MDM                                                 # noqa: E402
from interdiff_amd.diffusion import create_gaussian_diffusion                     # noqa: E402

torch.set_grad_enabled(False)
ap = argparse.ArgumentParser()
ap.add_argument('--out')
ap.add_argument('--legs', default='abc')
ap.add_argument('--steps', type=int, default=1000)
ap.add_argument('--batch', type=int, default=64)
ap.add_argument('--commit', help='label of the tree being timed (default: git rev-parse --short HEAD)')
args = ap.parse_args()
dev = torch.device('cuda:0')
B, T, PAST, STEPS = args.batch, 20, 10, args.steps
rs = np.random.RandomState(64)
rn = lambda *s: torch.from_numpy(rs.standard_normal(s).astype(np.float32)).to(dev)
gt, noise, cond = rn(B, 1, 106, T), rn(B, 1, 106, T), rn(PAST, B, 256)
zero = (0.3 * rn(B, 12, 3)).contiguous()
mask = torch.ones(B, 1, 106, T, dtype=torch.bool, device=dev)
mask[..., PAST:] = False
y = dict(cond=cond, inpainted_motion=gt, inpainting_mask=mask)
diff = create_gaussian_diffusion('cosine', 1000)


def timed(model, kw, hook):
    def one():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        diff.p_sample_loop(model, tuple(noise.shape), noise=noise, clip_denoised=False, model_kwargs=kw, denoised_fn=hook, seed=7, n_steps=STEPS)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / STEPS
    one()                                   # warm-up: captures, kernel attributes, clocks
    ms = [one() for _ in range(3)]
    return dict(ms_per_step_median=round(statistics.median(ms), 5), ms_per_step_runs=[round(m, 5) for m in ms])


def standin():
    """The stand-in of tests/test_hip_parity.py test_config1_skeleton_tokens_through_the_denoiser_kernels: SMPL-style weights at C = 63 + 43."""
    sd = {k: torch.from_numpy(v) for k, v in syn.mdm_state_dict(233).items()}
    g = torch.Generator().manual_seed(106)
    sd['bodyEmbedding.weight'] = torch.randn(256, 63, generator=g) / 63 ** 0.5
    sd['objEmbedding.weight'] = torch.cat([torch.randn(256, 36, generator=g) / 6.0, torch.zeros(256, 7)], dim=1)
    sd['bodyFinalLinear.weight'], sd['bodyFinalLinear.bias'] = torch.randn(63, 256, generator=g) / 16.0, 0.1 * torch.randn(63, generator=g)
    sd['objFinalLinear.weight'], sd['objFinalLinear.bias'] = torch.randn(43, 256, generator=g) / 16.0, 0.1 * torch.randn(43, generator=g)
    return MDM(sd, device=dev)


try:
    commit = args.commit or subprocess.run(['git', 'rev-parse', '--short', 'HEAD'], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
except OSError:
    commit = None
out = dict(shape=dict(B=B, T=T, steps=STEPS), device=torch.cuda.get_device_name(0), commit=commit, timer='hip events, 1 warm-up sample, median of 3')
has_skel = hasattr(sk, 'SkeletonMDM')
if has_skel and ('a' in args.legs or 'b' in args.legs):
    model = sk.SkeletonMDM({k: torch.from_numpy(v) for k, v in syn.skeleton_mdm_state_dict().items()}, device=dev)
    kw = {'y': y, 'zero_pose_obj': zero}
    if 'a' in args.legs:
        out['a_skeleton_plain'] = timed(model, kw, None)
    if 'b' in args.legs:
        z = np.load(os.path.join(ROOT, 'tests', 'golden', 'skel_ckpt.npz'))
        hook = sk.HipSkeletonCorrection(sk.SkeletonObjProjector({k: torch.from_numpy(z[k]) for k in z.files}, device=dev), device=dev)
        out['b_skeleton_hook'] = timed(model, kw, hook)
    out['ffn_math'] = model.ffn_math
if 'c' in args.legs:
    out['c_standin_ff1024_plain'] = timed(standin(), {'y': y}, None)
if 'a_skeleton_plain' in out and 'c_standin_ff1024_plain' in out:
    out['a_over_c'] = round(out['a_skeleton_plain']['ms_per_step_median'] / out['c_standin_ff1024_plain']['ms_per_step_median'], 4)
line = json.dumps(out)
print(line, flush=True)
if args.out:
    with open(args.out, 'w') as f:
        f.write(line + '\n')
