"""Whole-sample wall time and ms per step of the headline shape (bench.py: B = 16, T = 100, P = 2048, correction mode, one GPU) under the few-step samplers,
one process, one session (not product code):

  ddim50_fused     timestep_respacing 'ddim50', ddim_sample_loop eta = 0, the fused plain step (the product route)
  ddim50_twocall   the same with ``fuse_plain_step=False``: [forward -> update] as two launches on one chain -- the form a PLMS step has to take
  plms4_50         timestep_respacing '50', plms_sample_loop order 4 (51 denoiser calls: the first step makes two)
  plms4_25         timestep_respacing '25', plms_sample_loop order 4 (26 calls)
  ddpm100_skip50   timestep_respacing '100', p_sample_loop with skip_timesteps=50 (spaced steps 99 .. 50)

The clock is the host's around one sample (synchronize on both sides): what a caller waits for, graph replays, eager hook steps and the once-per-sample
memory fold included.  Per leg: one warm-up sample (captures, kernel attributes, clocks), then the legs are visited round-robin ``--rounds`` times so
that drift hits all alike; reported are the median, the minimum and every run.  ``steps`` counts loop steps, ``model_calls`` denoiser forwards.  No target
is set: nobody has measured a PLMS step before.  Nothing here speaks about sample quality at fewer steps or another sampler -- the weights are synthetic.

    python tools/plms_time.py [--out profiles/plms_time.json] [--rounds 7]
"""
import argparse, json, os, statistics, subprocess, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench                                                                      # noqa: E402
from interdiff_amd.diffusion import create_gaussian_diffusion, sample_loop        # noqa: E402

torch.set_grad_enabled(False)
ap = argparse.ArgumentParser()
ap.add_argument('--out')
ap.add_argument('--rounds', type=int, default=7)
args = ap.parse_args()
dev = torch.device('cuda:0')
torch.cuda.set_device(dev)
model, corr, bt, y, _ = bench.build_world(dev, 0)
# name -> (respacing, loop keywords, schedule attributes, (first index, last index) of the loop)
LEGS = dict(ddim50_fused=('ddim50', dict(sampler='ddim', eta=0.0), {}, (49, 0)),
            ddim50_twocall=('ddim50', dict(sampler='ddim', eta=0.0), dict(fuse_plain_step=False), (49, 0)),
            plms4_50=('50', dict(sampler='plms', order=4), {}, (49, 0)),
            plms4_25=('25', dict(sampler='plms', order=4), {}, (24, 0)),
            ddpm100_skip50=('100', dict(sampler='ddpm', skip_timesteps=50), {}, (99, 50)))
diffs = {}
for name, (spec, _, attrs, _) in LEGS.items():
    diffs[name] = create_gaussian_diffusion('cosine', bench.STEPS, spec)
    for k, v in attrs.items():
        setattr(diffs[name], k, v)


def one(name, seed):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = sample_loop(diffs[name], model, tuple(bt['noise'].shape), noise=bt['noise'], clip_denoised=False, model_kwargs={'y': y}, denoised_fn=corr, seed=seed, **LEGS[name][1])
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    assert bool(torch.isfinite(out).all())
    return ms


for name in LEGS:
    one(name, 1)
runs = {name: [] for name in LEGS}
for r in range(args.rounds):
    for name in LEGS:
        runs[name].append(one(name, 100 + r))
try:
    commit = subprocess.run(['git', 'rev-parse', '--short', 'HEAD'], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
except OSError:
    commit = None
out = dict(shape=dict(B=bench.B_PER_GPU, T=bench.T, P=bench.P, mode='correction'), device=torch.cuda.get_device_name(0), commit=commit,
           timer='host clock around one sample, synchronize on both sides; 1 warm-up sample per leg, then %d round-robin rounds' % args.rounds, legs={})
for name, (spec, kw, _, (hi, lo)) in LEGS.items():
    n = hi - lo + 1
    plms = kw['sampler'] == 'plms'
    hooks = sum(1 for i in range(lo, hi + 1) if corr.is_active(i)) + (1 if plms and corr.is_active(hi - 1) else 0)
    med = statistics.median(runs[name])
    out['legs'][name] = dict(respacing=spec, steps=n, model_calls=n + (1 if plms else 0), hook_calls=hooks, sample_ms_median=round(med, 3), sample_ms_min=round(min(runs[name]), 3),
                             sample_ms_runs=[round(m, 3) for m in runs[name]], ms_per_step_median=round(med / n, 5),
                             ms_per_model_call_median=round(med / (n + (1 if plms else 0)), 5))
base = out['legs']['ddim50_fused']['sample_ms_median']
for name in LEGS:
    out['legs'][name]['sample_time_over_ddim50_fused'] = round(out['legs'][name]['sample_ms_median'] / base, 4)
line = json.dumps(out)
print(line, flush=True)
if args.out:
    with open(args.out, 'w') as f:
        f.write(line + '\n')
