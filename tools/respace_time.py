"""Whole-sample wall time and ms per step of the headline shape (bench.py: B = 16, T = 100, P = 2048, correction mode, one GPU) under three schedules,
one process, one session (not product code):

  full1000   the shipped 1000-step schedule, p_sample_loop
  ddpm100    timestep_respacing '100', p_sample_loop
  ddim50     timestep_respacing 'ddim50', ddim_sample_loop with eta = 0

The clock is the host's around one sample (synchronize on both sides): what a caller waits for, graph replays, eager hook steps and the once-per-sample
memory fold included.  Per schedule: one warm-up sample (captures, kernel attributes, clocks), then the legs are visited round-robin ``--rounds`` times
so that drift hits all three alike; reported are the median, the minimum and every run.  A short schedule replays fewer and shorter graph blocks and
pays the per-sample work (memory fold, input copies, the hook's setup at its steps) over fewer steps, so its ms per step is expected ABOVE the
1000-step schedule's: ``ms_per_step_over_full1000`` says by how much.  Nothing here speaks about sample quality at fewer steps -- the weights are synthetic.

    python tools/respace_time.py [--out profiles/respace_time.json] [--rounds 7]
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
LEGS = dict(full1000=('', dict(sampler='ddpm')), ddpm100=('100', dict(sampler='ddpm')), ddim50=('ddim50', dict(sampler='ddim', eta=0.0)))
diffs = {name: create_gaussian_diffusion('cosine', bench.STEPS, spec) for name, (spec, _) in LEGS.items()}


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
for name in LEGS:
    n = diffs[name].num_timesteps
    med = statistics.median(runs[name])
    out['legs'][name] = dict(steps=n, hook_steps=sum(1 for i in range(n) if corr.is_active(i)), sample_ms_median=round(med, 3), sample_ms_min=round(min(runs[name]), 3),
                             sample_ms_runs=[round(m, 3) for m in runs[name]], ms_per_step_median=round(med / n, 5))
full = out['legs']['full1000']['ms_per_step_median']
for name in LEGS:
    out['legs'][name]['ms_per_step_over_full1000'] = round(out['legs'][name]['ms_per_step_median'] / full, 3)
    out['legs'][name]['sample_time_over_full1000'] = round(out['legs'][name]['sample_ms_median'] / out['legs']['full1000']['sample_ms_median'], 4)
line = json.dumps(out)
print(line, flush=True)
if args.out:
    with open(args.out, 'w') as f:
        f.write(line + '\n')
