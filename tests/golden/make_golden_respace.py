"""Generate tests/golden/respace.npz by running the REFERENCE's own ``space_timesteps`` / ``SpacedDiffusion`` (diffusion/respace.py) and
``p_sample_loop`` / ``ddim_sample_loop`` (diffusion/gaussian_diffusion.py), imported read-only through refshim.py, around the reference
MDM with the seeded synthetic weights (as loop.npz was recorded).  Run in the build container only:

    python tests/golden/make_golden_respace.py

Recorded:
  spec_<k>            space_timesteps(n, spec) of tests/respace_oracle.py SPECS[k], sorted; the BAD_SPECS are asserted to raise ValueError here
  <s>_timestep_map, <s>_betas, <s>_alphas_cumprod, <s>_posterior_*   the fp64 tables of the two schedules SCHEDULES[s]
                      ('a': cosine 1000 respaced '10'; 'b': cosine 30 respaced [4, 3, 2])
  <s>_<loop>          the whole-loop output [3,1,144,20] of p_sample_loop ('ddpm') and ddim_sample_loop (eta 0 and 1): B = 3, T = 20,
                      x_T and the per-step noise injected (``randn_like`` patched in the generator, draw k = loop index k), the first 10
                      frames inpainted, and a stub denoised_fn that returns x * (1 - t / 2000) of the t IT is handed
  <s>_<loop>_t_model, <s>_<loop>_t_hook    the timesteps the model and the stub were called with, in loop order
  <s>_<loop>_e_ref    max |reference fp32 - fp64 oracle| of that loop (tests/respace_oracle.py sample_loop around oracle/denoiser.py in fp64):
                      the reference's own rounding error, which sets the GPU gate 4 e_ref
"""
import os
import sys
import warnings
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, '..', '..'))
warnings.filterwarnings('ignore')
import refshim                                    # noqa: E402
import make_golden as mg                          # noqa: E402
from tests import fixtures as fx                  # noqa: E402
from tests import respace_oracle as ro            # noqa: E402

torch.set_grad_enabled(False)
np_ = lambda t: t.detach().cpu().numpy()
TABLES = ('betas', 'alphas_cumprod', 'alphas_cumprod_prev', 'posterior_variance', 'posterior_log_variance_clipped', 'posterior_mean_coef1',
          'posterior_mean_coef2')


def ref_spaced(base, spec):
    gd, rsp = refshim.load('diffusion.gaussian_diffusion'), refshim.load('diffusion.respace')
    return rsp.SpacedDiffusion(use_timesteps=rsp.space_timesteps(base, spec), betas=gd.get_named_beta_schedule('cosine', base, 1.),
                               model_mean_type=gd.ModelMeanType.START_X, model_var_type=gd.ModelVarType.FIXED_SMALL,
                               loss_type=gd.LossType.MSE, rescale_timesteps=False, lambda_vel=1.)


class Recorder:
    """The reference MDM behind a wrapper that notes the timesteps it is called with (what _WrappedModel hands it)."""

    def __init__(self, net):
        self.net, self.seen = net, []

    def parameters(self):
        return self.net.parameters()

    def __call__(self, x, ts, **kw):
        self.seen.append(int(ts[0]))
        assert bool((ts == ts[0]).all())
        return self.net(x, ts, **kw)


def main():
    out = {}
    rsp, gd = refshim.load('diffusion.respace'), refshim.load('diffusion.gaussian_diffusion')
    for k, (n, spec) in enumerate(ro.SPECS):
        out['spec_%d' % k] = np.array(sorted(rsp.space_timesteps(n, spec)), np.int64)
    for n, spec in ro.BAD_SPECS:
        try:
            rsp.space_timesteps(n, spec)
        except ValueError:
            continue
        raise AssertionError('the reference accepts %r on %d' % (spec, n))

    net = mg.ref_mdm()
    model64 = ro.mdm_fp64(fx.mdm_weights())
    noise, cond, gt, mask, steps = ro.inputs()
    y = dict(cond=cond, inpainted_motion=gt, inpainting_mask=mask)
    for tag, (base, spec) in ro.SCHEDULES.items():
        d = ref_spaced(base, spec)
        out[tag + '_timestep_map'] = np.array(d.timestep_map, np.int64)
        for name in TABLES:
            out['%s_%s' % (tag, name)] = np.asarray(getattr(d, name), np.float64)
        tb = ro.spaced_tables(ro.cosine_betas(base), rsp.space_timesteps(base, spec))
        for sampler, eta in ro.LOOPS:
            rec, hook_t, draws = Recorder(net), [], iter(steps)

            def stub(x, t, model_kwargs):
                hook_t.append(int(t[0]))
                return x * ro.stub_scale(int(t[0]))
            real = gd.th.randn_like
            gd.th.randn_like = lambda x: next(draws).clone()          # inject the per-step noise
            try:
                kw = dict(clip_denoised=False, noise=noise.clone(), model_kwargs={'y': y}, denoised_fn=stub)
                got = d.p_sample_loop(rec, tuple(noise.shape), **kw) if sampler == 'ddpm' else d.ddim_sample_loop(rec, tuple(noise.shape), eta=eta, **kw)
            finally:
                gd.th.randn_like = real
            name = ro.loop_name(tag, sampler, eta)
            want = ro.sample_loop(lambda x, ts: model64(x, ts, cond), tb, noise.numpy(), steps.numpy(), sampler, eta or 0.0, mask.numpy(), gt.numpy().astype(np.float64),
                                  lambda x0, i: x0 * ro.stub_scale(i))
            e_ref = float(np.abs(np_(got).astype(np.float64) - want).max())
            out[name], out[name + '_e_ref'] = np_(got), np.float64(e_ref)
            out[name + '_t_model'], out[name + '_t_hook'] = np.array(rec.seen, np.int64), np.array(hook_t, np.int64)
            print('%-16s |x| max %.3f   e_ref %.3e   model t %s   hook t %s' % (name, np.abs(want).max(), e_ref, rec.seen, hook_t))
    mg.save('respace.npz', **out)


if __name__ == '__main__':
    main()
