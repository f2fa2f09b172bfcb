"""Generate tests/golden/plms.npz by running the REFERENCE's own ``plms_sample_loop`` and its ``p_sample_loop`` / ``ddim_sample_loop`` with
``skip_timesteps`` / ``init_image`` (diffusion/gaussian_diffusion.py), imported read-only through refshim.py, around the reference MDM with
the seeded synthetic weights, on the inputs of tests/respace_oracle.py (as respace.npz was recorded).  Run in the build container only:

    python tests/golden/make_golden_plms.py

Recorded per case of tests/plms_oracle.py CASES, under its ``case_name``:
  <case>              the whole-loop output [3,1,144,20]: B = 3, T = 20, x_T injected, the first 10 frames inpainted, the stub denoised_fn that
                      returns x * (1 - t / 2000) of the t IT is handed, init_image = 0.5 gt where the case has one, and for the DDPM / DDIM
                      cases the per-step noise injected (``randn_like`` patched in the generator, draw k = loop index k)
  <case>_t_model, <case>_t_hook    the timesteps the model and the stub were called with, in call order (the first PLMS step calls both twice)
  <case>_e_ref        max |reference fp32 - fp64 oracle| of that loop (tests/plms_oracle.py around oracle/denoiser.py in fp64): the reference's
                      own rounding error, which sets the GPU gate 4 e_ref
``order=1`` is asserted to fail in the reference (TypeError on its first step).
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
import make_golden_respace as mgr                 # noqa: E402
from tests import fixtures as fx                  # noqa: E402
from tests import respace_oracle as ro            # noqa: E402
from tests import plms_oracle as po               # noqa: E402

torch.set_grad_enabled(False)


def run_reference(d, gd, rec, case, noise, y, gt, steps, hook_t):
    loop, tag, par, skip, with_init = case
    draws = iter(steps)

    def stub(x, t, model_kwargs):
        hook_t.append(int(t[0]))
        return x * ro.stub_scale(int(t[0]))
    kw = dict(clip_denoised=False, noise=noise.clone(), model_kwargs={'y': y}, denoised_fn=stub, skip_timesteps=skip,
              init_image=po.INIT_SCALE * gt if with_init else None)
    real = gd.th.randn_like
    gd.th.randn_like = lambda x: next(draws).clone()          # inject the per-step noise
    try:
        if loop == 'plms':
            return d.plms_sample_loop(rec, tuple(noise.shape), order=par, **kw)
        if loop == 'ddpm':
            return d.p_sample_loop(rec, tuple(noise.shape), **kw)
        return d.ddim_sample_loop(rec, tuple(noise.shape), eta=par, **kw)
    finally:
        gd.th.randn_like = real


def main():
    out = {}
    gd = refshim.load('diffusion.gaussian_diffusion')
    net = mg.ref_mdm()
    model64 = ro.mdm_fp64(fx.mdm_weights())
    inputs = ro.inputs()
    noise, cond, gt, mask, steps = inputs
    y = dict(cond=cond, inpainted_motion=gt, inpainting_mask=mask)
    spaced = {tag: mgr.ref_spaced(base, spec) for tag, (base, spec) in ro.SCHEDULES.items()}
    try:
        run_reference(spaced['b'], gd, mgr.Recorder(net), ('plms', 'b', 1, 0, False), noise, y, gt, steps, [])
    except TypeError:
        pass
    else:
        raise AssertionError('the reference runs order=1')
    for case in po.CASES:
        rec, hook_t = mgr.Recorder(net), []
        got = run_reference(spaced[case[1]], gd, rec, case, noise, y, gt, steps, hook_t).detach().cpu().numpy()
        want = po.run_case(model64, case, inputs)
        name = po.case_name(*case)
        e_ref = float(np.abs(got.astype(np.float64) - want).max())
        out[name], out[name + '_e_ref'] = got, np.float64(e_ref)
        out[name + '_t_model'], out[name + '_t_hook'] = np.array(rec.seen, np.int64), np.array(hook_t, np.int64)
        print('%-22s |x| max %.3f   e_ref %.3e   model t %s   hook t %s' % (name, np.abs(want).max(), e_ref, rec.seen, hook_t))
    mg.save('plms.npz', **out)


if __name__ == '__main__':
    main()
