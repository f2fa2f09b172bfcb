"""PLMS sampling and ``skip_timesteps`` / ``init_image`` on the three loops, restated in fp64 numpy (diffusion/gaussian_diffusion.py:663-736,
:927-1000, :1001-1196), and the recorded cases that tests/golden/make_golden_plms.py feeds the reference and tests/test_plms.py the HIP path.

The loops keep the reference's UNFOLDED arithmetic: eps re-derived from x0 through the sqrt_recip tables, the Adams-Bashforth sums in the order
written there, sqrt(alpha_bar_prev) formed per step -- so they check the table and the fused operations of csrc/plms.hip instead of repeating them.
The model is a callable (x fp64 [B,1,C,T], model timesteps int64 [B]) -> x0 fp64; inputs and the stub hook are tests/respace_oracle.py's.
"""
import numpy as np
from tests import respace_oracle as ro

INIT_SCALE = 0.5                                  # the recorded init_image is INIT_SCALE * gt
# (loop, schedule, order / eta, skip_timesteps, with init_image)
CASES = (('plms', 'b', 2, 0, False), ('plms', 'b', 3, 0, False), ('plms', 'b', 4, 0, False), ('plms', 'b', 4, 2, True), ('plms', 'a', 4, 2, True),
         ('plms', 'a', 2, 3, False), ('ddpm', 'a', None, 3, True), ('ddpm', 'b', None, 2, False), ('ddim', 'a', 0.0, 3, True), ('ddim', 'b', 1.0, 2, False))
# e_ref of the PLMS cases as measured when the issue was written (the DDPM / DDIM ones were not): the fixture must stay in their range
E_REF_QUOTED = {'plms_b_o2': 2.2e-6, 'plms_b_o3': 3.2e-6, 'plms_b_o4': 4.1e-6, 'plms_b_o4_skip2_init': 1.7e-6, 'plms_a_o4_skip2_init': 7.0e-6,
                'plms_a_o2_skip3': 2.3e-6}


def case_name(loop, tag, par, skip, init):
    how = {'plms': 'o%s' % par, 'ddpm': '', 'ddim': 'eta%d' % int(par or 0)}[loop]
    return '_'.join(p for p in (loop, tag, how, 'skip%d' % skip if skip else '', 'init' if init else '') if p)


CASE_IDS = [case_name(*c) for c in CASES]


def q_sample(tb, x_start, i, noise):
    """gaussian_diffusion.py:233-250 at spaced step i."""
    ac = tb['alphas_cumprod'][i]
    return np.sqrt(ac) * x_start + np.sqrt(1.0 - ac) * noise


def indices(n, loop, skip):
    """The spaced steps a loop runs: p_sample_loop slices the FRONT of the ascending list off (:705), the other two its end (:967, :1161)."""
    return list(range(n))[skip:][::-1] if loop == 'ddpm' else list(range(n - skip))[::-1]


def start(tb, loop, x_T, skip, init):
    """:701-709 / :965-972 / :1158-1165: (x the loop starts from, its indices)."""
    x = np.asarray(x_T, np.float64)
    idx = indices(len(tb['betas']), loop, skip)
    if skip and init is None:
        init = np.zeros_like(x)
    if init is not None:
        x = q_sample(tb, np.asarray(init, np.float64), idx[0], x)
    return x, idx


def predict(model, tb, x, i, mask, gt, denoised_fn):
    """p_mean_variance's pred_xstart (:277-388): model at timestep_map[i] -> inpaint -> denoised_fn told i."""
    x0 = model(x, np.full(x.shape[0], tb['timestep_map'][i], np.int64))
    if mask is not None:
        x0 = np.where(mask, gt, x0)
    return x0 if denoised_fn is None else denoised_fn(x0, i)


def eps_from_x0(tb, i, x, x0):
    """_predict_eps_from_xstart."""
    return (tb['sqrt_recip_alphas_cumprod'][i] * x - x0) / tb['sqrt_recipm1_alphas_cumprod'][i]


def plms_mean(tb, i, x, ep):
    """:1057-1058 / :1074-1075."""
    abp = tb['alphas_cumprod_prev'][i]
    pred = tb['sqrt_recip_alphas_cumprod'][i] * x - tb['sqrt_recipm1_alphas_cumprod'][i] * ep
    return pred * np.sqrt(abp) + np.sqrt(1 - abp) * ep


def plms_step(tb, i, x, x0, old, order, second_x0):
    """plms_sample (:1001-1083) at spaced step i from the first call's x0; ``old``: the earlier eps (None at the first step), ``second_x0``:
    (x_mid) -> the x0 of the second call at i - 1.  Returns (sample, the eps list handed on)."""
    eps = eps_from_x0(tb, i, x, x0)
    if old is None:
        old = [eps]
        abp = tb['alphas_cumprod_prev'][i]
        mid = x0 * np.sqrt(abp) + np.sqrt(1 - abp) * eps
        ep = (eps + eps_from_x0(tb, i - 1, mid, second_x0(mid))) / 2
    else:
        old = old + [eps]
        k = min(order, len(old))
        ep = (old[-1], (3 * old[-1] - old[-2]) / 2 if k > 1 else None, (23 * old[-1] - 16 * old[-2] + 5 * old[-3]) / 12 if k > 2 else None,
              (55 * old[-1] - 59 * old[-2] + 37 * old[-3] - 9 * old[-4]) / 24 if k > 3 else None)[k - 1]
    if len(old) >= order:
        old = old[1:]
    return (plms_mean(tb, i, x, ep) if i != 0 else x0), old


def plms_loop(model, tb, x_T, order, skip=0, init=None, mask=None, gt=None, denoised_fn=None):
    x, idx = start(tb, 'plms', x_T, skip, init)
    old = None
    for i in idx:
        x0 = predict(model, tb, x, i, mask, gt, denoised_fn)
        x, old = plms_step(tb, i, x, x0, old, order, lambda mid: predict(model, tb, mid, i - 1, mask, gt, denoised_fn))
    return x


def skipped_loop(model, tb, x_T, step_noise, loop, eta, skip, init, mask=None, gt=None, denoised_fn=None):
    """p_sample_loop / ddim_sample_loop with skip_timesteps / init_image; ``step_noise`` [>= steps, ...] in loop order."""
    x, idx = start(tb, loop, x_T, skip, init)
    for it, i in enumerate(idx):
        x0 = predict(model, tb, x, i, mask, gt, denoised_fn)
        nz = np.asarray(step_noise[it], np.float64)
        x = ro.ddpm_step(tb, i, x0, x, nz) if loop == 'ddpm' else ro.ddim_step(tb, i, x0, x, nz, eta)
    return x


def run_case(model, case, inputs):
    """One of CASES in fp64 around ``model`` (x, ts, cond) -> x0; ``inputs`` = respace_oracle.inputs()."""
    loop, tag, par, skip, with_init = case
    noise, cond, gt, mask, steps = (a.numpy() for a in inputs)
    base, spec = ro.SCHEDULES[tag]
    from interdiff_amd.diffusion import space_timesteps
    tb = ro.spaced_tables(ro.cosine_betas(base), space_timesteps(base, spec))
    gt64 = gt.astype(np.float64)
    init = INIT_SCALE * gt64 if with_init else None
    kw = dict(mask=mask, gt=gt64, denoised_fn=lambda x0, i: x0 * ro.stub_scale(i))
    net = lambda x, ts: model(x, ts, inputs[1])
    if loop == 'plms':
        return plms_loop(net, tb, noise, par, skip, init, **kw)
    return skipped_loop(net, tb, noise, steps, loop, par or 0.0, skip, init, **kw)


def expected_calls(tag, loop, skip):
    """(model timesteps, hook timesteps) of a case, from the schedule alone: the duplicated t - 1 of the first PLMS step included."""
    from interdiff_amd.diffusion import space_timesteps
    base, spec = ro.SCHEDULES[tag]
    tmap = sorted(space_timesteps(base, spec))
    idx = indices(len(tmap), loop, skip)
    if loop == 'plms':
        idx = [idx[0], idx[0] - 1] + idx[1:]
    return [tmap[i] for i in idx], idx
