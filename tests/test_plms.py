"""PLMS sampling and ``skip_timesteps`` / ``init_image`` on the three loops (interdiff_amd/diffusion.py ``plms_sample_loop``, csrc/plms.hip, the PLMS
route of graph_sampler.py): against tests/golden/plms.npz, recorded from the reference's own loops by tests/golden/make_golden_plms.py, and
against the fp64 restatement tests/plms_oracle.py.

Gate of the whole-loop comparisons: |HIP - fp64 oracle| <= max(4 e_ref, one fp32 ulp of the largest element), e_ref =
max |reference fp32 - fp64 oracle| of the same loop, stored in the fixture.  Route comparisons (graph / eager, shard / whole, loop / steps by
hand) are bit-identity: no tolerance.  The step entries alone are held to 2 fp32 ulp of each expected element (``step_tolerance``).
"""
import functools
import os
import re
import numpy as np
import pytest
import torch
from tests import fixtures as fx
from tests import respace_oracle as ro
from tests import plms_oracle as po
from interdiff_amd import diffusion as dfn
from interdiff_amd import graph_sampler as gs
from interdiff_amd import _lib

DEV = 'cuda'
NEW_ENTRIES = ('interdiff_plms_step_dev', 'interdiff_plms_first_half_dev', 'interdiff_plms_second_half_dev')


@functools.lru_cache(None)
def golden():
    z = fx.golden('plms.npz')
    return {k: z[k] for k in z.files}


def schedule(tag):
    base, spec = ro.SCHEDULES[tag]
    return dfn.create_gaussian_diffusion('cosine', base, spec)


@functools.lru_cache(None)
def oracle_loop(case):
    """The fp64 loop of one recorded case: computed once, shared by the CPU and the GPU comparison, never modified."""
    out = po.run_case(ro.mdm_fp64(fx.mdm_weights()), case, ro.inputs())
    out.setflags(write=False)
    return out


def gate(name):
    """(4 e_ref, the ulp floor) of a recorded loop."""
    return 4.0 * float(golden()[name + '_e_ref']), float(np.spacing(np.float32(np.abs(golden()[name]).max())))


# ------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize('case', po.CASES, ids=po.CASE_IDS)
def test_fp64_oracle_reproduces_recorded_loops(case):
    """The reference's fp32 loop lies e_ref from the fp64 oracle (re-measured here), and the gate 4 e_ref stays between one ulp and the 4e-5 read off
    the figures measured when the loops were first recorded (at most 7.0e-6): a regenerated fixture cannot quietly loosen it."""
    name, z = po.case_name(*case), golden()
    e = float(np.abs(z[name].astype(np.float64) - oracle_loop(case)).max())
    g, ulp = gate(name)
    print('%s: e_ref recorded %.3e, re-measured %.3e, gate %.3e, ulp floor %.3e' % (name, z[name + '_e_ref'], e, g, ulp))
    assert abs(e - float(z[name + '_e_ref'])) <= 1e-9
    assert ulp < g < 4e-5
    if name in po.E_REF_QUOTED:                 # two significant digits were quoted
        assert abs(float(z[name + '_e_ref']) - po.E_REF_QUOTED[name]) <= 0.06e-6, name


def test_recorded_call_sequences():
    """Who was told which timestep by the reference: the second evaluation of the first PLMS step is at t - 1, model and hook alike; p_sample_loop
    skips the END of the schedule (it stops at index skip), the other two its start."""
    z = golden()
    for case in po.CASES:
        name = po.case_name(*case)
        t_model, t_hook = po.expected_calls(case[1], case[0], case[3])
        assert z[name + '_t_model'].tolist() == t_model and z[name + '_t_hook'].tolist() == t_hook, name
    assert z['plms_b_o2_t_model'].tolist() == [29, 20, 20, 19, 14, 10, 9, 6, 3, 0] and z['plms_b_o4_t_hook'].tolist() == [8, 7, 7, 6, 5, 4, 3, 2, 1, 0]
    assert z['ddpm_a_skip3_init_t_hook'].tolist() == [9, 8, 7, 6, 5, 4, 3] and z['ddim_a_eta0_skip3_init_t_hook'].tolist() == [6, 5, 4, 3, 2, 1, 0]
    assert z['plms_a_o2_skip3_t_hook'].tolist() == [6, 5, 5, 4, 3, 2, 1, 0] and z['plms_a_o2_skip3_t_model'].tolist() == [666, 555, 555, 444, 333, 222, 111, 0]


def test_new_entries_are_declared_and_abi_stays():
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(os.path.dirname(fx.GOLDEN), '..', 'include', 'interdiff_hip.h')).read(), flags=re.S)
    lib = _lib.load()
    for name in NEW_ENTRIES:
        assert name in _lib.exported_symbols() and re.search(r'\b%s\s*\(' % name, hdr) and hasattr(lib, name), name
    assert lib.interdiff_abi_version() == _lib.ABI_VERSION == 17


def test_plms_table_is_the_fp64_tables_rounded_once():
    for tag, (base, spec) in ro.SCHEDULES.items():
        d = schedule(tag)
        tb = ro.spaced_tables(ro.cosine_betas(base), dfn.space_timesteps(base, spec))
        abp = tb['alphas_cumprod_prev']
        want = np.stack([tb['sqrt_recip_alphas_cumprod'], tb['sqrt_recipm1_alphas_cumprod'], np.sqrt(abp), np.sqrt(1 - abp)], axis=1)
        rows = d._plms_rows()
        assert rows.dtype == np.float32 and rows.shape == (d.num_timesteps, 4) and rows.flags['C_CONTIGUOUS']
        assert np.array_equal(rows, want.astype(np.float32)), tag
        assert rows[0, 2] == 1.0 and rows[0, 3] == 0.0          # alpha_bar_prev[0] = 1


def test_order_and_sampler_arguments_without_a_device():
    d = schedule('b')
    for bad in (0, 5, 2.0, True, None, '2'):
        with pytest.raises(ValueError):
            d.plms_sample_loop(None, (1, 1, 4, 4), clip_denoised=False, order=bad)
    with pytest.raises(ValueError, match='reference fails there too'):
        d.plms_sample_loop(None, (1, 1, 4, 4), clip_denoised=False, order=1)
    with pytest.raises(ValueError):
        dfn.sample_loop(d, None, (1, 1, 4, 4), sampler='plms')
    with pytest.raises(TypeError):
        d.plms_sample_loop(None, (1, 1, 4, 4), clip_denoised=False, first_t=3)
    assert gs.plan_steps(8, 9, lambda t: t == 0, [3], True, it0=1)[:4] == [('plain', 1), ('plain', 1), ('plain', 1), ('dump', 3)]
    assert gs.plan_steps(9, 10, lambda t: t == 0, None, True) == [('plain', 7), ('plain', 1), ('hook', 1)]


# ------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope='module')
def mdm(lib):
    from interdiff_amd.mdm import MDM
    return MDM(fx.mdm_weights(), device=DEV)


@pytest.fixture(scope='module')
def smpl(lib):
    from interdiff_amd.smpl import SMPL_Layer
    return SMPL_Layer(fx.smpl_model(), device=DEV)


def make_correction(smpl, T, P):
    from interdiff_amd.objprojector import ObjProjector
    from interdiff_amd.correction import HipCorrection
    return HipCorrection(smpl, ObjProjector(fx.objproj_weights(), T=T, past_len=fx.PAST, device=DEV), n_points=P, past_len=fx.PAST, device=DEV)


def dev(x):
    return {k: dev(v) for k, v in x.items()} if isinstance(x, dict) else (x.to(DEV) if isinstance(x, torch.Tensor) else x)


def run_loop(d, loop, par, model, shape, **kw):
    if loop == 'plms':
        return d.plms_sample_loop(model, shape, clip_denoised=False, order=par, **kw)
    if loop == 'ddpm':
        return d.p_sample_loop(model, shape, clip_denoised=False, **kw)
    return d.ddim_sample_loop(model, shape, clip_denoised=False, eta=par, **kw)


class Spy:
    """The denoiser behind a wrapper that notes the timesteps it is called with (not graph-safe: the eager route)."""

    def __init__(self, model):
        self.model, self.seen = model, []

    def __call__(self, x, t, **kw):
        self.seen.append(t.cpu().tolist())
        return self.model(x, t, **kw)


def recorded_inputs():
    noise, cond, gt, mask, steps = (a.to(DEV) for a in ro.inputs())
    return noise, {'y': dict(cond=cond, inpainted_motion=gt, inpainting_mask=mask)}, steps


def stub_hook(seen):
    def hook(x, t, model_kwargs):
        seen.append((t.host_value, t.cpu().tolist()))
        return x * ro.stub_scale(t.host_value)
    return hook


def case_kw(case, kw, steps):
    """The keywords of a recorded case beside the loop's own."""
    loop, tag, par, skip, with_init = case
    out = dict(skip_timesteps=skip, init_image=po.INIT_SCALE * kw['y']['inpainted_motion'] if with_init else None)
    if loop != 'plms':
        out['step_noise'] = steps
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('case', po.CASES, ids=po.CASE_IDS)
def test_eager_loops_against_reference(mdm, case):
    """1: the eager route with the recorded noise against the fp64 oracle at the reference's own error, and who is told which timestep.

    Measured on an MI355X, |HIP - fp64 oracle| / gate 4 e_ref: plms_b_o2 1.42e-6 / 8.97e-6, plms_b_o3 1.59e-6 / 1.29e-5, plms_b_o4 2.01e-6 / 1.66e-5, plms_b_o4_skip2_init 8.41e-7 / 6.97e-6,
    plms_a_o4_skip2_init 1.27e-6 / 2.80e-5, plms_a_o2_skip3 7.13e-7 / 9.19e-6, ddpm_a_skip3_init 4.72e-7 / 2.98e-6, ddpm_b_skip2 5.34e-7 / 3.61e-6, ddim_a_eta0_skip3_init 6.41e-7 / 1.08e-5,
    ddim_b_eta1_skip2 6.44e-7 / 5.19e-6: each below the reference's own e_ref."""
    loop, tag, par, skip, with_init = case
    name, z, d = po.case_name(*case), golden(), schedule(tag)
    noise, kw, steps = recorded_inputs()
    spy, seen = Spy(mdm), []
    got = run_loop(d, loop, par, spy, tuple(noise.shape), noise=noise, model_kwargs=kw, denoised_fn=stub_hook(seen), device=DEV, **case_kw(case, kw, steps))
    got64 = got.cpu().numpy().astype(np.float64)
    dist, to_ref = float(np.abs(got64 - oracle_loop(case)).max()), float(np.abs(got64 - z[name]).max())
    g, ulp = gate(name)
    print('%s: |HIP - fp64 oracle| %.3e (gate 4 e_ref = %.3e, ulp floor %.3e), |HIP - reference fp32| %.3e' % (name, dist, g, ulp, to_ref))
    assert [s[0] for s in spy.seen] == z[name + '_t_model'].tolist() and all(len(set(s)) == 1 and len(s) == ro.B for s in spy.seen)
    assert [h for h, _ in seen] == z[name + '_t_hook'].tolist() and all(t == [h] * ro.B for h, t in seen)
    assert dist <= max(g, ulp), '%s: %.3e > %.3e' % (name, dist, max(g, ulp))


# ---- 2: the step entries alone
def f64(t):
    return t.detach().cpu().numpy().astype(np.float64)


def ab_weights(k):
    return {1: ((1.0,), 1.0), 2: ((3.0, -1.0), 2.0), 3: ((23.0, -16.0, 5.0), 12.0), 4: ((55.0, -59.0, 37.0, -9.0), 24.0)}[k]


def step_tolerance(want, scale):
    """2 fp32 ulp of every expected element (the bound the step entries are held to), plus the error of the fp64 EVALUATION it is compared with:
    a sum of products formed in fp64 is off by at most a few 2^-53 of the sum of the magnitudes of its terms (``scale``, elementwise) -- 16 x
    2^-53 covers the six operations of the longest expression here and matters only where the terms cancel to below 1e-8 of their size."""
    return 2.0 * np.spacing(np.abs(want.astype(np.float32))).astype(np.float64) + 16.0 * 2.0 ** -53 * scale


def expect_eps(row, x, p):
    return (row[0] * x - p) / row[1], (np.abs(row[0] * x) + np.abs(p)) / row[1]


def expect_update(row, x, ep, ep_scale):
    want = row[2] * (row[0] * x - row[1] * ep) + row[3] * ep
    return want, row[2] * (np.abs(row[0] * x) + row[1] * ep_scale) + row[3] * ep_scale


def check_close(got, want, scale, what):
    err = np.abs(f64(got).ravel() - want.astype(np.float32).astype(np.float64))
    tol = step_tolerance(want, scale)
    worst = int(np.argmax(err - tol))
    print('%s: max err %.3e, in ulp of its element %.2f' % (what, err.max(), (err / np.spacing(np.abs(want.astype(np.float32))).astype(np.float64)).max()))
    assert (err <= tol).all(), '%s: element %d off by %.3e > %.3e' % (what, worst, err[worst], tol[worst])


@pytest.mark.gpu
@pytest.mark.parametrize('n,B', [(1003, 5), (8640, 3)], ids=['scalar_n1003', 'vector_n8640'])
@pytest.mark.parametrize('inpaint', [False, True], ids=['plain', 'gt_mask'])
def test_step_entries_against_numpy(lib, n, B, inpaint):
    """2: n = 1003 takes the scalar form (four workgroups), n = 8640 the 16-byte one (nine); schedule 'b' (a real timestep map) from its last index
    down to 0: both halves of the first step, then eight plain steps at order 4 -- cur_order 2, 3, 4, the ring wrapping through five steps at
    cur_order 4, t == 0 last -- and one lone plain step at loop index 0 (cur_order 1).  Every step is compared on ITS device inputs (x, the ring
    as the kernels left it), so nothing accumulates: each result within 2 ulp of the fp64 evaluation rounded to fp32; state and ts exact."""
    d = schedule('b')
    rows, tmap_l, N = d._plms_rows().astype(np.float64), d.timestep_map, d.num_timesteps
    ptable, tmap = d._plms_table(torch.device(DEV)), d._tmap(DEV)
    gen = torch.Generator().manual_seed(4100 + n)
    rnd = lambda *s: torch.randn(*s, generator=gen).to(DEV)
    gt, mask = (rnd(n), (torch.rand(n, generator=gen) < 0.4).to(DEV).view(torch.uint8)) if inpaint else (None, None)
    pick = lambda x0: np.where(f64(mask) != 0, f64(gt), f64(x0)) if inpaint else f64(x0)
    x, ring, x_mid = rnd(n), torch.full((3, n), float('nan'), device=DEV), torch.full((n,), float('nan'), device=DEV)
    state, ts = dfn.seeded_state(N - 1, 77, 0).to(DEV), torch.full((B,), tmap_l[N - 1], dtype=torch.int64, device=DEV)
    # first step, half one at t = N - 1
    t, x_in, x0 = N - 1, f64(x), rnd(n)
    gs.plms_first_half(x, x0, gt, mask, ring, x_mid, ptable, state, ts, tmap)
    eps, eps_s = expect_eps(rows[t], x_in, pick(x0))
    check_close(ring[0], eps, eps_s, 'half one eps')
    check_close(x_mid, pick(x0) * rows[t][2] + rows[t][3] * eps, np.abs(pick(x0)) * rows[t][2] + rows[t][3] * eps_s, 'x_mid')
    assert np.array_equal(f64(x), x_in), 'half one must not write x'
    assert state.tolist() == [t - 1, 0, 77, 0, 0, 0, 0, 0] and ts.tolist() == [tmap_l[t - 1]] * B
    # ... half two with the second x0
    x0b, e1, mid = rnd(n), f64(ring[0]), f64(x_mid)
    gs.plms_second_half(x, x0b, gt, mask, ring, x_mid, ptable, state)
    eps2, eps2_s = expect_eps(rows[t - 1], mid, pick(x0b))
    want, scale = expect_update(rows[t], x_in, (e1 + eps2) / 2, (np.abs(e1) + eps2_s) / 2)
    check_close(x, want, scale, 'half two x')
    assert np.array_equal(f64(ring[0]), e1), 'the ring keeps eps, not eps prime'
    assert state.tolist() == [t - 1, 1, 77, 0, 0, 0, 0, 0] and ts.tolist() == [tmap_l[t - 1]] * B
    # plain steps t = N - 2 .. 0 at order 4
    for it, t in enumerate(range(N - 2, -1, -1), start=1):
        x_in, ring_in, x0 = f64(x), f64(ring), rnd(n)
        gs.plms_step(x, x0, gt, mask, ring, 4, ptable, state, ts, tmap)
        eps, eps_s = expect_eps(rows[t], x_in, pick(x0))
        k = min(4, it + 1)
        w, den = ab_weights(k)
        old = [ring_in[(it - j) % 3] for j in range(1, k)]
        ep = sum(wj * e for wj, e in zip(w, [eps] + old)) / den
        ep_s = sum(abs(wj) * e for wj, e in zip(w, [eps_s] + [np.abs(o) for o in old])) / den
        want, scale = expect_update(rows[t], x_in, ep, ep_s) if t else (pick(x0), np.zeros(n))
        check_close(x, want, scale, 'step t = %d, cur_order %d' % (t, k))
        check_close(ring[it % 3], eps, eps_s, 'ring eps, t = %d' % t)
        for j in range(3):
            assert j == it % 3 or np.array_equal(f64(ring[j]), ring_in[j], equal_nan=True), 'only the oldest slot is written'      # (slots not yet filled hold the NaN they were given)
        assert state.tolist() == [t - 1, it + 1, 77, 0, 0, 0, 0, 0] and ts.tolist() == [tmap_l[max(t - 1, 0)]] * B
    assert it == N - 1 >= 8                      # cur_order 4 from loop index 3 on: five steps and more
    # cur_order 1: a plain step at loop index 0 (the ring holds nothing yet)
    state.copy_(dfn.seeded_state(5, 3, 0))
    x_in, x0 = f64(x), rnd(n)
    gs.plms_step(x, x0, gt, mask, ring, 3, ptable, state, ts, tmap)
    eps, eps_s = expect_eps(rows[5], x_in, pick(x0))
    want, scale = expect_update(rows[5], x_in, eps, eps_s)
    check_close(x, want, scale, 'cur_order 1')
    assert state.tolist() == [4, 1, 3, 0, 0, 0, 0, 0] and ts.tolist() == [tmap_l[4]] * B


@pytest.mark.gpu
def test_step_entries_refuse_bad_arguments(lib):
    x, ring, state, ts = torch.zeros(8, device=DEV), torch.zeros(3, 8, device=DEV), dfn.seeded_state(1, 0, 0).to(DEV), torch.zeros(2, dtype=torch.int64, device=DEV)
    ptable = schedule('b')._plms_table(torch.device(DEV))
    for order in (0, 5):
        with pytest.raises(RuntimeError, match='IDF_E_INVAL'):
            gs.plms_step(x, x, None, None, ring, order, ptable, state, ts)
    rc = lib.interdiff_plms_step_dev(_lib.dptr(x), _lib.dptr(x), None, _lib.dptr(torch.zeros(8, dtype=torch.uint8, device=DEV)), _lib.dptr(ring), 8, 2,
                                     _lib.dptr(ptable), None, _lib.dptr(state), _lib.dptr(ts), 2, _lib.stream())
    assert rc == -22, 'a mask without gt'
    assert state.tolist()[:2] == [1, 0]


# ---- 3: loop against steps by hand
@pytest.mark.gpu
def test_plms_loop_equals_steps_by_hand(lib, mdm):
    """3: forward, inpaint, stub and the step entries by hand are the loop bit for bit (order 3 on schedule 'b', skip 1 with an init_image)."""
    d = schedule('b')
    noise, kw, _ = recorded_inputs()
    y, N, skip = kw['y'], d.num_timesteps, 1
    init = po.INIT_SCALE * y['inpainted_motion']
    loop = d.plms_sample_loop(mdm, tuple(noise.shape), noise=noise, clip_denoised=False, model_kwargs=kw, denoised_fn=stub_hook([]), order=3, skip_timesteps=skip,
                              init_image=init)
    first = N - 1 - skip
    x = d.q_sample(init, torch.full((ro.B,), first, dtype=torch.int64, device=DEV), noise=noise)
    ptable, tmap = d._plms_table(torch.device(DEV)), d._tmap(DEV)
    state, ts = dfn.seeded_state(first, 0, 0).to(DEV), torch.full((ro.B,), d.timestep_map[first], dtype=torch.int64, device=DEV)
    ring, x_mid = torch.empty(3, x.numel(), device=DEV), torch.empty_like(x)

    def x0_of(xin, i):
        assert ts.tolist() == [d.timestep_map[i]] * ro.B and state[0].item() == i
        x0 = mdm(xin, ts.clone(), **kw)
        dfn.inpaint(x0, y['inpainted_motion'], y['inpainting_mask'].view(torch.uint8))
        return x0 * ro.stub_scale(i)
    for it, i in enumerate(range(first, -1, -1)):
        x0 = x0_of(x, i)
        if it == 0:
            gs.plms_first_half(x, x0, None, None, ring, x_mid, ptable, state, ts, tmap)
            gs.plms_second_half(x, x0_of(x_mid, i - 1), None, None, ring, x_mid, ptable, state)
        else:
            gs.plms_step(x, x0, None, None, ring, 3, ptable, state, ts, tmap)
    assert torch.equal(x, loop), (x - loop).abs().max()
    assert torch.isfinite(loop).all() and not torch.equal(loop, noise)


@pytest.mark.gpu
def test_skipped_ddpm_loop_equals_steps_by_hand(lib, mdm):
    """3: p_sample_loop(skip_timesteps=2) on schedule 'b' with an init_image: q_sample at N - 1, then indices N - 1 .. 2, the last one with noise."""
    d = schedule('b')
    noise, kw, steps = recorded_inputs()
    y, N, skip = kw['y'], d.num_timesteps, 2
    init = po.INIT_SCALE * y['inpainted_motion']
    loop = d.p_sample_loop(mdm, tuple(noise.shape), noise=noise, clip_denoised=False, model_kwargs=kw, denoised_fn=stub_hook([]), step_noise=steps,
                           skip_timesteps=skip, init_image=init)
    x, rows = d.q_sample(init, torch.full((ro.B,), N - 1, dtype=torch.int64, device=DEV), noise=noise), d._rows()
    for it, i in enumerate(range(N - 1, skip - 1, -1)):
        x0 = mdm(x, torch.full((ro.B,), d.timestep_map[i], dtype=torch.int64, device=DEV), **kw)
        dfn.inpaint(x0, y['inpainted_motion'], y['inpainting_mask'].view(torch.uint8))
        x0 = x0 * ro.stub_scale(i)
        assert rows[i, 2] > 0
        _lib.check(lib.interdiff_posterior_step(_lib.dptr(x), _lib.dptr(x0), _lib.dptr(steps[it].contiguous()), x.numel(), float(rows[i, 0]), float(rows[i, 1]),
                                                float(rows[i, 2]), 0, it, _lib.stream()), 'posterior_step')
    assert it == N - skip - 1 and torch.equal(x, loop), (x - loop).abs().max()


# ---- 4: graph route against eager route
def hooked_case(seed, B, smpl):
    bt = fx._clip(seed, B, ro.T, ro.P)
    return bt['noise'].to(DEV), {'y': dev(fx.model_kwargs_y(bt, ro.T))}, make_correction(smpl, ro.T, ro.P)


def entries(model, d, shape):
    return [v for k, v in model._graph_cache.items() if k[0] == d._uid and k[1] == tuple(shape)]


@pytest.mark.gpu
@pytest.mark.parametrize('order', [2, 4])
def test_plms_graph_route_equals_eager_route(mdm, smpl, order):
    """4: PLMS on '10' (the hook gate passes the spaced index 0), captured first step, blocks and hook step == the eager loop; B = 3 and 4; graph
    reuse; dump_steps equal on both routes (the first step is loop step 0)."""
    d = dfn.create_gaussian_diffusion('cosine', 1000, '10')
    for B in (3, 4):
        noise, kw, corr = hooked_case(60 + B, B, smpl)
        for hook in (None, corr):
            run = lambda seed=11, **k: d.plms_sample_loop(mdm, tuple(noise.shape), noise=noise, clip_denoised=False, model_kwargs=kw, denoised_fn=hook, order=order, seed=seed, **k)
            graph, eager = run(), run(use_graph=False)
            assert torch.isfinite(graph).all()
            assert torch.equal(graph, eager), 'B = %d, hook %s: %g' % (B, hook is not None, (graph - eager).abs().max())
            assert torch.equal(graph, run()), 'graph reuse'
            assert torch.equal(graph, run(seed=12)), 'x_T given: nothing is drawn'
            dumps = (0, 1, 4, 9)
            dg, de = run(dump_steps=dumps), run(dump_steps=dumps, use_graph=False)
            assert len(dg) == len(de) == 4 and all(torch.equal(p, q) for p, q in zip(dg, de)) and torch.equal(dg[-1], graph)
            assert not torch.equal(dg[0], dg[1])
        st = [e for e in entries(mdm, d, noise.shape) if e.ring is not None]
        assert len(st) == 1 and st[0].graphs and not st[0].chains, 'the captured PLMS route was not taken (one chain)'
        assert any(isinstance(k, tuple) and k[0] == 'first' for k in st[0].graphs), 'no captured first step'
        assert any(isinstance(k, tuple) and k[0] == 'hook' for k in st[0].graphs), 'no captured hook step'
    other = d.plms_sample_loop(mdm, tuple(noise.shape), noise=noise, clip_denoised=False, model_kwargs=kw, order=6 - order, seed=11)
    assert not torch.equal(other, d.plms_sample_loop(mdm, tuple(noise.shape), noise=noise, clip_denoised=False, model_kwargs=kw, order=order, seed=11)), 'orders 2 and 4 differ'


class CountingHook:
    """A correction hook that is not capturable (the graph route calls it eagerly) and notes the steps at which its gate passed."""

    def __init__(self, hook):
        self.hook, self.taken = hook, []

    def is_active(self, t):
        return self.hook.is_active(t)

    def __call__(self, x, t, model_kwargs):
        if self.hook.is_active(t.host_value):
            self.taken.append(t.host_value)
        return self.hook(x, t, model_kwargs)


@pytest.mark.gpu
def test_plms_first_step_with_an_active_second_hook_call(mdm, smpl):
    """4: order 4 on '100' with skip_timesteps=48: the first step is at spaced 51, so its SECOND call is the active hook step 50 (the blend weight
    read at ``state[0]`` == 50); hook steps 50 (in the first step's second call and again as the step at 50 itself) and 0 are taken; captured hook == eager hook on the graph route == the eager loop."""
    d = dfn.create_gaussian_diffusion('cosine', 1000, '100')
    for B in (3, 4):
        noise, kw, corr = hooked_case(90 + B, B, smpl)
        run = lambda hook, **k: d.plms_sample_loop(mdm, tuple(noise.shape), noise=noise, clip_denoised=False, model_kwargs=kw, denoised_fn=hook, order=4,
                                                   skip_timesteps=48, **k)
        counted = CountingHook(corr)
        eager = run(counted, use_graph=False)
        assert counted.taken == [50, 50, 0]      # 50 twice, as the reference tells its hook t - 1 and then t = 50 itself ([8, 7, 7, ...] in the fixture)
        graph = run(corr)
        assert torch.isfinite(graph).all() and torch.equal(graph, eager), (graph - eager).abs().max()
        st = [e for e in entries(mdm, d, noise.shape) if e.ring is not None]
        assert len(st) == 1 and ('first', corr._uid, False, True) in st[0].graphs, 'the second call of the first step was not captured with the hook'
        assert any(isinstance(k, tuple) and k[0] == 'hook' for k in st[0].graphs)
        counted.taken.clear()
        assert torch.equal(run(counted), eager), 'eager hook calls between replays'
        assert counted.taken == [50, 50, 0]
        assert not torch.equal(run(None), eager), 'the hook must matter'


@pytest.mark.gpu
@pytest.mark.parametrize('loop,par', [('ddpm', None), ('ddim', 1.0)])
def test_skipped_graph_route_equals_eager_route(mdm, smpl, loop, par):
    """4: skip_timesteps on the captured DDPM / DDIM routes, with and without the hook ('100', skip 40: DDPM runs 99 .. 40 and takes hook step 50,
    DDIM runs 59 .. 0 and takes 50 and 0); a skipped DDPM run at B = 4 still splits into two chains."""
    d = dfn.create_gaussian_diffusion('cosine', 1000, '100')
    d.split_min_rows = 0
    for B in (3, 4):
        noise, kw, corr = hooked_case(70 + B, B, smpl)
        init = po.INIT_SCALE * kw['y']['inpainted_motion']
        for hook in (None, corr):
            run = lambda **k: run_loop(d, loop, par, mdm, tuple(noise.shape), noise=noise, model_kwargs=kw, denoised_fn=hook, seed=11, skip_timesteps=40, init_image=init, **k)
            graph, eager = run(), run(use_graph=False)
            assert torch.isfinite(graph).all() and torch.equal(graph, eager), 'B = %d, hook %s: %g' % (B, hook is not None, (graph - eager).abs().max())
        st = entries(mdm, d, noise.shape)
        assert len(st) == 1 and st[0].graphs, 'the captured route was not taken'
        assert (len(st[0].chains) == 2) == (B == 4)
        assert any(isinstance(k, tuple) and k[0] == 'hook' for k in st[0].graphs), 'no captured hook step'


# ---- 5: shards
@pytest.mark.gpu
@pytest.mark.parametrize('loop,par', [('plms', 3), ('ddpm', None)])
def test_shard_equals_whole(mdm, loop, par):
    """5: B = 4 as 2 + 2, x_T drawn in the kernel at the whole batch's counters; PLMS order 3 with an init_image (the shard's slice), DDPM with skip_timesteps."""
    d = schedule('a')
    bt = fx._clip(71, 4, ro.T, ro.P)
    y = dev(fx.model_kwargs_y(bt, ro.T))
    shape = tuple(bt['noise'].shape)
    cut = lambda sl: {'y': dict(cond=y['cond'][:, sl].contiguous(), inpainted_motion=y['inpainted_motion'][sl].contiguous(), inpainting_mask=y['inpainting_mask'][sl].contiguous())}
    init = po.INIT_SCALE * y['inpainted_motion'] if loop == 'plms' else None
    extra = lambda sl: dict(skip_timesteps=2, init_image=None if init is None else init[sl].contiguous())
    whole = run_loop(d, loop, par, mdm, shape, model_kwargs=cut(slice(0, 4)), seed=5, **extra(slice(0, 4)))
    for first in (0, 2):
        sl = slice(first, first + 2)
        part = run_loop(d, loop, par, mdm, (2,) + shape[1:], model_kwargs=cut(sl), seed=5, shard=(first, 4), **extra(sl))
        assert torch.equal(part, whole[sl]), (first, (part - whole[sl]).abs().max())
    alone = run_loop(d, loop, par, mdm, (2,) + shape[1:], model_kwargs=cut(slice(2, 4)), seed=5, **extra(slice(2, 4)))
    assert not torch.equal(alone, whole[2:]), 'a shard without its position must be another sample'


# ---- 6: the skeleton denoiser
@pytest.mark.gpu
def test_skeleton_denoiser_plms_graph_equals_eager(lib):
    """6: PLMS order 4 on cosine 50 -> '10' around SkeletonMDM (a top-level zero_pose_obj beside y), B = 1, T = 20."""
    from interdiff_amd import skeleton as sk
    from interdiff_amd import synthetic as syn
    seed = int(fx.golden('skel_mdm.npz')['seed'])
    model = sk.SkeletonMDM({k: torch.from_numpy(v) for k, v in syn.skeleton_mdm_state_dict(seed).items()}, device=DEV, n_steps=50)
    B, T = 1, 20
    bt = syn.make_skeleton_batch(5021, B=B, T=T)
    rs = np.random.RandomState(5022)
    gt = torch.from_numpy(np.ascontiguousarray(np.concatenate([bt['body'].reshape(B, T, -1), bt['obj'].reshape(B, T, -1), bt['pose']], axis=2).transpose(0, 2, 1)[:, None]))
    mask = torch.ones(gt.shape, dtype=torch.bool)
    mask[..., fx.PAST:] = False
    kw = {'y': {'cond': fx._randn(rs, fx.PAST, B, 256).to(DEV), 'inpainted_motion': gt.to(DEV), 'inpainting_mask': mask.to(DEV)},
          'zero_pose_obj': torch.from_numpy(bt['zero_pose_obj']).to(DEV)}
    noise = fx._randn(rs, B, 1, 106, T).to(DEV)
    d = dfn.create_gaussian_diffusion('cosine', 50, '10')
    run = lambda **k: d.plms_sample_loop(model, tuple(noise.shape), noise=noise, clip_denoised=False, model_kwargs=kw, order=4, **k)
    graph, eager = run(), run(use_graph=False)
    assert torch.isfinite(graph).all() and torch.equal(graph, eager), (graph - eager).abs().max()
    assert any(k[0] == d._uid and st.graphs and st.ring is not None for k, st in model._graph_cache.items()), 'the captured route was not taken'
    assert torch.equal(graph[..., :fx.PAST], gt.to(DEV)[..., :fx.PAST]), 'the last step returns the inpainted x0'


# ---- 7: semantics
@pytest.mark.gpu
def test_skip_and_init_semantics(mdm):
    """7."""
    d = schedule('a')
    noise, kw, _ = recorded_inputs()
    N, k, shape = d.num_timesteps, 3, tuple(noise.shape)
    zeros = torch.zeros_like(noise)
    for loop, par in (('ddpm', None), ('ddim', 0.0), ('plms', 2)):
        a = run_loop(d, loop, par, mdm, shape, noise=noise, model_kwargs=kw, seed=4, skip_timesteps=k)
        b = run_loop(d, loop, par, mdm, shape, noise=noise, model_kwargs=kw, seed=4, skip_timesteps=k, init_image=zeros)
        assert torch.equal(a, b), loop
        c = run_loop(d, loop, par, mdm, shape, noise=noise, model_kwargs=kw, seed=4, init_image=zeros)
        assert torch.isfinite(c).all() and not torch.equal(a, c), loop          # init_image alone: noised at the first index, every step run
    # p_sample_loop(skip_timesteps=k) is the window first_t = N - 1, n_steps = N - k of today's loop, started from q_sample(zeros, N - 1, z)
    start = d.q_sample(zeros, torch.full((ro.B,), N - 1, dtype=torch.int64, device=DEV), noise=noise)
    for route in (True, False):
        a = d.p_sample_loop(mdm, shape, noise=noise, clip_denoised=False, model_kwargs=kw, seed=4, skip_timesteps=k, use_graph=route)
        b = d.p_sample_loop(mdm, shape, noise=start, clip_denoised=False, model_kwargs=kw, seed=4, first_t=N - 1, n_steps=N - k, use_graph=route)
        assert torch.equal(a, b), route
    assert not torch.equal(a, d.p_sample_loop(mdm, shape, noise=noise, clip_denoised=False, model_kwargs=kw, seed=5, skip_timesteps=k)), 'its last step draws noise'
    # a drawn x_T of p_sample_loop is inpainted BEFORE it is noised; PLMS leaves its drawn x_T alone, and with x_T given the seed is idle
    p = lambda seed, **kk: d.plms_sample_loop(mdm, shape, clip_denoised=False, model_kwargs=kw, order=2, seed=seed, **kk)
    assert torch.equal(p(1, noise=noise), p(2, noise=noise)) and not torch.equal(p(1), p(2)) and torch.equal(p(1), p(1))
    assert not torch.equal(p(1, noise=noise), d.plms_sample_loop(mdm, shape, noise=noise, clip_denoised=False, model_kwargs=kw, order=4, seed=1)), 'orders differ'
    xT = torch.empty_like(noise)
    _lib.check(_lib.load().interdiff_randn_at(_lib.dptr(xT), xT.numel(), 9, 0xFFFFFFFF, 0, _lib.stream()), 'randn')
    assert torch.equal(p(9), p(9, noise=xT)), 'x_T is drawn at the counter the other loops use, and not inpainted'
    y = kw['y']
    xT_in = torch.where(y['inpainting_mask'], y['inpainted_motion'], xT)
    assert torch.equal(d.p_sample_loop(mdm, shape, clip_denoised=False, model_kwargs=kw, seed=9, skip_timesteps=k, init_image=zeros),
                       d.p_sample_loop(mdm, shape, noise=xT_in, clip_denoised=False, model_kwargs=kw, seed=9, skip_timesteps=k, init_image=zeros))


# ---- 8: argument checks
@pytest.mark.gpu
def test_argument_checks(mdm):
    """8: every refusal of the new keywords, and the loop_kw callers."""
    from interdiff_amd import losses as L
    d = schedule('a')
    noise, kw, _ = recorded_inputs()
    shape, N = tuple(noise.shape), d.num_timesteps
    base = dict(noise=noise, clip_denoised=False, model_kwargs=kw)
    loops = (d.p_sample_loop, d.ddim_sample_loop, lambda *a, **k: d.plms_sample_loop(*a, order=2, **k))
    for loop in loops:
        for bad in (N, N + 5, -1):
            with pytest.raises(ValueError):
                loop(mdm, shape, skip_timesteps=bad, **base)
        for bad_init in (noise[:2], noise[..., :5], noise.double(), noise.half()):
            with pytest.raises(ValueError):
                loop(mdm, shape, init_image=bad_init, **base)
        with pytest.raises(NotImplementedError):
            loop(mdm, shape, noise=noise, clip_denoised=True, model_kwargs=kw)
        for refused in (dict(cond_fn=lambda *a: None), dict(randomize_class=True), dict(cond_fn_with_grad=True)):
            with pytest.raises(NotImplementedError):
                loop(mdm, shape, **refused, **base)
    for loop in (d.p_sample_loop, d.ddim_sample_loop):
        for both in (dict(skip_timesteps=2), dict(init_image=noise)):
            with pytest.raises(ValueError):
                loop(mdm, shape, first_t=5, **both, **base)
    with pytest.raises(TypeError):
        d.plms_sample_loop(mdm, shape, order=2, first_t=5, **base)
    with pytest.raises(ValueError):
        d.plms_sample_loop(mdm, shape, order=2, skip_timesteps=N - 1, **base)          # one step left: the reference would index step -1
    assert torch.isfinite(d.plms_sample_loop(mdm, shape, order=2, skip_timesteps=N - 2, **base)).all()
    assert torch.isfinite(d.ddim_sample_loop(mdm, shape, skip_timesteps=N - 1, **base)).all()
    for bad in (0, 1, 5, 2.5):
        with pytest.raises(ValueError):
            d.plms_sample_loop(mdm, shape, order=bad, **base)
    with pytest.raises(ValueError, match='reference fails there too'):
        d.plms_sample_loop(mdm, shape, order=1, **base)
    with pytest.raises(ValueError):
        dfn.sample_loop(d, mdm, shape, sampler='plms', **base)
    with pytest.raises(ValueError):
        dfn.sample_loop(d, mdm, shape, sampler='euler', **base)
    via = dfn.sample_loop(d, mdm, shape, sampler='plms', order=3, skip_timesteps=1, **base)
    assert torch.equal(via, d.plms_sample_loop(mdm, shape, order=3, skip_timesteps=1, **base))
    bt = fx._clip(33, 2, ro.T, ro.P)
    batch = dict(gt=bt['gt'].to(DEV), cond=bt['cond'].to(DEV), hand_pose=bt['hand_pose'].to(DEV))
    loss, terms, _ = L.validation_step(mdm, d, batch, past_len=fx.PAST, seed=41, sampler='plms', order=2, n_steps=3)
    assert bool(torch.isfinite(loss).all()) and all(bool(torch.isfinite(v).all()) for v in terms.values())
