"""Respaced schedules and DDIM sampling (interdiff_amd/diffusion.py ``space_timesteps`` / ``SpacedDiffusion`` / ``ddim_sample_loop``; the
device timestep map of csrc/philox.h): against tests/golden/respace.npz, recorded from the reference's own respace.py / gaussian_diffusion.py
by tests/golden/make_golden_respace.py, and against the fp64 restatement tests/respace_oracle.py.

Gate of the whole-loop comparisons: |HIP - fp64 oracle| <= max(4 e_ref, one fp32 ulp of the largest element), e_ref =
max |reference fp32 - fp64 oracle| of the same loop, measured when the fixture was made and stored in it.  Route comparisons (graph / eager,
shard / whole, identity map / none) are bit-identity: no tolerance.
"""
import functools
import numpy as np
import pytest
import torch
from tests import fixtures as fx
from tests import respace_oracle as ro
from interdiff_amd import diffusion as dfn
from interdiff_amd import _lib

DEV = 'cuda'
TABLES = ('betas', 'alphas_cumprod', 'alphas_cumprod_prev', 'posterior_variance', 'posterior_log_variance_clipped', 'posterior_mean_coef1',
          'posterior_mean_coef2')
LOOP_IDS = [ro.loop_name(tag, s, e) for tag in ro.SCHEDULES for s, e in ro.LOOPS]
LOOP_CASES = [(tag, s, e) for tag in ro.SCHEDULES for s, e in ro.LOOPS]


@functools.lru_cache(None)
def golden():
    z = fx.golden('respace.npz')
    return {k: z[k] for k in z.files}


def schedule(tag):
    base, spec = ro.SCHEDULES[tag]
    return dfn.create_gaussian_diffusion('cosine', base, spec)


@functools.lru_cache(None)
def oracle_loop(tag, sampler, eta):
    """The fp64 loop of one recorded case: computed once, shared by the CPU and the GPU comparison, never modified."""
    base, spec = ro.SCHEDULES[tag]
    noise, cond, gt, mask, steps = ro.inputs()
    model = ro.mdm_fp64(fx.mdm_weights())
    tb = ro.spaced_tables(ro.cosine_betas(base), dfn.space_timesteps(base, spec))
    out = ro.sample_loop(lambda x, ts: model(x, ts, cond), tb, noise.numpy(), steps.numpy(), sampler, eta or 0.0, mask.numpy(),
                         gt.numpy().astype(np.float64), lambda x0, i: x0 * ro.stub_scale(i))
    out.setflags(write=False)
    return out


def gate(tag, sampler, eta):
    """(4 e_ref, the ulp floor) of a recorded loop."""
    name = ro.loop_name(tag, sampler, eta)
    ulp = float(np.spacing(np.float32(np.abs(golden()[name]).max())))
    return 4.0 * float(golden()[name + '_e_ref']), ulp


# ------------------------------------------------------------------------------------------ CPU
def test_space_timesteps_equals_reference():
    z = golden()
    for k, (n, spec) in enumerate(ro.SPECS):
        got = dfn.space_timesteps(n, spec)
        assert isinstance(got, set) and sorted(got) == z['spec_%d' % k].tolist(), (n, spec)
    assert len(dfn.space_timesteps(1000, 'ddim8')) == 8 and len(dfn.space_timesteps(30, [4, 3, 2])) == 9 and len(dfn.space_timesteps(1000, '10')) == 10
    for n, spec in ro.BAD_SPECS:
        with pytest.raises(ValueError):
            dfn.space_timesteps(n, spec)


def test_spaced_tables_equal_reference_fp64():
    z = golden()
    for tag, (base, spec) in ro.SCHEDULES.items():
        d = schedule(tag)
        assert d.timestep_map == z[tag + '_timestep_map'].tolist() and d.original_num_steps == base and d.num_timesteps == len(d.timestep_map)
        assert d.is_respaced
        tb = ro.spaced_tables(ro.cosine_betas(base), dfn.space_timesteps(base, spec))
        for name in TABLES:
            want = z['%s_%s' % (tag, name)]
            for got in (getattr(d, name), tb[name]):
                assert got.dtype == np.float64 and np.abs(got - want).max() <= 1e-14 * np.abs(want).max(), (tag, name)


def test_folded_ddim_scalars_reproduce_unfolded_step():
    rs = np.random.RandomState(12)
    for tag, (base, spec) in ro.SCHEDULES.items():
        d = schedule(tag)
        tb = ro.spaced_tables(ro.cosine_betas(base), dfn.space_timesteps(base, spec))
        for eta in (0.0, 0.3, 1.0):
            c1, c2, sigma = dfn.ddim_coefficients(d.alphas_cumprod, d.alphas_cumprod_prev, eta)
            assert c1.dtype == c2.dtype == sigma.dtype == np.float64
            rows = d._rows(('ddim', eta))
            assert rows.dtype == np.float32 and rows[0, 2] == 0.0 and np.array_equal(rows[:, 3], (np.arange(len(c1), dtype=np.float32) / np.float32(1000)))
            assert np.array_equal(rows[1:, 2], sigma[1:].astype(np.float32)) and np.array_equal(rows[:, 0], c1.astype(np.float32))
            for i in range(d.num_timesteps):
                x0, x, nz = rs.standard_normal((3, 64))
                want = ro.ddim_step(tb, i, x0, x, nz, eta)
                got = c1[i] * x0 + c2[i] * x + (0.0 if i == 0 else sigma[i]) * nz
                assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), (tag, eta, i)


@pytest.mark.parametrize('tag,sampler,eta', LOOP_CASES, ids=LOOP_IDS)
def test_fp64_oracle_reproduces_recorded_loops(tag, sampler, eta):
    """The recorded fp32 loop of the reference lies e_ref from the fp64 oracle (re-measured here: the same figure up to the fp64 rounding of another
    BLAS), and the gate 4 e_ref that the GPU tests use is a few 1e-6 absolute on values of size 1.7 -- the reference's own error, not a loose bound."""
    name = ro.loop_name(tag, sampler, eta)
    z = golden()
    e = float(np.abs(z[name].astype(np.float64) - oracle_loop(tag, sampler, eta)).max())
    g, ulp = gate(tag, sampler, eta)
    print('%s: e_ref recorded %.3e, re-measured %.3e, gate %.3e, ulp floor %.3e' % (name, z[name + '_e_ref'], e, g, ulp))
    assert abs(e - float(z[name + '_e_ref'])) <= 1e-9
    assert ulp < g < 2e-5
    tm = np.array(schedule(tag).timestep_map)[::-1]
    assert np.array_equal(z[name + '_t_model'], tm) and np.array_equal(z[name + '_t_hook'], np.arange(len(tm))[::-1])


def test_no_respacing_builds_todays_tables():
    betas = dfn.get_named_beta_schedule('cosine', 1000, 1.)
    last, nb = 1.0, []
    for ac in dfn.GaussianDiffusion(betas).alphas_cumprod:              # what create_gaussian_diffusion has always done: every step kept, betas re-derived
        nb.append(1 - ac / last)
        last = ac
    today = dfn.GaussianDiffusion(np.array(nb))
    sig = today._sigma.copy()
    sig[0] = 0.0
    want = np.stack([today._c1, today._c2, sig, (np.arange(1000, dtype=np.float32) / np.float32(1000))], axis=1).astype(np.float32)
    for spec in ('', '1000'):
        d = dfn.create_gaussian_diffusion('cosine', 1000, timestep_respacing=spec)
        assert np.array_equal(d._rows(), want) and np.array_equal(d.betas, today.betas) and np.array_equal(d.sqrt_alphas_cumprod, today.sqrt_alphas_cumprod)
        assert d.timestep_map == list(range(1000)) and not d.is_respaced and d._tmap('cpu') is None
    assert np.array_equal(dfn.create_gaussian_diffusion('cosine', 1000)._rows(), want)


def test_new_entries_are_declared_and_abi_stays():
    import os
    import re
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(os.path.dirname(fx.GOLDEN), '..', 'include', 'interdiff_hip.h')).read(), flags=re.S)
    for name in ('interdiff_posterior_step_dev_map', 'interdiff_sampler_advance_map', 'interdiff_mdm_forward_step_map', 'interdiff_skeleton_mdm_forward_step_map'):
        assert name in _lib.exported_symbols() and re.search(r'\b%s\s*\(' % name, hdr), name
    assert _lib.load().interdiff_abi_version() == _lib.ABI_VERSION == 17


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


def run_loop(d, sampler, eta, model, shape, **kw):
    return d.p_sample_loop(model, shape, clip_denoised=False, **kw) if sampler == 'ddpm' else d.ddim_sample_loop(model, shape, clip_denoised=False, eta=eta, **kw)


class Spy:
    """The denoiser behind a wrapper that notes the timesteps it is called with (not graph-safe: the eager route)."""

    def __init__(self, model):
        self.model, self.seen = model, []

    def __call__(self, x, t, **kw):
        self.seen.append(t.cpu().tolist())
        return self.model(x, t, **kw)


def recorded_case(tag):
    noise, cond, gt, mask, steps = (a.to(DEV) for a in ro.inputs())
    return noise, {'y': dict(cond=cond, inpainted_motion=gt, inpainting_mask=mask)}, steps[:schedule(tag).num_timesteps]


def stub_hook(seen):
    def hook(x, t, model_kwargs):
        seen.append((t.host_value, t.cpu().tolist()))
        return x * ro.stub_scale(t.host_value)
    return hook


@pytest.mark.gpu
@pytest.mark.parametrize('tag,sampler,eta', LOOP_CASES, ids=LOOP_IDS)
def test_eager_loops_against_reference(mdm, tag, sampler, eta):
    """1 + 2: the eager route with the recorded per-step noise against the fp64 oracle at the reference's own error, and who is told which timestep.

    Measured on an MI355X, |HIP - fp64 oracle| / gate 4 e_ref: a_ddpm 6.83e-7 / 6.65e-6, a_ddim_eta0 6.00e-7 / 9.53e-6, a_ddim_eta1 6.74e-7 / 6.50e-6, b_ddpm 6.58e-7 / 4.67e-6,
    b_ddim_eta0 6.31e-7 / 4.73e-6, b_ddim_eta1 7.40e-7 / 5.69e-6: the split-f16 denoiser's error, below the reference's own fp32 rounding."""
    d = schedule(tag)
    noise, kw, steps = recorded_case(tag)
    spy, seen = Spy(mdm), []
    got = run_loop(d, sampler, eta, spy, tuple(noise.shape), noise=noise, model_kwargs=kw, denoised_fn=stub_hook(seen), step_noise=steps, device=DEV)
    name = ro.loop_name(tag, sampler, eta)
    z = golden()
    dist = float(np.abs(got.cpu().numpy().astype(np.float64) - oracle_loop(tag, sampler, eta)).max())
    to_ref = float(np.abs(got.cpu().numpy().astype(np.float64) - z[name]).max())
    g, ulp = gate(tag, sampler, eta)
    print('%s: |HIP - fp64 oracle| %.3e (gate 4 e_ref = %.3e, ulp floor %.3e), |HIP - reference fp32| %.3e' % (name, dist, g, ulp, to_ref))
    assert [s[0] for s in spy.seen] == z[name + '_t_model'].tolist() and all(len(set(s)) == 1 and len(s) == ro.B for s in spy.seen)
    assert [h for h, _ in seen] == z[name + '_t_hook'].tolist() and all(t == [h] * ro.B for h, t in seen)
    assert dist <= max(g, ulp), '%s: %.3e > %.3e' % (name, dist, max(g, ulp))


@pytest.mark.gpu
@pytest.mark.parametrize('sampler,eta', ro.LOOPS)
def test_loop_equals_steps_by_hand(lib, mdm, sampler, eta):
    """2: model(x, timestep_map[i]) -> inpaint -> hook(i) -> the step kernel with the sampler's row i, by hand, is the loop bit for bit."""
    d = schedule('b')
    noise, kw, steps = recorded_case('b')
    loop = run_loop(d, sampler, eta, mdm, tuple(noise.shape), noise=noise, model_kwargs=kw, denoised_fn=stub_hook([]), step_noise=steps)
    rows = d._rows(('ddpm',) if sampler == 'ddpm' else ('ddim', float(eta)))
    x, y = noise.clone(), kw['y']
    for it, i in enumerate(range(d.num_timesteps - 1, -1, -1)):
        x0 = mdm(x, torch.full((ro.B,), d.timestep_map[i], dtype=torch.int64, device=DEV), **kw)
        dfn.inpaint(x0, y['inpainted_motion'], y['inpainting_mask'].view(torch.uint8))
        x0 = x0 * ro.stub_scale(i)
        _lib.check(lib.interdiff_posterior_step(_lib.dptr(x), _lib.dptr(x0), _lib.dptr(steps[it].contiguous()), x.numel(), float(rows[i, 0]), float(rows[i, 1]),
                                                float(rows[i, 2]), 0, it, _lib.stream()), 'posterior_step')
    assert torch.equal(x, loop), (x - loop).abs().max()
    assert not torch.equal(loop, noise)


def hooked_case(seed, B, smpl):
    bt = fx._clip(seed, B, ro.T, ro.P)
    return bt['noise'].to(DEV), {'y': dev(fx.model_kwargs_y(bt, ro.T))}, make_correction(smpl, ro.T, ro.P)


@pytest.mark.gpu
@pytest.mark.parametrize('spec,n_steps', [('10', None), ('100', 60)], ids=['10steps', '100steps_60run'])
@pytest.mark.parametrize('sampler,eta', ro.LOOPS)
def test_graph_route_equals_eager_route(mdm, smpl, sampler, eta, spec, n_steps):
    """3: captured graphs (fused steps, chained embeddings, a captured hook step) == the eager loop, both on the in-kernel generator: a schedule shorter
    than the largest graph block and a longer one, with and without the correction hook (gate on the SPACED index: step 0 of '10', step 50 of '100'),
    one chain (B = 3) and two chains (B = 4, split taken at test size)."""
    d = dfn.create_gaussian_diffusion('cosine', 1000, spec)
    d.split_min_rows = 0
    for B in (3, 4):
        noise, kw, corr = hooked_case(60 + B, B, smpl)
        for hook in (None, corr):
            run = lambda **k: run_loop(d, sampler, eta, mdm, tuple(noise.shape), noise=noise, model_kwargs=kw, denoised_fn=hook, seed=11, n_steps=n_steps, **k)
            graph, eager = run(), run(use_graph=False)
            assert torch.isfinite(graph).all()
            assert torch.equal(graph, eager), 'B = %d, hook %s: %g' % (B, hook is not None, (graph - eager).abs().max())
            assert torch.equal(graph, run()), 'graph reuse'
        st = [v for k, v in mdm._graph_cache.items() if k[0] == d._uid and k[1] == tuple(noise.shape)]
        assert len(st) == 1 and st[0].graphs, 'the captured route was not taken'
        assert (len(st[0].chains) == 2) == (B == 4)
        assert any(isinstance(k, tuple) and k[0] == 'hook' for k in st[0].graphs), 'no captured hook step'


@pytest.mark.gpu
@pytest.mark.parametrize('sampler,eta', [('ddpm', None), ('ddim', 1.0)])
def test_shard_equals_unsharded_under_respacing(mdm, sampler, eta):
    """4: B = 4 as 2 + 2 (C T = 2880 elements per clip: the second shard starts at a multiple of 4)."""
    d = schedule('a')
    bt = fx._clip(71, 4, ro.T, ro.P)
    y, noise = dev(fx.model_kwargs_y(bt, ro.T)), bt['noise'].to(DEV)
    cut = lambda sl: {'y': dict(cond=y['cond'][:, sl].contiguous(), inpainted_motion=y['inpainted_motion'][sl].contiguous(), inpainting_mask=y['inpainting_mask'][sl].contiguous())}
    whole = run_loop(d, sampler, eta, mdm, tuple(noise.shape), noise=noise, model_kwargs=cut(slice(0, 4)), seed=5)
    for first in (0, 2):
        sl = slice(first, first + 2)
        part = run_loop(d, sampler, eta, mdm, (2,) + tuple(noise.shape[1:]), noise=noise[sl].contiguous(), model_kwargs=cut(sl), seed=5, shard=(first, 4))
        assert torch.equal(part, whole[sl]), (first, (part - whole[sl]).abs().max())
    alone = run_loop(d, sampler, eta, mdm, (2,) + tuple(noise.shape[1:]), noise=noise[2:].contiguous(), model_kwargs=cut(slice(2, 4)), seed=5)
    assert not torch.equal(alone, whole[2:]), 'a shard without its position must be another sample'


@pytest.mark.gpu
def test_skeleton_denoiser_respaced_ddim_graph_equals_eager(lib):
    """5: the skeleton denoiser's fused step (csrc/skel_head.h path) under a timestep map, B = 1, T = 20."""
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
    d = dfn.create_gaussian_diffusion('cosine', 50, 'ddim10')
    assert d.timestep_map == list(range(0, 50, 5))
    run = lambda **k: d.ddim_sample_loop(model, tuple(noise.shape), noise=noise, clip_denoised=False, model_kwargs=kw, eta=1.0, seed=23, **k)
    graph, eager = run(), run(use_graph=False)
    assert torch.isfinite(graph).all() and torch.equal(graph, eager), (graph - eager).abs().max()
    assert any(k[0] == d._uid and st.graphs for k, st in model._graph_cache.items()), 'the captured route was not taken'
    other = dfn.create_gaussian_diffusion('cosine', 50, '10').ddim_sample_loop(model, tuple(noise.shape), noise=noise, clip_denoised=False, model_kwargs=kw, eta=1.0, seed=23)
    assert not torch.equal(other, graph), 'another timestep map must give another sample'


@pytest.mark.gpu
def test_eta_zero_ignores_the_seed_and_eta_one_does_not(mdm):
    """6: on the graph route."""
    d = schedule('a')
    noise, kw, _ = recorded_case('a')
    run = lambda eta, seed: d.ddim_sample_loop(mdm, tuple(noise.shape), noise=noise, clip_denoised=False, model_kwargs=kw, eta=eta, seed=seed)
    assert torch.equal(run(0.0, 1), run(0.0, 2))
    assert not torch.equal(run(1.0, 1), run(1.0, 2))
    assert torch.equal(run(1.0, 1), run(1.0, 1))


@pytest.mark.gpu
def test_identity_map_through_new_entries_equals_todays_route(lib, mdm, smpl):
    """7: N = 30, every step kept: the _map entries with an identity array == the NULL map (what the un-suffixed entries pass)."""
    betas = dfn.get_named_beta_schedule('cosine', 30, 1.)
    today, mapped = dfn.create_gaussian_diffusion('cosine', 30), dfn.SpacedDiffusion(range(30), betas)
    mapped.identity_tmap_is_null = False
    assert today._tmap(DEV) is None and mapped._tmap(DEV).tolist() == list(range(30))
    for d in (today, mapped):
        d.split_min_rows = 0
    for B in (3, 4):
        noise, kw, corr = hooked_case(80 + B, B, smpl)
        for hook in (None, corr):
            a, b = (d.p_sample_loop(mdm, tuple(noise.shape), noise=noise, clip_denoised=False, model_kwargs=kw, denoised_fn=hook, seed=3) for d in (today, mapped))
            assert torch.equal(a, b), (B, hook is not None)
    # the stand-alone entries
    x, x0 = torch.randn(1003, device=DEV), torch.randn(1003, device=DEV)
    table, tmap = today._table(torch.device(DEV)), mapped._tmap(DEV)
    outs = []
    for use_map in (False, True):
        xa, state, ts = x.clone(), dfn.seeded_state(17, 9, 0).to(DEV), torch.full((5,), 17, dtype=torch.int64, device=DEV)
        if use_map:
            _lib.check(lib.interdiff_posterior_step_dev_map(_lib.dptr(xa), _lib.dptr(x0), None, None, xa.numel(), _lib.dptr(table), _lib.dptr(tmap), _lib.dptr(state), _lib.dptr(ts), 5, _lib.stream()))
            _lib.check(lib.interdiff_sampler_advance_map(_lib.dptr(state), _lib.dptr(ts), _lib.dptr(tmap), 5, _lib.stream()))
        else:
            _lib.check(lib.interdiff_posterior_step_dev(_lib.dptr(xa), _lib.dptr(x0), None, None, xa.numel(), _lib.dptr(table), _lib.dptr(state), _lib.dptr(ts), 5, _lib.stream()))
            _lib.check(lib.interdiff_sampler_advance(_lib.dptr(state), _lib.dptr(ts), 5, _lib.stream()))
        outs.append((xa, state, ts))
    assert all(torch.equal(p, q) for p, q in zip(*outs))
    assert outs[0][2].tolist() == [15] * 5 and outs[0][1][:2].tolist() == [15, 2]
    # ... and a real map: ts follows it, the state stays loop-side, down to the clamp at the end of the schedule
    rmap = torch.tensor(schedule('b').timestep_map, dtype=torch.int64, device=DEV)
    state, ts = dfn.seeded_state(2, 0, 0).to(DEV), torch.zeros(5, dtype=torch.int64, device=DEV)
    seen = []
    for _ in range(3):
        _lib.check(lib.interdiff_sampler_advance_map(_lib.dptr(state), _lib.dptr(ts), _lib.dptr(rmap), 5, _lib.stream()))
        seen.append((state[0].item(), ts.tolist()))
    assert seen == [(1, [3] * 5), (0, [0] * 5), (-1, [0] * 5)]


@pytest.mark.gpu
def test_training_losses_on_a_spaced_schedule(mdm):
    """``q_sample`` takes the SPACED tables at the spaced ``t``; the model is told ``timestep_map[t]`` (respace.py:94-97)."""
    d = schedule('a')
    noise, kw, _ = recorded_case('a')
    x0, t = kw['y']['inpainted_motion'], torch.tensor([9, 0, 4], dtype=torch.int64)
    spy = Spy(mdm)
    out, target = d.training_losses(spy, x0, t, model_kwargs={'y': {'cond': kw['y']['cond']}}, noise=noise)
    assert spy.seen == [[999, 0, 444]] and target is x0
    sa, s1 = (torch.from_numpy(v.astype(np.float32)).to(DEV)[t.to(DEV)].view(-1, 1, 1, 1) for v in (d.sqrt_alphas_cumprod, d.sqrt_one_minus_alphas_cumprod))
    x_t = sa * x0 + s1 * noise
    assert (d.q_sample(x0, t, noise=noise) - x_t).abs().max().item() <= 2 * float(np.spacing(np.float32(x_t.abs().max().item())))      # (one product may be fused into the sum)
    assert torch.equal(out, mdm(d.q_sample(x0, t, noise=noise), torch.tensor([999, 0, 444], device=DEV), y={'cond': kw['y']['cond']}))


@pytest.mark.gpu
def test_argument_checks(mdm):
    """8."""
    betas = dfn.get_named_beta_schedule('cosine', 1000, 1.)
    with pytest.raises(NotImplementedError):
        dfn.SpacedDiffusion(dfn.space_timesteps(1000, '10'), betas, rescale_timesteps=True)
    with pytest.raises(ValueError):
        dfn.create_gaussian_diffusion('cosine', 1000, 'ddim999')
    d = schedule('a')
    noise, kw, _ = recorded_case('a')
    for bad in (10, 999, -1):
        for loop in (d.p_sample_loop, d.ddim_sample_loop):
            with pytest.raises(ValueError):
                loop(mdm, tuple(noise.shape), noise=noise, clip_denoised=False, model_kwargs=kw, first_t=bad)
    with pytest.raises(NotImplementedError):
        d.ddim_sample_loop(mdm, tuple(noise.shape), noise=noise, clip_denoised=True, model_kwargs=kw)
    with pytest.raises(ValueError):
        dfn.sample_loop(d, mdm, tuple(noise.shape), sampler='plms', noise=noise, clip_denoised=False, model_kwargs=kw)
    # a window of the spaced schedule: first_t / n_steps count spaced steps
    part = d.ddim_sample_loop(mdm, tuple(noise.shape), noise=noise, clip_denoised=False, model_kwargs=kw, first_t=6, n_steps=3, seed=1)
    assert torch.isfinite(part).all() and not torch.equal(part, noise)
