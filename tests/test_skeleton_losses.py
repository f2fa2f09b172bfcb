"""Scoring of a skeleton diffusion checkpoint (interdiff_amd/skeleton_losses.py, csrc/skeleton_losses.hip) against the reference
trainer's OWN outputs (tests/golden/skel_losses.npz, recorded by tests/golden/make_golden_skeleton_losses.py from
train_diffusion_skeleton.py's _common_step / forward_backward / calc_val_loss) and against the fp64 restatement
tests/skeleton_losses_oracle.py.

Gate: the project's per-op rule max|d| / max|ref| <= 1e-4, applied PER TERM; identity claims are ``torch.equal``.
Two kinds of recorded chain terms cannot be held to a relative gate, and the generator says which (it asserts the list): the ``*_past``
terms of a sample whose past frames were inpainted are EXACTLY zero in the reference -- asked for exactly here --, and the quaternion
regulariser of the 1000-step chain, whose hook ends on a matrix -> quaternion conversion, is the reference's own fp32 rounding noise of a unit
quaternion (2.5e-15) -- held to the absolute bound (5e-7)^2 = 2.5e-13 that four fp32 roundings of q . q = 1 allow.  Every figure is printed
before it is asserted."""
import os
import re
import numpy as np
import pytest
import torch
from tests import fixtures as fx
from tests import skeleton_losses_oracle as slo

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
DEV = 'cuda'
GATE = 1e-4
UNIT_QUAT_REG_MAX = 2.5e-13
NEW_SYMBOLS = {
    'interdiff_skeleton_sample_losses_workspace_bytes': 'int32_t K, int32_t B',
    'interdiff_skeleton_sample_losses': 'const float *pred, const float *gt, int32_t K, int32_t B, int32_t C, int32_t T, int32_t past_len, int32_t n_body, '
                                        'int32_t n_points, float *out_terms, float *out_per_clip, void *ws, size_t ws_bytes, void *stream',
    'interdiff_skeleton_denoising_losses': 'const float *pred, const float *target, int32_t B, int32_t T, int32_t past_len, int32_t n_body, '
                                           'int32_t n_points, float *out, void *stream',
}
EDGE_SHAPES = [(1, 3, 1, None), (1, 11, 10, None), (3, 20, 10, None), (65, 20, 10, None), (5, 35, 10, 3)]       # (B, T, past_len, K)


def rel(a, b):
    a, b = (x.detach().cpu().double().numpy() if isinstance(x, torch.Tensor) else np.asarray(x, np.float64) for x in (a, b))
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def close(a, b, tol, what):
    e = rel(a, b)
    print('%s: rel err %.3e (gate %.1e)' % (what, e, tol))
    assert e <= tol, '%s: rel err %.3e > %.1e' % (what, e, tol)
    return e


def close_terms(got, ref, keys, what):
    """per-term gate over stacked terms [13, ...]; a reference term that is exactly zero must come out exactly zero"""
    worst = 0.0
    for i, k in enumerate(keys):
        r = np.asarray(ref[i], np.float64)
        gi = got[i].detach().cpu().double().numpy() if isinstance(got[i], torch.Tensor) else np.asarray(got[i], np.float64)
        if not r.any():
            assert not gi.any(), '%s %s: the reference is exactly 0, got %g' % (what, k, np.abs(gi).max())
            continue
        e = rel(gi, r)
        worst = max(worst, e)
        assert e <= GATE, '%s %s: rel err %.3e > %.1e' % (what, k, e, GATE)
    print('%s: worst of %d terms %.3e (gate %.1e)' % (what, len(keys), worst, GATE))
    return worst


def g():
    z = fx.golden('skel_losses.npz')
    return {k: z[k] for k in z.files}


def tn(a, dtype=None):
    t = torch.from_numpy(np.asarray(a))
    return t.to(dtype) if dtype is not None and t.is_floating_point() else t


def chains():
    """(prefix, final sample, ground truth) of the two reference chains recorded in skel_mdm.npz"""
    m = fx.golden('skel_mdm.npz')
    return [('c50_', m['c50_final'], m['c50_gt']), ('c1000_', m['c1000_dump_999'], m['c1000_gt'])]


def split_tiny(z, pre):
    """indices of the chain terms under the relative gate / the one held to the unit-quaternion bound"""
    ref = z[pre + 'terms']
    tiny = [i for i in range(13) if 0.0 < ref[i] < 1e-6]
    return [i for i in range(13) if i not in tiny], tiny


# ------------------------------------------------------------------------------------------------------------ CPU

def test_restatement_reproduces_the_fixture():
    z = g()
    P, keys = int(z['past_len']), [str(k) for k in z['keys']]
    assert keys == list(slo.KEYS)
    t = slo.terms(z['fb_out'], z['gt'], P)
    close_terms(t, z['fb_terms'], keys, 'forward_backward terms')
    close_terms(slo.per_clip_terms(z['fb_out'], z['gt'], P), z['fb_per_clip'], keys, 'forward_backward per-clip terms')
    loss, wt = slo.weighted(t)
    close_terms(wt, z['fb_weighted'], keys, 'forward_backward weighted terms')
    close(loss, z['fb_loss'], GATE, 'forward_backward loss')
    assert [str(k) for k in z['fb_logged_keys']] == ['train_loss'] and float(z['fb_logged_values'][0]) == float(z['fb_loss'])
    t = slo.terms(z['val_sample'], z['gt'], P)
    close_terms(t, z['val_terms'], keys, 'calc_val_loss terms')
    loss, wt = slo.weighted(t)
    close_terms(wt, z['val_weighted'], keys, 'calc_val_loss weighted terms')
    close(loss, z['val_loss'], GATE, 'val_loss')
    for name in ('fb_terms', 'fb_weighted', 'fb_per_clip', 'val_terms', 'val_weighted'):
        assert float(z[name].min()) >= 1e-6
    assert float(z['min_qq']) >= 0.25
    for pre, s, gt in chains():
        gated, tiny = split_tiny(z, pre)
        assert [keys[i] for i in tiny] == (['quaternion_reg_loss'] if pre == 'c1000_' else [])
        t = slo.terms(s, gt, P)
        loss, wt = slo.weighted(t)
        close_terms(t[gated], z[pre + 'terms'][gated], [keys[i] for i in gated], pre + 'calc_val_loss terms')
        close_terms(wt[gated], z[pre + 'weighted'][gated], [keys[i] for i in gated], pre + 'calc_val_loss weighted terms')
        for i in tiny:
            print('%s%s: restatement %.3e, reference %.3e (bound %.1e)' % (pre, keys[i], t[i], z[pre + 'terms'][i], UNIT_QUAT_REG_MAX))
            assert 0.0 <= t[i] <= UNIT_QUAT_REG_MAX and z[pre + 'terms'][i] <= UNIT_QUAT_REG_MAX
        close(loss, z[pre + 'loss'], GATE, pre + 'val_loss')
        assert z[pre + 'terms'][0] == 0.0 and t[0] == 0.0                      # body_past of an inpainted sample


def test_keys_and_weight_defaults():
    from interdiff_amd import skeleton_losses as SL
    z = g()
    assert list(SL.KEYS) == [str(k) for k in z['keys']] == list(slo.KEYS)
    w = SL.SkeletonLossWeights()
    assert {str(k): float(v) for k, v in zip(z['weight_names'], z['weights'])} == {k: getattr(w, k) for k in w.__dataclass_fields__}
    assert len(w.vector()) == 13
    np.testing.assert_allclose(w.vector(), slo.weight_vector(), rtol=0, atol=0)
    # the recorded weighted / unweighted pairs ARE the defaults
    for pre in ('fb_', 'val_'):
        np.testing.assert_allclose(z[pre + 'weighted'] / z[pre + 'terms'], np.asarray(w.vector()), rtol=1e-6)
    assert SL.SkeletonLossWeights(weight_v=3.0, weight_past=0.25).vector()[9:] == (3.0, 3.0, 6.0, 3.0)
    assert SL.SkeletonLossWeights(weight_v=3.0, weight_past=0.25).vector()[:4] == (0.5, 2.0, 0.25, 1.0)


def test_new_symbols_declared_typed_and_exported():
    """Fails on the parent commit: the entries do not exist there."""
    from interdiff_amd import _lib
    src = re.sub(r'\s+', ' ', open(os.path.join(ROOT, 'include', 'interdiff_hip.h')).read())
    for name, args in NEW_SYMBOLS.items():
        assert '%s(%s);' % (name, args) in src, name
        assert name in _lib._SIGS and len(_lib._SIGS[name][1]) == args.count(',') + 1, name
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name)
    assert lib.interdiff_abi_version() == 17 and _lib.ABI_VERSION == 17
    assert 'skeleton_losses.hip' in __import__('interdiff_amd.csrc.build', fromlist=['sources']).sources()
    assert lib.interdiff_skeleton_sample_losses_workspace_bytes(3, 65) >= 3 * 13 * 65 * 4
    assert lib.interdiff_skeleton_sample_losses_workspace_bytes(0, 5) == 0


# ------------------------------------------------------------------------------------------------------------ GPU

@pytest.fixture(scope='module')
def diff():
    from interdiff_amd.diffusion import create_gaussian_diffusion
    return create_gaussian_diffusion('cosine', 1000)


def skel_weights(z):
    from interdiff_amd import synthetic as syn
    return {k: torch.from_numpy(v) for k, v in syn.skeleton_mdm_state_dict(int(z['seed'])).items()}


@pytest.fixture(scope='module')
def model(lib):
    from interdiff_amd import skeleton as sk
    return sk.SkeletonMDM(skel_weights(g()), device=DEV)


@pytest.mark.gpu
def test_calc_val_loss_vs_fixture(lib):
    from interdiff_amd import skeleton_losses as SL
    z = g()
    P = int(z['past_len'])
    loss, ld, wd = SL.calc_val_loss(tn(z['val_sample']).to(DEV), tn(z['gt']).to(DEV), P)
    assert list(ld) == list(SL.KEYS) == list(wd) and loss.dim() == 0
    close_terms(torch.stack(list(ld.values())), z['val_terms'], SL.KEYS, 'calc_val_loss terms')
    close_terms(torch.stack(list(wd.values())), z['val_weighted'], SL.KEYS, 'calc_val_loss weighted terms')
    close(loss, z['val_loss'], GATE, 'val_loss')
    # the final samples of the reference's own 50-step and 1000-step chains
    for pre, s, gt in chains():
        gated, tiny = split_tiny(z, pre)
        loss, ld, wd = SL.calc_val_loss(tn(s).to(DEV), tn(gt).to(DEV), P)
        t, wt = torch.stack(list(ld.values())).cpu(), torch.stack(list(wd.values())).cpu()
        close_terms(t[gated], z[pre + 'terms'][gated], [SL.KEYS[i] for i in gated], pre + 'calc_val_loss terms')
        close_terms(wt[gated], z[pre + 'weighted'][gated], [SL.KEYS[i] for i in gated], pre + 'calc_val_loss weighted terms')
        for i in tiny:
            print('%s%s: HIP %.3e, reference %.3e (bound %.1e)' % (pre, SL.KEYS[i], float(t[i]), z[pre + 'terms'][i], UNIT_QUAT_REG_MAX))
            assert 0.0 <= float(t[i]) <= UNIT_QUAT_REG_MAX
        close(loss, z[pre + 'loss'], GATE, pre + 'val_loss')
        assert float(t[0]) == 0.0


@pytest.fixture(scope='module')
def edge_refs():
    """inputs and fp64 references of every edge shape, computed once"""
    out = {}
    for B, T, P, K in EDGE_SHAPES:
        pred, gt = slo.near_unit_case(4000 + 100 * B + T, B, T, K)
        ps = pred if K else pred[None]
        per = np.stack([slo.per_clip_terms(p, gt, P) for p in ps])               # [K,13,B]
        out[(B, T, P, K)] = (pred, gt, per, per.mean(axis=2))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('B,T,P,K', EDGE_SHAPES)
def test_kernel_vs_restatement_at_edge_shapes(lib, edge_refs, B, T, P, K):
    from interdiff_amd import skeleton_losses as SL, _lib
    pred, gt, per64, terms64 = edge_refs[(B, T, P, K)]
    assert np.abs((pred.reshape(-1, B, 106, T)[:, :, -4:] ** 2).sum(2) - 1).max() < 0.75          # near-unit quaternions
    samples, gtd = tn(pred).to(DEV), tn(gt).to(DEV)
    samples = samples if K else samples[None]
    terms, per = SL.score_samples(samples, gtd, P)
    assert terms.shape == (K or 1, 13) and per.shape == (K or 1, 13, B)
    close_terms(per.permute(1, 0, 2), per64.transpose(1, 0, 2), SL.KEYS, 'out_per_clip B=%d T=%d past=%d K=%s vs fp64' % (B, T, P, K))
    close_terms(terms.t(), terms64.T, SL.KEYS, 'out_terms B=%d T=%d past=%d K=%s vs fp64' % (B, T, P, K))
    again = SL.score_samples(samples, gtd, P)
    assert torch.equal(again[0], terms) and torch.equal(again[1], per)                              # two identical calls
    # the workspace form (out_per_clip NULL) gives the same out_terms
    need = lib.interdiff_skeleton_sample_losses_workspace_bytes(samples.shape[0], B)
    ws, t2 = torch.empty(need, dtype=torch.uint8, device=DEV), torch.empty_like(terms)
    _lib.check(lib.interdiff_skeleton_sample_losses(_lib.dptr(samples), _lib.dptr(gtd), samples.shape[0], B, 106, T, P, 63, 12, _lib.dptr(t2), None,
                                                    _lib.dptr(ws), need, _lib.stream()))
    assert torch.equal(t2, terms)
    # the teacher-forced entry is the first launch alone
    out = torch.empty(13, B, device=DEV)
    _lib.check(lib.interdiff_skeleton_denoising_losses(_lib.dptr(samples[0].contiguous()), _lib.dptr(gtd), B, T, P, 63, 12, _lib.dptr(out), _lib.stream()))
    assert torch.equal(out, per[0])
    if B == 65:                                                                                     # a clip's numbers are its own
        for b in (0, 31, 64):
            alone = SL.score_samples(samples[:, b:b + 1].contiguous(), gtd[b:b + 1].contiguous(), P)[1]
            assert torch.equal(alone[:, :, 0], per[:, :, b]), 'clip %d' % b
    loss, ld, wd = SL.calc_val_loss(samples[0], gtd, P)
    l64, w64 = slo.weighted(terms64[0])
    close_terms(torch.stack(list(wd.values())), w64, SL.KEYS, 'weighted terms')
    close(loss, l64, GATE, 'loss')


@pytest.mark.gpu
def test_argument_checks_launch_nothing(lib):
    from interdiff_amd import skeleton_losses as SL, _lib
    pred, gt = (tn(a).to(DEV) for a in slo.near_unit_case(1, 2, 12))
    with pytest.raises(ValueError):
        SL.score_samples(pred[None], gt, past_len=12)                              # T = past_len
    with pytest.raises(ValueError):
        SL.score_samples(pred[None], gt, past_len=0)
    with pytest.raises(ValueError):
        SL.score_samples(pred[None], gt, past_len=10, n_points=11)                 # 63 + 33 + 7 != 106
    with pytest.raises(ValueError):
        SL.score_samples(pred[None, :, :, :105].contiguous(), gt[:, :, :105].contiguous(), past_len=10)
    sentinel = -7.0
    terms, out = torch.full((13,), sentinel, device=DEV), torch.full((13, 2), sentinel, device=DEV)
    need = lib.interdiff_skeleton_sample_losses_workspace_bytes(1, 2)
    ws = torch.full((need // 4,), sentinel, device=DEV)
    call = lambda T, P, Cc, nb, npts, ws_bytes: lib.interdiff_skeleton_sample_losses(_lib.dptr(pred), _lib.dptr(gt), 1, 2, Cc, T, P, nb, npts, _lib.dptr(terms),
                                                                                     None, _lib.dptr(ws), ws_bytes, _lib.stream())
    assert call(12, 12, 106, 63, 12, need) == -22 and call(12, 0, 106, 63, 12, need) == -22
    assert call(12, 10, 105, 63, 12, need) == -22 and call(12, 10, 106, 64, 12, need) == -22
    assert call(12, 10, 106, 63, 12, need - 1) == -12                              # a workspace one byte short
    with pytest.raises(RuntimeError):
        _lib.check(call(12, 10, 106, 63, 12, need - 1))
    den = lambda T, P, nb: lib.interdiff_skeleton_denoising_losses(_lib.dptr(pred), _lib.dptr(gt), 2, T, P, nb, 12, _lib.dptr(out), _lib.stream())
    assert den(12, 12, 63) == -22 and den(12, 0, 63) == -22 and den(12, 10, 0) == -22
    torch.cuda.synchronize()
    assert bool((terms == sentinel).all()) and bool((out == sentinel).all()) and bool((ws == sentinel).all())      # nothing ran
    assert call(12, 10, 106, 63, 12, need) == 0
    torch.cuda.synchronize()
    assert bool((terms != sentinel).all())


@pytest.mark.gpu
def test_denoising_losses_vs_fixture(model, diff):
    from interdiff_amd import skeleton_losses as SL, _lib
    z = g()
    P = int(z['past_len'])
    gt, cond, zp, t, eps = (tn(z[k]).to(DEV) for k in ('gt', 'cond', 'batch_zero_pose_obj', 't', 'eps'))
    B, T = gt.shape[0], gt.shape[-1]
    w = torch.tensor(SL.SkeletonLossWeights().vector(), device=DEV)
    # the kernel alone, on the reference's own model output
    out = torch.empty(13, B, device=DEV)
    _lib.check(model.lib.interdiff_skeleton_denoising_losses(_lib.dptr(tn(z['fb_out']).to(DEV)), _lib.dptr(gt), B, T, P, 63, 12, _lib.dptr(out), _lib.stream()))
    close_terms(out, z['fb_per_clip'], SL.KEYS, 'interdiff_skeleton_denoising_losses on the recorded model output, per clip')
    close_terms(out.mean(dim=1), z['fb_terms'], SL.KEYS, '... batch terms')
    close_terms(out.mean(dim=1) * w, z['fb_weighted'], SL.KEYS, '... weighted')
    # q_sample at C = 106 + one HIP forward with per-clip t
    close(diff.q_sample(gt, t, noise=eps), z['fb_x_t'], 2e-6, 'interdiff_q_sample at C = 106, injected noise')
    mo, target = diff.training_losses(model, gt, t, model_kwargs={'y': {'cond': cond}, 'zero_pose_obj': zp}, noise=eps)
    assert torch.equal(target, gt)
    close(mo, z['fb_out'], GATE, 'training_losses model output (SkeletonMDM.forward, per-clip timesteps)')
    loss, ld, t_used = SL.denoising_losses(model, diff, gt, zp, cond, t=tn(z['t']), noise=eps, past_len=P)
    assert list(ld) == list(SL.KEYS) and torch.equal(t_used.cpu(), tn(z['t'])) and loss.dim() == 0
    per = torch.stack(list(ld.values()))
    close_terms(per, z['fb_per_clip'], SL.KEYS, 'denoising_losses per-clip terms')
    close_terms(per.mean(dim=1), z['fb_terms'], SL.KEYS, 'denoising_losses batch terms')
    close(loss, z['fb_loss'], GATE, 'forward_backward loss (= train_loss, all the trainer logs)')
    # drawn t and in-kernel noise: reproducible under a seed
    gen = lambda: torch.Generator().manual_seed(5)
    a = SL.denoising_losses(model, diff, gt, zp, cond, seed=11, generator=gen())
    b = SL.denoising_losses(model, diff, gt, zp, cond, seed=11, generator=gen())
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and all(torch.equal(a[1][k], b[1][k]) for k in SL.KEYS)
    assert not torch.equal(a[0], SL.denoising_losses(model, diff, gt, zp, cond, seed=12, generator=gen())[0])


@pytest.mark.gpu
def test_skeleton_forward_per_clip_timesteps(model):
    """``SkeletonMDM.forward`` already took a timestep vector (the kernels add temb[ts[b]] per clip; no code changed for it): each clip of one
    forward with three different timesteps equals that clip's own B = 1 forward at its t, within the gate."""
    z = g()
    x, cond, zp, t = (tn(z[k]).to(DEV) for k in ('fb_x_t', 'cond', 'batch_zero_pose_obj', 't'))
    assert len(set(t.tolist())) == t.numel()
    got = model(x, t, zero_pose_obj=zp, y={'cond': cond}).clone()
    for b in range(x.shape[0]):
        one = model(x[b:b + 1].contiguous(), t[b:b + 1].contiguous(), zero_pose_obj=zp[b:b + 1].contiguous(), y={'cond': cond[:, b:b + 1].contiguous()})
        close(got[b:b + 1], one, GATE, 'clip %d of the per-clip-timestep forward vs its own B = 1 forward at t = %d' % (b, int(t[b])))
    close(got, z['fb_out'], GATE, 'SkeletonMDM.forward, per-clip timesteps, vs the reference model')


@pytest.mark.gpu
def test_validation_and_test_step_plumbing(lib):
    """validation_step / test_step under a fixed seed == calc_val_loss applied to p_sample_loop run separately under the same seed."""
    from interdiff_amd import skeleton_losses as SL, skeleton as sk, synthetic as syn
    from interdiff_amd.diffusion import create_gaussian_diffusion
    z = g()
    P, steps, B, T = int(z['past_len']), 50, 2, 20
    m50, d50 = sk.SkeletonMDM(skel_weights(z), device=DEV, n_steps=steps), create_gaussian_diffusion('cosine', steps)
    bt = {k: torch.from_numpy(v) for k, v in syn.make_skeleton_batch(7600, B=B, T=T).items()}
    batch = (bt['body'], bt['obj'], bt['pose'], bt['zero_pose_obj'])
    gt, kw = SL.sample_kwargs(m50, batch, P)
    assert gt.shape == (B, 1, 106, T)
    s0 = d50.p_sample_loop(m50, tuple(gt.shape), clip_denoised=False, model_kwargs=kw, seed=41)
    assert torch.equal(s0[..., :P], gt[..., :P]) and bool(torch.isfinite(s0).all())                # x_T inpainted, past frames kept
    assert any(isinstance(k, tuple) and len(k) == 3 for st in m50._graph_cache.values() for k in st.graphs), 'the captured route was not taken'
    rl, rd, rw = SL.calc_val_loss(s0, gt, P)
    vl, vd, vw = SL.validation_step(m50, d50, batch, past_len=P, seed=41)
    assert torch.equal(vl, rl) and all(torch.equal(vd[k], rd[k]) and torch.equal(vw[k], rw[k]) for k in SL.KEYS)
    assert all(float(vd[k]) == 0.0 for k in SL.KEYS if k.endswith('_past')) and float(vd['body_future']) > 0.0
    tl, td, tw = SL.test_step(m50, d50, batch, past_len=P, seed=41)
    assert list(td) == ['test_' + k for k in SL.KEYS] and list(tw) == list(SL.KEYS)
    assert torch.equal(tl, rl) and all(torch.equal(td['test_' + k], rd[k]) and torch.equal(tw[k], rw[k]) for k in SL.KEYS)
    assert not torch.equal(SL.validation_step(m50, d50, batch, past_len=P, seed=42)[0], vl)
    print('validation_step loss %.6f (50-step schedule, B = %d)' % (float(vl), B))
