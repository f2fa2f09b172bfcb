"""Checkpoint scoring (interdiff_amd/losses.py, csrc/losses.hip) against the reference trainer's OWN outputs (tests/golden/losses.npz,
recorded by tests/golden/make_golden_losses.py from train_diffusion_smpl.py's forward_backward / _common_step / calc_val_loss /
calc_loss and gaussian_diffusion.py's training_losses / q_sample) and against the CPU restatement tests/losses_oracle.py.

Gate: the project's per-op rule max|d| / max|ref| <= 1e-4, applied PER TERM (a [B] vector or a scalar);
bit-identity claims are ``torch.equal``.  The fixture keeps every two samples of a clip more than 1e-3 apart in every term (asserted
by the generator on the reference's own numbers), so no ``_min`` term is excluded from any comparison.  Every figure is printed
before it is asserted.  EDGE_SHAPES: both kernels against the fp64 restatement where the frame split and the normalisers can go wrong; worst term on
MI355X 8.4e-6, and an unmarked test holds the restatement's own fp32 run to a quarter of the gate at every one of them."""
import os
import re
import numpy as np
import pytest
import torch
from tests import fixtures as fx
from tests import losses_oracle as lo

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
DEV = 'cuda'
GATE = 1e-4
NEW_SYMBOLS = {
    'interdiff_q_sample': 'float *x_t, const float *x0, const float *noise, const int64_t *ts, const float *sqrt_ac, const float *sqrt_1mac, '
                          'int32_t n_steps, const float *gt, const uint8_t *mask, int32_t B, int64_t per_clip, uint64_t seed, uint64_t elem0, void *stream',
    'interdiff_denoising_losses': 'const float *pred, const float *target, int32_t B, int32_t T, int32_t past_len, float *out, void *stream',
    'interdiff_sample_losses_workspace_bytes': 'int32_t K, int32_t B',
    'interdiff_sample_losses': 'const float *samples, const float *gt, const float *hand_pose, int32_t K, int32_t B, int32_t T, int32_t past_len, '
                               'int32_t variant, float *out_terms, float *out_per_clip, void *ws, size_t ws_bytes, void *stream',
}


def rel(a, b):
    a, b = (x.detach().cpu().double().numpy() if isinstance(x, torch.Tensor) else np.asarray(x, np.float64) for x in (a, b))
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def close(a, b, tol, what):
    e = rel(a, b)
    print('%s: rel err %.3e (gate %.1e)' % (what, e, tol))
    assert e <= tol, '%s: rel err %.3e > %.1e' % (what, e, tol)
    return e


def close_terms(got, ref, keys, what):
    """per-term gate over stacked terms [n, ...]"""
    worst = 0.0
    for i, k in enumerate(keys):
        e = rel(got[i], ref[i])
        worst = max(worst, e)
        assert e <= GATE, '%s %s: rel err %.3e > %.1e' % (what, k, e, GATE)
    print('%s: worst of %d terms %.3e (gate %.1e)' % (what, len(keys), worst, GATE))
    return worst


def g():
    z = fx.golden('losses.npz')
    return {k: z[k] for k in z.files}


def tn(a, dtype=None):
    t = torch.from_numpy(np.asarray(a))
    return t.to(dtype) if dtype is not None and t.is_floating_point() else t


def past_mask(gt, past):
    m = torch.ones(gt.shape, dtype=torch.bool)
    m[..., past:] = False
    return m


def betas():
    from interdiff_amd.diffusion import get_named_beta_schedule
    return get_named_beta_schedule('cosine', 1000, 1.)


def big_case(seed=9100, B=16, T=100, K=4, past=fx.PAST, scales=(0.02, 0.03, 0.045, 0.07)):
    """The second, seeded scoring input: B = 16, T = 100, K = 4 -- ground truth of a synthetic clip batch, samples = gt + N(0, s_k)."""
    from interdiff_amd import synthetic as syn
    bt = syn.make_clip_batch(seed=seed, B=B, T=T, past_len=past, n_points=8)
    rs = np.random.RandomState(seed + 1)
    gt, hands = tn(bt['gt']), tn(bt['hand_pose'])
    samples = torch.stack([gt + s * fx._randn(rs, *gt.shape) for s in scales[:K]])
    return samples, gt, hands


# (B, T, past_len, K).  (1,3,1,1): sample_losses only (denoising_losses needs past_len >= 2); (1,4,2,1): the smallest shape both kernels admit; (1,12,10,1): T = P + 2, one
# frame in _v_future, and the test variant starts one frame later still; (3,9,4,2): frame runs of 2, a one-frame last run, three empty waves, P on a run boundary;
# (65,20,10,1): more clips than a wave has lanes; (2,131,10,2): a prime T past 128 (these kernels have no T limit).
EDGE_SHAPES = [(1, 3, 1, 1), (1, 4, 2, 1), (1, 12, 10, 1), (3, 9, 4, 2), (65, 20, 10, 1), (5, 35, 10, 3), (2, 131, 10, 2)]
# At (1,4,2,1) obj_rot_past is the mean of two frames of nine squared differences of O(1) matrix entries that lie 0.02 apart: fp32 itself computes it only to 2.9e-5.
# The noise scale 0.07 (big_case's largest) in the place of 0.02 conditions the difference 3.5 times better; the gate stays where it is.
EDGE_SCALES = {(1, 4, 2, 1): (0.07,)}
FP32_CAP = 2.5e-5                                                  # a quarter of GATE: what the restatement's own fp32 arithmetic may use up at an edge shape
_EDGE = {}


def edge_case(shape):
    B, T, P, K = shape
    return big_case(seed=9200 + T, B=B, T=T, K=K, past=P, **({'scales': EDGE_SCALES[shape]} if shape in EDGE_SCALES else {}))


def edge_ref(shape, dtype=torch.float64):
    """The restatement at an edge shape, computed once per (shape, dtype) and never modified: 'test' on all K samples, 'val' and the denoising terms on samples[0]."""
    if (shape, dtype) not in _EDGE:
        P = shape[2]
        samples, gt, hands = (a.to(dtype) for a in edge_case(shape))
        t_test, per_test = lo.sample_terms(samples, gt, hands, P, 'test')
        t_val, per_val = lo.sample_terms(samples[:1], gt, hands, P, 'val')
        den = torch.stack(list(lo.denoising_terms(samples[0], gt, P).values())) if P >= 2 else None
        _EDGE[(shape, dtype)] = dict(test=torch.stack(list(t_test.values())), per_test=per_test, val=torch.stack(list(t_val.values())), per_val=per_val, den=den)
    return _EDGE[(shape, dtype)]


# ------------------------------------------------------------------------------------------------------------ CPU

@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_oracle_vs_golden(dtype):
    """Every recorded quantity: fp32 oracle == the fp32 reference to rounding; the fp64 oracle's distance is printed (the error budget)."""
    z = g()
    P = int(z['past_len'])
    tol = 2e-6 if dtype == torch.float32 else GATE
    x0, eps, t = tn(z['x0'], dtype), tn(z['eps'], dtype), tn(z['t'])
    close(lo.q_sample(betas(), x0, t, eps), z['fb_x_t'], tol, 'q_sample')
    close(lo.q_sample(betas(), x0, t, eps, gt=x0 + 1.0, mask=past_mask(x0, P)), z['qs_x_t'], tol, 'q_sample + inpainting')
    terms = lo.denoising_terms(tn(z['fb_out'], dtype), x0, P)
    assert list(terms) == [str(k) for k in z['fb_keys']]
    loss, wd = lo.weighted(terms)
    close_terms(torch.stack([wd[k] for k in lo.LOSS_KEYS]), z['fb_weighted'], lo.LOSS_KEYS, 'forward_backward weighted terms (%s)' % dtype)
    close(loss.mean(), z['fb_loss'], max(tol, 1e-5), 'forward_backward loss')
    q = lo.quartiles(t, wd, 1000)
    assert sorted(q) == [str(k) for k in z['fb_quartile_keys']]
    close(np.asarray([q[k] for k in sorted(q)]), z['fb_quartile_values'], max(tol, 1e-5), 'timestep quartiles')
    samples, hands = tn(z['samples'], dtype), tn(z['hand_pose'], dtype)
    vt, _ = lo.sample_terms(samples[:1], x0, hands, P, 'val')
    assert list(vt) == [str(k) for k in z['val_keys']]
    close_terms(torch.stack(list(vt.values())), z['val_terms'], list(vt), 'calc_val_loss terms (%s)' % dtype)
    vl, vw = lo.weighted(vt)
    close_terms(torch.stack(list(vw.values())), z['val_weighted'], list(vw), 'calc_val_loss weighted')
    close(vl, z['val_loss'], GATE, 'val_loss')
    tt, per = lo.sample_terms(samples, x0, hands, P, 'test')
    assert list(tt) == [str(k) for k in z['test_keys']]
    close_terms(torch.stack(list(tt.values())), z['test_terms'], list(tt), 'calc_loss terms (%s)' % dtype)
    close_terms(per.permute(1, 0, 2), np.transpose(z['test_per_clip'], (1, 0, 2)), lo.LOSS_KEYS, 'calc_loss per-clip means')
    tl, tw = lo.weighted(tt)
    close_terms(torch.stack(list(tw.values())), z['test_weighted'], list(tw), 'calc_loss weighted')
    close(tl, z['test_loss'], GATE, 'test loss')
    assert float(z['min_gap']) > 1e-3
    best = per.argmin(dim=0)
    assert int(best[8, 0]) != int(best[10, 0])              # the on-purpose case: clip 0's best sample differs between two _min terms


def test_keys_and_weight_defaults():
    from interdiff_amd import losses as L
    z = g()
    assert list(L.LOSS_KEYS) == [str(k) for k in z['fb_keys']] == list(lo.LOSS_KEYS)
    assert list(L.LOSS_KEYS + L.MIN_KEYS) == [str(k) for k in z['test_keys']]
    w = L.LossWeights()
    assert {str(k): float(v) for k, v in zip(z['weight_names'], z['weights'])} == {k: getattr(w, k) for k in w.__dataclass_fields__}
    np.testing.assert_allclose(w.vector(), lo.weight_vector(), rtol=0, atol=0)
    # the recorded weighted / unweighted pairs ARE the defaults
    np.testing.assert_allclose(z['val_weighted'], z['val_terms'] * np.asarray(w.vector(), np.float32), rtol=1e-6)


def test_q_sample_tables_known_answers():
    from interdiff_amd.diffusion import create_gaussian_diffusion
    d = create_gaussian_diffusion('cosine', 1000)
    sa, s1 = lo.sqrt_tables(betas())
    np.testing.assert_allclose(d.sqrt_alphas_cumprod, sa, rtol=0, atol=1e-15)
    np.testing.assert_allclose(d.sqrt_one_minus_alphas_cumprod, s1, rtol=0, atol=1e-15)
    abar0 = (np.cos((1 / 1000 + 0.008) / 1.008 * np.pi / 2) / np.cos(0.008 / 1.008 * np.pi / 2)) ** 2      # cosine schedule, closed form
    assert abs(d.sqrt_alphas_cumprod[0] - np.sqrt(abar0)) < 1e-12
    assert d.sqrt_one_minus_alphas_cumprod[999] > 0.999999 and d.sqrt_alphas_cumprod[999] < 1e-3
    assert abs(d.sqrt_alphas_cumprod[999] ** 2 + d.sqrt_one_minus_alphas_cumprod[999] ** 2 - 1) < 1e-12
    t, w = d.sample_timesteps(64, 'cpu', generator=torch.Generator().manual_seed(3))
    assert t.dtype == torch.int64 and int(t.min()) >= 0 and int(t.max()) < 1000 and torch.equal(w, torch.ones(64))


def test_new_symbols_declared_typed_and_exported():
    """Fails on the parent commit: the entries do not exist there."""
    from interdiff_amd import _lib
    src = re.sub(r'\s+', ' ', open(os.path.join(ROOT, 'include', 'interdiff_hip.h')).read())
    for name, args in NEW_SYMBOLS.items():
        assert '%s(%s);' % (name, args) in src, name
        assert name in _lib._SIGS and len(_lib._SIGS[name][1]) == args.count(',') + 1, name
    assert 'IDF_LOSS_VAL = 0, IDF_LOSS_TEST = 1' in src and (_lib.LOSS_VAL, _lib.LOSS_TEST) == (0, 1)
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name)
    assert 'losses.hip' in __import__('interdiff_amd.csrc.build', fromlist=['sources']).sources()


@pytest.mark.parametrize('shape', EDGE_SHAPES, ids=str)
def test_fp32_restatement_at_edge_shapes(shape):
    """The condition the edge-shape GPU test rests on: the restatement run in fp32 on the same inputs is within FP32_CAP = GATE / 4 of fp64 on every term and every
    per-clip mean, so the inputs and not the gate carry the margin; and two samples of a clip are never so close that the ``_min`` pick could turn on rounding."""
    r32, r64 = edge_ref(shape, torch.float32), edge_ref(shape)
    worst = 0.0
    for name in ('test', 'val', 'den'):
        if r64[name] is not None:
            for i in range(r64[name].shape[0]):
                worst = max(worst, rel(r32[name][i], r64[name][i]))
    for name in ('per_test', 'per_val'):
        for i in range(16):
            worst = max(worst, rel(r32[name][:, i], r64[name][:, i]))
    gap = 1.0
    if shape[3] > 1:
        two = r64['per_test'].sort(dim=0)[0]
        gap = float(((two[1] - two[0]) / two[0]).min())
    print('B=%d T=%d past=%d K=%d: fp32 restatement vs fp64, worst term %.3e (cap %.1e); smallest best-of-K margin %.3e' % (*shape, worst, FP32_CAP, gap))
    assert worst <= FP32_CAP and gap >= 1e-3
    assert torch.equal(r32['per_test'].argmin(dim=0), r64['per_test'].argmin(dim=0))


# ------------------------------------------------------------------------------------------------------------ GPU

@pytest.fixture(scope='module')
def diff():
    from interdiff_amd.diffusion import create_gaussian_diffusion
    return create_gaussian_diffusion('cosine', 1000)


@pytest.fixture(scope='module')
def mdm(lib):
    from interdiff_amd.mdm import MDM
    return MDM(fx.mdm_weights(), device=DEV)


def clip_batch(z):
    return dict(gt=tn(z['x0']).to(DEV), cond=tn(z['cond']).to(DEV), hand_pose=tn(z['hand_pose']).to(DEV))


@pytest.mark.gpu
def test_q_sample_injected_noise_vs_golden(lib, diff):
    z = g()
    x0, eps, t = tn(z['x0']).to(DEV), tn(z['eps']).to(DEV), tn(z['t']).to(DEV)
    close(diff.q_sample(x0, t, noise=eps), z['fb_x_t'], 2e-6, 'interdiff_q_sample, injected noise')
    m = past_mask(x0, int(z['past_len'])).to(DEV)
    got = diff.q_sample(x0, t, noise=eps, inpainted_motion=x0 + 1.0, inpainting_mask=m)
    close(got, z['qs_x_t'], 2e-6, 'interdiff_q_sample + inpainting')
    assert torch.equal(got[..., :int(z['past_len'])], (x0 + 1.0)[..., :int(z['past_len'])])
    with pytest.raises(ValueError):
        diff.q_sample(x0, torch.tensor([0, 1, 2, 1000]), noise=eps)


@pytest.mark.gpu
def test_q_sample_philox_path(lib, diff):
    B, C, T = 64, 144, 100
    x0 = torch.zeros(B, 1, C, T, device=DEV)
    t = torch.full((B,), 999, dtype=torch.int64, device=DEV)
    a, a2, b = diff.q_sample(x0, t, seed=233), diff.q_sample(x0, t, seed=233), diff.q_sample(x0, t, seed=234)
    assert torch.equal(a, a2) and not torch.equal(a, b)
    s1 = float(np.float32(diff.sqrt_one_minus_alphas_cumprod[999]))
    for v in (a / s1, b / s1):                                       # x0 = 0: x_t = sqrt(1 - abar) eps
        print('q_sample noise: mean %.2e std-1 %.2e kurt-3 %.2e' % (v.mean().item(), v.std().item() - 1, (v ** 4).mean().item() - 3))
        assert abs(v.mean().item()) < 3e-3 and abs(v.std().item() - 1) < 3e-3
        assert abs((v ** 4).mean().item() - 3) < 0.05 and v.abs().max().item() < 7
    assert abs((a * b).mean().item()) / s1 ** 2 < 3e-3
    # not the sampler's streams: x_T (0xFFFFFFFF) and the loop indices draw other numbers under the same seed
    from interdiff_amd import _lib
    for step in (0xFFFFFFFF, 0, 999):
        r = torch.empty_like(a)
        _lib.check(lib.interdiff_randn(_lib.dptr(r), r.numel(), 233, step, _lib.stream()))
        assert not torch.equal(r * s1, a)
    # per-clip timesteps and a clip shard: clips [5, 9) drawn at the whole batch's counters
    tt = torch.arange(B, dtype=torch.int64, device=DEV) * 15
    x1 = torch.randn(B, 1, C, T, device=DEV)
    whole = diff.q_sample(x1, tt, seed=7)
    part = diff.q_sample(x1[5:9].contiguous(), tt[5:9].contiguous(), seed=7, elem0=5 * C * T)
    assert torch.equal(part, whole[5:9])


@pytest.mark.gpu
def test_mdm_forward_per_clip_timesteps(mdm):
    """Clip by clip and bit for bit: one forward with a different timestep per clip == B forwards that broadcast one clip's timestep."""
    z = g()
    x, cond, t = tn(z['fb_x_t']).to(DEV), tn(z['cond']).to(DEV), tn(z['t']).to(DEV)
    assert len(set(t.tolist())) == t.numel()
    got = mdm(x, t, y={'cond': cond}).clone()
    for b in range(x.shape[0]):
        one = mdm(x, torch.full_like(t, int(t[b])), y={'cond': cond})
        assert torch.equal(one[b], got[b]), 'clip %d' % b
        if b:
            assert not torch.equal(one[0], got[0])                  # (the timestep does reach the output)
    close(got, z['fb_out'], GATE, 'MDM.forward, per-clip timesteps, vs the reference model')


@pytest.mark.gpu
def test_denoising_losses_vs_golden(mdm, diff):
    from interdiff_amd import losses as L, _lib
    z = g()
    P, bt = int(z['past_len']), clip_batch(z)
    # the kernel alone, on the reference's own model output
    pred, B, T = tn(z['fb_out']).to(DEV), bt['gt'].shape[0], bt['gt'].shape[-1]
    out = [torch.empty(16, B, device=DEV) for _ in range(2)]
    for o in out:
        _lib.check(mdm.lib.interdiff_denoising_losses(_lib.dptr(pred), _lib.dptr(bt['gt']), B, T, P, _lib.dptr(o), _lib.stream()))
    assert torch.equal(out[0], out[1])
    w = torch.tensor(L.LossWeights().vector(), device=DEV)[:, None]
    close_terms(out[0] * w, z['fb_weighted'], L.LOSS_KEYS, 'interdiff_denoising_losses on the recorded model output')
    # training_losses + the kernel: q_sample, one HIP forward with per-clip t, the 16 x [B] vectors
    mo, target = diff.training_losses(mdm, bt['gt'], tn(z['t']).to(DEV), model_kwargs={'y': {'cond': bt['cond']}}, noise=tn(z['eps']).to(DEV))
    assert torch.equal(target, bt['gt'])
    close(mo, z['fb_out'], GATE, 'training_losses model output')
    loss, ld, wd, quart = L.denoising_losses(mdm, diff, bt, t=tn(z['t']), noise=tn(z['eps']).to(DEV), past_len=P)
    close_terms(torch.stack([wd[k] for k in L.LOSS_KEYS]), z['fb_weighted'], L.LOSS_KEYS, 'denoising_losses weighted terms')
    close_terms(torch.stack([ld[k] for k in L.LOSS_KEYS]) * w, z['fb_weighted'], L.LOSS_KEYS, 'denoising_losses loss_dict x weights')
    assert loss.shape == (B,)
    close(loss.mean(), z['fb_loss'], GATE, 'forward_backward loss')
    assert sorted(quart) == [str(k) for k in z['fb_quartile_keys']]
    close_terms(np.asarray([quart[k] for k in sorted(quart)]), z['fb_quartile_values'], sorted(quart), 'timestep quartiles')
    # drawn t and in-kernel noise: reproducible under a seed
    gen = lambda: torch.Generator().manual_seed(5)
    a = L.denoising_losses(mdm, diff, bt, seed=11, generator=gen())[0]
    assert torch.equal(a, L.denoising_losses(mdm, diff, bt, seed=11, generator=gen())[0])
    assert not torch.equal(a, L.denoising_losses(mdm, diff, bt, seed=12, generator=gen())[0])


@pytest.mark.gpu
def test_calc_val_loss_and_calc_loss_vs_golden(lib):
    from interdiff_amd import losses as L
    z = g()
    P, bt, samples = int(z['past_len']), clip_batch(z), tn(z['samples']).to(DEV)
    loss, ld, wd = L.calc_val_loss(samples[0], bt, P)
    assert list(ld) == [str(k) for k in z['val_keys']] and list(wd) == list(L.LOSS_KEYS)
    close_terms(torch.stack(list(ld.values())), z['val_terms'], list(ld), 'calc_val_loss terms')
    close_terms(torch.stack(list(wd.values())), z['val_weighted'], list(wd), 'calc_val_loss weighted')
    close(loss, z['val_loss'], GATE, 'val_loss')
    loss, ld, wd, per = L.calc_loss(samples, bt, P, return_per_clip=True)
    assert list(ld) == [str(k) for k in z['test_keys']]
    close_terms(torch.stack(list(ld.values())), z['test_terms'], list(ld), 'calc_loss terms (16 + 16 _min)')
    close_terms(per.permute(1, 0, 2), np.transpose(z['test_per_clip'], (1, 0, 2)), L.LOSS_KEYS, 'calc_loss per-clip means')
    close_terms(torch.stack(list(wd.values())), z['test_weighted'], list(wd), 'calc_loss weighted')
    close(loss, z['test_loss'], GATE, 'test loss')
    assert torch.equal(per.argmin(dim=0).cpu(), tn(z['test_per_clip']).argmin(dim=0))         # every _min term picks the reference's sample
    again = L.calc_loss(list(samples), bt, P, return_per_clip=True)                            # a list of samples; two calls: same bits
    assert torch.equal(torch.stack(list(again[1].values())), torch.stack(list(ld.values()))) and torch.equal(again[3], per) and torch.equal(again[0], loss)
    # distance of both sides from the fp64 restatement (reported, not gated)
    o64, _ = lo.sample_terms(tn(z['samples'], torch.float64), tn(z['x0'], torch.float64), tn(z['hand_pose'], torch.float64), P, 'test')
    ref64 = torch.stack(list(o64.values()))
    print('calc_loss terms vs fp64 restatement: HIP %.3e, fp32 reference %.3e' % (rel(torch.stack(list(ld.values())), ref64), rel(z['test_terms'], ref64)))
    l64 = lo.weighted(o64)[0]
    print('test loss vs fp64 restatement: HIP %.3e, fp32 reference %.3e' % (rel(loss, l64), rel(z['test_loss'], l64)))


@pytest.mark.gpu
def test_calc_losses_vs_oracle_large(lib):
    """B = 16, T = 100, K = 4 against the fp64 restatement."""
    from interdiff_amd import losses as L
    samples, gt, hands = big_case()
    bt = dict(gt=gt.to(DEV), hand_pose=hands.to(DEV))
    o_test, per64 = lo.sample_terms(samples.double(), gt.double(), hands.double(), fx.PAST, 'test')
    o_val, _ = lo.sample_terms(samples[1:2].double(), gt.double(), hands.double(), fx.PAST, 'val')
    loss, ld, wd, per = L.calc_loss(samples.to(DEV), bt, fx.PAST, return_per_clip=True)
    close_terms(torch.stack(list(ld.values())), torch.stack(list(o_test.values())), list(ld), 'calc_loss B=16 T=100 K=4 vs fp64 restatement')
    close_terms(per.permute(1, 0, 2), per64.permute(1, 0, 2), L.LOSS_KEYS, '... per-clip means')
    close(loss, lo.weighted(o_test)[0], GATE, '... loss')
    vloss, vd, _ = L.calc_val_loss(samples[1].to(DEV), bt, fx.PAST)
    close_terms(torch.stack(list(vd.values())), torch.stack(list(o_val.values())), list(vd), 'calc_val_loss B=16 T=100 vs fp64 restatement')
    close(vloss, lo.weighted(o_val)[0], GATE, '... val_loss')
    assert float(vd['body_rot_v_future']) != float(L.calc_loss(samples[1:2].to(DEV), bt, fx.PAST)[1]['body_rot_v_future'])      # the two variants' future-velocity frames differ
    again = L.calc_loss(samples.to(DEV), bt, fx.PAST, return_per_clip=True)
    assert torch.equal(again[3], per) and torch.equal(again[0], loss)


@pytest.mark.gpu
@pytest.mark.parametrize('shape', EDGE_SHAPES, ids=str)
def test_kernels_vs_restatement_at_edge_shapes(lib, shape):
    """Both scoring kernels against the fp64 restatement at the shapes where the eight-wave frame split, the normalisers and the two variants' future-velocity
    windows can go wrong (EDGE_SHAPES): GATE per term and per clip, the ``_min`` picks equal to the oracle's argmin, two calls the same bits.
    Measured on MI355X: worst term over the seven shapes 8.4e-6 (0.084 of the gate; obj_rot_past at (1, 3, 1, 1), where the fp32 restatement is 8.3e-6 itself),
    per clip 8.4e-6 (0.084), the denoising entry 4.4e-7 (0.004)."""
    from interdiff_amd import losses as L, _lib
    B, T, P, K = shape
    tag = 'B=%d T=%d past=%d K=%d' % shape
    ref = edge_ref(shape)
    samples, gt, hands = (a.to(DEV) for a in edge_case(shape))
    bt = dict(gt=gt, hand_pose=hands)
    loss, ld, wd, per = L.calc_loss(samples, bt, P, return_per_clip=True)
    assert list(ld) == list(L.LOSS_KEYS + L.MIN_KEYS) and per.shape == (K, 16, B)
    close_terms(torch.stack(list(ld.values())), ref['test'], list(ld), 'calc_loss %s vs fp64 restatement' % tag)
    close_terms(per.permute(1, 0, 2), ref['per_test'].permute(1, 0, 2), L.LOSS_KEYS, '... per-clip means')
    l64, w64 = lo.weighted(dict(zip(L.LOSS_KEYS, ref['test'][:16])))
    close_terms(torch.stack(list(wd.values())), torch.stack(list(w64.values())), L.LOSS_KEYS, '... weighted')
    close(loss, l64, GATE, '... loss')
    assert torch.equal(per.argmin(dim=0).cpu(), ref['per_test'].argmin(dim=0))                     # every _min term picks the oracle's sample
    again = L.calc_loss(samples, bt, P, return_per_clip=True)
    assert torch.equal(again[3], per) and torch.equal(again[0], loss) and torch.equal(torch.stack(list(again[1].values())), torch.stack(list(ld.values())))
    vloss, vd, vw, vper = L._score(samples[:1], bt, P, L.LossWeights(), _lib.LOSS_VAL)
    assert list(vd) == list(L.LOSS_KEYS)
    close_terms(torch.stack(list(vd.values())), ref['val'], list(vd), 'calc_val_loss %s vs fp64 restatement' % tag)
    close_terms(vper.permute(1, 0, 2), ref['per_val'].permute(1, 0, 2), L.LOSS_KEYS, '... per-clip means')
    close(vloss, lo.weighted(dict(zip(L.LOSS_KEYS, ref['val'])))[0], GATE, '... val_loss')
    v2 = L.calc_val_loss(samples[0], bt, P)
    assert torch.equal(v2[0], vloss) and all(torch.equal(v2[1][k], vd[k]) for k in L.LOSS_KEYS)
    # the raw teacher-forced entry on pred = samples[0]
    sentinel = -7.0
    out = [torch.full((16, B), sentinel, device=DEV) for _ in range(2)]
    pred = samples[0].contiguous()
    rc = [lib.interdiff_denoising_losses(_lib.dptr(pred), _lib.dptr(gt), B, T, P, _lib.dptr(o), _lib.stream()) for o in out]
    torch.cuda.synchronize()
    if P < 2:
        assert rc == [-22, -22] and bool((out[0] == sentinel).all())                               # IDF_E_INVAL, nothing launched
        return
    assert rc == [0, 0] and torch.equal(out[0], out[1])
    close_terms(out[0], ref['den'], L.LOSS_KEYS, 'interdiff_denoising_losses %s on samples[0] vs fp64 restatement' % tag)
    if B == 65:                                                                                     # a clip's numbers are its own
        for b in (0, 31, 64):
            alone = L.calc_loss(samples[:, b:b + 1].contiguous(), dict(gt=gt[b:b + 1].contiguous(), hand_pose=hands[:, b:b + 1].contiguous()), P, return_per_clip=True)[3]
            assert torch.equal(alone[:, :, 0], per[:, :, b]), 'clip %d' % b


@pytest.mark.gpu
def test_validation_and_test_step_plumbing(lib):
    """validation_step / test_step under a fixed seed == calc_* applied to samples drawn from the same sampler under the same seeds."""
    from interdiff_amd import losses as L
    from interdiff_amd.diffusion import create_gaussian_diffusion
    from interdiff_amd.mdm import MDM
    z = g()
    P, bt, steps, K = int(z['past_len']), clip_batch(z), 50, 3
    model, d50 = MDM(fx.mdm_weights_wc(), device=DEV, n_steps=steps), create_gaussian_diffusion('cosine', steps)
    kw = {'y': dict(cond=bt['cond'], inpainted_motion=bt['gt'], inpainting_mask=past_mask(bt['gt'], P).to(DEV))}
    draw = lambda seed: d50.p_sample_loop(model, tuple(bt['gt'].shape), clip_denoised=False, model_kwargs=kw, seed=seed)
    s0 = draw(41)
    assert torch.equal(s0[..., :P], bt['gt'][..., :P]) and bool(torch.isfinite(s0).all())      # x_T inpainted, past frames kept
    vl, vd, vw = L.validation_step(model, d50, bt, past_len=P, seed=41)
    rl, rd, rw = L.calc_val_loss(s0, bt, P)
    assert torch.equal(vl, rl) and all(torch.equal(vd[k], rd[k]) and torch.equal(vw[k], rw[k]) for k in L.LOSS_KEYS)
    assert float(vd['body_rot_past']) == 0.0 and float(vd['body_rot_future']) > 0.0
    tl, td, tw = L.test_step(model, d50, bt, past_len=P, seed=41, diverse_samples=K)
    samples = [draw(s) for s in L.sample_seeds(41, K)]
    assert torch.equal(samples[0], s0) and not torch.equal(samples[1], s0)
    rl, rd, rw = L.calc_loss(samples, bt, P)
    assert list(td) == list(L.LOSS_KEYS + L.MIN_KEYS)
    assert torch.equal(tl, rl) and all(torch.equal(td[k], rd[k]) for k in td) and all(torch.equal(tw[k], rw[k]) for k in tw)
    assert all(float(td[k + '_min']) <= float(td[k]) for k in L.LOSS_KEYS)
    print('validation_step loss %.6f, test_step loss %.6f (50-step schedule, K = %d)' % (float(vl), float(tl), K))
