"""The denoiser trainer (interdiff_amd/mdm_train.py, csrc/mdm_train.h / .hip): the backward of MDM.forward under the loss of forward_backward, and AdamW,
against the fp64 oracle tests/mdm_train_oracle.py and the reference's OWN fp32 run recorded by tests/golden/make_golden_mdm_train.py
(tests/golden/mdm_train_{A,B,traj}.npz: the reference module under its own forward_backward with autograd on, torch.optim.AdamW).

Gradient gate (the project's): per tensor max|g - g64| / max|g64| <= max(4 e_ref, 1e-5), e_ref = the same measure of the reference's fp32 gradient against
the fp64 oracle, recorded per tensor; the recorder asserts 4 e_ref <= 1e-4 everywhere.  Loss and terms: 1e-5 relative to fp64.  pred: the flat 1e-4 against
MDM.forward.  Trajectory: 6 AdamW steps, losses 1e-5 relative, at most 0.1 % of the 7,069,900 parameters further than 8 y_traj from the fp64 trajectory
(y_traj = the reference's own fp32 distance; a cap, not a measurement).  Bit-identity claims are ``torch.equal``.  Every figure is printed before it is asserted.

Points: A  B = 4, T = 35, t = [37, 412, 655, 999] (M = 140 rows);  B  B = 3, T = 100, t = [0, 500, 999] (M = 300: self-attention over more than one 64-key tile,
t = 0, an odd batch).  Weights: fixtures.mdm_weights_wc(), with the rows of the sinusoidal table that the reference runs read taken from the recordings (``weights()``:
sin / cos of fp32 arguments differ in the last bits between CPUs, and e_ref is that small).  Without the feature this module fails at import (interdiff_amd.mdm_train does not exist).

Edge shapes (no recording, the fp64 oracle on synthetic points): the loss-gradient entry at LOSS_GRAD_SHAPES (1e-5 of max|d|; worst on MI355X 8.1e-8), the decoder-only
entry with a free memory length at SHAPES (pred / terms / d_cond 1e-4, the tensors under helpers.shape_gate; worst tensor 0.164 of its gate, pred 9.6e-8, terms 2.8e-7,
d_cond 5.6e-7), AdamW on injected gradients against torch.optim.AdamW (worst 0.998 of the one-ulp gate, moments 9.9e-8 of max), and the refused shapes.
"""
import numpy as np
import pytest
import torch
from tests import fixtures as fx
from tests import losses_oracle as lo
from tests import mdm_train_oracle as mo
from tests.denoiser_train_helpers import (adam_vectors, betas, check_new_symbols, compare_all, far_parameters, gate, rel, shape_gate, synthetic_point, tn,
                                          worst_d32)
from interdiff_amd.mdm_train import PARAM_NAMES

DEV = 'cuda'
N_PARAM = 7069900
NEW_SYMBOLS = {
    'interdiff_denoising_loss_grad': 'const float *pred, const float *target, int32_t B, int32_t T, int32_t past_len, const float *weights16, float *d_pred, void *stream',
    'interdiff_mdm_train_param_table': 'int64_t *offsets, int64_t *sizes, int32_t *n_tensors, int64_t *n_param',
    'interdiff_mdm_train_workspace_bytes': 'int32_t B, int32_t T, int32_t mem_len',
    'interdiff_mdm_train_grads': 'const float *params, const float *pe, int32_t pe_rows, const float *x_t, const int64_t *ts, const float *cond, const float *target, '
                                 'int32_t B, int32_t T, int32_t mem_len, int32_t past_len, const float *weights16, const float *d_pred_in, float *grads, float *d_cond, '
                                 'float *pred, float *terms, void *ws, size_t ws_bytes, void *stream',
    'interdiff_mdm_train_step': 'float *params, const float *grads, float *exp_avg, float *exp_avg_sq, int64_t n, int32_t step, double lr, double beta1, double beta2, '
                                'double eps, double weight_decay, void *stream',
}


_POINTS = {}


def weights():
    """fixtures.mdm_weights_wc() with the positional-table rows the reference runs read (all three recordings; they agree where they overlap)."""
    files = [fx.golden('mdm_train_%s.npz' % n) for n in ('A', 'B', 'traj')]
    return mo.with_pe_rows(fx.mdm_weights_wc(), *[(z['pe_idx'], z['pe_val']) for z in files])


def point(name):
    """The recorded inputs of a point and the fp64 oracle on them, computed once per process and never modified."""
    if name not in _POINTS:
        z = fx.golden('mdm_train_%s.npz' % name)
        z = {k: z[k] for k in z.files}
        x0, cond, t, eps = tn(z['x0']), tn(z['cond']), tn(z['t']), tn(z['eps'])
        x_t = lo.q_sample(betas(), x0, t, eps)
        ref = mo.grads(weights(), x_t, t, cond, x0, int(z['past_len']))
        e_ref = dict(zip([str(k) for k in z['names']], z['e_ref']))
        _POINTS[name] = dict(z=z, x0=x0, cond=cond, t=t, eps=eps, x_t=x_t, ref=ref, e_ref=e_ref)
    return _POINTS[name]


NONDEFAULT = dict(weight_smplx_rot=0.7, weight_smplx_nonrot=1.3, weight_obj_rot=0.4, weight_obj_nonrot=2.0, weight_past=0.5, weight_v=3.0)
# (B, T, past_len) of the loss-gradient entry: the smallest shape, T = P + 2, P = 2 with more than one future frame, the T limit of the trainer, and a P whose
# P - 1 and T - P - 1 normalisers both differ from the recorded points'
LOSS_GRAD_SHAPES = [(1, 4, 2), (1, 12, 10), (2, 5, 2), (3, 128, 10), (2, 12, 9)]
# (B, T, past_len, mem_len) of the decoder-only entry, whose memory length is free: one memory row (softmax over one key), the memory-length limit, an odd batch with an
# odd memory, the T limit, the smallest clip
SHAPES = [(2, 12, 10, 1), (1, 35, 10, 16), (3, 20, 10, 7), (1, 128, 10, 10), (2, 4, 2, 3)]
FP32_CAP, D32_CAP = 2.5e-5, 1e-2
_SHAPE_POINTS = {}


def shape_point(shape):
    """A synthetic point (seed 9400 + T + mem_len) with the oracle on it in fp64 and in fp32, computed once per process and never modified."""
    if shape not in _SHAPE_POINTS:
        B, T, past, mem = shape
        p = synthetic_point(9400 + T + mem, B, T, past, mem)
        run = lambda dtype: mo.grads(weights(), p['x_t'], p['t'], p['cond'], p['x0'], past, dtype=dtype)
        _SHAPE_POINTS[shape] = dict(p, ref=run(torch.float64), r32=run(torch.float32))
    return _SHAPE_POINTS[shape]


def loss_grad_case(B, T, P):
    """gt = the tokens of a synthetic clip batch, pred = gt + 0.3 N(0, 1)."""
    from interdiff_amd import synthetic as syn
    gt = tn(syn.make_clip_batch(9500 + T + P, B, T, past_len=P, n_points=8)['gt'])
    return gt + 0.3 * fx._randn(np.random.RandomState(9501 + T + P), *gt.shape), gt


# ------------------------------------------------------------------------------------------------------------ CPU

@pytest.mark.parametrize('shape', SHAPES)
def test_fp32_oracle_cap_at_shapes(shape):
    """The condition ``test_shapes_vs_fp64`` rests on: the oracle in fp32 -- the reference arithmetic, not the code under test -- is within FP32_CAP of the fp64 oracle on
    pred, terms and d_cond, and 4 d32(k), the part of ``shape_gate`` that can exceed the flat 1e-4, stays under D32_CAP = 1e-2 of max|g64| for every non-``wk`` tensor."""
    s = shape_point(shape)
    ref, r32 = s['ref'], s['r32']
    worst, name, wk_top, wk_scale = worst_d32(ref, r32, mo.WK_NAMES)
    e = {k: rel(r32[k], ref[k]) for k in ('pred', 'd_cond')}
    e['terms'] = rel(r32['terms'], ref['terms'])                       # (the [16,B] stack on its largest entry, as tests/test_skeleton_mdm_train.py measures it)
    print('B=%d T=%d past_len=%d mem_len=%d: fp32 oracle vs fp64: 4 d32 worst %.3e of max|g64| (%s; cap %.0e); wk %.3e of max|g64|, %.3e on wk_scale; pred %.3e, '
          'terms %.3e, d_cond %.3e (cap %.1e)' % (*shape, worst, name, D32_CAP, wk_top, wk_scale, e['pred'], e['terms'], e['d_cond'], FP32_CAP))
    assert worst <= D32_CAP and max(e.values()) <= FP32_CAP
    assert all(float(ref['grads'][k].abs().max()) > 0 for k in PARAM_NAMES) and min(ref['wk_scale'].values()) > 0
    if shape[3] == 1:                                                      # one key: dS = 0, so the q and k rows of every cross-attention in-projection get exactly nothing
        for l in range(8):
            for k in ('decoder.layers.%d.multihead_attn.in_proj_weight' % l, 'decoder.layers.%d.multihead_attn.in_proj_bias' % l):
                assert not bool(ref['grads'][k][:512].ne(0).any()) and bool(ref['grads'][k][512:].ne(0).any()), k


@pytest.mark.parametrize('name', ['A', 'B'])
def test_oracle_vs_reference_samples(name):
    """The fp64 oracle against every 64th entry of the reference's own fp32 gradients, within the recorded e_ref (which is the reference's distance over ALL
    entries, so the sampled distance cannot exceed it but for the rounding of the two products below), and the recorded fp32 loss."""
    p = point(name)
    z, ref, stride = p['z'], p['ref'], int(p['z']['stride'])
    assert [str(k) for k in z['names']] == list(PARAM_NAMES) + ['d_cond', 'd_pred']
    assert 4 * float(z['e_ref'].max()) <= 1e-4
    at, worst = 0, 0.0
    for k in PARAM_NAMES:
        g = ref['grads'][k].reshape(-1)[::stride]
        s = tn(z['ref_grad_samples'][at:at + g.numel()]).double()
        at += g.numel()
        e = float((s - g).abs().max() / ref['grads'][k].abs().max())
        worst = max(worst, e / p['e_ref'][k])
        assert e <= 1.01 * p['e_ref'][k], k                                 # (1.01: the recorder's own assertion; fp64 sums differ in the last bits between machines)
        assert float(ref['grads'][k].abs().max()) > 0
    assert at == len(z['ref_grad_samples'])
    for key, samples in (('d_cond', 'ref_d_cond_samples'), ('d_pred', 'ref_d_pred_samples')):
        g = ref[key].reshape(-1)
        e = float((tn(z[samples]).double() - g[::stride]).abs().max() / g.abs().max())
        assert e <= 1.01 * p['e_ref'][key], key
    el = abs(float(ref['loss']) - float(z['ref_loss'])) / float(ref['loss'])
    w = torch.tensor(lo.weight_vector(), dtype=torch.float64)[:, None]
    ew = rel(tn(z['ref_weighted']), ref['terms'] * w)
    print('point %s: sampled reference vs oracle: worst e / e_ref %.3f; loss %.2e, weighted terms %.2e' % (name, worst, el, ew))
    assert el <= 1e-5 and ew <= 1e-5


@pytest.mark.parametrize('name', ['A', 'B'])
def test_closed_form_d_pred_vs_autograd(name):
    p = point(name)
    e = rel(mo.d_pred_closed_form(p['ref']['pred'], p['x0'].double(), 10), p['ref']['d_pred'])
    print('point %s: closed-form d_pred vs autograd (fp64): %.2e' % (name, e))
    assert e <= 1e-12
    # other weights and another past length take the same form
    g = torch.Generator().manual_seed(5)
    gt = torch.randn(2, 1, 144, 17, generator=g, dtype=torch.float64)
    pred = gt + 0.3 * torch.randn(2, 1, 144, 17, generator=g, dtype=torch.float64)
    wts = NONDEFAULT
    with torch.enable_grad():
        pr = pred.clone().requires_grad_(True)
        auto = torch.autograd.grad(mo.loss_of(pr, gt, 4, wts)[0], pr)[0]
    assert rel(mo.d_pred_closed_form(pred, gt, 4, wts), auto) <= 1e-12
    # ... and so do the edges: the smallest shape (one second-difference term on either side of the boundary) and P = 2 with T = P + 3
    for T, P in ((4, 2), (5, 2)):
        gt = torch.randn(2, 1, 144, T, generator=g, dtype=torch.float64)
        pred = gt + 0.3 * torch.randn(2, 1, 144, T, generator=g, dtype=torch.float64)
        for w in (None, wts):
            with torch.enable_grad():
                pr = pred.clone().requires_grad_(True)
                auto = torch.autograd.grad(mo.loss_of(pr, gt, P, w)[0], pr)[0]
            assert rel(mo.d_pred_closed_form(pred, gt, P, w), auto) <= 1e-12, (T, P)


def test_new_symbols_declared_typed_and_exported():
    """Fails on the parent commit: the entries do not exist there."""
    check_new_symbols(NEW_SYMBOLS)
    assert 'mdm_train.hip' in __import__('interdiff_amd.csrc.build', fromlist=['sources']).sources()


def test_param_table_covers_the_144_names():
    from interdiff_amd.mdm_train import param_table
    sd = fx.mdm_weights()
    carried = ('finalLinear.', 'bodyFutureEmbedding.', 'objFutureEmbedding.', 'PositionalEmbedding.', 'encoder.', 'pcEmbedding.')
    assert sorted(PARAM_NAMES) == sorted(k for k in sd if not k.startswith(carried))
    assert len(PARAM_NAMES) == len(set(PARAM_NAMES)) == 144
    off, size, n = param_table()
    assert n == N_PARAM == sum(sd[k].numel() for k in PARAM_NAMES)
    at = 0
    for k, o, s in zip(PARAM_NAMES, off, size):                            # in order, back to back: no overlap, no gap
        assert o == at and s == sd[k].numel(), k
        at += s
    assert at == n


def test_constructor_refuses_dropout_and_condition_masking():
    from interdiff_amd.mdm_train import DenoiserTrainer
    for kw in (dict(dropout=0.1), dict(cond_mask_prob=0.1)):
        with pytest.raises(ValueError):
            DenoiserTrainer(fx.mdm_weights_wc(), device='cpu', **kw)


# ------------------------------------------------------------------------------------------------------------ GPU

def new_trainer(**kw):
    from interdiff_amd.mdm_train import DenoiserTrainer
    return DenoiserTrainer(weights(), device=DEV, **kw)


@pytest.fixture(scope='module')
def trainer(lib):
    return new_trainer()                                                   # never stepped: every test that steps builds its own


def on_dev(p):
    return {k: p[k].to(DEV) for k in ('x0', 'cond', 't', 'eps', 'x_t')}


@pytest.fixture(scope='module')
def trainers(trainer):
    return {(10, False): trainer}                                          # (past_len, non-default loss weights) -> a trainer that is never stepped


def trainer_for(trainers, past, nondefault=False):
    from interdiff_amd.losses import LossWeights
    if (past, nondefault) not in trainers:
        trainers[(past, nondefault)] = new_trainer(past_len=past, **({'weights': LossWeights(**NONDEFAULT)} if nondefault else {}))
    return trainers[(past, nondefault)]


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['A', 'B'] + LOSS_GRAD_SHAPES, ids=str)
def test_loss_grad_entry_vs_closed_form(trainers, name):
    """The recorded points at their own gate; the synthetic (B, T, past_len) at 1e-5 of max|d|, with the default weights and, through a second trainer, with others.
    Measured on MI355X: worst of the ten synthetic cases 8.1e-8 (0.008 of the gate)."""
    if isinstance(name, tuple):
        B, T, P = name
        pred, gt = loss_grad_case(B, T, P)
        for nondefault in (False, True):
            want = mo.d_pred_closed_form(pred.double(), gt.double(), P, NONDEFAULT if nondefault else None)
            got = trainer_for(trainers, P, nondefault).loss_grad(pred.to(DEV), gt.to(DEV))
            e = rel(got, want)
            print('B=%d T=%d past_len=%d, %s weights: interdiff_denoising_loss_grad vs the fp64 closed form: %.3e of max|d| (gate 1e-5)' % (
                B, T, P, 'other' if nondefault else 'default', e))
            assert got.shape == pred.shape and e <= 1e-5
        return
    p = point(name)
    want = mo.d_pred_closed_form(p['ref']['pred'], p['x0'].double(), 10)
    got = trainers[(10, False)].loss_grad(p['ref']['pred'].float().to(DEV), p['x0'].to(DEV))
    e, g = rel(got, want), gate(p['e_ref']['d_pred'])
    print('point %s: interdiff_denoising_loss_grad vs the fp64 closed form: %.3e (gate %.1e)' % (name, e, g))
    assert e <= g


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['A', 'B'])
def test_gradients_vs_fp64(trainer, name):
    from interdiff_amd.mdm import MDM
    p, d = point(name), on_dev(point(name))
    ref = p['ref']
    loss, ld, wd, grads, d_cond = trainer.loss_and_grads(dict(gt=d['x0'], cond=d['cond']), t=d['t'], noise=d['eps'])
    worst, worst_frac, bad = 0.0, 0.0, []
    for k in PARAM_NAMES:
        e, g = rel(grads[k], ref['grads'][k]), gate(p['e_ref'][k])
        worst, worst_frac = max(worst, e), max(worst_frac, e / g)
        if e > g:
            bad.append('%s %.3e > %.1e' % (k, e, g))
    ec, gc = rel(d_cond, ref['d_cond']), gate(p['e_ref']['d_cond'])
    print('point %s: 144 gradient tensors: worst rel err %.3e, worst fraction of its gate %.3f; d_cond %.3e (gate %.1e)' % (name, worst, worst_frac, ec, gc))
    assert not bad, bad
    assert ec <= gc
    el = abs(float(loss.double().mean()) - float(ref['loss'])) / float(ref['loss'])
    terms = torch.stack([ld[k] for k in lo.LOSS_KEYS])
    et = max(rel(terms[i], ref['terms'][i]) for i in range(16))
    print('point %s: loss %.3e, worst of 16 terms %.3e (gate 1e-5)' % (name, el, et))
    assert el <= 1e-5 and et <= 1e-5
    w = torch.tensor(lo.weight_vector(), dtype=torch.float64)
    assert rel(torch.stack([wd[k] for k in lo.LOSS_KEYS]), ref['terms'] * w[:, None]) <= 1e-5
    fwd = MDM(weights(), device=DEV)(trainer.diffusion.q_sample(d['x0'], d['t'], noise=d['eps']), d['t'], y={'cond': d['cond']})
    ep, e64 = rel(trainer.pred, fwd), rel(trainer.pred, ref['pred'])
    print('point %s: pred vs MDM.forward %.3e (gate 1e-4), vs fp64 %.3e' % (name, ep, e64))
    assert ep <= 1e-4


@pytest.mark.gpu
def test_two_calls_give_identical_bits(trainer):
    d = on_dev(point('B'))
    a = trainer.grads_at(d['x_t'], d['t'], d['cond'], d['x0'])
    ga = trainer.grads.clone()
    b = trainer.grads_at(d['x_t'], d['t'], d['cond'], d['x0'])
    assert torch.equal(ga, trainer.grads) and all(torch.equal(x, y) for x, y in zip(a, b))        # flat gradient; pred, terms, d_cond


@pytest.mark.gpu
def test_d_pred_seam(trainer):
    d = on_dev(point('A'))
    pred, _, dc0 = trainer.grads_at(d['x_t'], d['t'], d['cond'], d['x0'])
    g0 = trainer.grads.clone()
    dp = trainer.loss_grad(pred, d['x0'])
    _, _, dc1 = trainer.grads_at(d['x_t'], d['t'], d['cond'], d['x0'], d_pred=dp)
    assert torch.equal(g0, trainer.grads) and torch.equal(dc0, dc1)        # the default path IS the loss-gradient entry's output fed to the seam
    _, _, dc2 = trainer.grads_at(d['x_t'], d['t'], d['cond'], d['x0'], d_pred=2 * dp)
    assert torch.equal(2 * g0, trainer.grads) and torch.equal(2 * dc0, dc2)                        # the backward is linear in d_pred, bit for bit


@pytest.mark.gpu
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_shapes_vs_fp64(trainers, shape):
    """The decoder-only entry at (B, T, past_len, mem_len) where its kernels can go wrong (SHAPES), against the fp64 oracle on a synthetic point: pred, terms and d_cond
    at 1e-4, the 144 tensors under ``shape_gate`` (1e-4 of max|g64| or four times the fp32 oracle's own distance; ``test_fp32_oracle_cap_at_shapes`` caps the latter).
    Measured on MI355X: worst tensor 0.164 of its gate (at (2, 4, 2, 3)); pred 9.6e-8, terms 2.8e-7, d_cond 5.6e-7; no gate was wider than the flat 1e-4 but wk's
    (at most 1.8e-3 of max|g64|, at (1, 128, 10, 10); the kernel's wk is at most 1.0e-4 of max|g64| away)."""
    B, T, past, mem = shape
    s = shape_point(shape)
    ref, tag = s['ref'], 'B=%d T=%d past_len=%d mem_len=%d' % shape
    tr = trainer_for(trainers, past)
    pred, terms, d_cond = tr.grads_at(s['x_t'].to(DEV), s['t'].to(DEV), s['cond'].to(DEV), s['x0'].to(DEV))
    e_pred, e_cond = rel(pred, ref['pred']), rel(d_cond, ref['d_cond'])
    e_terms = rel(terms, ref['terms'])
    gate_abs, widest_wk, widest = shape_gate(ref, s['r32'], mo.WK_NAMES)
    print('%s: pred %.3e, terms %.3e, d_cond %.3e (1e-4); widest wk gate %.3e, widest other gate %.3e of max|g64|' % (tag, e_pred, e_terms, e_cond, widest_wk, widest))
    grads = tr.named_views(tr.grads)
    compare_all(grads, ref, PARAM_NAMES, gate_abs, tag)
    assert e_pred <= 1e-4 and e_terms <= 1e-4 and e_cond <= 1e-4
    assert pred.shape == s['x0'].shape and tuple(d_cond.shape) == (mem, B, 256) and tuple(terms.shape) == (16, B)
    if mem == 1:                                                           # softmax over one key: dS = 0 exactly, in the oracle and in the kernel
        for l in range(8):
            for k in ('decoder.layers.%d.multihead_attn.in_proj_weight' % l, 'decoder.layers.%d.multihead_attn.in_proj_bias' % l):
                assert not bool(ref['grads'][k][:512].ne(0).any()) and not bool(grads[k][:512].ne(0).any()), k


def adamw_entry(lib, p, g, m, v, n, step, wd, lr=3e-4):
    from interdiff_amd import _lib
    ptr = lambda t: _lib.vp(None) if t is None else _lib.dptr(t)
    return lib.interdiff_mdm_train_step(ptr(p), ptr(g), ptr(m), ptr(v), n, step, lr, 0.9, 0.999, 1e-8, wd, _lib.stream())


ADAMW_PAD = 64


def padded(a):
    """A device buffer of len(a) + ADAMW_PAD floats: ``a`` and a tail the entry must not touch."""
    return torch.cat([a.float(), torch.linspace(-3.0, 3.0, ADAMW_PAD)]).to(DEV)


@pytest.mark.gpu
@pytest.mark.parametrize('case', ['wd0', 'wd_resync', 'late'])
@pytest.mark.parametrize('n', [1, 255, 257, 70001])
def test_adamw_on_injected_gradients(lib, n, case):
    """``interdiff_mdm_train_step`` on small device vectors against torch.optim.AdamW (``_single_tensor_adamw``) on CPU fp32 tensors, three steps; each step's
    parameter change within 2^-20 relative of torch's change plus one ulp of the parameter, the moments within 1e-6 of their largest entry (the gate of
    tests/test_skeleton_finetune.py::test_adam_on_injected_gradients; the allowed differences are the association of value * m / denom and FMA contraction).
    'wd0': weight_decay 0, one uninterrupted run from zero moments.  'wd_resync': weight_decay 1e-2; before steps 2 and 3 torch starts from the kernel's own
    parameters and moments, for the reason that test's docstring records (with decay the one-ulp differences the gate allows feed the next step's moments).
    'late': weight_decay 0, both sides start from given non-zero moments with 99,998 steps behind them, where both bias corrections have long been 1; resynchronised
    like 'wd_resync', because from non-zero moments a gradient near -9 m cancels exp_avg to a few ulps of its old size, and a one-ulp difference of the moment that the
    1e-6 gate allows then is a relative difference of the NEXT step's move far above 2^-20 (seen in a numpy restatement of the kernel: 3e-5 on an entry with |p| = 9e-5).
    n: one element, one short of a block, one past a block, many blocks with a tail.  Every buffer carries 64 more floats than n, which must keep their bits.
    Measured on MI355X: worst |d_hip - d_torch| over all cases 0.998 of its gate (one ulp of the parameter: the two sums round to neighbouring floats); moments
    9.9e-8 of max (0.099 of the gate)."""
    rs = np.random.RandomState(7500 + n)
    wd, step0 = (1e-2 if case == 'wd_resync' else 0.0), (99998 if case == 'late' else 0)
    p0 = tn((0.05 * rs.standard_normal(n)).astype(np.float32))
    m0 = tn((1e-3 * rs.standard_normal(n)).astype(np.float32)) if case == 'late' else torch.zeros(n)
    # (moments a run can have: an average of g^2 is never below the square of the average of g, so |m| / sqrt(v) <= 1 and a step moves at most lr)
    v0 = (m0 ** 2 + tn((1e-3 * rs.standard_normal(n)).astype(np.float32)) ** 2) if case == 'late' else torch.zeros(n)
    pd, md, vd = padded(p0), padded(m0), padded(v0)
    tails = [t[n:].clone() for t in (pd, md, vd)]
    p = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([p], lr=3e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd, foreach=False)
    opt.state[p] = dict(step=torch.tensor(float(step0)), exp_avg=m0.clone(), exp_avg_sq=v0.clone())
    worst, worst_m = 0.0, 0.0
    for k, gv in enumerate(adam_vectors(n)):
        if k and case != 'wd0':
            with torch.no_grad():
                p.copy_(pd[:n].cpu())
                opt.state[p]['exp_avg'].copy_(md[:n].cpu())
                opt.state[p]['exp_avg_sq'].copy_(vd[:n].cpu())
        before_t, before_h = p.detach().clone().double(), pd[:n].cpu().double()
        assert case == 'wd0' or torch.equal(before_t, before_h)
        p.grad = tn(gv.copy())
        opt.step()
        gd = padded(tn(gv))
        assert adamw_entry(lib, pd, gd, md, vd, n, step0 + k + 1, wd) == 0
        assert int(opt.state[p]['step']) == step0 + k + 1
        dt, dh = p.detach().double() - before_t, pd[:n].cpu().double() - before_h
        ulp = tn(np.spacing(np.abs(p.detach().numpy()))).double()
        allowed = 2.0 ** -20 * dt.abs() + ulp
        worst = max(worst, float(((dh - dt).abs() / allowed).max()))
        for mine, theirs in ((md, opt.state[p]['exp_avg']), (vd, opt.state[p]['exp_avg_sq'])):
            worst_m = max(worst_m, float((mine[:n].cpu() - theirs).abs().max()) / float(theirs.abs().max()))
        print('n=%d %s step %d: worst |d_hip - d_torch| %.3f of its gate; moments %.3e of max (gate 1e-6); largest move %.3e' % (
            n, case, step0 + k + 1, worst, worst_m, float(dt.abs().max())))
        assert worst <= 1.0 and worst_m <= 1e-6
        assert float(dt.abs().max()) > 1e-5                                # (the step moved something)
        assert all(torch.equal(t[n:], tail) for t, tail in zip((pd, md, vd), tails)) and torch.equal(gd[n:], padded(tn(gv))[n:])


@pytest.mark.gpu
@pytest.mark.parametrize('n', [1, 255, 257, 70001])
def test_adamw_zero_gradient_and_refusals(lib, n):
    """Bit for bit: with g = 0 and zero moments the entry leaves p as it was at weight_decay 0 and gives p * float32(1 - lr wd) with decay; the 64 floats behind n keep
    their bits.  n <= 0, step < 1 and a null pointer return IDF_E_INVAL and change nothing."""
    rs = np.random.RandomState(7600 + n)
    p0 = tn((0.05 * rs.standard_normal(n)).astype(np.float32))
    for wd in (0.0, 1e-2):
        pd, gd, md, vd = padded(p0), padded(torch.zeros(n)), padded(torch.zeros(n)), padded(torch.zeros(n))
        start = [t.clone() for t in (pd, gd, md, vd)]
        assert adamw_entry(lib, pd, gd, md, vd, n, 1, wd) == 0
        want = p0 if wd == 0.0 else p0 * torch.tensor(np.float32(1.0 - 3e-4 * wd))
        assert torch.equal(pd[:n].cpu(), want) and (wd == 0.0 or not torch.equal(want, p0))
        assert not bool(md[:n].ne(0).any()) and not bool(vd[:n].ne(0).any())
        assert all(torch.equal(t[n:], s[n:]) for t, s in zip((pd, gd, md, vd), start))
    pd, gd, md, vd = (padded(tn(rs.standard_normal(n).astype(np.float32))) for _ in range(4))
    vd.abs_()
    start = [t.clone() for t in (pd, gd, md, vd)]
    assert adamw_entry(lib, pd, gd, md, vd, 0, 1, 0.0) == -22 and adamw_entry(lib, pd, gd, md, vd, -1, 1, 0.0) == -22
    assert adamw_entry(lib, pd, gd, md, vd, n, 0, 0.0) == -22 and adamw_entry(lib, pd, gd, md, vd, n, -3, 0.0) == -22
    for hole in range(4):
        args = [pd, gd, md, vd]
        args[hole] = None
        assert adamw_entry(lib, *args, n, 1, 0.0) == -22
    torch.cuda.synchronize()
    assert all(torch.equal(t, s) for t, s in zip((pd, gd, md, vd), start))
    assert adamw_entry(lib, pd, gd, md, vd, n, 1, 0.0) == 0 and not torch.equal(pd[:n], start[0][:n])       # (the same buffers, accepted, do move)


@pytest.mark.gpu
def test_limits_raise(lib, trainers):
    """Refused shapes are refused -- ValueError from the wrapper or the RuntimeError of ``_lib.check``, whichever the code raises -- and touch nothing: the flat gradient
    keeps its bits.  The raw entry refuses a workspace that is too small (IDF_E_NOMEM) or misaligned (IDF_E_INVAL) and writes no output; the sizing entry returns 0
    past the limits."""
    from interdiff_amd import _lib
    tr = trainer_for(trainers, 10)
    s = {k: v.to(DEV) for k, v in synthetic_point(9499, 2, 12, 10, 3).items() if k != 'past'}
    pred, terms, d_cond = tr.grads_at(s['x_t'], s['t'], s['cond'], s['x0'])
    before = tr.grads.clone()
    assert bool(before.ne(0).any())
    zeros = lambda *shape: torch.zeros(*shape, device=DEV)
    t1 = torch.zeros(1, dtype=torch.int64, device=DEV)
    refused = [
        ('T = 129', lambda: tr.grads_at(zeros(1, 1, 144, 129), t1, zeros(10, 1, 256), zeros(1, 1, 144, 129))),
        ('T = past_len + 1', lambda: tr.grads_at(zeros(1, 1, 144, 11), t1, zeros(10, 1, 256), zeros(1, 1, 144, 11))),
        ('mem_len = 17', lambda: tr.grads_at(s['x_t'], s['t'], zeros(17, 2, 256), s['x0'])),
        ('mem_len = 0', lambda: tr.grads_at(s['x_t'], s['t'], zeros(0, 2, 256), s['x0'])),
        ('cond of another B', lambda: tr.grads_at(s['x_t'], s['t'], zeros(3, 3, 256), s['x0'])),
        ('cond of another width', lambda: tr.grads_at(s['x_t'], s['t'], zeros(3, 2, 255), s['x0'])),
        ('d_pred of another shape', lambda: tr.grads_at(s['x_t'], s['t'], s['cond'], s['x0'], d_pred=zeros(2, 1, 144, 11))),
        ('target of another shape', lambda: tr.grads_at(s['x_t'], s['t'], s['cond'], zeros(2, 1, 144, 11))),
        ('143 channels', lambda: tr.grads_at(zeros(2, 1, 143, 12), s['t'], s['cond'], zeros(2, 1, 143, 12))),
    ]
    for what, call in refused:
        with pytest.raises((ValueError, RuntimeError)):
            call()
        torch.cuda.synchronize()
        assert torch.equal(tr.grads, before), what
    # the raw entry and its workspace
    B, T, S = 2, 12, 3
    need = lib.interdiff_mdm_train_workspace_bytes(B, T, S)
    assert need > 0
    ws = torch.empty(need + 256, dtype=torch.uint8, device=DEV)
    sentinel = -7.0
    outs = [torch.full(shape, sentinel, device=DEV) for shape in ((S, B, 256), (B, 1, 144, T), (16, B))]
    def raw(ws_ptr, ws_bytes, T_=T, S_=S, past=10):
        return lib.interdiff_mdm_train_grads(_lib.dptr(tr.params), _lib.dptr(tr.pe), tr.pe.shape[0], _lib.dptr(s['x_t']), _lib.dptr(s['t']), _lib.dptr(s['cond']),
                                             _lib.dptr(s['x0']), B, T_, S_, past, tr._wvec, _lib.vp(None), _lib.dptr(tr.grads), _lib.dptr(outs[0]), _lib.dptr(outs[1]),
                                             _lib.dptr(outs[2]), ws_ptr, ws_bytes, _lib.stream())
    base = ws.data_ptr()
    assert base % 256 == 0
    assert raw(_lib.vp(base), need - 1) == -12                             # one byte short: IDF_E_NOMEM
    assert raw(_lib.vp(base + 4), need) == -22                             # not 256-byte aligned: IDF_E_INVAL
    assert raw(_lib.vp(None), need) == -22
    assert raw(_lib.vp(base), need, past=11) == -22 and raw(_lib.vp(base), need, T_=129) == -22 and raw(_lib.vp(base), need, S_=17) == -22
    assert raw(_lib.vp(base), need, S_=0) == -22 and raw(_lib.vp(base), need, past=1) == -22
    with pytest.raises(RuntimeError):
        _lib.check(raw(_lib.vp(base), need - 1))
    torch.cuda.synchronize()
    assert torch.equal(tr.grads, before) and all(bool((o == sentinel).all()) for o in outs)
    assert raw(_lib.vp(base), need) == 0                                   # the same call with its workspace runs, and gives the wrapper's bits
    torch.cuda.synchronize()
    assert torch.equal(tr.grads, before) and torch.equal(outs[0], d_cond) and torch.equal(outs[1], pred) and torch.equal(outs[2], terms)
    size = lib.interdiff_mdm_train_workspace_bytes
    assert size(1, 129, 10) == 0 and size(1, 12, 17) == 0 and size(1, 12, 0) == 0 and size(0, 12, 10) == 0
    assert size(1, 128, 16) > size(1, 128, 1) > 0 and size(1, 4, 3) > 0


@pytest.fixture(scope='module')
def traj():
    """The recorded per-step t / noise and the fp64 oracle's trajectory on them, computed once."""
    z = fx.golden('mdm_train_traj.npz')
    z = {k: z[k] for k in z.files}
    p = point('A')
    ts, noises = [tn(t) for t in z['t']], [tn(e) for e in z['noise']]
    losses, theta = mo.trajectory(weights(), betas(), p['x0'], p['cond'], ts, noises, 10, lr=float(z['lr']))
    return dict(z=z, ts=ts, noises=noises, losses=losses, theta=theta)


def test_oracle_trajectory_vs_reference_samples(traj):
    """CPU: the fp64 trajectory against every 64th entry of the reference's final fp32 parameters, within the recorded y_traj, and its losses."""
    z, stride = traj['z'], int(traj['z']['stride'])
    flat = torch.cat([traj['theta'][k].reshape(-1)[::stride] for k in PARAM_NAMES])
    d = float((tn(z['ref_theta_samples']).double() - flat).abs().max())
    el = max(abs(a - float(b)) / a for a, b in zip(traj['losses'], z['ref_losses']))
    print('trajectory: sampled reference theta vs fp64 %.3e (y_traj %.3e); losses %.2e' % (d, float(z['y_traj']), el))
    assert d <= 1.01 * float(z['y_traj']) and el <= 1e-5


@pytest.mark.gpu
def test_trajectory_vs_fp64(lib, traj):
    p, z = on_dev(point('A')), traj['z']
    tr = new_trainer(lr=float(z['lr']))
    batch = dict(gt=p['x0'], cond=p['cond'])
    for k, (t, eps) in enumerate(zip(traj['ts'], traj['noises'])):
        loss = tr.training_step(batch, t=t.to(DEV), noise=eps.to(DEV))[0]
        e = abs(float(loss.double().mean()) - traj['losses'][k]) / traj['losses'][k]
        print('step %d: loss %.6f, rel err vs fp64 %.2e (gate 1e-5)' % (k + 1, float(loss.mean()), e))
        assert e <= 1e-5
    got = tr.state_dict()
    y = float(z['y_traj'])
    far, worst = far_parameters(got, traj['theta'], PARAM_NAMES, y)
    print('trajectory: %d of %d parameters further than 8 y_traj = %.3e from fp64 (cap %d); max distance %.3e' % (far, N_PARAM, 8 * y, N_PARAM // 1000, worst))
    assert far <= N_PARAM // 1000


@pytest.mark.gpu
def test_plumbing(lib, traj):
    from interdiff_amd.mdm_train import DenoiserTrainer
    p = on_dev(point('A'))
    sd = weights()
    batch = dict(gt=p['x0'], cond=p['cond'])
    step = lambda tr, k: tr.training_step(batch, t=traj['ts'][k].to(DEV), noise=traj['noises'][k].to(DEV))
    a = new_trainer()
    step(a, 0), step(a, 1)
    # state + optimizer state continue the trajectory bit for bit
    b = DenoiserTrainer(a.state_dict(), device=DEV)
    b.load_optimizer_state(a.optimizer_state())
    assert b.step == 2 and torch.equal(a.params, b.params)
    step(a, 2), step(b, 2)
    assert torch.equal(a.params, b.params) and torch.equal(a.exp_avg, b.exp_avg) and torch.equal(a.exp_avg_sq, b.exp_avg_sq)
    assert not torch.equal(a.params, new_trainer().params)
    # the untouched tensors come back with identical bits, the trained ones under the reference's names and shapes
    out = a.state_dict()
    assert set(out) == set(sd)
    carried = [k for k in sd if k not in PARAM_NAMES]
    assert 'encoder.layers.3.queries' in carried and 'pcEmbedding.Linear.weight' in carried
    for k in carried:
        assert torch.equal(out[k], sd[k]), k
    assert all(out[k].shape == sd[k].shape for k in PARAM_NAMES)
    # the exported sampler model computes what the trainer's forward computes
    loss = a.loss_and_grads(batch, t=p['t'], noise=p['eps'])[0]
    fwd = a.export_mdm()(a.diffusion.q_sample(p['x0'], p['t'], noise=p['eps']), p['t'], y={'cond': p['cond']})
    e = rel(a.pred, fwd)
    print('export_mdm().forward vs the trainer\'s pred after 3 steps: %.3e (gate 1e-4); loss %.4f' % (e, float(loss.mean())))
    assert e <= 1e-4
    # T > 128 is refused
    big = torch.zeros(1, 1, 144, 129, device=DEV)
    with pytest.raises(ValueError):
        a.loss_and_grads(dict(gt=big, cond=torch.zeros(10, 1, 256, device=DEV)), t=torch.zeros(1, dtype=torch.int64))
