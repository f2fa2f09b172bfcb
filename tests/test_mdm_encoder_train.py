"""The denoiser trainer with the encoder in the pass (``DenoiserTrainer(state_dict, train_encoder=True)``, csrc/mdm_train.h / .hip ``interdiff_mdm_train_full_grads``):
the backward of ``MDM._get_embeddings`` from pc_embedding on, chained behind the decoder's, against the fp64 oracle tests/mdm_encoder_train_oracle.py and the reference's
OWN fp32 run recorded by tests/golden/make_golden_mdm_encoder_train.py (tests/golden/mdm_enc_train_{E1,E2,traj}.npz).

Gradient gate (the project's): per tensor max|g - g64| <= max(4 e_ref, 1e-5) of the tensor's scale, e_ref = the same measure of the reference's fp32 gradient, recorded
per tensor (228 tensors, d_cond, d_pc); the recorder asserts 4 e_ref <= 1e-4 for every one of them, and that a second fp32 run (the oracle in fp32) lies within every gate.
The scale is max|g64|, except for the twelve ten-entry ``wk`` tensors of the QaN layers (six decoder, six encoder): d wk[n] = sum_{b,t,c} d block[t,b,c] o_n[b,t,c] behind a
post-norm LayerNorm is a sum that cancels to 1/300 .. 1/160,000 of the sum of its products' magnitudes, fp32 rounding of the products is 1e-6 .. 2.4e-3 of the remainder (the
reference's own run at E2), and the sum of magnitudes (``wk_scale``, tests/mdm_encoder_train_oracle.py) is the scale on which it is well conditioned:
there the reference is within 1.5e-8.  Their gate is max(4 e_ref wk_scale, 1e-5 max|g64|) -- the floor stays on max|g64|.
Loss 1e-5 relative to fp64; each of the 16 terms on its OWN size within max(4 e_ref_term, 1e-5), e_ref_term recorded from the reference's fp32 terms (the velocity terms
are means of squared second differences of O(1) values, 1e-5 of the largest term in size; the reference's own worst is 4.9e-6 at E1 and 1.8e-5 at E2).  cond 1e-4 against the
oracle's encoder output.  Trajectory: 6 AdamW steps, losses 1e-5, at most 0.1 % of the 11,824,392 parameters further than 8 y_traj from the fp64 trajectory.  Bit-identity
claims are ``torch.equal``.  Every figure is printed before it is asserted.

Points: E1  B = 4, T = 35, past_len 10, t = [37, 412, 655, 999] (the scene of mdm_train_A; 40 encoder rows);  E2  B = 3, T = 12, past_len 5, t = [0, 500, 999] (an
odd batch, a memory length other than 10, the shortest decoder the limits allow, t = 0; 15 encoder rows, one 32-row GEMM tile not filled).  pc_embedding is a recorded leaf.
Measured on MI355X: DESIGN.md 8.16.  Without the feature every test below fails: the keyword, the names and the entries do not exist.

Edge shapes (no recording, the fp64 oracle on synthetic points, SHAPES): pred / cond / terms / d_cond / d_pc 1e-4, the 228 tensors under helpers.shape_gate, whose wider
part an unmarked test caps at 1e-2 of max|g64|.  Worst on MI355X: a tensor at 0.514 of its gate (``encoder.layers.6.queries`` at past_len 2), pred 1.2e-7, cond 5.5e-7,
terms 1.1e-7, d_cond 6.9e-7, d_pc 5.0e-7.  ``test_limits_raise``: refused shapes touch nothing.
"""
import numpy as np
import pytest
import torch
from tests import fixtures as fx
from tests import losses_oracle as lo
from tests import mdm_train_oracle as mo
from tests.denoiser_train_helpers import betas, check_new_symbols, compare_all, far_parameters, gate, rel, shape_gate, synthetic_point, tn, worst_d32

DEV = 'cuda'
N_PARAM, N_PARAM_DEC = 11824392, 7069900
# (B, T, past_len) of the full entry: one clip, an odd length, the T limit, the smallest clip with the shortest memory (every QaN token of the encoder has a masked
# neighbour), that memory under a longer clip, the memory-length limit
SHAPES = [(1, 12, 10), (2, 33, 10), (1, 128, 10), (2, 4, 2), (2, 12, 2), (1, 18, 16)]
FP32_CAP, D32_CAP = 2.5e-5, 1e-2
# The seed of a shape's synthetic point is 9300 + T + past_len, but for the two past_len 2 shapes.  There the gradient of the encoder's ``queries`` shrinks about threefold per
# layer (7e-8 in layer 1, 1e-9 .. 2e-8 in layer 6, by the seed) while fp32 leaves about 1e-12 on each, so 4 d32 / max|g64| of ``encoder.layers.6.queries`` is 3.7e-3 / 1.4e-3 at
# seeds 9306 / 9314 on one CPU and 1.3e-2 / 3.2e-3 on another (the fp32 oracle's rounding is not the same on every CPU): past D32_CAP.  These two seeds are chosen on the fp64 oracle alone -- of the twelve seeds from
# 9300 + T + past_len on, the one where max|g64| of that tensor is largest (2.0e-8 and 1.5e-8 against 1.6e-9 and 3.2e-9) -- so the point and not the cap carries the margin.
SEEDS = {(2, 4, 2): 9312, (2, 12, 2): 9324}
_SHAPE_POINTS = {}
NEW_SYMBOLS = {
    'interdiff_mdm_train_full_param_table': 'int64_t *offsets, int64_t *sizes, int32_t *n_tensors, int64_t *n_param',
    'interdiff_mdm_train_full_workspace_bytes': 'int32_t B, int32_t T, int32_t past_len',
    'interdiff_mdm_train_full_grads': 'const float *params, const float *pe, int32_t pe_rows, const float *x_t, const int64_t *ts, const float *pc, const float *target, '
                                      'int32_t B, int32_t T, int32_t past_len, const float *weights16, const float *d_pred_in, float *grads, float *cond, float *d_cond, '
                                      'float *d_pc, float *pred, float *terms, void *ws, size_t ws_bytes, void *stream',
}
SHARED = ('bodyEmbedding.weight', 'bodyEmbedding.bias', 'objEmbedding.weight', 'objEmbedding.bias')


def names():
    from interdiff_amd import mdm_train as mt
    return mt.PARAM_NAMES, mt.ENCODER_PARAM_NAMES, mt.FULL_PARAM_NAMES


def meo():
    from tests import mdm_encoder_train_oracle
    return mdm_encoder_train_oracle


_POINTS = {}


def weights():
    """fixtures.mdm_weights_wc() with the positional-table rows the reference runs read (all three recordings; they agree where they overlap)."""
    files = [fx.golden('mdm_enc_train_%s.npz' % n) for n in ('E1', 'E2', 'traj')]
    return mo.with_pe_rows(fx.mdm_weights_wc(), *[(z['pe_idx'], z['pe_val']) for z in files])


def point(name):
    """The recorded inputs of a point and the fp64 oracle on them, computed once per process and never modified."""
    if name not in _POINTS:
        z = fx.golden('mdm_enc_train_%s.npz' % name)
        z = {k: z[k] for k in z.files}
        x0, pc, t, eps, past = tn(z['x0']), tn(z['pc']), tn(z['t']), tn(z['eps']), int(z['past_len'])
        x_t = lo.q_sample(betas(), x0, t, eps)
        ref = meo().grads(weights(), x_t, t, pc, x0, past)
        e_ref = dict(zip([str(k) for k in z['names']], z['e_ref']))
        assert [str(k) for k in z['wk_names']] == list(meo().WK_NAMES)
        _POINTS[name] = dict(z=z, x0=x0, pc=pc, t=t, eps=eps, x_t=x_t, past=past, ref=ref, e_ref=e_ref)
    return _POINTS[name]


@pytest.fixture(scope='module')
def traj():
    """The recorded per-step t / noise and the fp64 oracle's trajectory on them (E2's scene), computed once."""
    z = fx.golden('mdm_enc_train_traj.npz')
    z = {k: z[k] for k in z.files}
    p = point('E2')
    ts, noises = [tn(t) for t in z['t']], [tn(e) for e in z['noise']]
    losses, theta = meo().trajectory(weights(), betas(), p['x0'], p['pc'], ts, noises, p['past'], lr=float(z['lr']))
    return dict(z=z, ts=ts, noises=noises, losses=losses, theta=theta)


def shape_point(shape):
    """A synthetic point (seed 9300 + T + past_len, or SEEDS) with the oracle on it in fp64 and in fp32, computed once per process and never modified."""
    if shape not in _SHAPE_POINTS:
        B, T, past = shape
        p = synthetic_point(SEEDS.get(shape, 9300 + T + past), B, T, past)
        run = lambda dtype: meo().grads(weights(), p['x_t'], p['t'], p['pc'], p['x0'], past, dtype=dtype)
        _SHAPE_POINTS[shape] = dict(p, ref=run(torch.float64), r32=run(torch.float32))
    return _SHAPE_POINTS[shape]


# ------------------------------------------------------------------------------------------------------------ CPU

@pytest.mark.parametrize('shape', SHAPES)
def test_fp32_oracle_cap_at_shapes(shape):
    """The condition ``test_shapes_vs_fp64`` rests on: the oracle in fp32 -- the reference arithmetic, not the code under test -- is within FP32_CAP of the fp64 oracle on
    pred, cond, terms, d_cond and d_pc, and 4 d32(k), the part of ``shape_gate`` that can exceed the flat 1e-4, stays under D32_CAP = 1e-2 of max|g64| for every
    non-``wk`` tensor (it exceeds 1e-4 for ``encoder.layers.6.queries`` at past_len 2 alone: 6.0e-4 .. 8.8e-4 on two CPUs at SEEDS)."""
    _, _, FULL = names()
    s = shape_point(shape)
    ref, r32 = s['ref'], s['r32']
    worst, name, wk_top, wk_scale = worst_d32(ref, r32, meo().WK_NAMES)
    e = {k: rel(r32[k], ref[k]) for k in ('pred', 'cond', 'd_cond', 'd_pc')}
    e['terms'] = rel(r32['terms'], ref['terms'])                       # (the [16,B] stack on its largest entry, as tests/test_skeleton_mdm_train.py measures it)
    print('B=%d T=%d past_len=%d: fp32 oracle vs fp64: 4 d32 worst %.3e of max|g64| (%s; cap %.0e); wk %.3e of max|g64|, %.3e on wk_scale; pred %.3e, cond %.3e, '
          'terms %.3e, d_cond %.3e, d_pc %.3e (cap %.1e)' % (*shape, worst, name, D32_CAP, wk_top, wk_scale, e['pred'], e['cond'], e['terms'], e['d_cond'], e['d_pc'],
                                                           FP32_CAP))
    assert worst <= D32_CAP and max(e.values()) <= FP32_CAP
    assert all(float(ref['grads'][k].abs().max()) > 0 for k in FULL) and min(ref['wk_scale'].values()) > 0


@pytest.mark.parametrize('name', ['E1', 'E2'])
def test_oracle_vs_reference_samples(name):
    """The fp64 oracle (cond NOT detached, pc a leaf) against every 64th entry of the reference's own fp32 gradients, within the recorded e_ref, and its fp32 loss;
    and the shared embedding's gradient is not the decoder-only one."""
    _, _, FULL = names()
    p = point(name)
    z, ref, stride = p['z'], p['ref'], int(p['z']['stride'])
    assert [str(k) for k in z['names']] == list(FULL) + ['d_cond', 'd_pc', 'd_pred']
    at, worst = 0, 0.0
    for k in FULL:
        g = ref['grads'][k].reshape(-1)[::stride]
        s = tn(z['ref_grad_samples'][at:at + g.numel()]).double()
        at += g.numel()
        e = float((s - g).abs().max()) / meo().grad_scale(ref, k)
        worst = max(worst, e / p['e_ref'][k])
        assert e <= 1.01 * p['e_ref'][k], k
        assert float(ref['grads'][k].abs().max()) > 0, k
    assert at == len(z['ref_grad_samples'])
    for key in ('d_cond', 'd_pc', 'd_pred'):
        g = ref[key].reshape(-1)
        e = float((tn(z['ref_%s_samples' % key]).double() - g[::stride]).abs().max() / g.abs().max())
        assert e <= 1.01 * p['e_ref'][key], key
    worst_e = max(p['e_ref'].values())
    scales = rel(tn(z['wk_scale']), torch.tensor([ref['wk_scale'][k] for k in meo().WK_NAMES], dtype=torch.float64))
    el = abs(float(ref['loss']) - float(z['ref_loss'])) / float(ref['loss'])
    w = torch.tensor(lo.weight_vector(), dtype=torch.float64)[:, None]
    ew = rel(tn(z['ref_weighted']), ref['terms'] * w)
    et = [rel(tn(z['ref_weighted'][i]), ref['terms'][i] * w[i]) for i in range(16)]
    print('point %s: sampled reference vs oracle: worst e / e_ref %.3f; worst e_ref %.2e; wk_scale recorded vs recomputed %.1e; loss %.2e, weighted terms %.2e; '
          'term by term worst %.2e (recorded %.2e)' % (name, worst, worst_e, scales, el, ew, max(et), float(z['e_ref_terms'].max())))
    assert 4 * worst_e <= 1e-4 and 4 * float(z['e_ref_terms'].max()) <= 1e-4          # every tensor, the wk tensors on their own scale; every term
    assert scales <= 1e-9 and all(abs(a - b) <= 1e-3 * b + 1e-12 for a, b in zip(et, z['e_ref_terms']))
    assert el <= 1e-5 and ew <= 1e-5
    dec = meo().grads(weights(), p['x_t'], p['t'], p['pc'], p['x0'], p['past'], detach_cond=True)
    shared = rel(ref['grads'][SHARED[0]], dec['grads'][SHARED[0]])
    print('point %s: d %s with the encoder path vs without: %.2e' % (name, SHARED[0], shared))
    assert shared > 4 * p['e_ref'][SHARED[0]]


def test_oracle_trajectory_vs_reference_samples(traj):
    _, _, FULL = names()
    z, stride = traj['z'], int(traj['z']['stride'])
    flat = torch.cat([traj['theta'][k].reshape(-1)[::stride] for k in FULL])
    d = float((tn(z['ref_theta_samples']).double() - flat).abs().max())
    el = max(abs(a - float(b)) / a for a, b in zip(traj['losses'], z['ref_losses']))
    print('trajectory: sampled reference theta vs fp64 %.3e (y_traj %.3e); losses %.2e' % (d, float(z['y_traj']), el))
    assert d <= 1.01 * float(z['y_traj']) and el <= 1e-5


def test_new_symbols_declared_typed_and_exported():
    lib = check_new_symbols(NEW_SYMBOLS)
    # the limits, on the host: T <= 128, 2 <= past_len <= 16, T >= past_len + 2
    ok = lib.interdiff_mdm_train_full_workspace_bytes
    assert ok(3, 12, 5) > lib.interdiff_mdm_train_workspace_bytes(3, 12, 5) > 0 and ok(1, 4, 2) > 0 and ok(2, 128, 16) > 0
    assert ok(3, 129, 10) == 0 and ok(3, 12, 1) == 0 and ok(3, 30, 17) == 0 and ok(3, 11, 10) == 0 and ok(0, 12, 5) == 0


def test_full_param_table():
    from interdiff_amd.mdm_train import param_table
    DEC, ENC, FULL = names()
    sd = fx.mdm_weights()
    assert len(ENC) == len(set(ENC)) == 84 and len(FULL) == len(set(FULL)) == 228 and FULL[:144] == DEC
    carried = ('finalLinear.', 'bodyFutureEmbedding.', 'objFutureEmbedding.', 'PositionalEmbedding.', 'pcEmbedding.')
    assert sorted(FULL) == sorted(k for k in sd if not k.startswith(carried))
    assert sorted(ENC) == sorted(k for k in sd if k.startswith('encoder.'))
    off, size, n = param_table(full=True)
    off0, size0, n0 = param_table()
    assert n0 == N_PARAM_DEC and len(off0) == 144 and off[:144] == off0 and size[:144] == size0
    assert n == N_PARAM == sum(sd[k].numel() for k in FULL)
    at = 0
    for k, o, s in zip(FULL, off, size):                                   # in order, back to back: no overlap, no gap
        assert o == at and s == sd[k].numel(), k
        at += s
    assert at == n and off[144] == n0
    assert sum(size[144:156]) == sum(size[216:228]) == 789760 and sum(size[156:166]) == 529162


def test_constructor_refuses_dropout_masking_and_a_missing_encoder_tensor():
    from interdiff_amd.mdm_train import DenoiserTrainer
    for kw in (dict(dropout=0.1), dict(cond_mask_prob=0.1)):
        with pytest.raises(ValueError):
            DenoiserTrainer(fx.mdm_weights_wc(), device='cpu', train_encoder=True, **kw)
    sd = {k: v for k, v in fx.mdm_weights_wc().items() if k != 'encoder.layers.3.wk'}
    with pytest.raises(KeyError):
        DenoiserTrainer(sd, device='cpu', train_encoder=True)
    assert DenoiserTrainer(sd, device='cpu').n_param == N_PARAM_DEC        # the default mode does not ask for it


def test_cond_batch_is_refused_in_encoder_mode():
    from interdiff_amd.mdm_train import DenoiserTrainer
    tr = DenoiserTrainer(fx.mdm_weights_wc(), device='cpu', train_encoder=True)
    assert tr.cond is None                                                 # before the first gradient call
    assert tr.n_param == N_PARAM and tr.params.numel() == tr.exp_avg.numel() == tr.exp_avg_sq.numel() == tr.grads.numel() == N_PARAM
    with pytest.raises(ValueError):
        tr.loss_and_grads(dict(gt=torch.zeros(2, 1, 144, 12), cond=torch.zeros(10, 2, 256)), t=torch.zeros(2, dtype=torch.int64))


# ------------------------------------------------------------------------------------------------------------ GPU

def new_trainer(past, **kw):
    from interdiff_amd.mdm_train import DenoiserTrainer
    return DenoiserTrainer(weights(), device=DEV, train_encoder=True, past_len=past, **kw)


@pytest.fixture(scope='module')
def trainers(lib):
    return {}                                                              # past_len -> a trainer that is never stepped


def trainer_for(trainers, past):
    if past not in trainers:
        trainers[past] = new_trainer(past)
    return trainers[past]


def on_dev(p):
    return {k: p[k].to(DEV) for k in ('x0', 'pc', 't', 'eps', 'x_t')}


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['E1', 'E2'])
def test_gradients_vs_fp64(trainers, name):
    _, _, FULL = names()
    p, d = point(name), on_dev(point(name))
    tr, ref = trainer_for(trainers, p['past']), p['ref']
    loss, ld, wd, grads, d_cond, d_pc = tr.loss_and_grads(dict(gt=d['x0'], pc=d['pc']), t=d['t'], noise=d['eps'])
    worst, worst_frac, worst_wk, bad = 0.0, 0.0, 0.0, []
    for k in FULL:
        top = float(ref['grads'][k].abs().max())
        dist, g = float((grads[k].cpu().double() - ref['grads'][k]).abs().max()), meo().grad_gate_abs(ref, k, p['e_ref'][k])
        if k.endswith('.wk'):
            worst_wk = max(worst_wk, dist / top)
        else:
            worst = max(worst, dist / top)
        worst_frac = max(worst_frac, dist / g)
        if dist > g:
            bad.append('%s %.3e > %.3e (of max|g64|: %.3e)' % (k, dist, g, dist / top))
    ec, gc = rel(d_cond, ref['d_cond']), gate(p['e_ref']['d_cond'])
    ep, gp = rel(d_pc, ref['d_pc']), gate(p['e_ref']['d_pc'])
    print('point %s: 228 gradient tensors: worst rel err %.3e (the 12 wk tensors, on max|g64|: %.3e), worst fraction of its gate %.3f; d_cond %.3e (gate %.1e), d_pc %.3e (gate %.1e)'
          % (name, worst, worst_wk, max(worst_frac, ec / gc, ep / gp), ec, gc, ep, gp))
    assert not bad, bad
    assert ec <= gc and ep <= gp
    el = abs(float(loss.double().mean()) - float(ref['loss'])) / float(ref['loss'])
    terms = torch.stack([ld[k] for k in lo.LOSS_KEYS])
    # the 16 terms, each on its own size, within max(4 e_ref_term, 1e-5) (module docstring); the weighted ones the same way
    w = torch.tensor(lo.weight_vector(), dtype=torch.float64)
    g_term = [gate(e) for e in p['z']['e_ref_terms']]
    e_term = [rel(terms[i], ref['terms'][i]) for i in range(16)]
    e_wt = [rel(wd[k], ref['terms'][i] * w[i]) for i, k in enumerate(lo.LOSS_KEYS)]
    frac = max(max(a, b) / g for a, b, g in zip(e_term, e_wt, g_term))
    econd = rel(tr.cond, ref['cond'])
    print('point %s: loss %.3e (gate 1e-5); 16 terms, each on its own size: worst %.3e (%s; the reference\'s own fp32 worst: %.3e), worst fraction of max(4 e_ref, 1e-5) %.3f; '
          'cond vs the fp64 encoder %.3e (gate 1e-4)' % (name, el, max(e_term), lo.LOSS_KEYS[int(np.argmax(e_term))], float(p['z']['e_ref_terms'].max()), frac, econd))
    assert el <= 1e-5
    assert all(a <= g and b <= g for a, b, g in zip(e_term, e_wt, g_term)), [(k, a, g) for k, a, g in zip(lo.LOSS_KEYS, e_term, g_term) if a > g]
    assert econd <= 1e-4
    assert tuple(tr.cond.shape) == (p['past'], d['x0'].shape[0], 256) and d_pc.shape == d['pc'].shape


@pytest.mark.gpu
def test_composition_with_the_decoder_only_entry(trainers):
    """At E1: the full call IS the encoder around the decoder-only entry -- fed the cond the full call returned, that entry gives the same bits wherever the
    encoder path adds nothing, and other bits on the shared embeddings."""
    from interdiff_amd.mdm_train import DenoiserTrainer
    DEC, _, _ = names()
    p, d = point('E1'), on_dev(point('E1'))
    tr = trainer_for(trainers, p['past'])
    pred, terms, d_cond, d_pc = tr.grads_at(d['x_t'], d['t'], d['pc'], d['x0'])
    full = {k: v.clone() for k, v in tr.named_views(tr.grads).items()}
    dec = DenoiserTrainer(weights(), device=DEV, past_len=p['past'])
    pred2, terms2, d_cond2 = dec.grads_at(d['x_t'], d['t'], tr.cond, d['x0'])
    assert torch.equal(pred, pred2) and torch.equal(terms, terms2) and torch.equal(d_cond, d_cond2)
    part = dec.named_views(dec.grads)
    for k in DEC:
        if k in SHARED:
            assert not torch.equal(full[k], part[k]), k
        else:
            assert torch.equal(full[k], part[k]), k


@pytest.mark.gpu
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_shapes_vs_fp64(trainers, shape):
    """The full entry at (B, T, past_len) where the encoder's glue (gather_past, swap_rows, add_into) and the shared stack on past_len tokens can go wrong (SHAPES),
    against the fp64 oracle on a synthetic point: pred, cond, terms, d_cond and d_pc at 1e-4, the 228 tensors under ``shape_gate`` (1e-4 of max|g64| or four times the
    fp32 oracle's own distance; ``test_fp32_oracle_cap_at_shapes`` caps the latter).  At (2, 12, 2) the decoder-only entry fed ``tr.cond`` must reproduce the bits of the
    full entry's decoder path (the property of ``test_composition_with_the_decoder_only_entry``, at a memory of two rows).
    Measured on MI355X: worst tensor 0.514 of its gate (``encoder.layers.6.queries`` at (2, 12, 2): 4.5e-4 of max|g64| under a gate of 8.8e-4, the one tensor whose
    gate is wider than the flat 1e-4; 0.149 at (2, 4, 2), at most 0.112 elsewhere); pred 1.2e-7, cond 5.5e-7, terms 1.1e-7, d_cond 6.9e-7, d_pc 5.0e-7.  The wk gate at
    past_len 2 is 0.36 and 1.1 of max|g64| (the fp32 oracle is 0.09 away there, the kernel 0.03 and 0.07): it holds them on ``wk_scale`` alone."""
    from interdiff_amd.mdm_train import DenoiserTrainer
    DEC, _, FULL = names()
    B, T, past = shape
    s = shape_point(shape)
    ref, tag = s['ref'], 'B=%d T=%d past_len=%d' % shape
    d = on_dev(s)
    tr = trainer_for(trainers, past)
    pred, terms, d_cond, d_pc = tr.grads_at(d['x_t'], d['t'], d['pc'], d['x0'])
    e = {k: rel(v, ref[k]) for k, v in (('pred', pred), ('cond', tr.cond), ('d_cond', d_cond), ('d_pc', d_pc))}
    e['terms'] = rel(terms, ref['terms'])
    gate_abs, widest_wk, widest = shape_gate(ref, s['r32'], meo().WK_NAMES)
    print('%s: pred %.3e, cond %.3e, terms %.3e, d_cond %.3e, d_pc %.3e (1e-4); widest wk gate %.3e, widest other gate %.3e of max|g64|' % (
        tag, e['pred'], e['cond'], e['terms'], e['d_cond'], e['d_pc'], widest_wk, widest))
    compare_all(tr.named_views(tr.grads), ref, FULL, gate_abs, tag)
    assert max(e.values()) <= 1e-4
    assert tuple(tr.cond.shape) == tuple(d_cond.shape) == (past, B, 256) and d_pc.shape == d['pc'].shape and pred.shape == d['x0'].shape
    if shape == (2, 12, 2):
        full = {k: v.clone() for k, v in tr.named_views(tr.grads).items()}
        dec = DenoiserTrainer(weights(), device=DEV, past_len=past)
        pred2, terms2, d_cond2 = dec.grads_at(d['x_t'], d['t'], tr.cond, d['x0'])
        assert torch.equal(pred, pred2) and torch.equal(terms, terms2) and torch.equal(d_cond, d_cond2)
        part = dec.named_views(dec.grads)
        for k in DEC:
            if k in SHARED:
                assert not torch.equal(full[k], part[k]), k
            else:
                assert torch.equal(full[k], part[k]), k


@pytest.mark.gpu
def test_limits_raise(lib, trainers):
    """Refused shapes are refused -- ValueError from the wrapper or the RuntimeError of ``_lib.check``, whichever the code raises -- and touch nothing: the flat gradient
    and ``tr.cond`` keep their bits.  The raw entry refuses a workspace that is too small (IDF_E_NOMEM) or misaligned (IDF_E_INVAL) and writes no output; the sizing
    entry returns 0 past the limits."""
    from interdiff_amd import _lib
    tr = trainer_for(trainers, 10)
    s = on_dev(synthetic_point(9399, 2, 12, 10))
    pred, terms, d_cond, d_pc = tr.grads_at(s['x_t'], s['t'], s['pc'], s['x0'])
    before, cond = tr.grads.clone(), tr.cond.clone()
    assert bool(before.ne(0).any())
    zeros = lambda *shape: torch.zeros(*shape, device=DEV)
    t1 = torch.zeros(1, dtype=torch.int64, device=DEV)
    refused = [
        ('T = 129', lambda: tr.grads_at(zeros(1, 1, 144, 129), t1, zeros(1, 256), zeros(1, 1, 144, 129))),
        ('T = past_len + 1', lambda: tr.grads_at(zeros(1, 1, 144, 11), t1, zeros(1, 256), zeros(1, 1, 144, 11))),
        ('pc of another B', lambda: tr.grads_at(s['x_t'], s['t'], zeros(3, 256), s['x0'])),
        ('pc of another width', lambda: tr.grads_at(s['x_t'], s['t'], zeros(2, 255), s['x0'])),
        ('pc with a memory axis', lambda: tr.grads_at(s['x_t'], s['t'], zeros(10, 2, 256), s['x0'])),
        ('d_pred of another shape', lambda: tr.grads_at(s['x_t'], s['t'], s['pc'], s['x0'], d_pred=zeros(2, 1, 144, 11))),
        ('target of another shape', lambda: tr.grads_at(s['x_t'], s['t'], s['pc'], zeros(2, 1, 144, 11))),
        ('cond and pc', lambda: tr.grads_at(s['x_t'], s['t'], zeros(10, 2, 256), s['x0'], pc=s['pc'])),
    ]
    for what, call in refused:
        with pytest.raises((ValueError, RuntimeError)):
            call()
        torch.cuda.synchronize()
        assert torch.equal(tr.grads, before) and torch.equal(tr.cond, cond), what
    for past in (1, 17):                                                   # a trainer built for a memory the stack does not take refuses every call
        bad = new_trainer(past)
        with pytest.raises((ValueError, RuntimeError)):
            bad.grads_at(zeros(2, 1, 144, 24), s['t'], s['pc'], zeros(2, 1, 144, 24))
        assert not bool(bad.grads.ne(0).any()) and bad.cond is None
    # the raw entry and its workspace
    B, T, S = 2, 12, 10
    need = lib.interdiff_mdm_train_full_workspace_bytes(B, T, S)
    assert need > lib.interdiff_mdm_train_workspace_bytes(B, T, S) > 0
    ws = torch.empty(need + 256, dtype=torch.uint8, device=DEV)
    sentinel = -7.0
    outs = [torch.full(shape, sentinel, device=DEV) for shape in ((S, B, 256), (S, B, 256), (B, 256), (B, 1, 144, T), (16, B))]
    def raw(ws_ptr, ws_bytes, T_=T, past=S):
        return lib.interdiff_mdm_train_full_grads(_lib.dptr(tr.params), _lib.dptr(tr.pe), tr.pe.shape[0], _lib.dptr(s['x_t']), _lib.dptr(s['t']), _lib.dptr(s['pc']),
                                                  _lib.dptr(s['x0']), B, T_, past, tr._wvec, _lib.vp(None), _lib.dptr(tr.grads), *[_lib.dptr(o) for o in outs],
                                                  ws_ptr, ws_bytes, _lib.stream())
    base = ws.data_ptr()
    assert base % 256 == 0
    assert raw(_lib.vp(base), need - 1) == -12                             # one byte short: IDF_E_NOMEM
    assert raw(_lib.vp(base), lib.interdiff_mdm_train_workspace_bytes(B, T, S)) == -12             # the decoder-only entry's size
    assert raw(_lib.vp(base + 4), need) == -22                             # not 256-byte aligned: IDF_E_INVAL
    assert raw(_lib.vp(None), need) == -22
    assert raw(_lib.vp(base), need, past=11) == -22 and raw(_lib.vp(base), need, T_=129) == -22 and raw(_lib.vp(base), need, past=1) == -22
    with pytest.raises(RuntimeError):
        _lib.check(raw(_lib.vp(base), need - 1))
    torch.cuda.synchronize()
    assert torch.equal(tr.grads, before) and all(bool((o == sentinel).all()) for o in outs)
    assert raw(_lib.vp(base), need) == 0                                   # the same call with its workspace runs, and gives the wrapper's bits
    torch.cuda.synchronize()
    assert torch.equal(tr.grads, before)
    assert all(torch.equal(o, w) for o, w in zip(outs, (cond, d_cond, d_pc, pred, terms)))
    size = lib.interdiff_mdm_train_full_workspace_bytes
    assert size(1, 11, 10) == 0 and size(1, 3, 2) == 0 and size(1, 129, 10) == 0 and size(1, 19, 17) == 0
    assert size(1, 12, 10) > 0 and size(1, 4, 2) > 0


@pytest.mark.gpu
def test_determinism_and_seams(trainers):
    p, d = point('E2'), on_dev(point('E2'))
    tr = trainer_for(trainers, p['past'])
    a = tr.grads_at(d['x_t'], d['t'], d['pc'], d['x0'])
    ga, ca = tr.grads.clone(), tr.cond.clone()
    b = tr.grads_at(d['x_t'], d['t'], pc=d['pc'], target=d['x0'])         # (the keyword form)
    assert torch.equal(ga, tr.grads) and torch.equal(ca, tr.cond) and all(torch.equal(x, y) for x, y in zip(a, b))   # pred, terms, d_cond, d_pc
    dp = tr.loss_grad(a[0], d['x0'])
    c = tr.grads_at(d['x_t'], d['t'], d['pc'], d['x0'], d_pred=dp)
    assert torch.equal(ga, tr.grads) and torch.equal(a[2], c[2]) and torch.equal(a[3], c[3])      # the default path is the loss-gradient entry fed to the seam
    c2 = tr.grads_at(d['x_t'], d['t'], d['pc'], d['x0'], d_pred=2 * dp)
    assert torch.equal(2 * ga, tr.grads) and torch.equal(2 * a[2], c2[2]) and torch.equal(2 * a[3], c2[3])          # linear in d_pred, bit for bit
    assert torch.equal(a[0], c2[0]) and torch.equal(a[1], c2[1]) and torch.equal(ca, tr.cond)
    c0 = tr.grads_at(d['x_t'], d['t'], d['pc'], d['x0'], d_pred=torch.zeros_like(dp))
    assert not bool(tr.grads.ne(0).any()) and not bool(c0[3].ne(0).any()) and not bool(c0[2].ne(0).any())
    assert bool(ga.ne(0).any())


@pytest.mark.gpu
def test_trajectory_vs_fp64(lib, traj):
    _, _, FULL = names()
    p, d, z = point('E2'), on_dev(point('E2')), traj['z']
    sd = weights()
    tr = new_trainer(p['past'], lr=float(z['lr']))
    batch = dict(gt=d['x0'], pc=d['pc'])
    for k, (t, eps) in enumerate(zip(traj['ts'], traj['noises'])):
        loss = tr.training_step(batch, t=t.to(DEV), noise=eps.to(DEV))[0]
        e = abs(float(loss.double().mean()) - traj['losses'][k]) / traj['losses'][k]
        print('step %d: loss %.6f, rel err vs fp64 %.2e (gate 1e-5)' % (k + 1, float(loss.mean()), e))
        assert e <= 1e-5
    got = tr.state_dict()
    y = float(z['y_traj'])
    far, worst = far_parameters(got, traj['theta'], FULL, y)
    moved = max(float((got[k].cpu() - sd[k]).abs().max()) for k in FULL if k.startswith('encoder.'))
    print('trajectory: %d of %d parameters further than 8 y_traj = %.3e from fp64 (cap %d); max distance %.3e; largest encoder move %.3e'
          % (far, N_PARAM, 8 * y, N_PARAM // 1000, worst, moved))
    assert far <= N_PARAM // 1000
    assert moved > 100 * y                                                 # the encoder trains
    assert set(got) == set(sd)
    for k in sd:
        if k not in FULL:
            assert torch.equal(got[k], sd[k]), k                           # pcEmbedding.* and every other pass-through tensor: identical bits


@pytest.mark.gpu
def test_plumbing(lib, traj):
    from interdiff_amd import synthetic as syn
    from interdiff_amd.mdm_train import DenoiserTrainer
    p, d = point('E2'), on_dev(point('E2'))
    batch = dict(gt=d['x0'], pc=d['pc'])
    step = lambda tr, k: tr.training_step(batch, t=traj['ts'][k].to(DEV), noise=traj['noises'][k].to(DEV))
    a = new_trainer(p['past'])
    step(a, 0), step(a, 1)
    # state + optimizer state continue the trajectory bit for bit
    b = DenoiserTrainer(a.state_dict(), device=DEV, train_encoder=True, past_len=p['past'])
    b.load_optimizer_state(a.optimizer_state())
    assert b.step == 2 and torch.equal(a.params, b.params) and b.params.numel() == N_PARAM
    step(a, 2), step(b, 2)
    assert torch.equal(a.params, b.params) and torch.equal(a.exp_avg, b.exp_avg) and torch.equal(a.exp_avg_sq, b.exp_avg_sq)
    assert not torch.equal(a.params, new_trainer(p['past']).params)
    # a raw clip (EMB_SHAPE-style fields, B = 3, P = 2048): three steps on it, then the exported sampler model's own _get_embeddings against the trainer's cond
    T, B, past = 12, 3, 10
    raw = {k: tn(v).to(DEV) for k, v in syn.make_embedding_inputs(seed=78, B=B, T=T, n_points=2048).items()}
    fields = (raw['body_pose'], raw['body_trans'], raw['obj_angles'], raw['obj_trans'], raw['obj_points'])
    c = new_trainer(past)
    _, gt = c.export_mdm()._get_embeddings(*fields, past_len=past)
    clip = dict(gt=gt.permute(1, 2, 0).unsqueeze(1).contiguous(), obj_points=raw['obj_points'])
    g = torch.Generator(device='cpu').manual_seed(11)
    ts = [torch.randint(0, 1000, (B,), generator=g) for _ in range(4)]
    for k in range(3):
        c.training_step(clip, t=ts[k], seed=100 + k)
    c.loss_and_grads(clip, t=ts[3], seed=103)                               # self.cond of the CURRENT weights
    cond, _ = c.export_mdm()._get_embeddings(*fields, past_len=past)
    e, e0 = rel(cond, c.cond), rel(new_trainer(past).export_mdm()._get_embeddings(*fields, past_len=past)[0], c.cond)
    print('export_mdm()._get_embeddings vs the trainer\'s cond after 3 steps: %.3e (gate 1e-4); the untrained encoder\'s is %.3e away' % (e, e0))
    assert e <= 1e-4 < e0
    # raw obj_points give the bits of the pc that interdiff_pointnet2_encode returns
    r1 = c.loss_and_grads(clip, t=ts[3], seed=103)
    g1, c1 = c.grads.clone(), c.cond.clone()
    r2 = c.loss_and_grads(dict(gt=clip['gt'], pc=c.encode_points(raw['obj_points'])), t=ts[3], seed=103)
    assert torch.equal(g1, c.grads) and torch.equal(c1, c.cond) and torch.equal(r1[0], r2[0]) and torch.equal(r1[-1], r2[-1]) and torch.equal(r1[-2], r2[-2])
