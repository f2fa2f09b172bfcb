"""The skeleton denoiser's trainer (``interdiff_amd.skeleton_mdm_train.SkeletonDenoiserTrainer``, csrc/skeleton_mdm_train.hip on the stacks of csrc/mdm_train.h):
one optimiser step of train_diffusion_skeleton.py -- ``_get_embeddings``, ``q_sample``, ``MDM.forward``, the 13-term loss, the whole backward, AdamW -- against the
fp64 oracle tests/skeleton_mdm_train_oracle.py and the reference's OWN fp32 run recorded by tests/golden/make_golden_skeleton_mdm_train.py
(tests/golden/skel_mdm_train_{S1,S2,traj}.npz).

Gradient gate (the project's): per tensor max|g - g64| <= max(4 e_ref, 1e-5) of the tensor's scale, e_ref = the same measure of the reference's fp32 gradient, recorded
per tensor (230 tensors); the recorder asserts 4 e_ref <= 1e-4 for every one and that a second fp32 run lies within every gate.  The scale is max|g64|, except for the
twelve ten-entry ``wk`` tensors, measured on the sum of the magnitudes of the products they add up (the rule and the reason of tests/test_mdm_encoder_train.py; the
reference's own fp32 run is 5e-7 .. 7e-5 of max|g64| on them and <= 1.1e-7 on that scale); their gate keeps the 1e-5 floor on max|g64|.  Loss 1e-5 relative to fp64;
each of the 13 terms (mean over the clips, as the reference logs them) on its own size within max(4 e_ref_term, 1e-5).  pred / cond 1e-4 against ``SkeletonMDM``.
The synthetic shapes and the head-alone cases have no recorded e_ref: a flat 1e-4 of max|g64| on every tensor; the wk tensors, where fp32 cannot reach that, at four
times the fp32 oracle's rounding noise on the same point (``flat_gate``), which an all-zero or wrong-sign gradient fails.  Trajectory: 6 AdamW steps, losses 1e-5, at most 0.1 % of the 5,499,582 parameters
further than 8 y_traj from the fp64 trajectory.  Bit-identity claims are ``torch.equal``.  Every figure is printed before it is asserted.

Points: S1  B = 3, T = 20, t = [37, 412, 875] (the scene of skel_losses.npz);  S2  B = 3, T = 70, t = [5, 500, 990] (more than one 64-key tile, an odd batch).
Measured on MI355X: DESIGN.md 8.17.  Without the feature every test below fails: the module, the names and the entries do not exist.
"""
import numpy as np
import pytest
import torch
from tests import fixtures as fx
from tests import losses_oracle as lo
from tests import skeleton_losses_oracle as slo
from tests.denoiser_train_helpers import betas, check_new_symbols, far_parameters, flat_gate, gate, rel, tn

DEV = 'cuda'
N_PARAM, SEED, PAST = 5499582, 1106, 10                                   # SEED: make_golden_skeleton_mdm.SEED, the weights every skeleton-denoiser fixture uses
NEW_SYMBOLS = {
    'interdiff_skeleton_denoising_loss_grad': 'const float *pred, const float *target, int32_t B, int32_t T, int32_t past_len, const float *weights13, float *d_pred, '
                                              'void *stream',
    'interdiff_skeleton_mdm_train_param_table': 'int64_t *offsets, int64_t *sizes, int32_t *n_tensors, int64_t *n_param',
    'interdiff_skeleton_mdm_train_workspace_bytes': 'int32_t B, int32_t T, int32_t past_len',
    'interdiff_skeleton_mdm_train_grads': 'const float *params, const float *pe, int32_t pe_rows, const float *x_t, const int64_t *ts, const float *target, '
                                          'const float *zero_pose_obj, int32_t B, int32_t T, int32_t past_len, const float *weights13, const float *d_pred_in, '
                                          'float *grads, float *cond, float *pred, float *terms, void *ws, size_t ws_bytes, void *stream',
}


def so():
    from tests import skeleton_mdm_train_oracle
    return skeleton_mdm_train_oracle


def raw_weights():
    from interdiff_amd import synthetic as syn
    return {k: torch.from_numpy(v) for k, v in syn.skeleton_mdm_state_dict(SEED).items()}


def weights():
    """The synthetic skeleton denoiser with the positional-table rows the reference runs read (all three recordings; they agree where they overlap)."""
    files = [fx.golden('skel_mdm_train_%s.npz' % n) for n in ('S1', 'S2', 'traj')]
    return so().with_pe_rows(raw_weights(), *[(z['pe_idx'], z['pe_val']) for z in files])


_POINTS = {}


def point(name):
    """The recorded inputs of a point and the fp64 oracle on them, computed once per process and never modified."""
    if name not in _POINTS:
        z = fx.golden('skel_mdm_train_%s.npz' % name)
        z = {k: z[k] for k in z.files}
        batch = tuple(tn(z['batch_' + k]) for k in ('body', 'obj', 'pose', 'zero_pose_obj'))
        x0, zpo, t, eps = so().tokens(*batch[:3]), batch[3], tn(z['t']), tn(z['eps'])
        x_t = lo.q_sample(betas(), x0, t, eps)
        ref = so().grads(weights(), x_t, t, zpo, x0, int(z['past_len']))
        e_ref = dict(zip([str(k) for k in z['names']], z['e_ref']))
        assert [str(k) for k in z['wk_names']] == list(so().WK_NAMES)
        _POINTS[name] = dict(z=z, batch=batch, x0=x0, zpo=zpo, t=t, eps=eps, x_t=x_t, ref=ref, e_ref=e_ref)
    return _POINTS[name]


def synthetic_point(seed, B, T, past=PAST):
    """A synthetic batch (no golden) with seeded t / eps and the fp64 oracle on it."""
    from interdiff_amd import synthetic as syn
    bt = {k: tn(v) for k, v in syn.make_skeleton_batch(seed, B=B, T=T).items()}
    rs = np.random.RandomState(seed + 1)
    x0, zpo = so().tokens(bt['body'], bt['obj'], bt['pose']), bt['zero_pose_obj']
    t, eps = tn(rs.randint(0, 1000, size=B).astype(np.int64)), fx._randn(rs, B, 1, 106, T)
    x_t = lo.q_sample(betas(), x0, t, eps)
    return dict(x0=x0, zpo=zpo, t=t, eps=eps, x_t=x_t, ref=so().grads(weights(), x_t, t, zpo, x0, past))


@pytest.fixture(scope='module')
def traj():
    """The recorded per-step t / noise and the fp64 oracle's trajectory on them (S1's scene), computed once."""
    z = fx.golden('skel_mdm_train_traj.npz')
    z = {k: z[k] for k in z.files}
    p = point('S1')
    ts, noises = [tn(t) for t in z['t']], [tn(e) for e in z['noise']]
    losses, theta = so().trajectory(weights(), betas(), p['x0'], p['zpo'], ts, noises, PAST, lr=float(z['lr']))
    return dict(z=z, ts=ts, noises=noises, losses=losses, theta=theta)


# ------------------------------------------------------------------------------------------------------------ CPU

@pytest.mark.parametrize('name', ['S1', 'S2'])
def test_oracle_vs_reference_samples(name):
    """The fp64 oracle (the conditioning in the graph) against every 64th entry of the reference's own fp32 gradients, within the recorded e_ref, its fp32 loss and
    its 13 weighted terms."""
    NAMES = so().PARAM_NAMES
    p = point(name)
    z, ref, stride = p['z'], p['ref'], int(p['z']['stride'])
    assert [str(k) for k in z['names']] == list(NAMES) + ['d_pred']
    at, worst = 0, 0.0
    for k in NAMES:
        g = ref['grads'][k].reshape(-1)[::stride]
        s = tn(z['ref_grad_samples'][at:at + g.numel()]).double()
        at += g.numel()
        e = float((s - g).abs().max()) / so().grad_scale(ref, k)
        worst = max(worst, e / p['e_ref'][k])
        assert e <= 1.01 * p['e_ref'][k], k
        assert float(ref['grads'][k].abs().max()) > 0, k
    assert at == len(z['ref_grad_samples'])
    g = ref['d_pred'].reshape(-1)
    assert float((tn(z['ref_d_pred_samples']).double() - g[::stride]).abs().max() / g.abs().max()) <= 1.01 * p['e_ref']['d_pred']
    scales = rel(tn(z['wk_scale']), torch.tensor([ref['wk_scale'][k] for k in so().WK_NAMES], dtype=torch.float64))
    el = abs(float(ref['loss']) - float(z['ref_loss'])) / float(ref['loss'])
    t64 = ref['terms'].mean(dim=1) * so().weight_vector()
    et = [abs(float(z['ref_weighted'][i]) - float(t64[i])) / float(t64[i]) for i in range(13)]
    qq = float((ref['pred'][:, 0, -4:] ** 2).sum(1).min())
    print('point %s: sampled reference vs oracle: worst e / e_ref %.3f; worst e_ref %.2e; wk_scale recorded vs recomputed %.1e; loss %.2e; 13 terms worst %.2e; '
          'min q.q %.3f; smallest term %.2e' % (name, worst, max(p['e_ref'].values()), scales, el, max(et), qq, float(ref['terms'].min())))
    assert 4 * max(p['e_ref'].values()) <= 1e-4 and 4 * float(z['e_ref_terms'].max()) <= 1e-4
    assert scales <= 1e-9 and el <= 1e-5 and max(et) <= 1e-5
    assert qq >= 0.25 and float(ref['terms'].min()) >= 1e-6
    # the 13 terms are the scoring oracle's (numpy, shares no code with this one)
    assert rel(ref['terms'], slo.per_clip_terms(ref['pred'].numpy(), p['x0'].numpy(), PAST)) <= 1e-12


def test_oracle_trajectory_vs_reference_samples(traj):
    z, stride = traj['z'], int(traj['z']['stride'])
    flat = torch.cat([traj['theta'][k].reshape(-1)[::stride] for k in so().PARAM_NAMES])
    d = float((tn(z['ref_theta_samples']).double() - flat).abs().max())
    el = max(abs(a - float(b)) / a for a, b in zip(traj['losses'], z['ref_losses']))
    print('trajectory: sampled reference theta vs fp64 %.3e (y_traj %.3e); losses %.2e' % (d, float(z['y_traj']), el))
    assert d <= 1.01 * float(z['y_traj']) and el <= 1e-5


def test_closed_form_d_pred_vs_autograd():
    p = point('S1')
    e = rel(so().d_pred_closed_form(p['ref']['pred'], p['x0'].double(), PAST), p['ref']['d_pred'])
    print('closed-form d_pred vs autograd (fp64) at S1: %.2e' % e)
    assert e <= 1e-12
    # other weights, another past length and the smallest legal shape take the same form
    wts = dict(weight_past=0.3, weight_body=0.7, weight_obj=1.3, weight_obj_rot=0.4, weight_obj_nonrot=2.0, weight_quat_reg=0.5, weight_v=3.0)
    for seed, B, T, past in ((5, 2, 17, 4), (6, 1, 12, 10)):
        pred, gt = (tn(a).double() for a in slo.near_unit_case(seed, B, T, noise=0.3))
        with torch.enable_grad():
            pr = pred.clone().requires_grad_(True)
            auto = torch.autograd.grad(so().loss_of(pr, gt, past, wts)[0], pr)[0]
        assert rel(so().d_pred_closed_form(pred, gt, past, wts), auto) <= 1e-12


def test_closed_form_head_backward_vs_autograd():
    g = torch.Generator().manual_seed(9)
    T, B = 5, 2
    rows = torch.randn(T, B, 70, generator=g, dtype=torch.float64)
    q = rows[0, 0, 66:70]
    rows[0, 0, 66:70] = q * (0.5 / q.norm())                              # q . q = 0.25: the derivative carries two_s = 8
    zpo = 0.3 * torch.randn(B, 12, 3, generator=g, dtype=torch.float64)
    d_pred = torch.randn(B, 1, 106, T, generator=g, dtype=torch.float64)
    with torch.enable_grad():
        r = rows.clone().requires_grad_(True)
        auto = torch.autograd.grad(so().head(r, zpo), r, grad_outputs=d_pred)[0]
    e = rel(so().head_backward_closed_form(d_pred, rows, zpo), auto)
    print('closed-form head backward vs autograd (fp64): %.2e' % e)
    assert e <= 1e-12


def test_param_names_and_table():
    from interdiff_amd.skeleton_mdm_train import PARAM_NAMES, SkeletonDenoiserTrainer, param_table
    sd = raw_weights()
    assert len(PARAM_NAMES) == len(set(PARAM_NAMES)) == 230 and SkeletonDenoiserTrainer.PARAM_NAMES == PARAM_NAMES
    # the reference module's trainable names: every state_dict entry but the positional buffers (the recorder asserts the same against named_parameters())
    assert sorted(PARAM_NAMES) == sorted(k for k in sd if not k.startswith(('PositionalEmbedding.', 'embedTimeStep.sequence_pos_encoder.')))
    off, size, n = param_table()
    assert n == N_PARAM == sum(sd[k].numel() for k in PARAM_NAMES)
    at = 0
    for k, o, s in zip(PARAM_NAMES, off, size):                            # in order, back to back: no overlap, no gap
        assert o == at and s == sd[k].numel(), k
        at += s
    assert at == n


def test_new_symbols_declared_typed_and_exported():
    lib = check_new_symbols(NEW_SYMBOLS)
    ok = lib.interdiff_skeleton_mdm_train_workspace_bytes
    assert ok(3, 20, 10) > 0 and ok(1, 12, 10) > 0 and ok(1, 128, 10) > 0 and ok(1, 4, 2) > 0
    assert ok(1, 129, 10) == 0 and ok(3, 12, 1) == 0 and ok(3, 30, 17) == 0 and ok(3, 11, 10) == 0 and ok(0, 12, 5) == 0


def test_constructor_refuses_dropout_masking_and_a_missing_tensor():
    from interdiff_amd.skeleton_mdm_train import SkeletonDenoiserTrainer
    for kw in (dict(dropout=0.1), dict(cond_mask_prob=0.1)):
        with pytest.raises(ValueError):
            SkeletonDenoiserTrainer(raw_weights(), device='cpu', **kw)
    with pytest.raises(KeyError):
        SkeletonDenoiserTrainer({k: v for k, v in raw_weights().items() if k != 'shapeEmbedding.weight'}, device='cpu')
    tr = SkeletonDenoiserTrainer(raw_weights(), device='cpu')
    assert tr.n_param == N_PARAM and tr.params.numel() == tr.exp_avg.numel() == tr.exp_avg_sq.numel() == tr.grads.numel() == N_PARAM
    assert tr.pred is None and tr.cond is None and tr.param_table()[2] == N_PARAM


# ------------------------------------------------------------------------------------------------------------ GPU

def new_trainer(past=PAST, sd=None, **kw):
    from interdiff_amd.skeleton_mdm_train import SkeletonDenoiserTrainer
    return SkeletonDenoiserTrainer(weights() if sd is None else sd, device=DEV, past_len=past, **kw)


@pytest.fixture(scope='module')
def trainers(lib):
    return {}                                                              # past_len -> a trainer that is never stepped


def trainer_for(trainers, past=PAST):
    if past not in trainers:
        trainers[past] = new_trainer(past)
    return trainers[past]


def on_dev(p):
    return {k: p[k].to(DEV) for k in ('x0', 'zpo', 't', 'eps', 'x_t')}


def compare_all(tr, ref, gate_abs, tag):
    """Every one of the 230 gradient tensors against the fp64 oracle; gate_abs(k) the absolute gate.  Prints before it asserts."""
    grads = tr.named_views(tr.grads)
    worst, worst_wk, worst_frac, bad = 0.0, 0.0, 0.0, []
    for k in so().PARAM_NAMES:
        top = float(ref['grads'][k].abs().max())
        dist, g = float((grads[k].cpu().double() - ref['grads'][k]).abs().max()), gate_abs(k)
        if top == 0.0:                                                     # a tensor the given d_pred does not reach (bodyFinalLinear under an object-only d_pred): exact zeros
            if dist != 0.0:
                bad.append('%s: %.3e where the oracle is exactly zero' % (k, dist))
            continue
        if k.endswith('.wk'):
            worst_wk = max(worst_wk, dist / top)
        else:
            worst = max(worst, dist / top)
        worst_frac = max(worst_frac, dist / g)
        if dist > g:
            bad.append('%s %.3e > %.3e (of max|g64|: %.3e)' % (k, dist, g, dist / top))
    print('%s: 230 gradient tensors: worst rel err %.3e (the 12 wk tensors, on max|g64|: %.3e), worst fraction of its gate %.3f' % (tag, worst, worst_wk, worst_frac))
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['S1', 'S2', 'smallest'])
def test_loss_grad_vs_closed_form(trainers, name):
    """interdiff_skeleton_denoising_loss_grad against the fp64 closed form: 1e-5 of max|d|.  'smallest': B = 1, T = 12, past_len 10 (T >= past_len + 2)."""
    if name == 'smallest':
        pred, gt = (tn(a) for a in slo.near_unit_case(31, 1, 12, noise=0.2))
    else:
        pred, gt = point(name)['ref']['pred'].float(), point(name)['x0']
    want = so().d_pred_closed_form(pred.double(), gt.double(), PAST)
    got = trainer_for(trainers).loss_grad(pred.to(DEV), gt.to(DEV))
    e = rel(got, want)
    print('loss gradient %s: %.3e of max|d| (gate 1e-5)' % (name, e))
    assert got.shape == pred.shape and e <= 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['S1', 'S2'])
def test_gradients_vs_fp64(trainers, name):
    p, d = point(name), on_dev(point(name))
    tr, ref = trainer_for(trainers), p['ref']
    loss, ld, wd, grads = tr.loss_and_grads(tuple(b.to(DEV) for b in p['batch']), t=d['t'], noise=d['eps'])
    assert list(grads) == list(so().PARAM_NAMES) and list(ld) == list(slo.KEYS)
    compare_all(tr, ref, lambda k: so().grad_gate_abs(ref, k, p['e_ref'][k]), 'point ' + name)
    el = abs(float(loss.double().mean()) - float(ref['loss'])) / float(ref['loss'])
    terms = torch.stack([ld[k] for k in slo.KEYS]).cpu().double().mean(dim=1)
    wterms = torch.stack([wd[k] for k in slo.KEYS]).cpu().double().mean(dim=1)
    t64, w = ref['terms'].mean(dim=1), so().weight_vector()
    g_term = [gate(e) for e in p['z']['e_ref_terms']]
    e_term = [abs(float(terms[i] - t64[i])) / float(t64[i]) for i in range(13)]
    e_wt = [abs(float(wterms[i] - t64[i] * w[i])) / float(t64[i] * w[i]) for i in range(13)]
    mdm = tr.export_mdm()
    e_pred = rel(tr.pred, mdm.forward(d['x_t'], d['t'], d['zpo'], y={'cond': tr.cond}))
    tb = lambda a: a.transpose(0, 1).contiguous().to(DEV)
    e_cond = rel(tr.cond, mdm._get_embeddings(tb(p['batch'][0]), tb(p['batch'][1]), tb(p['batch'][2]), d['zpo'], past_len=PAST)[0])
    print('point %s: loss %.3e (gate 1e-5); 13 terms, each on its own size: worst %.3e (%s), worst fraction of max(4 e_ref, 1e-5) %.3f; pred vs SkeletonMDM.forward '
          '%.3e, cond vs SkeletonMDM._get_embeddings %.3e (gates 1e-4); pred / cond vs the fp64 oracle %.3e / %.3e' % (
              name, el, max(e_term), slo.KEYS[int(np.argmax(e_term))], max(max(a, b) / g for a, b, g in zip(e_term, e_wt, g_term)), e_pred, e_cond,
              rel(tr.pred, ref['pred']), rel(tr.cond, ref['cond'])))
    assert el <= 1e-5
    assert all(a <= g and b <= g for a, b, g in zip(e_term, e_wt, g_term)), [(k, a, g) for k, a, g in zip(slo.KEYS, e_term, g_term) if a > g]
    assert e_pred <= 1e-4 and e_cond <= 1e-4
    assert tuple(tr.cond.shape) == (PAST, d['x0'].shape[0], 256) and tr.pred.shape == d['x0'].shape


@pytest.mark.gpu
@pytest.mark.parametrize('case', ['obj_block', 'pose_block', 'qq_quarter'])
def test_head_alone(trainers, case):
    """An external d_pred through the head backward, against the oracle in fp64 (``flat_gate``: 1e-4 of max|g64| on every tensor, the wk tensors at four times the fp32 noise of the point): d_pred nonzero only in the object-keypoint
    block, only in the pose block, and a model whose every predicted quaternion has q . q = 0.25 (objFinalLinear = its bias alone)."""
    p, d = point('S1'), on_dev(point('S1'))
    g = torch.Generator().manual_seed(17)
    d_pred = torch.zeros(p['x0'].shape)
    sd, tr = weights(), None
    if case == 'obj_block':
        d_pred[:, :, 63:99] = torch.randn(d_pred[:, :, 63:99].shape, generator=g)
    elif case == 'pose_block':
        d_pred[:, :, 99:] = torch.randn(d_pred[:, :, 99:].shape, generator=g)
    else:
        d_pred = torch.randn(d_pred.shape, generator=g)
        sd = dict(sd)
        sd['objFinalLinear.weight'] = torch.zeros_like(sd['objFinalLinear.weight'])
        sd['objFinalLinear.bias'] = torch.tensor([0.1, -0.2, 0.3, 0.25, -0.25, 0.25, 0.25])           # quaternion xyzw: q . q = 0.25
        tr = new_trainer(sd=sd)
    tr = tr or trainer_for(trainers)
    ref = so().grads(sd, p['x_t'], p['t'], p['zpo'], p['x0'], PAST, d_pred=d_pred)
    pred, _ = tr.grads_at(d['x_t'], d['t'], d['zpo'], d['x0'], d_pred=d_pred.to(DEV))
    qq = (pred[:, 0, -4:] ** 2).sum(1)
    if case == 'qq_quarter':
        assert float((qq - 0.25).abs().max()) <= 1e-6
    gate_abs, widest = flat_gate(ref, so().grads(sd, p['x_t'], p['t'], p['zpo'], p['x0'], PAST, dtype=torch.float32, d_pred=d_pred), so().WK_NAMES)
    print('head alone, %s: pred vs fp64 %.3e; q.q in [%.3f, %.3f]; widest wk gate %.3e of max|g64|' % (
        case, rel(pred, ref['pred']), float(qq.min()), float(qq.max()), widest))
    compare_all(tr, ref, gate_abs, 'head alone, ' + case)
    assert rel(pred, ref['pred']) <= 1e-4


@pytest.mark.gpu
@pytest.mark.parametrize('B,T,past', [(1, 12, 10), (2, 33, 10), (1, 128, 10), (2, 12, 2)])
def test_shapes_vs_fp64(trainers, B, T, past):
    """Shapes where the kernels can go wrong (one clip, the shortest clip, an odd length, the T limit, a two-row memory): the fp64 oracle on a synthetic batch,
    ``flat_gate``: 1e-4 of max|g64| on every tensor, the wk tensors at four times the fp32 rounding noise of the same point (never below 1e-4 max|g64|)."""
    p = synthetic_point(9100 + T, B, T, past)
    d, ref = on_dev(p), p['ref']
    tr = trainer_for(trainers, past)
    pred, terms = tr.grads_at(d['x_t'], d['t'], d['zpo'], d['x0'])
    e_pred, e_cond, e_terms = rel(pred, ref['pred']), rel(tr.cond, ref['cond']), rel(terms, ref['terms'])
    gate_abs, widest = flat_gate(ref, so().grads(weights(), p['x_t'], p['t'], p['zpo'], p['x0'], past, dtype=torch.float32), so().WK_NAMES)
    print('B=%d T=%d past_len=%d: pred %.3e, cond %.3e, terms %.3e (1e-4); widest wk gate %.3e of max|g64|' % (B, T, past, e_pred, e_cond, e_terms, widest))
    compare_all(tr, ref, gate_abs, 'B=%d T=%d past_len=%d' % (B, T, past))
    assert e_pred <= 1e-4 and e_cond <= 1e-4 and e_terms <= 1e-4


@pytest.mark.gpu
def test_limits_raise(trainers):
    tr = trainer_for(trainers)
    x = torch.zeros(1, 1, 106, 129, device=DEV)
    with pytest.raises(ValueError):
        tr.grads_at(x, torch.zeros(1, dtype=torch.int64, device=DEV), torch.zeros(1, 12, 3, device=DEV), x)
    x = torch.zeros(1, 1, 106, 11, device=DEV)
    with pytest.raises(ValueError):                                        # T >= past_len + 2
        tr.grads_at(x, torch.zeros(1, dtype=torch.int64, device=DEV), torch.zeros(1, 12, 3, device=DEV), x)
    for kw in (dict(dropout=0.1), dict(cond_mask_prob=0.1)):
        with pytest.raises(ValueError):
            new_trainer(**kw)


@pytest.mark.gpu
def test_determinism_and_seams(trainers):
    p, d = point('S2'), on_dev(point('S2'))
    tr = trainer_for(trainers)
    a = tr.grads_at(d['x_t'], d['t'], d['zpo'], d['x0'])
    ga, ca = tr.grads.clone(), tr.cond.clone()
    b = tr.grads_at(d['x_t'], d['t'], d['zpo'], d['x0'])
    assert torch.equal(ga, tr.grads) and torch.equal(ca, tr.cond) and all(torch.equal(x, y) for x, y in zip(a, b))      # two calls give the same bits
    dp = tr.loss_grad(a[0], d['x0'])
    c = tr.grads_at(d['x_t'], d['t'], d['zpo'], d['x0'], d_pred=dp)
    assert torch.equal(ga, tr.grads) and torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])      # the default path is the loss-gradient entry fed to the seam
    tr.grads_at(d['x_t'], d['t'], d['zpo'], d['x0'], d_pred=2 * dp)
    assert torch.equal(2 * ga, tr.grads) and torch.equal(ca, tr.cond)                              # linear in d_pred, bit for bit
    tr.grads_at(d['x_t'], d['t'], d['zpo'], d['x0'], d_pred=torch.zeros_like(dp))
    assert not bool(tr.grads.ne(0).any()) and bool(ga.ne(0).any())


@pytest.mark.gpu
def test_trajectory_vs_fp64(lib, traj):
    p, z = point('S1'), traj['z']
    sd = weights()
    tr = new_trainer(lr=float(z['lr']))
    batch = tuple(b.to(DEV) for b in p['batch'])
    for k, (t, eps) in enumerate(zip(traj['ts'], traj['noises'])):
        loss = tr.training_step(batch, t=t.to(DEV), noise=eps.to(DEV))[0]
        e = abs(float(loss.double().mean()) - traj['losses'][k]) / traj['losses'][k]
        print('step %d: loss %.6f, rel err vs fp64 %.2e (gate 1e-5)' % (k + 1, float(loss.mean()), e))
        assert e <= 1e-5
    got = tr.state_dict()
    y = float(z['y_traj'])
    far, worst = far_parameters(got, traj['theta'], so().PARAM_NAMES, y)
    moved = max(float((got[k].cpu() - sd[k]).abs().max()) for k in so().PARAM_NAMES)
    print('trajectory: %d of %d parameters further than 8 y_traj = %.3e from fp64 (cap %d); max distance %.3e; largest move %.3e'
          % (far, N_PARAM, 8 * y, N_PARAM // 1000, worst, moved))
    assert far <= N_PARAM // 1000 == 5499
    assert set(got) == set(sd)
    for k in sd:
        if k not in so().PARAM_NAMES:
            assert torch.equal(got[k], sd[k]), k                           # PositionalEmbedding.pe passes through: identical bits


@pytest.mark.gpu
def test_plumbing(lib, traj):
    from interdiff_amd import skeleton_losses as sl
    from interdiff_amd.diffusion import create_gaussian_diffusion
    p, d = point('S1'), on_dev(point('S1'))
    batch = tuple(b.to(DEV) for b in p['batch'])
    step = lambda tr, k: tr.training_step(batch, t=traj['ts'][k].to(DEV), noise=traj['noises'][k].to(DEV))
    a = new_trainer()
    step(a, 0), step(a, 1)
    # state + optimizer state continue the trajectory bit for bit; the dict form of a batch is the tuple form
    b = new_trainer(sd=a.state_dict())
    b.load_optimizer_state(a.optimizer_state())
    assert b.step == 2 and torch.equal(a.params, b.params) and b.params.numel() == N_PARAM
    step(a, 2)
    b.training_step(dict(gt=d['x0'], zero_pose_obj=d['zpo']), t=traj['ts'][2].to(DEV), noise=traj['noises'][2].to(DEV))
    assert torch.equal(a.params, b.params) and torch.equal(a.exp_avg, b.exp_avg) and torch.equal(a.exp_avg_sq, b.exp_avg_sq)
    assert not torch.equal(a.params, new_trainer().params)
    # after three steps the exported sampler model computes what the trainer computes
    a.loss_and_grads(batch, t=traj['ts'][3].to(DEV), noise=traj['noises'][3].to(DEV))
    mdm = a.export_mdm()
    x_t = a.diffusion.q_sample(d['x0'], traj['ts'][3].to(DEV), noise=traj['noises'][3].to(DEV))
    e = rel(mdm.forward(x_t, traj['ts'][3].to(DEV), d['zpo'], y={'cond': a.cond}), a.pred)
    e0 = rel(new_trainer().export_mdm().forward(x_t, traj['ts'][3].to(DEV), d['zpo'], y={'cond': a.cond}), a.pred)
    print('export_mdm().forward vs the trainer\'s pred after 3 steps: %.3e (gate 1e-4); the untrained model\'s is %.3e away' % (e, e0))
    assert e <= 1e-4 < e0
    # training_step, then the scoring entry on the exported model, end to end (a 20-step schedule keeps the sample short)
    short = new_trainer(n_steps=20)
    loss = short.training_step(batch, seed=5, generator=torch.Generator().manual_seed(3))[0]
    val, ld, wd = sl.validation_step(short.export_mdm(), create_gaussian_diffusion('cosine', 20), batch, past_len=PAST, seed=7)
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(val)) and list(ld) == list(sl.KEYS)
