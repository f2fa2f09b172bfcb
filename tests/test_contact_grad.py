"""The contact / penetration gradient of the SMPL correction trainers (csrc/corr_geometry_grad.hip, ``correction_losses.contact_gradient``), the two
entries that return the trainers' own prediction, and the one-call training step on the reference's full loss -- against the reference's own autograd
(tests/golden/corr_contact_grad*.npz; tests/golden/make_golden_corr_contact_grad.py) and the closed-form fp64 restatement tests/contact_grad_oracle.py.

Gates (none of them comes from the code under test):
  d_obj_pred   max|d - d64| <= 4 e_ref, e_ref = max|d32 - d64| of the reference's own fp32 autograd (the project's gate of DESIGN.md 8.12); per-frame
               counts equal the reference's on every frame; the two terms within the 1e-4 per-term gate of tests/test_correction_losses.py
  prediction   the 8 MSE terms recomputed in fp64 from the returned prediction against the gradient entry's: one fp32 rounding of the prediction,
               sum 2 |d| 2^-24 (|pred| summed over the frames d reads) / count per term, from the data
  gradients    per tensor max|g - g64| / max|g64| <= max(4 e_ref, 1e-5); ten terms and loss within 1e-4
  trajectory   no (compared) parameter further than 8 y_traj from the reference's after 10 Adam steps over the epoch boundary 9 -> 10
"""
import functools
import numpy as np
import pytest
import torch
from tests import fixtures as fx
from tests import corr_fixtures as cf
from tests import contact_grad_oracle as cgo
from tests import correction_finetune_oracle as fo
from tests import correction_train_oracle as to
from interdiff_amd import _lib
from interdiff_amd import correction_losses as cl
from interdiff_amd import correction_finetune as cft
from interdiff_amd import correction_train as ct

DEV = 'cuda'
GATE, TIGHT = 1e-4, 1e-5
EPOCHS = (5, 10, 20)
WEIGHTS = cl.CorrectionLossWeights()


@functools.lru_cache(None)
def g(name):
    z = fx.golden(name)
    return {k: z[k] for k in z.files}


def ckpt(zero_tracked=False):
    sd = dict(g('correction_ckpt.npz'))
    if zero_tracked:
        for k in sd:
            if k.endswith('num_batches_tracked'):
                sd[k] = np.zeros((), np.int64)
    return sd


@functools.lru_cache(None)
def scene(which):
    """'s': corr_fixtures.scene(); 'a': the same with clip 0's object moved out of its body; 'f': the full-size scene of the fixture's seed."""
    z = g('corr_contact_grad.npz')
    if which == 'f':
        sc = cf.scene(int(z['f_seed']), cf.FULL_T, cf.FULL_B, cf.FULL_V, cf.FULL_P)
    else:
        sc = cf.scene()
        if which == 'a':
            sc = cgo.apart(sc, shift=z['apart'])
    for k, v in sc.items():
        assert cf.checksum(v) == z['%s_crc_%s' % (which, k)], k
    return sc


def pose_batch(sc):
    """The stacked-tensor batch WITHOUT the geometry operands (what the trainers took before)."""
    return {k: torch.from_numpy(sc[k]) for k in ('obj_angle', 'obj_trans', 'markers')}


def full_batch(sc):
    return {k: torch.from_numpy(sc[k]) for k in ('obj_angle', 'obj_trans', 'markers', 'obj_points', 'human_verts')}


def rel_errors(got, want):
    return {n: float(np.abs(np.asarray(got[n], np.float64).ravel() - want[n].ravel()).max() / np.abs(want[n]).max()) for n in want}


# ------------------------------------------------------------------------------------------------------------ not on the GPU
@pytest.mark.parametrize('which', ('s', 'a'))
def test_closed_form_oracle_equals_the_recorded_fp64_gradient(which):
    z, sc = g('corr_contact_grad.npz'), scene(which)
    for e in EPOCHS:
        pre = '%s_e%d_' % (which, e)
        r = cgo.geometry(z[pre + 'pred'], sc['obj_points'], sc['human_verts'], *z[pre + 'w_geo'])
        assert np.abs(r['grad'] - z[pre + 'd64']).max() <= 1e-12 * float(z[pre + 'gmax']), pre
        assert np.array_equal(r['frames'][:, 2:], z[pre + 'frames'][:, 2:]), pre
        assert np.abs(r['frames'][:, :2] - z[pre + 'frames'][:, :2]).max() <= GATE * z[pre + 'frames'][:, :2].max()
        assert tuple(z[pre + 'w_geo']) == WEIGHTS.vector(e)[:2]
    none = z[which + '_e20_frames'][:, 2] == 0
    assert none.any() == (which == 'a')                                       # the apart scene: clip 0's frames have no penetrating point ...
    r = cgo.geometry(z[which + '_e20_pred'], sc['obj_points'], sc['human_verts'], 1.0, 0.0)
    assert not r['grad'].reshape(-1, 9)[none].any() and r['grad'].reshape(-1, 9)[~none].any(axis=1).all()      # ... and an exactly zero penetration gradient


def test_closed_form_oracle_against_a_finite_difference():
    """Two frames of the scene at the recorded prediction; the indices and masks are held (the difference asserts that no mask moves)."""
    z, sc = g('corr_contact_grad.npz'), scene('s')
    pred, hv = z['s_e20_pred'][:2].astype(np.float64), sc['human_verts'][:2]
    entries = np.random.RandomState(5).choice(pred.size, 16, replace=False)
    fd, base = cgo.finite_difference(pred, sc['obj_points'], hv, 0.1, 1.0, entries)
    err = np.abs(fd - base['grad'].ravel()[entries]).max() / np.abs(base['grad']).max()
    print('finite difference vs closed form: %.3e of the largest entry' % err)
    assert err <= 1e-7


# ------------------------------------------------------------------------------------------------------------ the geometry gradient
def device_case(which, e):
    z, sc = g('corr_contact_grad.npz'), scene(which)
    pre = '%s_e%d_' % (which, e)
    return z, pre, torch.from_numpy(z[pre + 'pred']).to(DEV), torch.from_numpy(sc['obj_points']).to(DEV), torch.from_numpy(sc['human_verts']).to(DEV)


@pytest.mark.gpu
@pytest.mark.parametrize('which', ('s', 'a', 'f'))
def test_geometry_gradient_against_the_reference(which):
    """Measured on MI355X: see DESIGN.md 8.14 (max|d - d64| / e_ref per case)."""
    for e in EPOCHS:
        z, pre, pred, pts, hv = device_case(which, e)
        w = WEIGHTS.vector(e)
        d, terms, frames = cl.geometry_gradient(pred, pts, hv, w[0], w[1], return_frames=True)
        err = float(np.abs(d.cpu().double().numpy() - z[pre + 'd64']).max())
        e_ref = float(z[pre + 'e_ref'])
        print('%s epoch %2d: max|d - d64| %.3e = %.2f e_ref (e_ref %.3e, gmax %.3e)' % (which, e, err, err / e_ref, e_ref, float(z[pre + 'gmax'])))
        assert err <= 4 * e_ref
        assert np.array_equal(frames[:, 2:].cpu().numpy(), z[pre + 'frames'][:, 2:].astype(np.float32))
        fwd, ffr = cl.correction_terms(pred, pred, pts, hv, return_frames=True)
        for i in range(2):
            assert abs(float(terms[i]) - float(z[pre + 'terms'][i])) <= GATE * float(z[pre + 'terms'][i])
            assert abs(float(terms[i]) - float(fwd[i])) <= GATE * float(fwd[i])
        assert torch.equal(frames[:, 2:], ffr[:, 2:]) and float((frames - ffr).abs().max()) <= GATE * float(ffr.abs().max())      # the forward entry's partials
        batch = dict(obj_points=pts, human_verts=hv)
        d2, named = cl.contact_gradient(pred, batch, WEIGHTS, e)
        assert torch.equal(d2, d) and float(named['penetration']) == float(terms[0]) and float(named['contact']) == float(terms[1])
    listed = dict(obj_points=pts, frames=[dict(human_verts=hv[t]) for t in range(hv.shape[0])])
    assert torch.equal(cl.contact_gradient(pred, listed, WEIGHTS, e)[0], d)        # the DataLoader's dict of lists


@pytest.mark.gpu
def test_zero_weights_repeat_and_scaling():
    z, pre, pred, pts, hv = device_case('a', 20)
    d0, t0 = cl.geometry_gradient(pred, pts, hv, 0.0, 0.0)
    assert int(torch.count_nonzero(d0)) == 0 and float(t0[0]) > 0 and float(t0[1]) > 0
    d0, _ = cl.contact_gradient(pred, dict(obj_points=pts, human_verts=hv), WEIGHTS, 0)            # epoch 0: both annealed weights are 0
    assert int(torch.count_nonzero(d0)) == 0
    d1, t1 = cl.geometry_gradient(pred, pts, hv, 0.1, 1.0)
    d1b, t1b = cl.geometry_gradient(pred, pts, hv, 0.1, 1.0)
    assert torch.equal(d1, d1b) and torch.equal(t1, t1b)
    d2, t2 = cl.geometry_gradient(pred, pts, hv, 0.2, 2.0)
    assert torch.equal(d2, 2 * d1) and torch.equal(t2, t1) and float(d1.abs().max()) > 0
    none = torch.from_numpy(z[pre + 'frames'][:, 2] == 0).to(DEV)
    dp, _ = cl.geometry_gradient(pred, pts, hv, 0.1, 0.0)
    assert bool(none.any()) and int(torch.count_nonzero(dp.reshape(-1, 9)[none])) == 0             # frames without a penetrating point: exact zeros
    wide = torch.cat([pts[..., :3], torch.full_like(pts[..., :1], 7.0)], dim=2).contiguous()       # point stride 4
    assert torch.equal(cl.geometry_gradient(pred, wide, hv, 0.1, 1.0)[0], d1)


@pytest.mark.gpu
def test_one_vertex_one_point():
    """B = V = P = 1.  The point lies 0.1 behind the vertex along its normal (it penetrates) and the vertex is labelled and farther than 2 cm.  Bound: the
    kernel forms y - x in fp32 from values of size <= 1 that differ by 0.1, a relative error <= 3 * 2^-24 * 1 / 0.1 = 1.8e-6 of the unit vector, and poses
    the point in fp32 (the same size); 1e-5 of the largest entry covers both."""
    pred = np.array([[[1.0, 0.1, -0.2, 0.05, 0.9, 0.3, 0.4, -0.3, 0.2]]], np.float32)
    pts = np.array([[[0.1, -0.2, 0.05]]], np.float32)
    y, _ = cgo.pose(pred.astype(np.float64), pts.astype(np.float64))
    n = np.array([0.6, 0.0, 0.8])
    hv = np.concatenate([y[0, 0] + 0.1 * n, n, [1.0]]).astype(np.float32).reshape(1, 1, 1, 7)
    want = cgo.geometry(pred, pts, hv, 0.1, 1.0)
    assert want['frames'][0, 2] == 1 and want['frames'][0, 3] == 1
    d, terms, frames = cl.geometry_gradient(torch.from_numpy(pred).to(DEV), torch.from_numpy(pts).to(DEV), torch.from_numpy(hv).to(DEV), 0.1, 1.0, True)
    assert np.abs(d.cpu().double().numpy() - want['grad']).max() <= TIGHT * np.abs(want['grad']).max()
    assert np.array_equal(frames[:, 2:].cpu().numpy(), want['frames'][:, 2:].astype(np.float32))
    assert np.abs(terms.cpu().double().numpy() - want['terms']).max() <= GATE * want['terms'].max()


@pytest.mark.gpu
def test_bad_arguments_are_refused():
    z, pre, pred, pts, hv = device_case('s', 20)
    for bad in (lambda: cl.geometry_gradient(pred[..., :8], pts, hv, 0.1, 1.0), lambda: cl.geometry_gradient(pred, pts[:3], hv, 0.1, 1.0),
                lambda: cl.geometry_gradient(pred, pts[..., :2], hv, 0.1, 1.0), lambda: cl.geometry_gradient(pred, pts, hv[:34], 0.1, 1.0),
                lambda: cl.geometry_gradient(pred, pts, hv[..., :6], 0.1, 1.0)):
        with pytest.raises(ValueError):
            bad()
    for w in ((-0.1, 1.0), (0.1, float('nan')), (float('inf'), 1.0)):
        with pytest.raises(RuntimeError):
            cl.geometry_gradient(pred, pts, hv, *w)
    lib = _lib.load()
    T, B, V, P = cf.T, cf.B, cf.V, cf.P
    need = lib.interdiff_correction_geometry_grads_workspace_bytes(T, B, V, P)
    assert need > 0 and lib.interdiff_correction_geometry_grads_workspace_bytes(T, 0, V, P) == 0
    ws, out, terms = torch.empty(need, dtype=torch.uint8, device=DEV), torch.empty_like(pred), torch.empty(2, device=DEV)
    call = lambda T=T, V=V, stride=6, n=need, o=out: lib.interdiff_correction_geometry_grads(
        _lib.dptr(pred), _lib.dptr(pts), stride, _lib.dptr(hv), T, B, V, P, 0.1, 1.0, _lib.dptr(o, allow_none=True), _lib.dptr(terms), None, _lib.dptr(ws), n,
        _lib.stream())
    assert call() == 0
    assert call(n=need - 1) == -12                                               # a short workspace
    assert call(T=0) == -22 and call(V=0) == -22 and call(stride=2) == -22 and call(o=None) == -22
    assert call(T=70000) == -22                                                  # T * B > 65535: frames ride on the grid's second dimension


# ------------------------------------------------------------------------------------------------------------ the trainers' own prediction
def mse_terms64(pred, gt, past):
    """The 8 MSE terms in fp64 (MSE_KEYS order) and, per term, the deviation ONE fp32 rounding of the prediction allows: sum 2 |d| u / count, u the
    sum of 2^-24 |pred| over the (one or two) frames the difference d reads."""
    p, q = pred.astype(np.float64), gt.astype(np.float64)
    u = np.abs(p) * 2.0 ** -24
    terms, allowed = [], []
    for vel in (False, True):
        for fut in (False, True):
            for c in (slice(0, 6), slice(6, 9)):
                if not vel:
                    t = slice(past, None) if fut else slice(0, past)
                    d, r = (p - q)[t, :, c], u[t, :, c]
                elif not fut:
                    d, r = ((p[1:past + 1] - p[:past]) - (q[1:past + 1] - q[:past]))[..., c], (u[1:past + 1] + u[:past])[..., c]
                else:
                    d, r = ((p[past:] - p[past - 1:-1]) - (q[past:] - q[past - 1:-1]))[..., c], (u[past:] + u[past - 1:-1])[..., c]
                terms.append((d * d).mean())
                allowed.append((2 * np.abs(d) * r).sum() / d.size)
    return np.asarray(terms), np.asarray(allowed)


def target(sc):
    aa = torch.from_numpy(sc['obj_angle'])
    return torch.cat([cft.rotation_6d_of_axis_angle(aa), torch.from_numpy(sc['obj_trans'])], dim=2).numpy()


def check_prediction(pred, out9, sc, what):
    terms, allowed = mse_terms64(pred.cpu().numpy(), target(sc), cf.PAST)
    got = out9.cpu().double().numpy()
    dev = np.abs(got - terms)
    print('%s: worst |term - recomputed| / allowed %.3f' % (what, (dev / allowed).max()))
    assert (dev <= allowed).all(), (what, dev / allowed)


@pytest.mark.gpu
def test_predict_entries_return_the_prediction_the_backward_sees():
    """Measured on MI355X: see DESIGN.md 8.14."""
    sc = scene('s')
    batch = pose_batch(sc)
    ft = cft.CorrectionFineTuner(ckpt(), T=cf.T, past_len=cf.PAST, device=DEV)
    for initialize in (True, False):
        pred = ft.predict(batch, initialize)
        out9, _ = ft._grads(batch, initialize)
        check_prediction(pred, out9[1:], sc, 'fine-tuner, initialize %s' % initialize)
        assert torch.equal(pred, ft.predict(batch, initialize))
        ref = ft.predictor.forward(batch, initialize)[0]                          # the MFMA inference forward: close, not the same arithmetic
        assert float((pred - ref).abs().max()) <= GATE * float(ref.abs().max())
    zt = g('corr_contact_grad_train.npz')
    p = float(zt['p_drop'])
    tr = ct.CorrectionTrainer(ckpt(True), T=cf.T, past_len=cf.PAST, dropout=p, seed=11, device=DEV)
    masks, nodes = torch.from_numpy(to.masks_for(int(zt['seed_mask']), 0, cf.B, p)), [int(n) for n in zt['nodes']]
    bn, params = tr.bn.clone(), tr.params.clone()
    for initialize, how in ((True, dict(masks=masks)), (False, dict(masks=masks, nodes=nodes)), (False, dict())):
        pred = tr.predict(batch, initialize, **how)
        out9, _, _ = tr._train_grads(batch, initialize, how.get('masks'), how.get('nodes'))
        check_prediction(pred, out9[1:], sc, 'trainer, initialize %s, %s' % (initialize, sorted(how) or 'generator'))
        assert torch.equal(tr.bn, bn) and torch.equal(tr.params, params) and tr.step == 0
    assert float((tr.predict(batch, False, masks=masks, nodes=nodes) - torch.from_numpy(zt['pred']).to(DEV)).abs().max()) <= GATE * float(np.abs(zt['pred']).max())
    with pytest.raises(ValueError):
        ft.predict({k: v[:34] for k, v in batch.items()})
    with pytest.raises(ValueError):
        tr.predict(batch, False, nodes=[1] + nodes[1:])


# ------------------------------------------------------------------------------------------------------------ the one-call step
def check_full_loss(out, z, pre, what):
    loss, ld, wd, _ = out
    assert tuple(ld) == cl.LOSS_KEYS and tuple(wd) == cl.WEIGHTED_KEYS
    got = np.asarray([float(ld[k]) for k in cl.LOSS_KEYS])
    assert (np.abs(got - z[pre + 'terms']) <= GATE * np.abs(z[pre + 'terms'])).all(), (what, got, z[pre + 'terms'])
    assert abs(float(loss) - float(z[pre + 'loss'])) <= GATE * float(z[pre + 'loss']), what
    assert abs(float(sum(wd.values())) - float(loss)) <= TIGHT * float(loss)


@pytest.mark.gpu
@pytest.mark.parametrize('epoch', EPOCHS)
def test_fine_tuner_gradients_of_the_full_loss(epoch):
    """Measured on MI355X: see DESIGN.md 8.14."""
    z, sc = g('corr_contact_grad.npz'), scene('s')
    pre = 's_e%d_' % epoch
    ft = cft.CorrectionFineTuner(ckpt(), T=cf.T, past_len=cf.PAST, device=DEV)
    out = ft.loss_and_grads(full_batch(sc), current_epoch=epoch)
    check_full_loss(out, z, pre, 'epoch %d' % epoch)
    _, _, g64 = fo.loss_and_grads(fo.leaves(ckpt()), sc, epoch < 10, z[pre + 'd64p'])
    err = rel_errors({n: v.cpu().numpy() for n, v in out[3].items()}, {n: v.numpy() for n, v in g64.items()})
    names = [str(n) for n in z['names']]
    worst = max(names, key=lambda n: err[n] / max(4 * float(z[pre + 'e_ref_p'][names.index(n)]), TIGHT))
    print('epoch %d: worst tensor %s: e %.3e, gate %.3e' % (epoch, worst, err[worst], max(4 * float(z[pre + 'e_ref_p'][names.index(worst)]), TIGHT)))
    for n, e in zip(names, z[pre + 'e_ref_p']):
        assert err[n] <= max(4 * float(e), TIGHT), (n, err[n], float(e))
    assert ft.step == 0


@pytest.mark.gpu
def test_trainer_gradients_of_the_full_loss():
    z, sc = g('corr_contact_grad_train.npz'), scene('s')
    p, nodes = float(z['p_drop']), [int(n) for n in z['nodes']]
    masks = to.masks_for(int(z['seed_mask']), 0, cf.B, p)
    tr = ct.CorrectionTrainer(ckpt(True), T=cf.T, past_len=cf.PAST, dropout=p, seed=11, device=DEV)
    bn = tr.bn.clone()
    out = tr.loss_and_grads(full_batch(sc), masks=torch.from_numpy(masks), nodes=nodes, current_epoch=20)
    check_full_loss(out, z, '', 'train()')
    sd = {k: v for k, v in ckpt().items() if not k.endswith('num_batches_tracked')}
    _, _, g64, _ = to.loss_and_grads(to.leaves(sd), sc, False, nodes, masks, p, z['d64p'])
    names = [str(n) for n in z['names']]
    got = {n: v.cpu().numpy() for n, v in out[3].items()}
    err = rel_errors({n: got[n] for n in to.compared(names)}, {n: g64[n].numpy() for n in to.compared(names)})
    print('train(): worst e / gate %.3f' % max(err[n] / max(4 * float(z['e_ref_p'][names.index(n)]), TIGHT) for n in err))
    for n in names:
        if n in err:
            assert err[n] <= max(4 * float(z['e_ref_p'][names.index(n)]), TIGHT), (n, err[n])
        else:
            assert not got[n].any(), n
    assert torch.equal(tr.bn, bn) and tr.step == 0


def make(kind, sd=None):
    if kind == 'ft':
        return cft.CorrectionFineTuner(sd or ckpt(), T=cf.T, past_len=cf.PAST, device=DEV)
    return ct.CorrectionTrainer(sd or ckpt(True), T=cf.T, past_len=cf.PAST, dropout=0.1, seed=23, device=DEV)


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ('ft', 'tr'))
def test_one_call_step_is_the_three_call_composition(kind):
    """``training_step`` at epoch 5 without ``d_obj_pred``: what the parent refused.  It equals predict -> contact_gradient -> training_step(d_obj_pred=...)
    bit for bit, raises without the geometry operands, lets an explicit ``d_obj_pred`` win, and at epoch 0 does what it did without the operands."""
    sc = scene('s')
    batch, bare = full_batch(sc), pose_batch(sc)
    for epoch in (5, 10):
        one, three = make(kind), make(kind)
        loss = one.training_step(batch, epoch)
        pred = three.predict(bare, epoch < 10)
        d, terms = cl.contact_gradient(pred, {k: v.to(DEV) for k, v in batch.items()}, WEIGHTS, epoch)
        assert float(d.abs().max()) > 0
        loss8 = three.training_step(bare, epoch, d_obj_pred=d)
        assert torch.equal(one.params, three.params) and torch.equal(one.bn, three.bn) and torch.equal(one.predictor.arena, three.predictor.arena)
        assert torch.equal(one.exp_avg, three.exp_avg) and torch.equal(one.exp_avg_sq, three.exp_avg_sq) and one.step == three.step == 1
        w = WEIGHTS.vector(epoch)
        assert abs(float(loss) - (float(loss8) + w[0] * float(terms['penetration']) + w[1] * float(terms['contact']))) <= TIGHT * float(loss)
        if kind == 'tr':
            assert all(int(v) == 1 for k, v in one.state_dict().items() if k.endswith('num_batches_tracked'))      # the statistics moved once
            ref = make(kind)
            ref.training_step(bare, 0)
            assert torch.equal(one.bn, ref.bn)                                    # (the stacks run before the node selection: the same statistics)
        with pytest.raises(ValueError):
            make(kind).training_step(bare, epoch)                                 # no geometry operands, no d_obj_pred
        with pytest.raises(ValueError):
            make(kind).loss_and_grads(bare, current_epoch=epoch)
        given = make(kind)
        given.training_step(batch, epoch, d_obj_pred=torch.zeros_like(d))         # an explicit d_obj_pred wins
        pose_only = make(kind)
        pose_only.training_step(bare, epoch, d_obj_pred=torch.zeros_like(d))
        assert torch.equal(given.params, pose_only.params) and not torch.equal(given.params, one.params)
    # epoch 0: one pass, bit-identical with and without the operands
    a, b = make(kind), make(kind)
    ga, gb = a.loss_and_grads(batch, current_epoch=0), b.loss_and_grads(bare, True)
    assert tuple(ga[1]) == cl.MSE_KEYS and torch.equal(ga[0], gb[0]) and all(torch.equal(ga[3][n], gb[3][n]) for n in gb[3])
    la, lb = a.training_step(batch, 0), b.training_step(bare, 0)
    assert torch.equal(la, lb) and torch.equal(a.params, b.params) and torch.equal(a.bn, b.bn) and torch.equal(a.predictor.arena, b.predictor.arena)


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ('ft', 'tr'))
def test_trajectory_over_the_epoch_boundary(kind):
    """Measured on MI355X: see DESIGN.md 8.14."""
    sc = scene('s')
    batch = full_batch(sc)
    z = g('corr_contact_grad_traj.npz' if kind == 'ft' else 'corr_contact_grad_traj_train.npz')
    names = [str(n) for n in z['names']]
    if kind == 'ft':
        tr = cft.CorrectionFineTuner(fo.perturbed(ckpt(), int(z['traj_seed_perturb']), float(z['traj_rel'])), T=cf.T, past_len=cf.PAST, lr=float(z['lr']), device=DEV)
        losses = [float(tr.training_step(batch, int(e))) for e in z['epochs']]
    else:
        p, nodes = float(z['p_drop']), [int(n) for n in z['nodes']]
        tr = ct.CorrectionTrainer(ckpt(True), T=cf.T, past_len=cf.PAST, dropout=p, lr=float(z['lr']), seed=11, device=DEV)
        losses = [float(tr.training_step(batch, int(e), masks=torch.from_numpy(to.masks_for(int(z['seed_mask']), s, cf.B, p)), nodes=nodes if e >= 10 else None))
                  for s, e in enumerate(z['epochs'])]
    relv = np.abs(np.asarray(losses) - z['traj_losses']) / z['traj_losses']
    mine = {n: v.detach().cpu().double().numpy().ravel() for n, v in tr.named_parameters().items()}
    sizes = [mine[n].size for n in names]
    ref = dict(zip(names, np.split(z['theta_final'].astype(np.float64), np.cumsum(sizes)[:-1])))
    cmp_ = names if kind == 'ft' else to.compared(names)
    diff = max(float(np.abs(mine[n] - ref[n]).max()) for n in cmp_)
    print('%s: losses %s; max relative loss difference %.3e; max |theta - reference| %.3e = %.2f y_traj' % (kind, ' '.join('%.6f' % v for v in losses), relv.max(), diff,
                                                                                                        diff / float(z['y_traj'])))
    assert relv.max() <= GATE
    assert diff <= 8 * float(z['y_traj'])
    assert tr.step == 10
