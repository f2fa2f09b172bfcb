"""Training of the skeleton correction predictor with batch statistics and dropout (interdiff_amd/skeleton_train.py, csrc/skeleton_bn_train.h,
csrc/skeleton_train.hip) against the reference's own module in train() (tests/golden/skel_train.npz, skel_train_b1.npz, skel_train_traj.npz;
tests/golden/make_golden_skeleton_train.py) and the fp64 restatement tests/skeleton_train_oracle.py.

Gates (none of them comes from the code under test; they follow tests/test_skeleton_finetune.py):
  gradient    per compared tensor e = max|g - g64| / max|g64| <= max(4 e_ref, 1e-5); compared = named_parameters() without the 24 convolution
              biases, whose gradient must be exactly 0
  statistics  batch statistics and updated buffers per buffer tensor <= max(4 e_ref_stats, 1e-5) resp. max(4 e_ref_buffers, 1e-5)
  loss        the 1e-4 per-term gate
  trajectory  losses within 1e-5 relative of the reference's at every step; at most 96 compared parameters further than 8 y_traj from the
              reference's; final buffers within 8 y_stats
  zeros       the gradient of st_gcnns_all.3.gcn.A has the reference's zero pattern -- which in train() is EMPTY (the recorder's docstring says why):
              the 9,240 exact zeros of the eval() gradient do not exist here, so what is asserted is that there is none
"""
import functools
import numpy as np
import pytest
import torch
from tests import fixtures as fx
from tests import skeleton_train_oracle as to
from interdiff_amd import skeleton as sk
from interdiff_amd import skeleton_finetune as sf
from interdiff_amd import skeleton_train as st

DEV = 'cuda'
TIGHT, TERM_GATE = 1e-5, 1e-4
ZERO_TENSOR = 'st_gcnns_all.3.gcn.A'
BATCH_KEYS = ('body', 'obj', 'pose', 'zero_pose_obj')


@functools.lru_cache(None)
def g(name):
    z = fx.golden(name)
    return {k: z[k] for k in z.files}


def ckpt():
    return dict(g('skel_ckpt.npz'))


def point(which):
    """-> (state_dict, batch as torch tensors, fixture dict, flat masks)."""
    z = g('skel_train.npz' if which == 'b3' else 'skel_train_b1.npz')
    sd = ckpt() if which == 'b3' else to.perturbed(ckpt(), int(z['seed_perturb']), float(z['rel']))
    batch = tuple(torch.from_numpy(z[k]) for k in BATCH_KEYS)
    return sd, batch, z, to.masks_for(int(z['seed_mask']), 0, batch[0].shape[0], float(z['p_drop']))


@functools.lru_cache(None)
def oracle_point(which):
    """fp64 loss, terms, gradients, batch statistics and updated buffers of a fixture point, computed once and shared."""
    sd, batch, z, masks = point(which)
    loss, terms, grads, stats = to.loss_and_grads(to.leaves(sd), batch, masks, float(z['p_drop']))
    buf = to.updated_buffers({k: torch.from_numpy(np.asarray(sd[k], np.float64)) for k in to.BUFFERS}, stats, batch[0].shape[0])
    return float(loss), {k: float(v) for k, v in terms.items()}, {k: v.numpy() for k, v in grads.items()}, {k: v.numpy() for k, v in stats.items()}, \
        {k: v.numpy() for k, v in buf.items()}


def split(z, flat, kind=''):
    return {str(n): flat[o:o + s] for n, o, s in zip(z['names' + kind], z['offsets' + kind], z['sizes' + kind])}


def rel_errors(got, want):
    return {n: float(np.abs(np.asarray(got[n], np.float64).ravel() - want[n].ravel()).max() / np.abs(want[n]).max()) for n in want}


# ------------------------------------------------------------------------------------------------------------ CPU

@pytest.mark.parametrize('which', ['b3', 'b1'])
def test_oracle_against_the_reference(which):
    _, _, z, _ = point(which)
    loss64, terms64, g64, s64, b64 = oracle_point(which)
    assert abs(loss64 - float(z['loss'])) <= 2e-6 * loss64 and abs(loss64 - float(z['loss64'])) <= 1e-12
    for k, v in zip(to.MSE_KEYS, z['terms']):
        assert abs(terms64[k] - float(v)) <= 1e-5 * terms64[k], k
    names = [str(n) for n in z['names']]
    assert names == list(g64) and len(to.compared(names)) == len(names) - 24
    ref = split(z, z['grads'])
    for i, n in enumerate(names):
        if n in to.CONV_BIASES:
            assert np.isnan(z['e_ref'][i])
            w = n[:-4] + 'weight'
            assert np.abs(ref[n]).max() <= 1e-5 * np.abs(ref[w]).max() and np.abs(g64[n]).max() <= 1e-12 * np.abs(g64[w]).max(), n
            continue
        e = float(np.abs(ref[n].astype(np.float64) - g64[n].ravel()).max() / np.abs(g64[n]).max())
        assert e <= 1.01 * float(z['e_ref'][i]) + 1e-12 and 4 * e <= 1e-4, (n, e)           # the recorded e_ref IS this comparison
    assert int(z['zeros_A']) == 0 and not (ref[ZERO_TENSOR] == 0).any() and not (g64[ZERO_TENSOR] == 0).any()
    for kind, want, key in (('stats', s64, 'e_ref_stats'), ('buffers_after', b64, 'e_ref_buffers')):
        err = rel_errors(split(z, z[kind], '_buffers'), want)
        for i, n in enumerate(to.BUFFERS):
            assert err[n] <= 1.01 * float(z[key][i]) + 1e-12 and 4 * err[n] <= 1e-4, (kind, n, err[n])


def test_oracle_trajectory_against_the_reference():
    sd, batch, _, _ = point('b3')
    z = g('skel_train_traj.npz')
    losses, theta, buf = to.adam_trajectory_train(sd, batch, int(z['steps']), int(z['seed_mask']), float(z['p_drop']), float(z['lr']), float(z['weight_decay']))
    assert np.abs(losses - z['traj_losses']).max() <= 1e-6 * losses.min() and losses[-1] < losses[0]
    names = [str(n) for n in z['names']]
    ref = split(g('skel_train.npz'), z['theta_final'])
    y = max(np.abs(theta[n].numpy().ravel() - ref[n].astype(np.float64)).max() for n in to.compared(names))
    assert abs(y - float(z['y_traj'])) <= 0.01 * float(z['y_traj'])
    ys = np.abs(np.concatenate([buf[k].numpy().ravel() for k in to.BUFFERS]) - z['buffers_final'].astype(np.float64)).max()
    assert abs(ys - float(z['y_stats'])) <= 0.01 * float(z['y_stats'])
    for n in to.CONV_BIASES:                                       # exact-zero gradients: Adam leaves these where they were
        assert np.array_equal(theta[n].numpy(), np.asarray(sd[n], np.float64)), n


def test_batchnorm_train_backward_against_autograd():
    """The formula of the kernels (numpy fp64) against autograd on one convolution + train-mode BatchNorm + mask."""
    torch.set_grad_enabled(True)                               # (other test modules switch autograd off process-wide)
    rs = np.random.RandomState(7520)
    cin, cout, n = 5, 7, 33
    t = lambda *s: torch.from_numpy(rs.standard_normal(s))
    x, Rw = t(cin, n), t(cout, n)
    mask = torch.from_numpy((rs.random_sample((cout, n)) >= 0.3).astype(np.float64) / 0.7)
    W, b, gamma, beta = (t(cout, cin).requires_grad_(), t(cout).requires_grad_(), t(cout).requires_grad_(), t(cout).requires_grad_())
    c = W @ x + b[:, None]
    mu, var = c.mean(dim=1, keepdim=True), ((c - c.mean(dim=1, keepdim=True)) ** 2).mean(dim=1, keepdim=True)
    y = ((c - mu) / torch.sqrt(var + to.BN_EPS) * gamma[:, None] + beta[:, None]) * mask
    want = torch.autograd.grad((y * Rw).sum(), [W, b, gamma, beta])
    dy = (Rw * mask).numpy()
    dc, dgamma, dbeta = to.bn_train_backward(dy, c.detach().numpy(), gamma.detach().numpy())
    got = (dc @ x.numpy().T, dc.sum(axis=1), dgamma, dbeta)
    scale = np.abs(want[0].numpy()).max()
    for a, w, s in zip(got, want, (scale, scale, None, None)):
        assert np.abs(a - w.numpy()).max() <= 1e-12 * (s or np.abs(w.numpy()).max())
    assert np.abs(got[1]).max() <= 1e-12 * scale                # the convolution bias cancels


def test_init_state_dict():
    ref = ckpt()
    sd = st.init_state_dict(11)
    assert [k for k in sd if not k.endswith('num_batches_tracked')] == list(ref)
    bounds = {}
    for k, v in ref.items():
        assert tuple(sd[k].shape) == tuple(v.shape) and sd[k].dtype == torch.as_tensor(v).dtype, k
        if k.endswith(('tcn.0.weight', 'tcn.0.bias', 'residual.0.weight', 'residual.0.bias')):
            bounds[k] = 1.0 / np.sqrt(ref[k[:k.rindex('.')] + '.weight'].shape[1])
        elif k.endswith(('gcn.T', 'gcn.A')):
            bounds[k] = 1.0 / np.sqrt(v.shape[1])
    assert len(bounds) == 12 * 4 + 12 + 4
    for k, bd in bounds.items():
        a = sd[k].double().numpy()
        assert np.abs(a).max() <= bd, k
        if a.size >= 256:
            assert abs(a.std(ddof=1) - bd / np.sqrt(3)) <= 0.1 * bd / np.sqrt(3), (k, a.std(ddof=1), bd)
            assert abs(a.mean()) <= 5 * bd / np.sqrt(3 * a.size), k
    const = {'tcn.1.weight': 1, 'residual.1.weight': 1, 'tcn.1.bias': 0, 'residual.1.bias': 0, 'running_mean': 0, 'running_var': 1, 'prelu.weight': 0.25}
    for k, v in sd.items():
        for suffix, c in const.items():
            if k.endswith(suffix):
                assert (v == c).all(), k
        if k.endswith('num_batches_tracked'):
            assert v.dtype == torch.int64 and v.dim() == 0 and int(v) == 0
    assert sum(k.endswith('num_batches_tracked') for k in sd) == 24
    again, other = st.init_state_dict(11), st.init_state_dict(12)
    assert all(torch.equal(sd[k], again[k]) for k in sd) and not torch.equal(sd['st_gcnns.0.gcn.T'], other['st_gcnns.0.gcn.T'])
    tr = st.SkeletonTrainer(sd, seed=5, device='cpu')            # the packer and the library's parameter table take it
    assert tr.n_param == 96110 and tr.mask_clip == to.MASK_CLIP and list(tr.state_dict()) == list(sd)
    with pytest.raises(ValueError):
        st.SkeletonTrainer(sd, dropout=1.0, device='cpu')
    with pytest.raises(ValueError):
        st.SkeletonTrainer(sd, dropout=-0.1, device='cpu')


# ------------------------------------------------------------------------------------------------------------ GPU

def check_point(which):
    """Measured on MI355X (the six tensors closest to their gates are printed).  B = 1 perturbed point: loss 0.17605771 (reference 0.17605773); closest to its
    gate st_gcnns.0.tcn.0.weight, e 1.67e-6 against 1.00e-5; max e 4.7e-6; statistics / buffers e 1.2e-7 / 1.0e-7.  B = 3: closest st_gcnns.3.prelu.weight,
    e 5.0e-6 against 4.8e-5; statistics / buffers e 1.1e-7 / 5.2e-8."""
    sd, batch, z, masks = point(which)
    _, _, g64, s64, b64 = oracle_point(which)
    tr = st.SkeletonTrainer(sd, dropout=float(z['p_drop']), seed=1, device=DEV)
    loss, ld, wd, grads = tr.loss_and_grads(batch, masks=torch.from_numpy(masks))
    got = {n: v.detach().cpu().numpy() for n, v in grads.items()}
    assert abs(float(loss) - float(z['loss'])) <= TERM_GATE * float(z['loss'])
    for k, v in zip(to.MSE_KEYS, z['terms']):
        assert abs(float(ld[k]) - float(v)) <= TERM_GATE * float(v), k
    assert abs(float(sum(wd.values())) - float(loss)) <= 1e-6 * float(loss)
    names = list(g64)
    for n in to.CONV_BIASES:
        assert (got[n] == 0).all(), n
    cmp_ = to.compared(names)
    err = rel_errors(got, {n: g64[n] for n in cmp_})
    gates = {n: max(4 * float(e), TIGHT) for n, e in zip(names, z['e_ref']) if n in cmp_}
    order = sorted(err, key=lambda n: -err[n] / gates[n])
    print('%s: loss %.8f (reference %.8f); max e %.3e' % (which, float(loss), float(z['loss']), max(err.values())))
    for n in order[:6]:
        print('    %-40s e %.3e  gate %.3e' % (n, err[n], gates[n]))
    missed = {n: (err[n], gates[n]) for n in cmp_ if err[n] > gates[n]}
    assert not missed, missed
    assert all(tuple(grads[n].shape) == g64[n].shape for n in names)
    assert not (got[ZERO_TENSOR] == 0).any()                      # the reference's zero pattern in train(): empty
    # loss_and_grads left the buffers alone; a training step with lr = 0 shows the update alone
    assert np.array_equal(tr.bn.cpu().numpy(), sf.flatten(sd, tr.btable))
    tr2 = st.SkeletonTrainer(sd, dropout=float(z['p_drop']), lr=0.0, seed=1, device=DEV)
    ws = tr2._train_grads(batch, torch.from_numpy(masks), update=True, want_stats=True)[2]
    stats = {n: ws[o:o + int(np.prod(s))].cpu().numpy() for n, o, s in tr2.btable}
    es, eb = rel_errors(stats, s64), rel_errors({k: v.cpu().numpy() for k, v in tr2.buffers().items()}, b64)
    print('    batch statistics: max e %.3e; updated buffers: max e %.3e' % (max(es.values()), max(eb.values())))
    for i, n in enumerate(to.BUFFERS):
        assert es[n] <= max(4 * float(z['e_ref_stats'][i]), TIGHT), (n, es[n])
        assert eb[n] <= max(4 * float(z['e_ref_buffers'][i]), TIGHT), (n, eb[n])


@pytest.mark.gpu
def test_gradients_statistics_b1():
    check_point('b1')


@pytest.mark.gpu
def test_gradients_statistics_b3():
    check_point('b3')


@pytest.mark.gpu
def test_b2_without_dropout_against_the_oracle():
    """No fixture: the oracle is the judge, with the gate of the B = 3 point."""
    sd, z = ckpt(), g('skel_train.npz')
    batch = tuple(torch.from_numpy(a) for a in to.make_batch(7510, 2))
    loss64, terms64, g64, s64 = to.loss_and_grads(to.leaves(sd), batch)
    tr = st.SkeletonTrainer(sd, dropout=0.0, seed=1, device=DEV)
    loss, ld, _, grads = tr.loss_and_grads(batch)
    assert abs(float(loss) - float(loss64)) <= TERM_GATE * float(loss64)
    for k in to.MSE_KEYS:
        assert abs(float(ld[k]) - float(terms64[k])) <= TERM_GATE * float(terms64[k]), k
    names = list(g64)
    got = {n: v.cpu().numpy() for n, v in grads.items()}
    err = rel_errors(got, {n: g64[n].numpy() for n in to.compared(names)})
    for n, e in zip(names, z['e_ref']):
        if n in err:
            assert err[n] <= max(4 * float(e), TIGHT), (n, err[n])
        else:
            assert (got[n] == 0).all(), n
    es = rel_errors({k: v.cpu().numpy() for k, v in tr.batch_statistics(batch).items()}, {k: v.numpy() for k, v in s64.items()})
    for i, n in enumerate(to.BUFFERS):
        assert es[n] <= max(4 * float(z['e_ref_stats'][i]), TIGHT), (n, es[n])


@pytest.fixture(scope='module')
def trained():
    """10 training steps with injected masks on the B = 3 batch from the real checkpoint: (trainer, losses, batch)."""
    sd, batch, _, _ = point('b3')
    z = g('skel_train_traj.npz')
    sd['st_gcnns.0.tcn.1.num_batches_tracked'] = np.asarray(7, np.int64)
    tr = st.SkeletonTrainer(sd, dropout=float(z['p_drop']), seed=1, device=DEV)
    losses = [tr.training_step(batch, masks=torch.from_numpy(to.masks_for(int(z['seed_mask']), s, 3, float(z['p_drop'])))) for s in range(int(z['steps']))]
    return tr, np.asarray([float(l) for l in losses]), batch


@pytest.mark.gpu
def test_trajectory_against_the_reference(trained):
    """Measured on MI355X: losses within 1.5e-7 relative; 0 of 95,416 compared parameters beyond 8 y_traj = 1.08e-3 (max |diff| 1.04e-6); buffers within
    7.8e-5 of the reference's (8 y_stats = 6.5e-4)."""
    tr, losses, batch = trained
    z, names = g('skel_train_traj.npz'), [str(n) for n in g('skel_train_traj.npz')['names']]
    relv = np.abs(losses - z['traj_losses']) / z['traj_losses']
    ref, mine = split(g('skel_train.npz'), z['theta_final']), {n: v.detach().cpu().double().numpy().ravel() for n, v in tr.named_parameters().items()}
    diff = np.concatenate([np.abs(mine[n] - ref[n].astype(np.float64)) for n in to.compared(names)])
    count = int((diff > 8 * float(z['y_traj'])).sum())
    bdiff = np.abs(tr.bn.cpu().double().numpy() - z['buffers_final'].astype(np.float64)).max()
    print('trajectory: losses %s; max relative loss difference %.3e; parameters beyond 8 y_traj = %.3e: %d of %d (max |diff| %.3e); buffers max |diff| %.3e, 8 y_stats %.3e'
          % (' '.join('%.6f' % v for v in losses), relv.max(), 8 * float(z['y_traj']), count, diff.size, diff.max(), bdiff, 8 * float(z['y_stats'])))
    assert relv.max() <= 1e-5
    assert losses[9] < losses[0]
    assert count <= 96
    assert bdiff <= 8 * float(z['y_stats'])
    sd0 = ckpt()
    for n in to.CONV_BIASES:                                      # exact-zero gradients and weight_decay = 0: they have not moved
        assert np.array_equal(mine[n], np.asarray(sd0[n], np.float64).ravel()), n
    out = tr.state_dict()
    assert tr.step == 10 and out['st_gcnns.0.tcn.1.num_batches_tracked'].dtype == torch.int64 and int(out['st_gcnns.0.tcn.1.num_batches_tracked']) == 17
    assert np.array_equal(np.concatenate([out[k].numpy().ravel() for k in to.BUFFERS]), tr.bn.cpu().numpy())
    # the arena was re-folded with the new weights AND the new buffers: the live predictor is the eval() model of state_dict()
    live = sk.skeleton_validation_step(tr.predictor, batch)[0]
    fresh = sk.skeleton_validation_step(sk.SkeletonObjProjector(out, device=DEV), batch)[0]
    stale = dict(out)
    stale.update({k: torch.as_tensor(sd0[k]) for k in to.BUFFERS})
    old = sk.skeleton_validation_step(sk.SkeletonObjProjector(stale, device=DEV), batch)[0]
    assert abs(float(live) - float(fresh)) <= 1e-6 * float(fresh)
    assert abs(float(old) - float(fresh)) > 1e-4 * float(fresh)              # (the buffers matter to that number)


@pytest.mark.gpu
def test_train_mode_loss_is_the_eval_loss_on_the_batch_statistics():
    """No reference involved: with the batch's own statistics written into the running buffers, the EXISTING eval-mode validation step computes what
    the trainer's train-mode forward computes at p = 0."""
    sd, batch, _, _ = point('b3')
    tr = st.SkeletonTrainer(sd, dropout=0.0, seed=1, device=DEV)
    loss, ld, _, _ = tr.loss_and_grads(batch)
    sd2 = dict(sd)
    sd2.update({k: v.cpu().numpy() for k, v in tr.batch_statistics(batch).items()})
    out = sk.skeleton_validation_step(sk.SkeletonObjProjector(sd2, device=DEV), batch)
    assert abs(float(out[0]) - float(loss)) <= TERM_GATE * float(loss)
    for k in to.MSE_KEYS:
        assert abs(float(out[1][k]) - float(ld[k])) <= TERM_GATE * float(ld[k]), k


def snapshot(tr):
    return tr.params.clone(), tr.bn.clone(), tr.predictor.arena.clone()


@pytest.mark.gpu
def test_generator_route():
    sd, batch, _, _ = point('b3')
    a, b = st.SkeletonTrainer(sd, dropout=0.1, seed=77, device=DEV), st.SkeletonTrainer(sd, dropout=0.1, seed=77, device=DEV)
    m0, m1 = a.dropout_masks(3), a.dropout_masks(3, step=1)
    for step in range(2):
        mb = b.dropout_masks(3, step)
        la, lb = a.training_step(batch), b.training_step(batch, masks=mb)
        assert torch.equal(la, lb) and all(torch.equal(x, y) for x, y in zip(snapshot(a), snapshot(b))), step
    flat0, flat1 = torch.cat([v.reshape(-1) for v in m0.values()]).cpu().numpy(), torch.cat([v.reshape(-1) for v in m1.values()]).cpu().numpy()
    assert [tuple(v.shape) for v in m0.values()] == [(3, co, 20, v) for _, co, v in to.LAYERS] and list(m0) == [p for p, _, _ in to.LAYERS]
    assert set(np.unique(flat0)) == {0, 1} and flat0.size == 3 * to.MASK_CLIP
    n, keep = flat0.size, 0.9
    assert abs(flat0.mean() - keep) <= 5 * np.sqrt(keep * (1 - keep) / n)
    for v in m0.values():                                         # and per layer
        f = v.cpu().numpy().ravel()
        assert abs(f.mean() - keep) <= 5 * np.sqrt(keep * (1 - keep) / f.size)
    assert not np.array_equal(flat0, flat1) and abs((flat0 == flat1).mean() - (keep ** 2 + (1 - keep) ** 2)) <= 0.01
    again = torch.cat([v.reshape(-1) for v in st.SkeletonTrainer(sd, dropout=0.1, seed=77, device=DEV).dropout_masks(3).values()]).cpu().numpy()
    other = torch.cat([v.reshape(-1) for v in st.SkeletonTrainer(sd, dropout=0.1, seed=78, device=DEV).dropout_masks(3).values()]).cpu().numpy()
    assert np.array_equal(flat0, again) and not np.array_equal(flat0, other)
    # p = 0: an all-ones mask, and the same bits as no mask
    c, d = st.SkeletonTrainer(sd, dropout=0.0, seed=77, device=DEV), st.SkeletonTrainer(sd, dropout=0.0, seed=77, device=DEV)
    ones = c.dropout_masks(3)
    assert all(bool((v == 1).all()) for v in ones.values())
    assert torch.equal(c.training_step(batch), d.training_step(batch, masks=ones)) and all(torch.equal(x, y) for x, y in zip(snapshot(c), snapshot(d)))


@pytest.mark.gpu
def test_determinism_and_resume():
    sd, batch, _, _ = point('b3')
    tr = st.SkeletonTrainer(sd, dropout=0.1, seed=31, device=DEV)
    before = snapshot(tr)
    l1, _, _, g1 = tr.loss_and_grads(batch)
    l2, _, _, g2 = tr.loss_and_grads(batch)
    assert torch.equal(l1, l2) and all(torch.equal(g1[n], g2[n]) for n in g1)
    assert tr.step == 0 and all(torch.equal(x, y) for x, y in zip(before, snapshot(tr)))
    tr.training_step(batch)
    tr.training_step(batch)
    tr2 = st.SkeletonTrainer(tr.state_dict(), dropout=0.1, seed=999, device=DEV)
    tr2.load_optimizer_state(tr.optimizer_state())
    assert tr2.step == 2 and tr2.seed == 31 and torch.equal(tr2.params, tr.params) and torch.equal(tr2.bn, tr.bn)
    assert torch.equal(tr.training_step(batch), tr2.training_step(batch))
    assert all(torch.equal(x, y) for x, y in zip(snapshot(tr), snapshot(tr2)))
    assert torch.equal(tr.exp_avg, tr2.exp_avg) and torch.equal(tr.exp_avg_sq, tr2.exp_avg_sq)


@pytest.mark.gpu
def test_argument_checks():
    sd, batch, _, masks = point('b3')
    tr = st.SkeletonTrainer(sd, dropout=0.1, seed=1, device=DEV)
    with pytest.raises(ValueError):
        tr.loss_and_grads(tuple(a[:, :19] if a.dim() > 3 or a.shape[-1] == 7 else a for a in batch))          # T = 19
    with pytest.raises(ValueError):
        tr.loss_and_grads(batch, masks=torch.from_numpy(masks[:-1]))
    md = {k: torch.from_numpy(v) for k, v in to.split_masks(masks, 3).items()}
    md['st_gcnns.1'] = md['st_gcnns.1'][:2]
    with pytest.raises(ValueError):
        tr.training_step(batch, masks=md)
    with pytest.raises(ValueError):
        st.SkeletonTrainer(sd, dropout=1.0, device=DEV)
    tr.dropout = 1.5                                                                                            # past the constructor: the library refuses it
    with pytest.raises(ValueError):
        tr.loss_and_grads(batch)
    tr.dropout = 0.1
    tr._tws = {3: torch.empty(1024, dtype=torch.uint8, device=DEV)}                                             # a short workspace: IDF_E_INVAL
    with pytest.raises(ValueError):
        tr.loss_and_grads(batch)
    assert tr.step == 0
