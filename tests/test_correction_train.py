"""Training of the SMPL correction predictor with batch statistics, dropout and drawn contact nodes (interdiff_amd/correction_train.py,
csrc/objproj_bn_train.h / .hip, csrc/stgcn_bn_train.h) against the reference's own module in train() (tests/golden/corr_train.npz,
corr_train_traj.npz; tests/golden/make_golden_correction_train.py) and the fp64 restatement tests/correction_train_oracle.py.

Gates (none of them comes from the code under test; they are those of tests/test_skeleton_train.py and tests/test_correction_finetune.py):
  gradient    per compared tensor e = max|g - g64| / max|g64| <= max(4 e_ref, 1e-5); compared = named_parameters() without the 24 convolution
              biases, whose gradient must be exactly 0
  statistics  batch statistics and updated buffers per buffer tensor <= max(4 e_ref_stats, 1e-5) resp. max(4 e_ref_buffers, 1e-5)
  loss        the 1e-4 per-term gate
  trajectory  losses within 1e-5 relative of the reference's at every step; at most 224 compared parameters (0.1 %) further than 8 y_traj from the
              reference's; final buffers within 8 y_stats
  zeros       the gradient of st_gcnns_all.3.gcn.A has the reference's zero pattern, which in train() is EMPTY at every recorded point (the last
              layer's batch-normalisation backward spreads the selected node's gradient over every node)
"""
import functools
import numpy as np
import pytest
import torch
from tests import fixtures as fx
from tests import corr_fixtures as cf
from tests import correction_train_oracle as to
from interdiff_amd import correction_finetune as cft
from interdiff_amd import correction_train as ct
from interdiff_amd.objprojector import ObjProjector, HAND_MARKERS
from interdiff_amd.skeleton_finetune import flatten

DEV = 'cuda'
TIGHT, TERM_GATE = 1e-5, 1e-4
ZERO_TENSOR = 'st_gcnns_all.3.gcn.A'
N_PARAM = 224174
POINTS = ('i1', 'i0', 'b1')


@functools.lru_cache(None)
def g(name):
    z = fx.golden(name)
    return {k: z[k] for k in z.files}


def ckpt():
    """The real checkpoint with ``num_batches_tracked`` at 0 (where the recorder's reference module starts)."""
    sd = dict(g('correction_ckpt.npz'))
    for k in sd:
        if k.endswith('num_batches_tracked'):
            sd[k] = np.zeros((), np.int64)
    return sd


@functools.lru_cache(None)
def scene():
    sc = cf.scene()
    z = g('corr_train.npz')
    for k, v in sc.items():
        assert cf.checksum(v) == z['crc_' + k], k
    return sc


def clip_of(sc, b):
    return {k: np.ascontiguousarray(v[b:b + 1] if k == 'obj_points' else v[:, b:b + 1]) for k, v in sc.items()}


def as_batch(sc):
    """The stacked-tensor form of the batch ``ObjProjector.forward`` takes."""
    return {k: torch.from_numpy(sc[k]) for k in ('obj_angle', 'obj_trans', 'markers')}


def point(which):
    """-> (state_dict, scene arrays, initialize, nodes or None, extra gradient or None, flat masks, fixture dict, key prefix)."""
    z, pre = g('corr_train.npz'), which + '_'
    p = float(z['p_drop'])
    if which == 'i1':
        sd, sc, nodes, extra = ckpt(), scene(), None, None
    elif which == 'i0':
        sd, sc, nodes, extra = ckpt(), scene(), [int(n) for n in z['i0_nodes']], to.extra_gradient(int(z['i0_seed_extra']), cf.T, cf.B)
    else:
        sd, sc = to.perturbed(ckpt(), int(z['b1_seed_perturb']), float(z['b1_rel'])), clip_of(scene(), int(z['b1_clip']))
        nodes, extra = [int(n) for n in z['b1_nodes']], None
    B = sc['obj_angle'].shape[1]
    return sd, sc, which == 'i1', nodes, extra, to.masks_for(int(z[pre + 'seed_mask']), 0, B, p), z, pre


@functools.lru_cache(None)
def oracle_point(which):
    """fp64 loss, terms, gradients, batch statistics and updated buffers of a fixture point, computed once and shared."""
    sd, sc, initialize, nodes, extra, masks, z, _ = point(which)
    loss, terms, grads, stats = to.loss_and_grads(to.leaves(sd), sc, initialize, nodes, masks, float(z['p_drop']), extra)
    buf = to.updated_buffers({k: torch.from_numpy(np.asarray(sd[k], np.float64)) for k in to.BUFFERS}, stats, sc['obj_angle'].shape[1])
    return float(loss), {k: float(v) for k, v in terms.items()}, {k: v.numpy() for k, v in grads.items()}, {k: v.numpy() for k, v in stats.items()}, \
        {k: v.numpy() for k, v in buf.items()}


def split(z, flat, kind=''):
    return {str(n): flat[o:o + s] for n, o, s in zip(z['names' + kind], z['offsets' + kind], z['sizes' + kind])}


def rel_errors(got, want):
    return {n: float(np.abs(np.asarray(got[n], np.float64).ravel() - want[n].ravel()).max() / np.abs(want[n]).max()) for n in want}


# ------------------------------------------------------------------------------------------------------------ CPU

@pytest.mark.parametrize('which', POINTS)
def test_oracle_against_the_reference(which):
    sd, sc, initialize, nodes, _, _, z, pre = point(which)
    loss64, terms64, g64, s64, b64 = oracle_point(which)
    assert abs(loss64 - float(z[pre + 'loss'])) <= 1e-5 * loss64 and abs(loss64 - float(z[pre + 'loss64'])) <= 1e-12
    for k, v in zip(to.MSE_KEYS, z[pre + 'terms']):
        assert abs(terms64[k] - float(v)) <= 1e-5 * terms64[k], k
    names = [str(n) for n in z['names']]
    assert names == list(g64) and len(to.compared(names)) == len(names) - 24
    flat64 = np.concatenate([g64[n].ravel() for n in names])
    assert flat64.size == N_PARAM and z[pre + 'g8'].size == flat64[::8].size
    diff8 = np.abs(z[pre + 'g8'].astype(np.float64) - flat64[::8])            # every 8th entry of the reference's fp32 gradient is what is recorded
    idx = np.arange(0, N_PARAM, 8)
    for i, (n, o, s) in enumerate(zip(names, z['offsets'], z['sizes'])):
        sel = (idx >= o) & (idx < o + s)
        if n in to.CONV_BIASES:
            assert np.isnan(z[pre + 'e_ref'][i])
            assert np.abs(g64[n]).max() <= 1e-12 * np.abs(g64[n[:-4] + 'weight']).max(), n
            continue
        e = float(z[pre + 'e_ref'][i])
        assert 4 * e <= 1e-4, (n, e)
        if sel.any():
            assert diff8[sel].max() / np.abs(g64[n]).max() <= 1.01 * e + 1e-12, n          # the recorded e_ref IS this comparison, over the whole tensor
    assert float(z[pre + 'bias_ratio'].max()) <= 1e-5
    assert int(z[pre + 'zeros_A']) == 0 and not (g64[ZERO_TENSOR] == 0).any()
    for kind, want, key in (('stats', s64, 'e_ref_stats'), ('buffers_after', b64, 'e_ref_buffers')):
        err = rel_errors(split(z, z[pre + kind], '_buffers'), want)
        for i, n in enumerate(to.BUFFERS):
            assert err[n] <= 1.01 * float(z[pre + key][i]) + 1e-12 and 4 * err[n] <= 1e-4, (kind, n, err[n])
    if nodes is not None:                                          # the injected nodes are ones the reference could have drawn, and not all the argmax ones
        w, arg = to.node_weights(sc), to.argmax_nodes(sc)
        assert all((n == 0 and a == 0) or (n > 0 and a > 0 and w[b, n - 1] > 0) for b, (n, a) in enumerate(zip(nodes, arg)))
        assert any(n != a for n, a in zip(nodes, arg))
    if which == 'i0':
        assert any(n > 0 and w[b, n - 1] == 0.5 for b, n in enumerate(nodes))                # a hand marker on its bonus alone


def test_oracle_trajectory_against_the_reference():
    z = g('corr_train_traj.npz')
    losses, theta, buf = to.adam_trajectory_train(ckpt(), scene(), int(z['steps']), int(z['seed_mask']), float(z['p_drop']), True, None, float(z['lr']),
                                                  float(z['weight_decay']))
    assert (np.abs(losses - z['traj_losses']) / losses).max() <= 1e-6 and losses[-1] < losses[0]
    assert np.abs(losses - z['traj_losses64']).max() <= 1e-12
    names = [str(n) for n in z['names']]
    ref = split(g('corr_train.npz'), z['theta_final'])
    y = max(np.abs(theta[n].numpy().ravel() - ref[n].astype(np.float64)).max() for n in to.compared(names))
    assert abs(y - float(z['y_traj'])) <= 0.01 * float(z['y_traj'])
    ys = np.abs(np.concatenate([buf[k].numpy().ravel() for k in to.BUFFERS]) - z['buffers_final'].astype(np.float64)).max()
    assert abs(ys - float(z['y_stats'])) <= 0.01 * float(z['y_stats'])
    sd = ckpt()
    for n in to.CONV_BIASES:                                       # exact-zero gradients: Adam leaves these where they were
        assert np.array_equal(theta[n].numpy(), np.asarray(sd[n], np.float64)), n
    assert int(z['tracked']) == 10


def test_batchnorm_train_backward_against_autograd():
    """The formula of the kernels (numpy fp64) against autograd on a [2, 9, 10, 68] block: convolution + train-mode BatchNorm2d + mask."""
    torch.set_grad_enabled(True)                               # (other test modules switch autograd off process-wide)
    rs = np.random.RandomState(7620)
    n, cin, cout, t_, v = 2, 5, 9, 10, 68
    t = lambda *s: torch.from_numpy(rs.standard_normal(s))
    x, Rw = t(n, cin, t_, v), t(n, cout, t_, v)
    mask = torch.from_numpy((rs.random_sample((n, cout, t_, v)) >= 0.1).astype(np.float64) * to.drop_scale(0.1))
    W, b, gamma, beta = (t(cout, cin).requires_grad_(), t(cout).requires_grad_(), t(cout).requires_grad_(), t(cout).requires_grad_())
    c = torch.einsum('oc,nctv->notv', W, x) + b.reshape(1, -1, 1, 1)
    y = torch.nn.functional.batch_norm(c, None, None, gamma, beta, training=True, eps=to.BN_EPS) * mask
    want = torch.autograd.grad((y * Rw).sum(), [W, b, gamma, beta])
    flat = lambda a: a.detach().permute(1, 0, 2, 3).reshape(a.shape[1], -1).numpy()          # [channel, all elements of the batch]
    dc, dgamma, dbeta = to.bn_train_backward(flat(Rw * mask), flat(c), gamma.detach().numpy())
    got = (dc @ flat(x).T, dc.sum(axis=1), dgamma, dbeta)
    scale = np.abs(want[0].numpy()).max()
    for a, w, s in zip(got, want, (scale, scale, None, None)):
        assert np.abs(a - w.numpy()).max() <= 1e-12 * (s or np.abs(w.numpy()).max())
    assert np.abs(got[1]).max() <= 1e-12 * scale                # the convolution bias cancels


def test_init_state_dict():
    ref = ckpt()
    sd = ct.init_state_dict(11)
    assert list(sd) == list(ref)
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
    again, other = ct.init_state_dict(11), ct.init_state_dict(12)
    assert all(torch.equal(sd[k], again[k]) for k in sd) and not torch.equal(sd['st_gcnns.0.gcn.T'], other['st_gcnns.0.gcn.T'])
    tr = ct.CorrectionTrainer(sd, T=cf.T, past_len=cf.PAST, seed=5, device='cpu')       # the packer and the library's parameter table take it
    assert tr.n_param == N_PARAM and tr.mask_clip == to.MASK_CLIP == 121040 and list(tr.state_dict()) == list(sd)
    for bad in (dict(dropout=1.0), dict(dropout=-0.1), dict(momentum=1.5), dict(momentum=-0.1)):
        with pytest.raises(ValueError):
            ct.CorrectionTrainer(sd, T=cf.T, past_len=cf.PAST, device='cpu', **bad)


def test_mask_layout_round_trip():
    tr = ct.CorrectionTrainer(ckpt(), T=cf.T, past_len=cf.PAST, seed=5, device='cpu')
    assert [(n, co, v) for n, co, v in tr.layers] == to.LAYERS
    B = 2
    flat = to.masks_for(7630, 0, B, 0.3)
    md = tr.split_masks(torch.from_numpy(flat), B)
    want = to.split_masks(flat, B)
    assert list(md) == [p for p, _, _ in to.LAYERS]
    for p, co, v in to.LAYERS:
        assert tuple(md[p].shape) == (B, co, 10, v) and np.array_equal(md[p].numpy(), want[p]), p
    assert np.array_equal(tr._mask_buffer(md, B).numpy(), flat) and np.array_equal(tr._mask_buffer(torch.from_numpy(flat * 7), B).numpy(), flat)
    with pytest.raises(ValueError):
        tr._mask_buffer(torch.from_numpy(flat[:-1]), B)
    md['st_gcnns.1'] = md['st_gcnns.1'][:1]
    with pytest.raises(ValueError):
        tr._mask_buffer(md, B)


def contact_of(sc):
    return torch.from_numpy(sc['markers'][cf.PAST:, :, :, 6].sum(axis=0)).to(torch.int32)


def test_nodes_validation():
    sc = scene()
    contact, arg, w = contact_of(sc), to.argmax_nodes(sc), to.node_weights(sc)
    assert ct.check_nodes(arg, contact).tolist() == arg and ct.check_nodes(torch.tensor(arg), contact).dtype == torch.int32
    assert np.array_equal(ct.node_weights(contact).numpy(), w.astype(np.float32))
    dead = next(m for m in range(67) if w[1, m] == 0)                       # a marker of clip 1 that is neither in contact nor a hand marker
    for bad in ([1] + arg[1:],                                             # clip 0 has no contact: only node 0
                [0, 0] + arg[2:],                                          # clip 1 has contact: not node 0
                arg[:1] + [68] + arg[2:], arg[:1] + [-1] + arg[2:],        # out of range
                arg[:1] + [1 + dead] + arg[2:],                            # weight 0: the reference cannot draw it
                arg[:3], [float(a) for a in arg], [arg]):                  # count, dtype, shape
        with pytest.raises(ValueError):
            ct.check_nodes(bad, contact)


def test_seeded_node_draw():
    sc = scene()
    contact, w = contact_of(sc), to.node_weights(sc)
    a, again, other_step, other_seed = (ct.draw_nodes(contact, *k) for k in ((41, 3), (41, 3), (41, 4), (42, 3)))
    assert a.dtype == torch.int32 and a.tolist() == again.tolist() and int(a[0]) == 0
    many = torch.stack([ct.draw_nodes(contact, 41, s) for s in range(40)]).numpy()
    assert (many[:, 0] == 0).all() and (many[:, 1:] >= 1).all() and (many[:, 1:] <= 67).all()
    for b in range(1, cf.B):
        assert (w[b, many[:, b] - 1] > 0).all()                             # only what the reference could draw
    assert len({tuple(r) for r in many}) > 1 and (a.tolist() != other_step.tolist() or a.tolist() != other_seed.tolist())
    # 4,000 draws of clip 1 in one call: its three contact markers (5, 20 and hand marker 10) and the other hand markers on their bonus
    n = 4000
    rows = contact[1:2].repeat(n, 1)
    d = ct.draw_nodes(rows, 7, 0).numpy() - 1
    assert np.array_equal(d, ct.draw_nodes(rows, 7, 0).numpy() - 1)
    p = w[1] / w[1].sum()
    freq = np.bincount(d, minlength=67) / n
    assert (freq[p == 0] == 0).all()
    assert (np.abs(freq - p) <= 5 * np.sqrt(p * (1 - p) / n) + 1e-12).all(), np.abs(freq - p).max()
    assert set(np.flatnonzero(p > 0)) == set(cf.TIE_MARKERS) | set(HAND_MARKERS)


# ------------------------------------------------------------------------------------------------------------ GPU

def trainer(sd, **kw):
    kw.setdefault('seed', 1)
    return ct.CorrectionTrainer(sd, T=cf.T, past_len=cf.PAST, device=DEV, **kw)


def check_point(which):
    """Measured on MI355X (the six tensors closest to their gates are printed).  i1: loss 0.00488446 (reference 0.00488447), closest to its gate
    st_gcnns_relative.3.residual.1.bias, e 1.03e-6 against 1.00e-5, max e 3.1e-6.  i0: st_gcnns_all.0.prelu.weight, e 3.31e-6 against 1.00e-5.  b1: loss 0.01897923
    (0.01897920), st_gcnns_all.3.residual.1.weight, e 3.48e-6 against 1.24e-5, max e 4.7e-6.  Statistics / buffers e at most 4.8e-7 / 6.3e-8."""
    sd, sc, initialize, nodes, extra, masks, z, pre = point(which)
    _, _, g64, s64, b64 = oracle_point(which)
    p, batch = float(z['p_drop']), as_batch(sc)
    tr = trainer(sd, dropout=p)
    kw = dict(masks=torch.from_numpy(masks), nodes=nodes, d_obj_pred=None if extra is None else torch.from_numpy(extra))
    loss, ld, wd, grads = tr.loss_and_grads(batch, initialize, **kw)
    got = {n: v.detach().cpu().numpy() for n, v in grads.items()}
    assert abs(float(loss) - float(z[pre + 'loss'])) <= TERM_GATE * float(z[pre + 'loss'])
    for k, v in zip(to.MSE_KEYS, z[pre + 'terms']):
        assert abs(float(ld[k]) - float(v)) <= TERM_GATE * float(v), k
    assert abs(float(sum(wd.values())) - float(loss)) <= 1e-6 * float(loss)
    names = list(g64)
    for n in to.CONV_BIASES:
        assert (got[n] == 0).all(), n
    cmp_ = to.compared(names)
    err = rel_errors(got, {n: g64[n] for n in cmp_})
    gates = {n: max(4 * float(e), TIGHT) for n, e in zip(names, z[pre + 'e_ref']) if n in cmp_}
    order = sorted(err, key=lambda n: -err[n] / gates[n])
    print('%s: loss %.8f (reference %.8f); max e %.3e' % (which, float(loss), float(z[pre + 'loss']), max(err.values())))
    for n in order[:6]:
        print('    %-40s e %.3e  gate %.3e' % (n, err[n], gates[n]))
    missed = {n: (err[n], gates[n]) for n in cmp_ if err[n] > gates[n]}
    assert not missed, missed
    assert all(tuple(grads[n].shape) == g64[n].shape for n in names)
    assert not (got[ZERO_TENSOR] == 0).any()                      # the reference's zero pattern in train(): empty
    # loss_and_grads left the buffers alone; the update alone, with the statistics
    assert np.array_equal(tr.bn.cpu().numpy(), flatten(sd, tr.btable)) and tr.step == 0
    ws = tr._train_grads(batch, initialize, update=True, want_stats=True, **kw)[2]
    stats = {n: ws[o:o + int(np.prod(s))].cpu().numpy() for n, o, s in tr.btable}
    es, eb = rel_errors(stats, s64), rel_errors({k: v.cpu().numpy() for k, v in tr.buffers().items()}, b64)
    print('    batch statistics: max e %.3e; updated buffers: max e %.3e' % (max(es.values()), max(eb.values())))
    for i, n in enumerate(to.BUFFERS):
        assert es[n] <= max(4 * float(z[pre + 'e_ref_stats'][i]), TIGHT), (n, es[n])
        assert eb[n] <= max(4 * float(z[pre + 'e_ref_buffers'][i]), TIGHT), (n, eb[n])


@pytest.mark.gpu
@pytest.mark.parametrize('which', POINTS)
def test_gradients_statistics(which):
    check_point(which)


@pytest.mark.gpu
def test_b2_without_dropout_against_the_oracle():
    """No fixture: the oracle is the judge, with the gates of the i0 point.  B = 2 is the smallest real Chan merge (clips 1 and 2, their argmax nodes)."""
    sd, z = ckpt(), g('corr_train.npz')
    sc = {k: np.ascontiguousarray(v[1:3] if k == 'obj_points' else v[:, 1:3]) for k, v in scene().items()}
    nodes = to.argmax_nodes(sc)
    loss64, terms64, g64, s64 = to.loss_and_grads(to.leaves(sd), sc, False, nodes)
    tr = trainer(sd, dropout=0.0)
    loss, ld, _, grads = tr.loss_and_grads(as_batch(sc), False, nodes=nodes)
    assert abs(float(loss) - float(loss64)) <= TERM_GATE * float(loss64)
    for k in to.MSE_KEYS:
        assert abs(float(ld[k]) - float(terms64[k])) <= TERM_GATE * float(terms64[k]), k
    names = list(g64)
    got = {n: v.cpu().numpy() for n, v in grads.items()}
    err = rel_errors(got, {n: g64[n].numpy() for n in to.compared(names)})
    print('B = 2, p = 0: loss %.8f (oracle %.8f); max e %.3e' % (float(loss), float(loss64), max(err.values())))
    for n, e in zip(names, z['i0_e_ref']):
        if n in err:
            assert err[n] <= max(4 * float(e), TIGHT), (n, err[n])
        else:
            assert (got[n] == 0).all(), n
    es = rel_errors({k: v.cpu().numpy() for k, v in tr.batch_statistics(as_batch(sc)).items()}, {k: v.numpy() for k, v in s64.items()})
    for i, n in enumerate(to.BUFFERS):
        assert es[n] <= max(4 * float(z['i0_e_ref_stats'][i]), TIGHT), (n, es[n])


@pytest.fixture(scope='module')
def trained():
    """10 training steps at epoch 0 with injected masks on the scene from the real checkpoint: (trainer, losses, batch)."""
    z = g('corr_train_traj.npz')
    tr = trainer(ckpt(), dropout=float(z['p_drop']))
    batch = as_batch(scene())
    losses = [tr.training_step(batch, 0, masks=torch.from_numpy(to.masks_for(int(z['seed_mask']), s, cf.B, float(z['p_drop'])))) for s in range(int(z['steps']))]
    return tr, np.asarray([float(l) for l in losses]), batch


@pytest.mark.gpu
def test_trajectory_against_the_reference(trained):
    """Measured on MI355X: losses within 1.3e-6 relative; 0 of 223,640 compared parameters beyond 8 y_traj = 2.08e-5 (max |diff| 3.0e-6); buffers within
    1.75e-4 of the reference's (8 y_stats = 1.40e-3)."""
    tr, losses, batch = trained
    z, names = g('corr_train_traj.npz'), [str(n) for n in g('corr_train_traj.npz')['names']]
    relv = np.abs(losses - z['traj_losses']) / z['traj_losses']
    ref, mine = split(g('corr_train.npz'), z['theta_final']), {n: v.detach().cpu().double().numpy().ravel() for n, v in tr.named_parameters().items()}
    diff = np.concatenate([np.abs(mine[n] - ref[n].astype(np.float64)) for n in to.compared(names)])
    count = int((diff > 8 * float(z['y_traj'])).sum())
    bdiff = np.abs(tr.bn.cpu().double().numpy() - z['buffers_final'].astype(np.float64)).max()
    print('trajectory: losses %s; max relative loss difference %.3e; parameters beyond 8 y_traj = %.3e: %d of %d (max |diff| %.3e); buffers max |diff| %.3e, 8 y_stats %.3e'
          % (' '.join('%.6f' % v for v in losses), relv.max(), 8 * float(z['y_traj']), count, diff.size, diff.max(), bdiff, 8 * float(z['y_stats'])))
    assert relv.max() <= 1e-5
    assert losses[9] < losses[0]
    assert count <= 224
    assert bdiff <= 8 * float(z['y_stats'])
    sd0 = ckpt()
    for n in to.CONV_BIASES:                                      # exact-zero gradients and weight_decay = 0: they have not moved
        assert np.array_equal(mine[n], np.asarray(sd0[n], np.float64).ravel()), n
    out = tr.state_dict()
    tracked = [k for k in out if k.endswith('num_batches_tracked')]
    assert tr.step == 10 and len(tracked) == 24 and all(out[k].dtype == torch.int64 and int(out[k]) == 10 for k in tracked)
    assert list(out) == list(sd0) and np.array_equal(np.concatenate([out[k].numpy().ravel() for k in to.BUFFERS]), tr.bn.cpu().numpy())
    # the arena was re-folded with the new weights AND the new buffers: the live predictor is the eval() model of state_dict(), bit for bit
    fresh = ObjProjector(out, cf.T, cf.PAST, device=DEV)
    for initialize in (True, False):
        assert torch.equal(tr.predictor.forward(batch, initialize)[0], fresh.forward(batch, initialize)[0]), initialize
    stale = dict(out)
    stale.update({k: torch.as_tensor(sd0[k]) for k in to.BUFFERS})
    old = ObjProjector(stale, cf.T, cf.PAST, device=DEV).forward(batch, True)[0]
    assert float((old - fresh.forward(batch, True)[0]).abs().max()) > 1e-4              # (the buffers matter to that prediction)


@pytest.mark.gpu
def test_train_mode_loss_is_the_eval_loss_on_the_batch_statistics():
    """No reference involved: with the batch's own statistics written into the running buffers, the EXISTING eval-mode fine-tuner computes the loss the
    trainer's train-mode forward computes at p = 0 -- at the 68-node mean, and at the argmax nodes (the fine-tuner's own rule)."""
    sd, sc = ckpt(), scene()
    batch = as_batch(sc)
    tr = trainer(sd, dropout=0.0)
    sd2 = dict(sd)
    sd2.update({k: v.cpu().numpy() for k, v in tr.batch_statistics(batch).items()})
    ft = cft.CorrectionFineTuner(sd2, T=cf.T, past_len=cf.PAST, device=DEV)
    for initialize in (True, False):
        loss, ld, _, _ = tr.loss_and_grads(batch, initialize, nodes=None if initialize else to.argmax_nodes(sc))
        want, wd, _, _ = ft.loss_and_grads(batch, initialize)
        assert abs(float(want) - float(loss)) <= 1e-5 * float(loss), initialize
        for k in to.MSE_KEYS:
            assert abs(float(wd[k]) - float(ld[k])) <= TERM_GATE * float(ld[k]), k


def snapshot(tr):
    return tr.params.clone(), tr.bn.clone(), tr.predictor.arena.clone()


@pytest.mark.gpu
def test_generator_route():
    sd, batch = ckpt(), as_batch(scene())
    B = cf.B
    a, b = trainer(sd, dropout=0.1, seed=77), trainer(sd, dropout=0.1, seed=77)
    m0, m1 = a.dropout_masks(B), a.dropout_masks(B, step=1)
    for step in range(2):
        mb = b.dropout_masks(B, step)
        la, lb = a.training_step(batch), b.training_step(batch, masks=mb)
        assert torch.equal(la, lb) and all(torch.equal(x, y) for x, y in zip(snapshot(a), snapshot(b))), step
    flat0, flat1 = torch.cat([v.reshape(-1) for v in m0.values()]).cpu().numpy(), torch.cat([v.reshape(-1) for v in m1.values()]).cpu().numpy()
    assert [tuple(v.shape) for v in m0.values()] == [(B, co, 10, v) for _, co, v in to.LAYERS] and list(m0) == [p for p, _, _ in to.LAYERS]
    assert set(np.unique(flat0)) == {0, 1} and flat0.size == B * to.MASK_CLIP
    n, keep = flat0.size, 0.9
    assert abs(flat0.mean() - keep) <= 5 * np.sqrt(keep * (1 - keep) / n)
    for v in m0.values():                                         # and per layer
        f = v.cpu().numpy().ravel()
        assert abs(f.mean() - keep) <= 5 * np.sqrt(keep * (1 - keep) / f.size)
    assert not np.array_equal(flat0, flat1) and abs((flat0 == flat1).mean() - (keep ** 2 + (1 - keep) ** 2)) <= 0.01
    again = torch.cat([v.reshape(-1) for v in trainer(sd, dropout=0.1, seed=77).dropout_masks(B).values()]).cpu().numpy()
    other = torch.cat([v.reshape(-1) for v in trainer(sd, dropout=0.1, seed=78).dropout_masks(B).values()]).cpu().numpy()
    assert np.array_equal(flat0, again) and not np.array_equal(flat0, other)
    # p = 0: an all-ones mask, and the same bits as no mask
    c, d = trainer(sd, dropout=0.0, seed=77), trainer(sd, dropout=0.0, seed=77)
    ones = c.dropout_masks(B)
    assert all(bool((v == 1).all()) for v in ones.values())
    assert torch.equal(c.training_step(batch), d.training_step(batch, masks=ones)) and all(torch.equal(x, y) for x, y in zip(snapshot(c), snapshot(d)))


@pytest.mark.gpu
def test_determinism_resume_and_drawn_nodes():
    sd, batch = ckpt(), as_batch(scene())
    tr = trainer(sd, dropout=0.1, seed=31)
    before = snapshot(tr)
    l1, _, _, g1 = tr.loss_and_grads(batch)
    l2, _, _, g2 = tr.loss_and_grads(batch)
    assert torch.equal(l1, l2) and all(torch.equal(g1[n], g2[n]) for n in g1)
    assert tr.step == 0 and all(torch.equal(x, y) for x, y in zip(before, snapshot(tr)))
    # nodes=None at initialize=False draws them from (seed, step): the same bits as injecting that draw
    contact = contact_of(scene()).to(DEV)
    drawn = ct.draw_nodes(contact, 31, 0)
    assert drawn.device.type == 'cuda' and int(drawn[0]) == 0 and bool((drawn[1:] >= 1).all())
    l3, _, _, g3 = tr.loss_and_grads(batch, nodes=drawn)
    assert torch.equal(l1, l3) and all(torch.equal(g1[n], g3[n]) for n in g1)
    # epoch 10: initialize False, drawn nodes; the contact / penetration gradient comes in through the seam (zeros here)
    seam = torch.zeros(cf.T, cf.B, 9)
    ref = trainer(sd, dropout=0.1, seed=31)
    for _ in range(5):
        ref.training_step(batch, 10, d_obj_pred=seam)
    for _ in range(3):
        tr.training_step(batch, 10, d_obj_pred=seam)
    tr2 = trainer(tr.state_dict(), dropout=0.1, seed=999)
    tr2.load_optimizer_state(tr.optimizer_state())
    assert tr2.step == 3 and tr2.seed == 31 and torch.equal(tr2.params, tr.params) and torch.equal(tr2.bn, tr.bn)
    for _ in range(2):
        tr2.training_step(batch, 10, d_obj_pred=seam)
    assert all(torch.equal(x, y) for x, y in zip(snapshot(ref), snapshot(tr2)))
    assert torch.equal(ref.exp_avg, tr2.exp_avg) and torch.equal(ref.exp_avg_sq, tr2.exp_avg_sq)
    with pytest.raises(ValueError):
        tr.training_step(batch, 10)                                                                              # geometry weights, no d_obj_pred
    assert tr.step == 3


@pytest.mark.gpu
def test_argument_checks():
    sd, sc, _, nodes, _, masks, _, _ = point('i0')
    batch = as_batch(sc)
    tr = trainer(sd, dropout=0.1)
    with pytest.raises(ValueError):
        tr.loss_and_grads({k: v[:34] for k, v in batch.items()})                                                  # T = 34
    with pytest.raises(ValueError):
        tr.loss_and_grads(batch, masks=torch.from_numpy(masks[:-1]))
    md = {k: torch.from_numpy(v) for k, v in to.split_masks(masks, cf.B).items()}
    md['st_gcnns.1'] = md['st_gcnns.1'][:2]
    with pytest.raises(ValueError):
        tr.training_step(batch, masks=md)
    for bad in ([1] + nodes[1:], nodes[:1] + [68] + nodes[2:], nodes[:3]):
        with pytest.raises(ValueError):
            tr.loss_and_grads(batch, nodes=bad)
    tr.loss_and_grads(batch, True, nodes=[1] + nodes[1:])                                                         # initialize: nodes are ignored
    with pytest.raises(ValueError):
        tr.loss_and_grads(batch, d_obj_pred=torch.zeros(cf.T, cf.B, 8))
    with pytest.raises(ValueError):
        trainer(sd, dropout=1.0)
    with pytest.raises(ValueError):
        trainer(sd, momentum=1.5)
    tr.dropout = 1.5                                                                                            # past the constructor: the library refuses it
    with pytest.raises(ValueError):
        tr.loss_and_grads(batch)
    tr.dropout, tr.momentum = 0.1, -0.5
    with pytest.raises(ValueError):
        tr.loss_and_grads(batch)
    tr.momentum = 0.1
    tr._tws = {cf.B: torch.empty(1024, dtype=torch.uint8, device=DEV)}                                           # a short workspace: IDF_E_INVAL
    with pytest.raises(ValueError):
        tr.loss_and_grads(batch)
    long = ct.CorrectionTrainer(sd, T=65, past_len=cf.PAST, device=DEV)                                           # T > 64: the head's LDS vectors
    rs = np.random.RandomState(7640)
    wide = dict(obj_angle=torch.from_numpy(0.1 * rs.standard_normal((65, 1, 3)).astype(np.float32)), obj_trans=torch.zeros(65, 1, 3),
                markers=torch.zeros(65, 1, 67, 7))
    with pytest.raises(ValueError):
        long.loss_and_grads(wide, True)
    assert tr.step == 0
