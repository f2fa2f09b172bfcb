"""Fine-tuning of the SMPL contact-frame correction predictor under the object-pose loss, with frozen normalisation statistics
(interdiff_amd/correction_finetune.py, csrc/objproj_train.h / .hip, csrc/stgcn_train.h) against the reference's own autograd and
torch.optim.Adam with the real checkpoint (tests/golden/corr_finetune*.npz; tests/golden/make_golden_correction_finetune.py) and the fp64
restatement tests/correction_finetune_oracle.py.  Inputs: tests/corr_fixtures.scene() (T = 35, B = 4), rebuilt from its seed.

Gates (the project's own, from tests/test_skeleton_finetune.py; none of them comes from the code under test):
  gradient    per parameter tensor e = max|g - g64| / max|g64| <= max(4 e_ref, 1e-5): e_ref is the same quantity for the reference's fp32
              autograd (recorded per point and objective); factor 4 for another summation order at the same fp32 depth; 1e-5 = the project's tight gate
  zeros       initialize False: exact zeros in the columns of st_gcnns_all.3.gcn.A that no clip selects, and only there; initialize True: none
  loss        1e-4 relative for the loss and each term
  trajectory  losses within 1e-5 relative of the reference's at every step; at most 224 parameters (0.1 %) further than 8 y_traj from the
              reference's, y_traj = max|theta32 - theta64| of the reference against the oracle (recorded)
  Adam        each step's parameter change within 2^-20 relative of torch's change plus one ulp of the parameter
"""
import functools
import numpy as np
import pytest
import torch
from tests import fixtures as fx
from tests import corr_fixtures as cf
from tests import correction_finetune_oracle as fo
from interdiff_amd import correction_finetune as cft
from interdiff_amd import correction_losses as cl
from interdiff_amd.objprojector import ObjProjector, pack_objprojector

DEV = 'cuda'
TIGHT, TERM_GATE = 1e-5, 1e-4
ZERO_TENSOR = 'st_gcnns_all.3.gcn.A'
N_PARAM, N_TENSORS = 224174, 124
POINTS = ('i0', 'i1', 'b1', 'x')


@functools.lru_cache(None)
def g(name):
    z = fx.golden(name)
    return {k: z[k] for k in z.files}


def ckpt():
    return dict(g('correction_ckpt.npz'))


@functools.lru_cache(None)
def scene():
    sc = cf.scene()
    z = g('corr_finetune.npz')
    for k, v in sc.items():
        assert cf.checksum(v) == z['crc_' + k], k
    return sc


def clip_of(sc, b):
    return {k: np.ascontiguousarray(v[b:b + 1] if k == 'obj_points' else v[:, b:b + 1]) for k, v in sc.items()}


def tiled(sc, n):
    return {k: np.tile(v, (n,) + (1,) * (v.ndim - 1)) if k == 'obj_points' else np.tile(v, (1, n) + (1,) * (v.ndim - 2)) for k, v in sc.items()}


def as_batch(sc):
    """The stacked-tensor form of the batch ``ObjProjector.forward`` takes."""
    return {k: torch.from_numpy(sc[k]) for k in ('obj_angle', 'obj_trans', 'markers')}


def point(which):
    """-> (state_dict, scene arrays, initialize, extra gradient or None, fixture dict, key prefix)."""
    if which == 'i0':
        return ckpt(), scene(), False, None, g('corr_finetune.npz'), 'i0_'
    z = g('corr_finetune_points.npz')
    if which == 'i1':
        return ckpt(), scene(), True, None, z, 'i1_'
    if which == 'b1':
        return fo.perturbed(ckpt(), int(z['b1_seed_perturb']), float(z['b1_rel'])), clip_of(scene(), int(z['b1_clip'])), False, None, z, 'b1_'
    return ckpt(), scene(), False, fo.extra_gradient(int(z['x_seed']), cf.T, cf.B), z, 'x_'


@functools.lru_cache(None)
def oracle_grads(which):
    """The fp64 gradient of a fixture point, computed once and shared."""
    sd, sc, initialize, extra, _, _ = point(which)
    loss, terms, grads = fo.loss_and_grads(fo.leaves(sd), sc, initialize, extra)
    return float(loss), {k: float(v) for k, v in terms.items()}, {k: v.numpy() for k, v in grads.items()}


def tensor_errors(got, g64):
    return {n: float(np.abs(np.asarray(got[n], np.float64).ravel() - g64[n].ravel()).max() / np.abs(g64[n]).max()) for n in g64}


def selected_columns(sc, initialize):
    if initialize:
        return list(range(68))
    contact = sc['markers'][cf.PAST:, :, :, 6].sum(axis=0)
    score = contact.copy()
    score[:, fo.HAND_MARKERS] += 0.5
    return sorted({int(1 + np.argmax(score[b])) if contact[b].sum() > 0 else 0 for b in range(contact.shape[0])})


def check_zeros(flat_is_zero, z, sc, initialize):
    """Exact zeros: the columns [t][v][w] of the last adjacency whose node w no clip selects, and nowhere else."""
    names = [str(n) for n in z['names']]
    o = int(z['offsets'][names.index(ZERO_TENSOR)])
    want = np.zeros(N_PARAM, bool)
    A = np.ones((10, 68, 68), bool)
    A[:, :, selected_columns(sc, initialize)] = False
    want[o:o + A.size] = A.ravel()
    assert np.array_equal(flat_is_zero, want), (int(flat_is_zero.sum()), int(want.sum()))


# ------------------------------------------------------------------------------------------------------------ CPU

@pytest.mark.parametrize('which', POINTS)
def test_oracle_gradients_against_the_reference(which):
    sd, sc, initialize, extra, z, pre = point(which)
    loss64, terms64, g64 = oracle_grads(which)
    # (the reference's fp32 loss is a mean of squares of differences ~1e-2 of O(1) values: ~1e-6 relative rounding noise of its own, so the per-term bound)
    assert abs(loss64 - float(z[pre + 'loss'])) <= 1e-5 * loss64 and abs(loss64 - float(z[pre + 'loss64'])) <= 1e-12
    for k, v in zip(fo.MSE_KEYS, z[pre + 'terms']):
        assert abs(terms64[k] - float(v)) <= 1e-5 * terms64[k], k
    names = [str(n) for n in z['names']]
    assert names == list(g64) and len(names) == N_TENSORS
    flat64 = np.concatenate([g64[n].ravel() for n in names])
    assert flat64.size == N_PARAM
    # what is recorded of the reference's fp32 gradient: all of it at i0, every 8th entry elsewhere -- against the oracle, per tensor, within the recorded e_ref
    stride = 1 if which == 'i0' else 8
    ref = z['grads'] if which == 'i0' else z[pre + 'g8']
    idx = np.arange(0, N_PARAM, stride)
    assert ref.size == idx.size
    diff = np.abs(ref.astype(np.float64) - flat64[idx])
    for i, n in enumerate(names):
        o, s = int(z['offsets'][i]), int(z['sizes'][i])
        sel = (idx >= o) & (idx < o + s)
        e_ref, scale = float(z[pre + 'e_ref'][i]), np.abs(g64[n]).max()
        assert 4 * e_ref <= 1e-4, n
        assert abs(float(z[pre + 'gmax'][i]) - scale) <= 1e-4 * scale, n
        if sel.any():
            assert diff[sel].max() / scale <= 1.01 * e_ref + 1e-12, (n, diff[sel].max() / scale)
    # exact zeros: identical entries in the reference and the oracle, and they are the unselected columns of the last adjacency
    ref_zero = np.zeros(N_PARAM, bool)
    ref_zero[z[pre + 'zeros']] = True
    assert np.array_equal(ref_zero, flat64 == 0)
    check_zeros(ref_zero, z, sc, initialize)
    assert int(ref_zero.sum()) == {'i0': 44200, 'i1': 0, 'b1': 45560, 'x': 44200}[which]
    assert all(np.abs(v).max() > 0 for v in g64.values())


def test_parameter_table_is_named_parameters_order():
    z, sd = g('corr_finetune.npz'), ckpt()
    tab = cft.param_table(sd)
    assert [n for n, _, _ in tab] == [str(n) for n in z['names']] == fo.param_names(sd)
    assert [o for _, o, _ in tab] == [int(o) for o in z['offsets']]
    assert [int(np.prod(s)) for _, _, s in tab] == [int(s) for s in z['sizes']]
    assert all(tuple(sd[n].shape) == s for n, _, s in tab)
    assert len(tab) == N_TENSORS and tab[-1][1] + 1 == N_PARAM and tab[-1][0] == 'st_gcnns_all.3.prelu.weight'
    assert sum(1 for n, _, s in tab if n.endswith('gcn.A') and s == (10, 68, 68)) == 4
    ft = cft.CorrectionFineTuner(sd, T=cf.T, past_len=cf.PAST, device='cpu')      # checks the library's own table (csrc/objproj_train.h ot_plan) against this one
    assert ft.n_param == N_PARAM and ft.bn.numel() == sum(4 * c for c in ft.predictor.cop.cout)


def test_state_dict_keys_shapes_dtypes():
    sd = ckpt()
    assert any(k.endswith('num_batches_tracked') for k in sd)                    # buffers pass through, whatever their dtype
    ft = cft.CorrectionFineTuner({'model.' + k: v for k, v in sd.items()}, T=cf.T, past_len=cf.PAST, device='cpu')
    out = ft.state_dict()
    assert list(out) == list(sd)
    for k, v in sd.items():
        assert tuple(out[k].shape) == tuple(v.shape) and out[k].dtype == torch.as_tensor(v).dtype, k
        assert np.array_equal(out[k].numpy(), v), k
    st = ft.optimizer_state()
    assert st['step'] == 0 and list(st['exp_avg']) == [n for n, _, _ in ft.table] and all(float(v.abs().max()) == 0 for v in st['exp_avg_sq'].values())


def test_geometry_epochs_need_their_gradient():
    """The step never silently trains on another loss than the reference's: epochs whose annealed contact / penetration weights are not zero need d_obj_pred."""
    ft = cft.CorrectionFineTuner(ckpt(), T=cf.T, past_len=cf.PAST, device='cpu')
    assert ft.weights.vector(0)[:2] == (0, 0) and ft.weights.vector(1)[1] > 0
    for epoch in (1, 10, 20):
        with pytest.raises(ValueError):
            ft.training_step(as_batch(scene()), current_epoch=epoch)
    assert ft.step == 0


# ------------------------------------------------------------------------------------------------------------ GPU

def tuner(sd, **kw):
    return cft.CorrectionFineTuner(sd, T=cf.T, past_len=cf.PAST, device=DEV, **kw)


def check_point(ft, sc, which, gate_from=None):
    """Loss, terms, every gradient tensor against the fp64 oracle and the exact zeros at one fixture point; prints the six tensors closest to their gates."""
    _, _, initialize, extra, z, pre = point(gate_from or which)
    loss64, _, g64 = oracle_grads(gate_from or which)
    loss, ld, wd, grads = ft.loss_and_grads(as_batch(sc), initialize, None if extra is None else torch.from_numpy(extra))
    got = {n: v.detach().cpu().numpy() for n, v in grads.items()}
    assert abs(float(loss) - float(z[pre + 'loss'])) <= TERM_GATE * float(z[pre + 'loss'])
    for k, v in zip(fo.MSE_KEYS, z[pre + 'terms']):
        assert abs(float(ld[k]) - float(v)) <= TERM_GATE * float(v), k
    assert abs(float(sum(wd.values())) - float(loss)) <= 1e-6 * float(loss)
    err = tensor_errors(got, g64)
    gates = {n: max(4 * float(e), TIGHT) for n, e in zip(g64, z[pre + 'e_ref'])}
    worst = max(err, key=lambda n: err[n] / gates[n])
    print('%s: loss %.8f (reference %.8f, fp64 %.8f); worst tensor %s: e %.3e, gate %.3e (e / gate %.3f); max e %.3e'
          % (which, float(loss), float(z[pre + 'loss']), loss64, worst, err[worst], gates[worst], err[worst] / gates[worst], max(err.values())))
    for n in sorted(err, key=lambda n: -err[n] / gates[n])[:6]:
        print('    %-40s e %.3e  gate %.3e' % (n, err[n], gates[n]))
    for n in g64:
        assert tuple(grads[n].shape) == g64[n].shape, n
    missed = {n: (err[n], gates[n]) for n in g64 if err[n] > gates[n]}
    assert not missed, missed
    check_zeros(np.concatenate([got[n].ravel() for n in g64]) == 0, z, sc, initialize)
    return grads


@pytest.mark.gpu
@pytest.mark.parametrize('which', POINTS)
def test_gradients(which):
    """The four points: initialize False (i0), initialize True (i1), B = 1 with perturbed parameters (b1), loss + (c . obj_pred).sum() through d_obj_pred (x).
    Measured on MI355X, the tensor with the worst e / gate per point (every loss equals the reference's to the 8 digits printed):
      i0  st_gcnns_relative.3.prelu.weight  e 1.29e-6, gate 1.20e-5 (0.11 of the gate); largest e of any tensor 2.69e-6
      i1  st_gcnns_relative.3.prelu.weight  e 1.71e-6, gate 1.16e-5 (0.15);             largest e 2.53e-6
      b1  st_gcnns_relative.1.prelu.weight  e 1.71e-6, gate 1.53e-5 (0.11);             largest e 1.71e-6
      x   st_gcnns.3.prelu.weight           e 2.05e-6, gate 1.00e-5 (0.21);             largest e 2.65e-6
    With the skip path and the DCT in fp32 (the first form of the kernel) x missed: st_gcnns.3.prelu.weight e 1.98e-5 against 1.00e-5, i0 stood at 0.61."""
    sd, sc, _, _, _, _ = point(which)
    check_point(tuner(sd), sc, which)


@pytest.mark.gpu
def test_determinism_and_clip_independence_b32():
    """The scene's four clips tiled 8 times: the batch means do not change, so the gradient is the B = 4 one (initialize False); 32 per-clip partials meet in
    the fold.  Two calls give the same bits.  Measured on MI355X: bit-equal; worst e / gate 0.11 (st_gcnns_relative.3.prelu.weight, e 1.29e-6, gate 1.20e-5),
    the B = 4 figures to every digit printed; largest e 2.69e-6."""
    sd, sc, _, _, _, _ = point('i0')
    big = tiled(sc, 8)
    ft = tuner(sd)
    l1, _, _, g1 = ft.loss_and_grads(as_batch(big))
    g1 = {n: v.clone() for n, v in g1.items()}
    l2, _, _, g2 = ft.loss_and_grads(as_batch(big))
    assert torch.equal(l1, l2) and all(torch.equal(g1[n], g2[n]) for n in g1)
    check_point(ft, big, 'b32', gate_from='i0')


def adam_vectors(n):
    """Seeded gradients laid out like the parameters, with the special values at known places."""
    rs = np.random.RandomState(7530)
    gs = [(s * rs.standard_normal(n) * np.exp(rs.uniform(-9, 0, n))).astype(np.float32) for s in (1.0, -0.5, 2.0)]
    for gv in gs:
        gv[0:64] = 0.0
        gv[64:96] = np.float32(1e-40)                                   # denormal
        gv[96:128] = np.float32(-1e-40)
        gv[128:192] = (1e-8 * np.exp(rs.uniform(-2, 2, 64)) * rs.choice([-1, 1], 64)).astype(np.float32)        # around eps
    return gs


@pytest.mark.gpu
@pytest.mark.parametrize('wd,resync', [(0.0, False), (1e-2, True)])
def test_adam_on_injected_gradients(wd, resync):
    """3 steps against torch.optim.Adam on CPU tensors; each step's parameter change within 2^-20 relative of torch's change plus one ulp of the parameter.
    weight_decay 0: one uninterrupted 3-step run on both sides.  weight_decay 1e-2: before steps 2 and 3 torch starts from the kernel's own parameters and
    moments, so each step is compared with torch's step from the SAME point (the skeleton test's protocol, tests/test_skeleton_finetune.py: with weight decay the
    gradient depends on p, so the one-ulp differences the gate allows after a step feed the next steps' moments)."""
    ft = tuner(ckpt(), weight_decay=wd)
    p = torch.nn.Parameter(ft.params.detach().cpu().clone())
    opt = torch.optim.Adam([p], lr=3e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    for step, gv in enumerate(adam_vectors(ft.n_param)):
        if step and resync:
            with torch.no_grad():
                p.copy_(ft.params.cpu())
                opt.state[p]['exp_avg'].copy_(ft.exp_avg.cpu())
                opt.state[p]['exp_avg_sq'].copy_(ft.exp_avg_sq.cpu())
        before_t, before_h = p.detach().clone().double(), ft.params.detach().cpu().double()
        assert not resync or torch.equal(before_t, before_h)
        p.grad = torch.from_numpy(gv.copy())
        opt.step()
        ft.apply_gradients(torch.from_numpy(gv).to(DEV))
        dt, dh = p.detach().double() - before_t, ft.params.detach().cpu().double() - before_h
        ulp = torch.from_numpy(np.spacing(np.abs(p.detach().numpy()))).double()
        bad = (dh - dt).abs() > 2.0 ** -20 * dt.abs() + ulp
        assert not bad.any(), (step, int(bad.sum()), float((dh - dt).abs().max()))
        assert float(dt.abs().max()) > 1e-4                              # (the step moved something)
        ref = opt.state[p]
        assert int(ref['step']) == step + 1 == ft.step
        for mine, theirs in ((ft.exp_avg, ref['exp_avg']), (ft.exp_avg_sq, ref['exp_avg_sq'])):
            assert float((mine.cpu() - theirs).abs().max()) <= 1e-6 * float(theirs.abs().max())
    st = ft.optimizer_state()
    assert st['step'] == 3 and list(st['exp_avg']) == [n for n, _, _ in ft.table]


@pytest.mark.gpu
def test_lr_zero_step_keeps_parameters_and_buffers():
    sd = ckpt()
    ft = tuner(sd, lr=0.0)
    p0, bn0 = ft.params.clone(), ft.bn.clone()
    arena0 = pack_objprojector(sd, cf.T, cf.PAST, 'cpu')[1].numpy()
    assert np.array_equal(ft.predictor.arena.cpu().numpy(), arena0)
    ft.training_step(as_batch(scene()))
    assert torch.equal(ft.params, p0) and torch.equal(ft.bn, bn0) and ft.step == 1
    a = ft.predictor.arena.cpu().numpy()
    assert np.isfinite(a).all() and np.array_equal(a == 0, arena0 == 0)
    ulps = np.abs(a.view(np.int32).astype(np.int64) - arena0.view(np.int32).astype(np.int64))
    assert ulps.max() <= 1, int(ulps.max())
    out = ft.state_dict()
    for k, v in sd.items():
        assert np.array_equal(out[k].numpy(), v), k


def trajectory_start():
    z = g('corr_finetune_traj.npz')
    return fo.perturbed(ckpt(), int(z['traj_seed_perturb']), float(z['traj_rel']))


@pytest.fixture(scope='module')
def trained():
    """10 training steps at the defaults (epoch 0: initialize True) on the scene from the fixture's start: (tuner, the 10 losses, batch)."""
    z = g('corr_finetune_traj.npz')
    ft = tuner(trajectory_start(), lr=float(z['lr']), weight_decay=float(z['weight_decay']))
    batch = as_batch(scene())
    losses = [ft.training_step(batch, current_epoch=0) for _ in range(len(z['traj_losses']))]
    return ft, np.asarray([float(l) for l in losses]), batch


@pytest.mark.gpu
def test_trajectory_against_the_reference(trained):
    """Measured on MI355X: losses 0.000307 -> 0.000094, relative differences from the reference's per step 6.6e-7 6.5e-8 4.5e-7 6.0e-7 9.1e-7 4.6e-7 4.4e-7
    4.0e-7 7.9e-7 7.0e-7; 0 of 224,174 parameters beyond 8 y_traj = 8.93e-6 (max |diff| 1.08e-6)."""
    ft, losses, _ = trained
    z = g('corr_finetune_traj.npz')
    rel = np.abs(losses - z['traj_losses']) / z['traj_losses']
    diff = np.abs(ft.params.detach().cpu().double().numpy() - z['theta_final'].astype(np.float64))
    count = int((diff > 8 * float(z['y_traj'])).sum())
    print('trajectory: losses %s; relative loss differences %s; parameters beyond 8 y_traj = %.3e: %d of %d (max |diff| %.3e)'
          % (' '.join('%.6f' % v for v in losses), ' '.join('%.1e' % v for v in rel), 8 * float(z['y_traj']), count, diff.size, diff.max()))
    assert rel.max() <= 1e-5
    assert losses[9] < losses[0]
    assert count <= 224


def mse_loss(predictor, batch):
    pred, gt = predictor.forward(batch)
    return float(cl.calc_loss(pred, gt, batch, predictor.past_len)[0])


@pytest.mark.gpu
def test_live_weights_reach_the_predictor(trained):
    ft, _, batch = trained
    live = mse_loss(ft.predictor, batch)
    fresh = mse_loss(ObjProjector(ft.state_dict(), cf.T, cf.PAST, device=DEV), batch)
    start = mse_loss(ObjProjector(trajectory_start(), cf.T, cf.PAST, device=DEV), batch)
    ckpt_value = mse_loss(ObjProjector(ckpt(), cf.T, cf.PAST, device=DEV), batch)
    assert abs(live - fresh) <= 1e-6 * fresh
    assert abs(live - ckpt_value) > 1e-2 * ckpt_value and abs(live - start) > 1e-2 * start
    # the BatchNorm buffers of the exported state_dict are the checkpoint's
    out, sd = ft.state_dict(), ckpt()
    assert all(np.array_equal(out[k].numpy(), v) for k, v in sd.items() if 'running_' in k or 'tracked' in k)
    # resuming: a second tuner from the exported parameters and optimiser state takes the same next step, bit for bit
    ft2 = tuner(out)
    ft2.load_optimizer_state(ft.optimizer_state())
    _, grads = ft._grads(batch, True)
    _, grads2 = ft2._grads(batch, True)
    assert torch.equal(grads, grads2)
    ft2.apply_gradients(grads2)
    p_before, arena_before, state = ft.params.clone(), ft.predictor.arena.clone(), ft.optimizer_state()
    ft.apply_gradients(grads)
    same = torch.equal(ft.params, ft2.params) and torch.equal(ft.predictor.arena, ft2.predictor.arena) and not torch.equal(ft.params, p_before)
    ft.params.copy_(p_before)                                            # (leave the shared tuner as the trajectory test expects it)
    ft.predictor.arena.copy_(arena_before)
    ft.load_optimizer_state(state)
    assert same


@pytest.mark.gpu
def test_argument_checks():
    sc = scene()
    ft = tuner(ckpt())
    batch = as_batch(sc)
    with pytest.raises(ValueError):
        ft.loss_and_grads({k: v[:34] for k, v in batch.items()})                                              # T = 34
    with pytest.raises(ValueError):
        ft.loss_and_grads(batch, d_obj_pred=torch.zeros(cf.T, cf.B, 8))
    with pytest.raises(ValueError):
        ft.apply_gradients(torch.zeros(ft.n_param - 1, device=DEV))
    with pytest.raises(ValueError):
        ft.training_step(batch, current_epoch=5)                                                              # non-zero geometry weights, no d_obj_pred
    ft._ws = {cf.B: torch.empty(1024, dtype=torch.uint8, device=DEV)}                                          # a short workspace: IDF_E_INVAL
    with pytest.raises(ValueError):
        ft.loss_and_grads(batch)
    assert ft.step == 0
