"""Fine-tuning of the skeleton correction predictor with frozen normalisation statistics (interdiff_amd/skeleton_finetune.py,
csrc/skeleton_train.h / .hip) against the reference's own autograd and torch.optim.Adam with the real checkpoint
(tests/golden/skel_finetune.npz, skel_finetune_b1.npz; tests/golden/make_golden_skeleton_finetune.py) and the fp64 restatement
tests/skeleton_finetune_oracle.py.

Gates (none of them comes from the code under test):
  gradient    per parameter tensor e = max|g - g64| / max|g64| <= max(4 e_ref, 1e-5): e_ref is the same quantity for the reference's fp32
              autograd (recorded); factor 4 for another summation order at the same fp32 depth; 1e-5 = the project's tight gate
  zeros       the 9,240 entries of st_gcnns_all.3.gcn.A that feed nodes other than node 0 are exactly 0
  loss        the 1e-4 per-term gate of tests/test_correction_losses.py
  trajectory  losses within 1e-5 relative of the reference's at every step; at most 96 parameters (0.1 %) further than 8 y_traj from the
              reference's, y_traj = max|theta32 - theta64| of the reference against the oracle (recorded)
  Adam        each step's parameter change within 2^-20 relative of torch's change plus one ulp of the parameter
"""
import functools
import numpy as np
import pytest
import torch
from tests import fixtures as fx
from tests import skeleton_finetune_oracle as fo
from interdiff_amd import skeleton as sk
from interdiff_amd import skeleton_finetune as sf

DEV = 'cuda'
TIGHT, TERM_GATE = 1e-5, 1e-4
ZERO_TENSOR = 'st_gcnns_all.3.gcn.A'


@functools.lru_cache(None)
def g(name):
    z = fx.golden(name)
    return {k: z[k] for k in z.files}


def ckpt():
    return dict(g('skel_ckpt.npz'))


def point(which):
    """-> (state_dict, batch as torch tensors, fixture dict, key prefix)."""
    if which == 'b3':
        z = g('skel_finetune.npz')
        return ckpt(), tuple(torch.from_numpy(z[k]) for k in ('body', 'obj', 'pose', 'zero_pose_obj')), z, ''
    z = g('skel_finetune_b1.npz')
    return (fo.perturbed(ckpt(), int(z['p1_seed_perturb']), float(z['p1_rel'])),
            tuple(torch.from_numpy(z['p1_' + k]) for k in ('body', 'obj', 'pose', 'zero_pose_obj')), z, 'p1_')


@functools.lru_cache(None)
def oracle_grads(which):
    """The fp64 gradient of a fixture point, computed once and shared."""
    sd, batch, _, _ = point(which)
    loss, terms, grads = fo.loss_and_grads(fo.leaves(sd), batch)
    return float(loss), {k: float(v) for k, v in terms.items()}, {k: v.numpy() for k, v in grads.items()}


def split(z, flat):
    return {str(n): flat[o:o + s] for n, o, s in zip(z['names'], z['offsets'], z['sizes'])}


def tensor_errors(got, g64):
    return {n: float(np.abs(np.asarray(got[n], np.float64).ravel() - g64[n].ravel()).max() / np.abs(g64[n]).max()) for n in g64}


# ------------------------------------------------------------------------------------------------------------ CPU

@pytest.mark.parametrize('which', ['b3', 'b1'])
def test_oracle_gradients_against_the_reference(which):
    _, batch, z, pre = point(which)
    loss64, terms64, g64 = oracle_grads(which)
    assert abs(loss64 - float(z[pre + 'loss'])) <= 1e-6 * loss64 and abs(loss64 - float(z[pre + 'loss64'])) <= 1e-12
    for k, v in zip(fo.MSE_KEYS, z[pre + 'terms']):
        assert abs(terms64[k] - float(v)) <= 1e-5 * terms64[k], k
    assert [str(n) for n in z['names']] == list(g64)
    ref = split(z, z[pre + 'grads'])
    err = tensor_errors(ref, g64)
    for i, n in enumerate(g64):
        assert err[n] <= 1.01 * float(z[pre + 'e_ref'][i]) + 1e-12, (n, err[n])           # the recorded e_ref IS this comparison
        assert 4 * err[n] <= 1e-4, n
    # exact zeros: the columns of the last adjacency that feed nodes other than node 0 -- in the reference and in the oracle, nowhere else
    for n in g64:
        zr, zo = (ref[n] == 0), (g64[n].ravel() == 0)
        assert np.array_equal(zr, zo), n
        if n == ZERO_TENSOR:
            assert zr.sum() == 9240 and zr.reshape(20, 22, 22)[:, :, 1:].all()
        else:
            assert not zr.any(), n


def test_oracle_trajectory_against_the_reference():
    sd, batch, z, _ = point('b3')
    losses, theta = fo.adam_trajectory(sd, batch, len(z['traj_losses']), float(z['lr']), float(z['weight_decay']))
    assert np.abs(losses - z['traj_losses']).max() <= 1e-6 * losses.min() and losses[-1] < losses[0]
    flat = np.concatenate([theta[str(n)].numpy().ravel() for n in z['names']])
    y = np.abs(flat - z['theta_final'].astype(np.float64)).max()
    assert abs(y - float(z['y_traj'])) <= 0.01 * float(z['y_traj']) and y <= 1e-5


def test_parameter_table_is_named_parameters_order():
    z, sd = g('skel_finetune.npz'), ckpt()
    tab = sf.param_table(sd)
    assert [n for n, _, _ in tab] == [str(n) for n in z['names']]
    assert [o for _, o, _ in tab] == [int(o) for o in z['offsets']]
    assert [int(np.prod(s)) for _, _, s in tab] == [int(s) for s in z['sizes']]
    assert all(tuple(sd[n].shape) == s for n, _, s in tab)
    assert tab[-1][1] + 1 == 96110 and tab[-1][0].endswith('prelu.weight')
    assert [n for n, _, _ in tab] == fo.param_names(sd)
    ft = sf.SkeletonFineTuner(sd, device='cpu')               # checks the library's own table (csrc/skeleton_train.h ft_plan) against this one
    assert ft.n_param == 96110 and ft.bn.numel() == sum(4 * c for c in ft.predictor.cop.cout)


def test_folded_gradient_conversion_against_autograd():
    """d(folded conv) -> d(conv weight, conv bias, BN gamma, BN beta), numpy fp64, against autograd on a single conv + eval BatchNorm."""
    torch.set_grad_enabled(True)                               # (other test modules switch autograd off process-wide)
    rs = np.random.RandomState(7420)
    cin, cout, n = 5, 7, 33
    t = lambda *s: torch.from_numpy(rs.standard_normal(s))
    x, R = t(cin, n), t(cout, n)
    W, b, gamma, beta, mean = (t(cout, cin).requires_grad_(), t(cout).requires_grad_(), t(cout).requires_grad_(), t(cout).requires_grad_(), t(cout))
    var = torch.from_numpy(rs.uniform(0.2, 2.0, cout))
    y = ((W @ x + b[:, None]) - mean[:, None]) / torch.sqrt(var + sf.BN_EPS)[:, None] * gamma[:, None] + beta[:, None]
    want = torch.autograd.grad((y * R).sum(), [W, b, gamma, beta])
    s = (gamma / torch.sqrt(var + sf.BN_EPS)).detach()
    Wf, bf = (W.detach() * s[:, None]).requires_grad_(), ((b.detach() - mean) * s + beta.detach()).requires_grad_()
    dWf, dbf = torch.autograd.grad(((Wf @ x + bf[:, None]) * R).sum(), [Wf, bf])
    got = sf.folded_to_reference_grads(dWf.numpy(), dbf.numpy(), W.detach().numpy(), b.detach().numpy(), gamma.detach().numpy(), mean.numpy(), var.numpy())
    for a, w in zip(got, want):
        assert np.abs(a - w.numpy()).max() <= 1e-12 * np.abs(w.numpy()).max()


def test_state_dict_keys_shapes_dtypes():
    sd = ckpt()
    sd['st_gcnns.0.tcn.1.num_batches_tracked'] = np.asarray(12345, np.int64)          # buffers pass through, whatever their dtype
    ft = sf.SkeletonFineTuner({'model.' + k: v for k, v in sd.items()}, device='cpu')
    out = ft.state_dict()
    assert list(out) == list(sd)
    for k, v in sd.items():
        assert tuple(out[k].shape) == tuple(v.shape) and out[k].dtype == torch.as_tensor(v).dtype, k
        assert np.array_equal(out[k].numpy(), v), k
    st = ft.optimizer_state()
    assert st['step'] == 0 and list(st['exp_avg']) == [n for n, _, _ in ft.table] and all(float(v.abs().max()) == 0 for v in st['exp_avg_sq'].values())


# ------------------------------------------------------------------------------------------------------------ GPU

def check_point(ft, batch, which):
    """Measured on MI355X (the six tensors closest to their gates are printed).  B = 1 perturbed point: loss 0.36241564 (reference 0.36241561); closest to its gate
    st_gcnns_all.1.prelu.weight, e 4.59e-6 against 1.62e-5 (0.28 of the gate); max e over all tensors 2.4e-5.  B = 3: closest st_gcnns_relative.3.tcn.1.weight,
    e 1.47e-6 against 1.33e-5 (0.11 of the gate)."""
    _, _, z, pre = point(which)
    _, _, g64 = oracle_grads(which)
    loss, ld, wd, grads = ft.loss_and_grads(batch)
    got = {n: v.detach().cpu().numpy() for n, v in grads.items()}
    assert abs(float(loss) - float(z[pre + 'loss'])) <= TERM_GATE * float(z[pre + 'loss'])
    for k, v in zip(fo.MSE_KEYS, z[pre + 'terms']):
        assert abs(float(ld[k]) - float(v)) <= TERM_GATE * float(v), k
    assert abs(float(sum(wd.values())) - float(loss)) <= 1e-6 * float(loss)
    err = tensor_errors(got, g64)
    gates = {n: max(4 * float(e), TIGHT) for n, e in zip(g64, z[pre + 'e_ref'])}
    worst = max(err, key=lambda n: err[n] / gates[n])
    print('%s: loss %.8f (reference %.8f); worst tensor %s: e %.3e, gate %.3e; max e %.3e' % (which, float(loss), float(z[pre + 'loss']), worst, err[worst],
                                                                                            gates[worst], max(err.values())))
    for n in sorted(err, key=lambda n: -err[n] / gates[n])[:6]:
        print('    %-40s e %.3e  gate %.3e' % (n, err[n], gates[n]))
    for n in g64:
        assert tuple(grads[n].shape) == g64[n].shape, n
    zeros = got[ZERO_TENSOR] == 0
    missed = {n: (err[n], gates[n]) for n in g64 if err[n] > gates[n]}
    assert not missed, missed
    assert zeros[:, :, 1:].all() and not zeros[:, :, 0].any()
    return got


@pytest.mark.gpu
def test_gradients_b1_perturbed_point():
    sd, batch, _, _ = point('b1')
    check_point(sf.SkeletonFineTuner(sd, device=DEV), batch, 'b1')


@pytest.mark.gpu
def test_gradients_b3():
    sd, batch, _, _ = point('b3')
    check_point(sf.SkeletonFineTuner(sd, device=DEV), batch, 'b3')


@pytest.mark.gpu
def test_determinism_and_clip_independence_b33():
    """The fixture's three clips tiled 11 times: the batch means do not change, so the gradient is the B = 3 one; 33 per-clip partials meet
    in the fold.  Two calls give the same bits."""
    sd, batch, z, _ = point('b3')
    _, _, g64 = oracle_grads('b3')
    big = tuple(a.repeat((11,) + (1,) * (a.dim() - 1)) for a in batch)
    ft = sf.SkeletonFineTuner(sd, device=DEV)
    l1, _, _, g1 = ft.loss_and_grads(big)
    l2, _, _, g2 = ft.loss_and_grads(big)
    assert torch.equal(l1, l2) and all(torch.equal(g1[n], g2[n]) for n in g1)
    assert abs(float(l1) - float(z['loss'])) <= TERM_GATE * float(z['loss'])
    err = tensor_errors({n: v.cpu().numpy() for n, v in g1.items()}, g64)
    for n, e in zip(g64, z['e_ref']):
        assert err[n] <= max(4 * float(e), TIGHT), (n, err[n])


def adam_vectors(n):
    """Seeded gradients laid out like the parameters, with the special values at known places."""
    rs = np.random.RandomState(7430)
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
    weight_decay 0: one uninterrupted 3-step run on both sides, so accumulated drift is covered.  weight_decay 1e-2: before steps 2 and 3 torch starts from
    the kernel's own parameters and moments, so each step is compared with torch's step from the SAME point.  Uninterrupted, that case was measured on MI355X
    to differ on 1 of 96,110 entries at the third step by 2.98e-8 = two ulps of the parameter, with and without the entries where g + wd p cancels at that
    step: with weight decay the gradient the optimiser sees depends on p, so the one-ulp differences of p that the gate itself allows after a step feed the
    moments of the next ones, and two runs that are not bit-identical drift apart by more than one step's allowance."""
    sd = ckpt()
    ft = sf.SkeletonFineTuner(sd, weight_decay=wd, device=DEV)
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
    sd, batch, _, _ = point('b3')
    ft = sf.SkeletonFineTuner(sd, lr=0.0, device=DEV)
    p0, bn0 = ft.params.clone(), ft.bn.clone()
    _, arena0 = sk.pack_skeleton_objprojector(sd)
    assert np.array_equal(ft.predictor.arena.cpu().numpy(), arena0)
    ft.training_step(batch)
    assert torch.equal(ft.params, p0) and torch.equal(ft.bn, bn0) and ft.step == 1
    a = ft.predictor.arena.cpu().numpy()
    assert np.isfinite(a).all() and np.array_equal(a == 0, arena0 == 0)
    ulps = np.abs(a.view(np.int32).astype(np.int64) - arena0.view(np.int32).astype(np.int64))
    assert ulps.max() <= 1, int(ulps.max())
    out = ft.state_dict()
    for k, v in sd.items():
        assert np.array_equal(out[k].numpy(), v), k


@pytest.fixture(scope='module')
def trained():
    """10 training steps at the defaults on the B = 3 batch from the real checkpoint: (tuner, the 10 losses, batch)."""
    sd, batch, z, _ = point('b3')
    ft = sf.SkeletonFineTuner(sd, device=DEV)
    losses = [ft.training_step(batch) for _ in range(len(z['traj_losses']))]
    return ft, np.asarray([float(l) for l in losses]), batch


@pytest.mark.gpu
def test_trajectory_against_the_reference(trained):
    """Measured on MI355X: losses within 2.2e-7 relative; 0 of 96,110 parameters beyond 8 y_traj = 2.14e-5 (max |diff| 2.19e-6)."""
    ft, losses, _ = trained
    z = g('skel_finetune.npz')
    rel = np.abs(losses - z['traj_losses']) / z['traj_losses']
    diff = np.abs(ft.params.detach().cpu().double().numpy() - z['theta_final'].astype(np.float64))
    count = int((diff > 8 * float(z['y_traj'])).sum())
    print('trajectory: losses %s; max relative loss difference %.3e; parameters beyond 8 y_traj = %.3e: %d of %d (max |diff| %.3e)'
          % (' '.join('%.6f' % v for v in losses), rel.max(), 8 * float(z['y_traj']), count, diff.size, diff.max()))
    assert rel.max() <= 1e-5
    assert losses[9] < losses[0]
    assert count <= 96


@pytest.mark.gpu
def test_live_weights_reach_the_predictor(trained):
    ft, _, batch = trained
    live = float(sk.skeleton_validation_step(ft.predictor, batch)[0])
    fresh = float(sk.skeleton_validation_step(sk.SkeletonObjProjector(ft.state_dict(), device=DEV), batch)[0])
    start = float(sk.skeleton_validation_step(sk.SkeletonObjProjector(ckpt(), device=DEV), batch)[0])
    assert abs(live - fresh) <= 1e-6 * fresh
    assert abs(live - start) > 1e-2 * start and live < start
    # the BatchNorm buffers of the exported state_dict are the checkpoint's
    out, sd = ft.state_dict(), ckpt()
    assert all(np.array_equal(out[k].numpy(), v) for k, v in sd.items() if 'running_' in k)
    # resuming: a second tuner from the exported parameters and optimiser state takes the same next step, bit for bit
    ft2 = sf.SkeletonFineTuner(out, device=DEV)
    ft2.load_optimizer_state(ft.optimizer_state())
    _, grads = ft._grads(batch)
    _, grads2 = ft2._grads(batch)
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
    sd, batch, _, _ = point('b3')
    ft = sf.SkeletonFineTuner(sd, device=DEV)
    with pytest.raises(ValueError):
        ft.loss_and_grads(tuple(a[:, :19] if a.dim() > 3 or a.shape[-1] == 7 else a for a in batch))          # T = 19
    with pytest.raises(ValueError):
        ft.apply_gradients(torch.zeros(ft.n_param - 1, device=DEV))
    ft._ws = {3: torch.empty(1024, dtype=torch.uint8, device=DEV)}                                              # a short workspace: IDF_E_INVAL
    with pytest.raises(ValueError):
        ft.loss_and_grads(batch)
    assert ft.step == 0
