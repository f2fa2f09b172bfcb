"""Fine-tuning of the SMPL denoiser's PointNet++ on HIP (``interdiff_amd.pointnet2_train``, ``DenoiserTrainer(train_encoder=True, train_pointnet=True)``) against the
fp64 oracle tests/pointnet2_train_oracle.py and the reference's OWN fp32 run recorded by tests/golden/make_golden_pointnet2_finetune.py
(tests/golden/pointnet2_finetune_{N1,N2,W1,traj}.npz): ``PointNet2Encoder`` (model/layers.py:111-175) as ``MDM._get_embeddings`` calls it (model/diffusion_smpl.py:210-211),
in eval() with autograd on -- frozen normalisation statistics.  The grouping indices are recorded and shared by all three.

Gates: every gradient tensor within max(4 e_ref, 1e-5) max|g64| of fp64, e_ref the reference's own recorded fp32 error; the fixture keeps every ReLU sign and pool
winner on the gradient's path at least 16 delta_max away from its discontinuity (recorded, re-checked below).  Trajectory: 6 AdamW steps, losses 1e-5, at most 0.1 % of
the 11,938,309 parameters further than 8 y_traj from the fp64 trajectory.  The exported sampler model's ``_get_embeddings`` against the trainer's ``cond``: 1e-4, the
gate tests/test_mdm_encoder_train.py holds the same comparison to (the sampler's encoder runs split-f16 products).  Measured on MI355X: DESIGN.md 8.18.
Without the feature every test below fails: the module, the keyword and the entries do not exist.
"""
import ctypes as C
import numpy as np
import pytest
import torch
from tests import fixtures as fx
from tests import losses_oracle as lo
from tests import mdm_train_oracle as mo
from tests.denoiser_train_helpers import betas, check_new_symbols, far_parameters, gate, rel, tn

DEV = 'cuda'
N_PN, N_FULL = 113917, 11824392
NEW_SYMBOLS = {
    'interdiff_pointnet2_saves_bytes': 'int32_t B',
    'interdiff_pointnet2_encode_saved': 'const idf_pointnet2 *pn, const float *obj_points, int32_t B, int32_t P, float *out, void *saves, size_t saves_bytes, void *stream',
    'interdiff_pointnet2_finetune_param_table': 'int64_t *offsets, int64_t *sizes, int32_t *n_tensors, int64_t *n_param',
    'interdiff_pointnet2_finetune_workspace_bytes': 'int32_t B',
    'interdiff_pointnet2_finetune_grads': 'const idf_pointnet2 *pn, const float *theta, const float *stats, const float *obj_points, int32_t B, int32_t P, '
                                          'const void *saves, const float *d_pc, float *grads, void *ws, size_t ws_bytes, void *stream',
    'interdiff_pointnet2_refold': 'const idf_pointnet2 *pn, const float *theta, const float *stats, void *stream',
}
SV_POS, SV_PID, SV_DUP, SV_CNT, SV_NB0, SV_NB1 = 0, 48, 96, 144, 244, 1012        # csrc/pointnet2_train.h


def po():
    from tests import pointnet2_train_oracle
    return pointnet2_train_oracle


def meo():
    from tests import mdm_encoder_train_oracle
    return mdm_encoder_train_oracle


def golden(name):
    z = fx.golden('pointnet2_finetune_%s.npz' % name)
    return {k: z[k] for k in z.files}


def weights():
    """fixtures.mdm_weights_wc() with the positional-table rows the reference runs read."""
    return mo.with_pe_rows(fx.mdm_weights_wc(), *[(z['pe_idx'], z['pe_val']) for z in (golden('W1'), golden('traj'))])


def indices(z):
    return {k: tn(z[k]).long() for k in ('pos', 'pid', 'nb0', 'nb1', 'hits1', 'hits2')}


_POINTS = {}


def point(name):
    """The recorded inputs of a point and the fp64 oracle on them, computed once per process and never modified."""
    if name not in _POINTS:
        z = golden(name)
        pts, idx = tn(z['points']), indices(z)
        p = dict(z=z, points=pts, idx=idx, e_ref=dict(zip([str(k) for k in z['names']], z['e_ref'])))
        if name == 'W1':
            x0, t, eps, past = tn(z['x0']), tn(z['t']), tn(z['eps']), int(z['past_len'])
            x_t = lo.q_sample(betas(), x0, t, eps)
            whole = meo().grads(weights(), x_t, t, po().encode(weights(), pts, idx), x0, past)
            p.update(x0=x0, t=t, eps=eps, past=past, whole=whole, d_pc=whole['d_pc'])
        else:
            p['d_pc'] = tn(z['d_pc'])
        p['ref'] = po().grads(weights(), pts, idx, p['d_pc'], taps=True)
        _POINTS[name] = p
    return _POINTS[name]


@pytest.fixture(scope='module')
def traj():
    """The recorded per-step t / noise and the fp64 oracle's trajectory on them (W1's scene and cloud), computed once."""
    z, p = golden('traj'), point('W1')
    ts, noises = [tn(t) for t in z['t']], [tn(e) for e in z['noise']]
    losses, theta = po().trajectory(weights(), betas(), p['x0'], p['points'], p['idx'], ts, noises, p['past'], float(z['lr']))
    return dict(z=z, ts=ts, noises=noises, losses=losses, theta=theta)


# ------------------------------------------------------------------------------------------------------------ CPU

@pytest.mark.parametrize('name', ['N1', 'N2', 'W1'])
def test_oracle_vs_reference_samples(name):
    """The fp64 oracle against every 64th entry of the reference's own fp32 gradients, within the recorded e_ref; the recorded indices are the restatement's."""
    PN = po().POINTNET_PARAM_NAMES
    p = point(name)
    z, ref, stride = p['z'], p['ref'], int(p['z']['stride'])
    assert [str(k) for k in z['names']] == list(PN)
    at, worst = 0, 0.0
    for k in PN:
        g = ref['grads'][k].reshape(-1)[::stride]
        s = tn(z['ref_grad_samples'][at:at + g.numel()]).double()
        at += g.numel()
        top = float(ref['grads'][k].abs().max())
        assert top > 0 and abs(top - float(z['g64_max'][PN.index(k)])) <= 1e-9 * top, k
        e = float((s - g).abs().max()) / top
        worst = max(worst, e / p['e_ref'][k])
        assert e <= 1.01 * p['e_ref'][k], k
    assert at == len(z['ref_grad_samples'])
    again = po().indices(p['points'])
    assert all(torch.equal(again[k], p['idx'][k]) for k in again)
    print('point %s: sampled reference vs oracle: worst e / e_ref %.3f; worst e_ref %.2e' % (name, worst, max(p['e_ref'].values())))
    if name == 'W1':
        k = 'pcEmbedding.Linear.weight'
        assert float(ref['grads'][k].abs().max()) > 0 and rel(tn(z['ref_d_pc']), p['d_pc']) <= 1e-4
        assert abs(float(p['whole']['loss']) - float(z['ref_loss'])) <= 1e-5 * float(p['whole']['loss'])
    else:
        assert rel(tn(z['ref_pc']), ref['pc']) <= 1e-5


@pytest.mark.parametrize('name', ['N1', 'N2', 'W1'])
def test_recorded_conditions(name):
    """The recorder's conditions, re-checked from the .npz and the oracle: 4 e_ref <= 1e-4, the margins of 16 delta_max, the coverage counts."""
    p = point(name)
    z = p['z']
    assert 4 * float(z['e_ref'].max()) <= 1e-4 and len(z['e_ref']) == 38
    zmin, gap = po().margins(p['ref']['taps'], p['idx'])
    d = float(z['delta_max'])
    print('point %s: delta_max %.2e; min live |z| %.2e (x%.0f), min pool gap %.2e (x%.0f); reversed fp32 run at %.3f of its gate; cover %s' % (
        name, d, zmin, zmin / d, gap, gap / d, float(z['fp32_reversed_gate_fraction']), z['cover'].tolist() if 'cover' in z else '-'))
    assert abs(zmin - float(z['min_live_z'])) <= 1e-9 * zmin and abs(gap - float(z['min_pool_gap'])) <= 1e-9 * gap
    assert zmin >= 16 * d and gap >= 16 * d and float(z['fp32_reversed_gate_fraction']) <= 1.0
    r32 = po().grads(weights(), p['points'], p['idx'], p['d_pc'], dtype=torch.float32, reverse=True, taps=True)
    assert po().same_decisions(r32['taps'], p['ref']['taps'], p['idx'])
    pts = p['points']
    assert bool(((pts * pts).sum(-1) <= 1e-3).any(dim=1).all())                 # every clip has a point FPS skips
    if name == 'W1':
        return
    hits1, hits2, cv = p['idx']['hits1'], p['idx']['hits2'], z['cover']
    rows = [hits1[..., 0], hits1[..., 1], hits2[:, 0], hits2[:, 1]]
    assert cv.tolist() == [[int((r < ns).sum()), int((r > ns).sum())] for r, ns in zip(rows, (16, 32, 16, 32))]
    assert (cv[:2] > 0).all()                                                   # SA1: padding slots and truncation at both radii
    B = pts.shape[0]
    if name == 'N1':
        assert cv[2, 0] == B and cv[3, 0] == B                                  # SA2: padding slots in every clip
    else:
        pid = p['idx']['pid']
        assert int(z['slot_repeats']) >= 2 and max(int(torch.unique(r, return_counts=True)[1].max()) for r in pid[:, :16]) >= 2
        assert pts.shape[1] < 1024 and cv[2, 1] == B and cv[3, 1] == B          # the FPS positions repeat a point, and the repeats are hits


def test_param_table_vs_reference_module():
    """The 38 names, shapes and the flat layout against the reference module's own state_dict (recorded names / shapes) and the synthetic weights."""
    from interdiff_amd import pointnet2_train as pt
    z = golden('N1')
    module = dict(zip([str(k) for k in z['module_names']], [tuple(int(v) for v in str(s).split()) for s in z['module_shapes']]))
    trained = [k for k in module if not k.endswith(('running_mean', 'running_var', 'num_batches_tracked'))]
    assert trained == list(pt.POINTNET_PARAM_NAMES) and len(trained) == 38          # the module's own order
    assert [k for k in module if k.endswith(('running_mean', 'running_var'))] == list(pt.POINTNET_STAT_NAMES)
    off, size, n = pt.param_table()
    sd = fx.mdm_weights()
    at = 0
    for k, o, s in zip(pt.POINTNET_PARAM_NAMES, off, size):                    # in order, back to back
        assert o == at and s == int(np.prod(module[k])) == sd[k].numel() and tuple(sd[k].shape) == module[k], k
        at += s
    assert at == n == N_PN
    assert sum(int(np.prod(module[k])) for k in pt.POINTNET_STAT_NAMES) == 1472


def test_new_symbols_declared_typed_and_exported():
    lib = check_new_symbols(NEW_SYMBOLS)
    assert lib.interdiff_pointnet2_saves_bytes(3) == 3 * 7156 * 4 and lib.interdiff_pointnet2_saves_bytes(0) == 0
    assert lib.interdiff_pointnet2_finetune_workspace_bytes(3) > 3 * 4 * (N_PN - 1472) and lib.interdiff_pointnet2_finetune_workspace_bytes(0) == 0


def test_raising_cases():
    """G7: train_pointnet without train_encoder; a state_dict without pcEmbedding.*; a batch that carries pc or cond, or no obj_points."""
    from interdiff_amd.mdm_train import DenoiserTrainer, FULL_PARAM_NAMES
    from interdiff_amd.pointnet2_train import POINTNET_PARAM_NAMES
    sd = fx.mdm_weights_wc()
    with pytest.raises(ValueError):
        DenoiserTrainer(sd, device='cpu', train_pointnet=True)
    with pytest.raises(KeyError):
        DenoiserTrainer({k: v for k, v in sd.items() if not k.startswith('pcEmbedding.')}, device='cpu', train_encoder=True, train_pointnet=True)
    with pytest.raises(KeyError):
        DenoiserTrainer({k: v for k, v in sd.items() if not k.endswith('mlps.1.4.running_var')}, device='cpu', train_encoder=True, train_pointnet=True)
    tr = DenoiserTrainer(sd, device='cpu', train_encoder=True, train_pointnet=True)
    assert tr.names == FULL_PARAM_NAMES + POINTNET_PARAM_NAMES and len(tr.names) == 266
    assert tr.n_param == N_FULL + N_PN == tr.params.numel() == tr.grads.numel() == tr.exp_avg.numel() == tr.exp_avg_sq.numel()
    assert tr.offsets[228] == N_FULL and tr.pointnet.params.data_ptr() == tr.params[N_FULL:].data_ptr()
    gt, t = torch.zeros(2, 1, 144, 12), torch.zeros(2, dtype=torch.int64)
    for bad in (dict(gt=gt, cond=torch.zeros(10, 2, 256)), dict(gt=gt, pc=torch.zeros(2, 256)), dict(gt=gt, pc=torch.zeros(2, 256), obj_points=torch.zeros(2, 64, 3)),
                dict(gt=gt)):
        with pytest.raises(ValueError):
            tr.loss_and_grads(bad, t=t)
    with pytest.raises(ValueError):
        tr.grads_at(gt, t, torch.zeros(2, 256), gt)                           # pc in the place of obj_points
    with pytest.raises(ValueError):
        DenoiserTrainer(sd, device='cpu', train_encoder=True).grads_at(gt, t, target=gt, obj_points=torch.zeros(2, 64, 3))
    # without train_pointnet the layout is what it was
    assert DenoiserTrainer(sd, device='cpu', train_encoder=True).n_param == N_FULL


# ------------------------------------------------------------------------------------------------------------ GPU

@pytest.fixture(scope='module')
def tuner(lib):
    """A fine-tuner that is never stepped."""
    from interdiff_amd.pointnet2_train import PointNetFineTuner
    return PointNetFineTuner(weights(), device=DEV)


def plain_encode(ft, pts):
    from interdiff_amd import _lib
    pd = pts.to(DEV).contiguous().float()
    out = torch.empty(pd.shape[0], 256, device=DEV)
    _lib.check(ft.lib.interdiff_pointnet2_encode(C.byref(ft.pn), _lib.dptr(pd), pd.shape[0], pd.shape[1], _lib.dptr(out), _lib.stream()))
    return out


def saves_match(ft, idx):
    """The device's record against the restatement's indices: slots, point ids, duplicate map, hit counts, and the neighbour lists of every distinct centre."""
    sv = ft.saves().cpu().long()
    B = sv.shape[0]
    pid = idx['pid']
    dup = torch.stack([torch.tensor([int((row[:s + 1] == row[s]).nonzero()[0]) for s in range(48)]) for row in pid])
    first = dup == torch.arange(48)[None]
    ok = torch.equal(sv[:, SV_POS:SV_POS + 48], idx['pos']) and torch.equal(sv[:, SV_PID:SV_PID + 48], pid) and torch.equal(sv[:, SV_DUP:SV_DUP + 48], dup)
    ok = ok and torch.equal(sv[:, SV_CNT:SV_CNT + 2], idx['hits2']) and torch.equal(sv[:, SV_CNT + 2:SV_CNT + 98].view(B, 2, 48).permute(0, 2, 1), idx['hits1'])
    nb0, nb1 = sv[:, SV_NB0:SV_NB0 + 768].view(B, 48, 16), sv[:, SV_NB1:SV_NB1 + 1536].view(B, 48, 32)
    return ok and torch.equal(nb0[first], idx['nb0'][first]) and torch.equal(nb1[first], idx['nb1'][first])


@pytest.mark.gpu
@pytest.mark.parametrize('case', ['P2048', 'P1500', 'P700', 'scaled3'])
def test_encode_saved_bits(tuner, case):
    """G1: encode_saved gives the bits of interdiff_pointnet2_encode, and its record is the restatement's sampling and grouping."""
    pts = fx.embedding_inputs()['obj_points']
    pts = dict(P2048=pts, P1500=pts[:, :1500], P700=pts[:, :700], scaled3=3.0 * pts[:2])[case].contiguous()
    got = tuner.encode_saved(pts)
    assert torch.equal(got, plain_encode(tuner, pts))
    assert saves_match(tuner, po().indices(pts))


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['N1', 'N2'])
def test_grads_vs_fp64(tuner, name):
    """G2: every one of the 38 tensors within max(4 e_ref, 1e-5) max|g64| of the fp64 oracle."""
    p = point(name)
    pc = tuner.encode_saved(p['points'])
    assert saves_match(tuner, p['idx'])
    g = tuner.grads(p['d_pc'].to(DEV))
    worst, at = 0.0, ''
    for k, ref in p['ref']['grads'].items():
        f = rel(g[k], ref) / gate(p['e_ref'][k])
        worst, at = max((worst, at), (f, k))
    print('point %s: pc vs fp64 %.2e; worst fraction of the gate max(4 e_ref, 1e-5): %.3f (%s)' % (name, rel(pc, p['ref']['pc']), worst, at))
    assert rel(pc, p['ref']['pc']) <= 1e-5 and worst <= 1.0


@pytest.mark.gpu
def test_grads_bits(tuner):
    """G3: two calls give the same bits; 2 d_pc doubles them exactly; d_pc = 0, and a d_pc that lives in columns 0..2 only, give exact zeros."""
    p = point('N1')
    d = p['d_pc'].to(DEV)
    tuner.encode_saved(p['points'])
    a = tuner.grads(d, flat=True).clone()
    assert torch.equal(a, tuner.grads(d, flat=True)) and bool(a.ne(0).any())
    assert torch.equal(2 * a, tuner.grads(2 * d, flat=True))
    assert not bool(tuner.grads(torch.zeros_like(d), flat=True).ne(0).any())
    xyz = torch.zeros_like(d)
    xyz[:, :3] = d[:, :3]
    assert not bool(tuner.grads(xyz, flat=True).ne(0).any())


@pytest.mark.gpu
def test_refold(lib):
    """G4: after the master vector moved, refold() then encode_saved is the forward oracle on state_dict() within 1e-5; the running statistics keep their bits."""
    from interdiff_amd.pointnet2_train import PointNetFineTuner, POINTNET_STAT_NAMES
    from interdiff_amd.mdm import pack_pointnet2
    from oracle import pointnet2 as opn
    sd = weights()
    ft = PointNetFineTuner(sd, device=DEV)
    pts = fx.embedding_inputs()['obj_points'][:2].contiguous()
    stats0, before = ft.stats.clone(), ft.encode_saved(pts).clone()
    g = torch.Generator().manual_seed(5)
    ft.params.mul_((1 + 0.05 * torch.randn(ft.params.shape, generator=g)).to(DEV))
    assert torch.equal(ft.encode_saved(pts), before)                            # the pack is what the encoder reads
    ft.refold()
    now = {k: v.cpu() for k, v in ft.state_dict().items()}
    got = ft.encode_saved(pts)
    e = rel(got, opn.pointnet2_encode(now, pts))
    host = pack_pointnet2(now, DEV)[1]
    print('refold: encode_saved vs the forward oracle on state_dict() %.2e (gate 1e-5); moved %.2e; arena vs pack_pointnet2: max diff %.1e, bit-equal %s' % (
        e, rel(got, before), float((host - ft.arena).abs().max()), torch.equal(host, ft.arena)))
    assert e <= 1e-5 and rel(got, before) > 1e-3 and rel(ft.arena, host) <= 1e-6
    assert torch.equal(ft.stats, stats0) and all(torch.equal(now[k], sd[k]) for k in POINTNET_STAT_NAMES)


def new_trainer(past, pointnet=True, **kw):
    from interdiff_amd.mdm_train import DenoiserTrainer
    return DenoiserTrainer(weights(), device=DEV, train_encoder=True, train_pointnet=pointnet, past_len=past, **kw)


@pytest.mark.gpu
def test_whole_model_vs_fp64(lib):
    """G5: at W1 the first 228 gradient tensors, d_cond, d_pc and the 16 terms are the bits of DenoiserTrainer(train_encoder=True) on the same raw-points batch; the 38
    new tensors are within their gates."""
    p = point('W1')
    batch = dict(gt=p['x0'].to(DEV), obj_points=p['points'].to(DEV))
    a, b = new_trainer(p['past']), new_trainer(p['past'], pointnet=False)
    ra = a.loss_and_grads(batch, t=p['t'].to(DEV), noise=p['eps'].to(DEV))
    rb = b.loss_and_grads(batch, t=p['t'].to(DEV), noise=p['eps'].to(DEV))
    assert torch.equal(a.grads[:N_FULL], b.grads) and a.grads.numel() == N_FULL + N_PN
    assert torch.equal(ra[0], rb[0]) and torch.equal(ra[-1], rb[-1]) and torch.equal(ra[-2], rb[-2]) and torch.equal(a.cond, b.cond) and torch.equal(a.pred, b.pred)
    assert all(torch.equal(ra[1][k], rb[1][k]) for k in ra[1])
    worst, at = 0.0, ''
    for k, ref in p['ref']['grads'].items():
        f = rel(ra[3][k], ref) / gate(p['e_ref'][k])
        worst, at = max((worst, at), (f, k))
    print('point W1: d_pc vs fp64 %.2e; the 38 tensors: worst fraction of the gate max(4 e_ref, 1e-5): %.3f (%s)' % (rel(ra[-1], p['d_pc']), worst, at))
    assert worst <= 1.0


@pytest.mark.gpu
def test_trajectory_vs_fp64(lib, traj):
    """G6: six AdamW steps on all 266 tensors."""
    from interdiff_amd.mdm_train import FULL_PARAM_NAMES
    from interdiff_amd.pointnet2_train import POINTNET_PARAM_NAMES
    p, z, sd = point('W1'), traj['z'], weights()
    tr = new_trainer(p['past'], lr=float(z['lr']))
    batch = dict(gt=p['x0'].to(DEV), obj_points=p['points'].to(DEV))
    for k, (t, eps) in enumerate(zip(traj['ts'], traj['noises'])):
        loss = tr.training_step(batch, t=t.to(DEV), noise=eps.to(DEV))[0]
        e, er = abs(float(loss.double().mean()) - traj['losses'][k]) / traj['losses'][k], abs(float(loss.double().mean()) - float(z['ref_losses'][k])) / float(z['ref_losses'][k])
        print('step %d: loss %.6f, rel err vs fp64 %.2e, vs the recorded reference loss %.2e (gate 1e-5)' % (k + 1, float(loss.mean()), e, er))
        assert e <= 1e-5 and er <= 1e-5
        if k == 0:
            now = tr.state_dict()
            assert all(not torch.equal(now[n].cpu(), sd[n]) for n in POINTNET_PARAM_NAMES)          # every one of the 38 tensors has moved after step 1
    got = tr.state_dict()
    y = float(z['y_traj'])
    far, worst = far_parameters(got, traj['theta'], FULL_PARAM_NAMES + POINTNET_PARAM_NAMES, y)
    far_pn = far_parameters(got, traj['theta'], POINTNET_PARAM_NAMES, y)[0]
    n = N_FULL + N_PN
    print('trajectory: %d of %d parameters further than 8 y_traj = %.3e from fp64 (cap %d; %d of them in pcEmbedding); max distance %.3e' % (far, n, 8 * y, n // 1000, far_pn, worst))
    assert far <= n // 1000
    assert set(got) == set(sd)
    for k in sd:
        if k not in tr.names:
            assert torch.equal(got[k].cpu(), sd[k]), k                          # running statistics and every other pass-through tensor: identical bits


@pytest.mark.gpu
def test_plumbing(lib, traj):
    """G6, second half: state_dict / optimizer_state continue a trajectory bit for bit; encode_points reads the re-folded pack; the exported sampler model's own
    _get_embeddings gives the trainer's cond."""
    from interdiff_amd import synthetic as syn
    from interdiff_amd.mdm_train import DenoiserTrainer
    p = point('W1')
    batch = dict(gt=p['x0'].to(DEV), obj_points=p['points'].to(DEV))
    step = lambda tr, k: tr.training_step(batch, t=traj['ts'][k].to(DEV), noise=traj['noises'][k].to(DEV))
    a = new_trainer(p['past'])
    step(a, 0), step(a, 1)
    b = DenoiserTrainer(a.state_dict(), device=DEV, train_encoder=True, train_pointnet=True, past_len=p['past'])
    b.load_optimizer_state(a.optimizer_state())
    assert b.step == 2 and torch.equal(a.params, b.params) and b.params.numel() == N_FULL + N_PN
    assert torch.equal(a.pointnet.arena, b.pointnet.arena)                      # the device re-fold and the constructor's host fold agree bit for bit
    assert torch.equal(a.encode_points(batch['obj_points']), a.pointnet.encode_saved(batch['obj_points']))
    step(a, 2), step(b, 2)
    assert torch.equal(a.params, b.params) and torch.equal(a.exp_avg, b.exp_avg) and torch.equal(a.exp_avg_sq, b.exp_avg_sq)
    # a raw clip: three steps on it, then the exported sampler model's own _get_embeddings against the trainer's cond
    T, B, past = 12, 3, 10
    raw = {k: tn(v).to(DEV) for k, v in syn.make_embedding_inputs(seed=78, B=B, T=T, n_points=2048).items()}
    fields = (raw['body_pose'], raw['body_trans'], raw['obj_angles'], raw['obj_trans'], raw['obj_points'])
    c = new_trainer(past, lr=3e-3)
    first = c.export_mdm()
    _, gt = first._get_embeddings(*fields, past_len=past)
    clip = dict(gt=gt.permute(1, 2, 0).unsqueeze(1).contiguous(), obj_points=raw['obj_points'])
    g = torch.Generator(device='cpu').manual_seed(11)
    ts = [torch.randint(0, 1000, (B,), generator=g) for _ in range(4)]
    pc0 = c.encode_points(raw['obj_points'])
    for k in range(3):
        c.training_step(clip, t=ts[k], seed=100 + k)
    c.loss_and_grads(clip, t=ts[3], seed=103)                                   # self.cond of the CURRENT weights
    model = c.export_mdm()
    cond, _ = model._get_embeddings(*fields, past_len=past)
    e, e0 = rel(cond, c.cond), rel(first._get_embeddings(*fields, past_len=past)[0], c.cond)
    pc_moved = rel(c.encode_points(raw['obj_points']), pc0)
    print('export_mdm()._get_embeddings vs the trainer\'s cond after 3 steps: %.3e (gate 1e-4); the untrained model\'s is %.3e away; pc moved %.2e' % (e, e0, pc_moved))
    assert e <= 1e-4 < e0 and pc_moved > 0
    assert torch.equal(model.pn_arena, c.pointnet.arena)                        # the exported pack (host fold) is the trainer's re-folded one
