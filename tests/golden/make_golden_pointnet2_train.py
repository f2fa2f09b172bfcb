"""Generate tests/golden/pointnet2_train_{N1,N2,W1,traj}.npz by running the REFERENCE's own ``PointNet2Encoder`` (model/layers.py:111-175, through refshim.py, whose
``_SA`` uses torch's own ``BatchNorm2d``), called as ``MDM._get_embeddings`` calls it (model/diffusion_smpl.py:210-211), with ``pcEmbedding`` in ``train()`` and autograd
on, next to the fp64 oracle tests/pointnet2_bn_train_oracle.py.  Run in the build container only, never at test time:

    python tests/golden/make_golden_pointnet2_train.py

The rest of the module stays in ``eval()``: the recorder's MDM is built with dropout 0.1, which the package refuses (the reference trains with ``--dropout 0``, where
``train()`` and ``eval()`` of everything but the normalisations compute the same function).  Clouds, weights, the W1 scene and the trajectory's draws are those of
make_golden_pointnet2_finetune.py (imported, not edited); the grouping of the 48 slots is recomputable from the recorded points by the oracle's ``tables``, so the
1024-centre tables are not recorded.

Points
  N1    B = 3, P = 2048, d_pc a seeded leaf
  N2    B = 2, P = 700: the FPS positions from 699 on repeat the key point; the repeats count in the SA1 statistics and are SA2 hits
  W1    the whole model under ``LitInteraction.forward_backward`` at B = 3, T = 12, past_len 5, t = [0, 500, 999]
  traj  6 ``torch.optim.AdamW`` steps at W1: all 266 tensors, the 24 running statistics, ``num_batches_tracked``
Recorded per point: the inputs, e_ref per tensor = max|g32_ref - g64| / max|g64|, e_pc, e_stat per statistic (relative to its largest entry), the reference's
updated statistics, every 64th entry of each reference gradient, the margin figures and F.

Asserted BEFORE anything is written, on the reference and the oracle alone (a cloud seed that fails is skipped for the next one; the conditions never move):
  * none of the 38 gradient tensors is exactly zero; the sampled reference entries are within 1.01 e_ref of the oracle;
  * 4 e_ref <= 1e-4 at N1 and W1.  At N2 (P = 700) the bound is 4 e_ref <= 1e-3: the reference's own fp32 gradient of SA_modules.0.mlps.0.0.weight is a cancelling
    sum under the normalisation there (4e-5 .. 2e-4 from fp64 at every seed tried); of the issue's two alternatives this recorder takes the wider bound, not the
    sum-of-magnitudes scale, and records the per-tensor figures;
  * margins on the DIRECT path (the slot rows whose gradient arrives through a pool, and those pools' candidates; the oracle's ``direct``): every live |z| and
    every winner gap against a different source point is >= F delta_max, delta_max the largest fp32-reference-vs-fp64 difference over those quantities; F = 16, or
    the largest power of two below it (never below 4) that some seed holds when none of TRIES seeds holds 16; F is recorded.  The dense rows cannot be kept off
    their discontinuities; their effect is what e_ref contains;
  * a second fp32 evaluation -- the oracle in fp32 with reversed channel order -- makes the same direct-path decisions and lies inside every gate;
  * coverage as in make_golden_pointnet2_finetune.py (fewer and more hits than nsample at both SA1 radii; N1: padding in both SA2 balls; N2: the key point in >= 2
    slots of one scale); every clip has a point FPS skips;
  * statistics: e_stat is recorded and the reversed fp32 run lies within max(4 e_stat, 1e-6);
  * W1 shows the feature: running_mean of SA_modules.0.mlps.0.1 moves by more than its gate;
  * trajectory: the reference alone holds the cap -- at most 0.1 % of the 11,938,309 parameters beyond 8 y_traj is trivially true of y_traj's definition, so what
    is asserted is losses within 1e-5 of fp64 and num_batches_tracked == 6.
"""
import os
import sys
import warnings
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, '..', '..'))
warnings.filterwarnings('ignore')
import make_golden as mg                          # noqa: E402
import make_golden_skeleton as mgs                # noqa: E402
import make_golden_losses as mgl                  # noqa: E402
import make_golden_mdm_train as mgt               # noqa: E402
import make_golden_mdm_encoder_train as mge       # noqa: E402
import make_golden_pointnet2_finetune as mp       # noqa: E402
from tests import fixtures as fx                  # noqa: E402
from tests import mdm_train_oracle as mo          # noqa: E402
from tests import mdm_encoder_train_oracle as meo  # noqa: E402
from tests import pointnet2_train_oracle as po    # noqa: E402
from tests import pointnet2_bn_train_oracle as bo  # noqa: E402

np_ = mgt.np_
STRIDE, TRAJ_STEPS, LR, TRIES, MAX_BYTES = 64, 6, 3e-4, 400, 1000000
PN, SN = bo.POINTNET_PARAM_NAMES, bo.POINTNET_STAT_NAMES
ALL = meo.FULL_PARAM_NAMES + PN
E_BOUND = dict(N1=1e-4, W1=1e-4, N2=1e-3)
FIRST_SITE = 'pcEmbedding.SA_modules.0.mlps.0.1.running_mean'


def save(name, **arrs):
    mgs.save(name, **arrs)
    size = os.path.getsize(os.path.join(HERE, name))
    assert size < MAX_BYTES, '%s is %d bytes' % (name, size)


def train_net(sd):
    net = mg.ref_mdm(sd)
    net.pcEmbedding.train()
    assert net.pcEmbedding.training and not net.encoder.training
    return net


def ref_stats(net):
    now = net.state_dict()
    assert all(int(now[k]) == 1 for k in now if k.startswith('pcEmbedding.') and k.endswith('num_batches_tracked'))
    return {k: now[k].detach().clone() for k in SN}


def check(name, sd, pts, tb, d_pc, g32, zref, pc32, st32, factor):
    """The conditions of the module docstring for one point at margin factor ``factor``; returns the record's figures."""
    dist = lambda a, b: float((a.double() - b.double()).abs().max())
    r64 = bo.grads(sd, pts, tb, d_pc)
    top = {k: float(r64['grads'][k].abs().max()) for k in PN}
    assert all(float(g32[k].abs().max()) > 0 and top[k] > 0 for k in PN), 'an exact-zero gradient tensor'
    e_ref = np.asarray([dist(g32[k], r64['grads'][k]) / top[k] for k in PN])
    assert 4 * e_ref.max() <= E_BOUND[name], 'the reference itself is not within the gate (%.2e, %s)' % (e_ref.max(), PN[int(e_ref.argmax())])
    for k, e in zip(PN, e_ref):
        assert float((g32[k].double() - r64['grads'][k]).abs().reshape(-1)[::STRIDE].max()) <= 1.01 * e * top[k]
    e_pc = dist(pc32, r64['pc']) / float(r64['pc'].abs().max())
    es = bo.stat_error(st32, r64['stats'])
    e_stat = np.asarray([es[k] for k in SN])
    # margins on the direct path
    d64 = bo.direct(sd, r64['batch'], pts, tb, d_pc)
    delta = 0.0
    for i, ((tap, z, a, da), z32) in enumerate(zip(d64['taps'], zref)):
        live = da != 0
        if live.any():
            delta = max(delta, float((z32.double() - z)[live].abs().max()))
        if i % 3 == 2:
            used = (da.abs().sum(dim=a.dim() - 2, keepdim=True) != 0).expand_as(a)
            if used.any():
                delta = max(delta, float((torch.relu(z32).double() - a)[used].abs().max()))
    zmin, gap = po.margins(d64['taps'], tb)
    print('point %s: e_ref median %.2e worst %.2e (%s); e_pc %.2e; e_stat %.2e .. %.2e; delta_max %.2e, min live |z| %.2e (x%.1f), min pool gap %.2e (x%.1f)' % (
        name, np.median(e_ref), e_ref.max(), PN[int(e_ref.argmax())], e_pc, e_stat.min(), e_stat.max(), delta, zmin, zmin / delta, gap, gap / delta))
    assert zmin >= factor * delta and gap >= factor * delta, 'a discontinuity is within %g delta_max of the fixture (x%.1f)' % (factor, min(zmin, gap) / delta)
    # a second fp32 evaluation in another summation order decides the same on the direct path and lies inside every gate
    r32 = bo.grads(sd, pts, tb, d_pc, dtype=torch.float32, reverse=True)
    d32 = bo.direct(sd, r32['batch'], pts, tb, d_pc, dtype=torch.float32, reverse=True)
    assert po.same_decisions(d32['taps'], d64['taps'], tb), 'the reversed fp32 run decides differently'
    frac = max(dist(r32['grads'][k], r64['grads'][k]) / (max(4 * e, 1e-5) * top[k]) for k, e in zip(PN, e_ref))
    e32 = bo.stat_error(r32['stats'], r64['stats'])
    sfrac = max(e32[k] / max(4 * es[k], 1e-6) for k in SN)
    print('point %s: the oracle in fp32, reversed channel order: worst fraction of its gradient gate %.3f, of its statistics gate %.3f' % (name, frac, sfrac))
    assert frac <= 1.0 and sfrac <= 1.0, 'the reversed fp32 run is outside a gate'
    return dict(e_ref=e_ref, e_pc=np.float64(e_pc), e_stat=e_stat, ref_stats=np.concatenate([np_(st32[k]).reshape(-1) for k in SN]),
                delta_max=np.float64(delta), min_live_z=np.float64(zmin), min_pool_gap=np.float64(gap), factor=np.float64(factor),
                fp32_reversed_gate_fraction=np.float64(frac), fp32_reversed_stat_fraction=np.float64(sfrac),
                g64_max=np.asarray([top[k] for k in PN]), ref_grad_samples=mgt.sampled([g32[k] for k in PN]), names=np.asarray(PN), stat_names=np.asarray(SN),
                stride=np.int64(STRIDE))


def leaf_point(name, sd, B, P, seed, factor):
    pts = mp.cloud(seed, B, P)
    tb = bo.tables(pts)
    d_pc = fx._randn(np.random.RandomState(seed + 1), B, 256)
    net = train_net(sd)
    taps = mp.BnTaps(net)
    pc = mp.ref_pc(net, pts)
    (pc * d_pc).sum().backward()
    params = dict(net.named_parameters())
    assert all(p.grad is None for k, p in params.items() if k not in PN), 'a tensor outside pcEmbedding received a gradient'
    rec = check(name, sd, pts, tb, d_pc, {k: params[k].grad for k in PN}, taps.slots(tb), pc.detach(), ref_stats(net), factor)
    cv = mp.cover(tb)
    skipped = int(((pts * pts).sum(-1) <= 1e-3).any(dim=1).sum())
    print('point %s: cover (fewer, more than nsample) %s; slots of one scale on one centre %d; clips with a skipped point %d' % (name, cv.tolist(), mp.repeats(tb), skipped))
    assert skipped == B
    assert (cv[:2] > 0).all(), 'SA1: a ball with fewer and one with more hits than nsample at both radii'
    if name == 'N1':
        assert cv[2, 0] == B and cv[3, 0] == B
    else:
        assert mp.repeats(tb) >= 2 and cv[2, 1] == B and cv[3, 1] == B
    return dict(rec, points=np_(pts), d_pc=np_(d_pc), ref_pc=np_(pc), cover=cv, slot_repeats=np.int64(mp.repeats(tb)), cloud_seed=np.int64(seed))


def first_seed(make, start):
    """The first seed that holds every condition at F = 16; when none of TRIES does, the first that holds the largest smaller power of two (never below 4)."""
    for factor in (16.0, 8.0, 4.0):
        for seed in range(start, start + TRIES):
            try:
                return make(seed, factor)
            except AssertionError as e:
                print('  seed %d (F = %g): %s' % (seed, factor, e))
    raise SystemExit('no seed in %d .. %d holds the conditions' % (start, start + TRIES - 1))


def main():
    sd = fx.mdm_weights_wc()
    torch.set_grad_enabled(True)
    if 'W' not in sys.argv[1:]:
        save('pointnet2_train_N1.npz', **first_seed(lambda s, f: leaf_point('N1', sd, 3, 2048, s, f), 9100))
        save('pointnet2_train_N2.npz', **first_seed(lambda s, f: leaf_point('N2', sd, 2, 700, s, f), 9200))
        if 'N' in sys.argv[1:]:
            return

    # ---- W1: the whole model, pc_embedding computed from points under batch statistics
    tds = mgl.trainer()
    gd, diff = mgl.mgs_diffusion()
    betas = gd.get_named_beta_schedule('cosine', 1000, 1.)
    torch.set_grad_enabled(True)
    e2 = mge.POINTS['E2']
    B, T, past = e2['B'], e2['T'], e2['past']
    x0, _, eps = mge.scene(B, T, past, e2['seed'], e2['pc_seed'])
    t = torch.tensor(e2['t'], dtype=torch.int64)

    def whole(seed, factor):
        pts = mp.cloud(seed, B, 2048)
        tb = bo.tables(pts)
        net = train_net(sd)
        taps = mp.BnTaps(net)
        params = dict(net.named_parameters())
        lit = mge.lit_for(tds, gd, diff, net, T, past)
        pc = mp.ref_pc(net, pts)
        pc.retain_grad()
        loss = lit.loss(x0, mge.ref_cond(net, x0, pc, past), t, eps)
        loss.backward()
        pr = mgt.pe_rows(net, T, [t])
        sdp = mo.with_pe_rows(sd, (pr['pe_idx'], pr['pe_val']))
        with torch.no_grad():
            pc64 = bo.forward(po.cast(sd, torch.float64), pts.double(), tb)[0]
        ref = meo.grads(sdp, lit.seen['x_t'], t, pc64, x0, past)
        print('point W1: loss %.6f (fp64 %.6f); d_pc vs fp64 %.2e' % (float(loss), float(ref['loss']), mgt.rel(pc.grad, ref['d_pc'])))
        st32 = ref_stats(net)
        rec = check('W1', sd, pts, tb, ref['d_pc'], {k: params[k].grad for k in PN}, taps.slots(tb), pc.detach(), st32, factor)
        i = SN.index(FIRST_SITE)
        moved = float((st32[FIRST_SITE].double() - sd[FIRST_SITE].double()).abs().max()) / float(st32[FIRST_SITE].double().abs().max())
        assert moved > max(4 * rec['e_stat'][i], 1e-6), 'the fixture does not show the feature'
        return dict(rec, points=np_(pts), x0=np_(x0), t=np_(t), eps=np_(eps), past_len=np.int64(past), ref_loss=np_(loss), ref_d_pc=np_(pc.grad), cloud_seed=np.int64(seed),
                    first_site_moved=np.float64(moved), **pr), pts, tb
    w1, pts, tb = first_seed(whole, 9300)
    save('pointnet2_train_W1.npz', **w1)

    # ---- trajectory: 6 AdamW steps at W1's shape and scene, all 266 tensors, the statistics and the counters
    rs = np.random.RandomState(9400)
    ts = [torch.from_numpy(rs.randint(0, 1000, size=B).astype(np.int64)) for _ in range(TRAJ_STEPS)]
    noises = [fx._randn(rs, *x0.shape) for _ in range(TRAJ_STEPS)]
    net = train_net(sd)
    params = dict(net.named_parameters())
    lit = mge.lit_for(tds, gd, diff, net, T, past)
    opt = torch.optim.AdamW(params=list(net.parameters()), lr=LR, weight_decay=0)
    losses = []
    for t_, eps_ in zip(ts, noises):
        opt.zero_grad()
        loss = lit.loss(x0, mge.ref_cond(net, x0, mp.ref_pc(net, pts), past), t_, eps_)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    after = net.state_dict()
    tracked = [k for k in after if k.startswith('pcEmbedding.') and k.endswith('num_batches_tracked')]
    assert len(tracked) == 12 and all(int(after[k]) == TRAJ_STEPS for k in tracked)
    pr = mgt.pe_rows(net, T, ts)
    l64, th64, st64 = bo.trajectory(mo.with_pe_rows(sd, (pr['pe_idx'], pr['pe_val'])), betas, x0, pts, tb, ts, noises, past, LR)
    dist = {k: (params[k].detach().double() - th64[k]).abs() for k in ALL}
    y = max(float(d.max()) for d in dist.values())
    ypn = max(float(dist[k].max()) for k in PN)
    es = bo.stat_error({k: after[k] for k in SN}, st64)
    y_stat = np.asarray([es[k] for k in SN])
    print('trajectory: losses %s (fp64 %s)  y_traj %.3e (pcEmbedding %.3e)  y_stat %.2e .. %.2e' % (['%.6f' % v for v in losses], ['%.6f' % v for v in l64], y, ypn,
                                                                                               y_stat.min(), y_stat.max()))
    assert max(abs(a - b) / b for a, b in zip(losses, l64)) <= 1e-5
    save('pointnet2_train_traj.npz', t=np.stack([np_(t_) for t_ in ts]), noise=np.stack([np_(e) for e in noises]), ref_losses=np.asarray(losses, np.float32),
         y_traj=np.float64(y), y_traj_pointnet=np.float64(ypn), y_stat=y_stat, ref_stats=np.concatenate([np_(after[k]).reshape(-1) for k in SN]), lr=np.float64(LR),
         stride=np.int64(STRIDE), ref_theta_samples=mgt.sampled([params[k] for k in ALL]), **pr)


if __name__ == '__main__':
    main()
