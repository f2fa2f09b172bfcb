"""Generate tests/golden/pointnet2_finetune_{N1,N2,W1,traj}.npz by running the REFERENCE's own ``PointNet2Encoder`` (model/layers.py:111-175, through refshim.py), called as
``MDM._get_embeddings`` calls it (model/diffusion_smpl.py:210-211), in eval() with autograd on, next to the fp64 oracle tests/pointnet2_train_oracle.py.  Run in the
build container only, never at test time:

    python tests/golden/make_golden_pointnet2_finetune.py

``pointnet2_ops`` parity stays unpinned (oracle/pointnet2.py): the sampling / grouping indices are the restatement's, computed once in fp32 and shared by the reference's
fp32 run (refshim's PointnetSAModuleMSG computes the same ones from the same fp32 cloud) and the fp64 oracle, so a ball membership cannot differ between them.

Points (weights ``fixtures.mdm_weights_wc()``; clouds ``cloud`` below: a 0.4 m box shell with one point inside |p|^2 <= 1e-3, which FPS skips, and a sparse, placed
neighbourhood of the key point)
  N1    B = 3, P = 2048, d_pc a seeded leaf
  N2    B = 2, P = 700: the FPS positions from 699 on repeat point 0 -- the key point -- and fewer than 16 real centres lie within r = 0.1 of it, so SA2's slot
        list holds that centre several times (and counts those positions as hits); d_pc a seeded leaf
  W1    the whole model under ``LitInteraction.forward_backward`` at B = 3, T = 12, past_len 5, t = [0, 500, 999] (the scene, eps and timesteps of mdm_enc_train_E2),
        ``pc_embedding`` computed from a P = 2048 cloud instead of a leaf
  traj  6 ``torch.optim.AdamW`` steps (lr 3e-4, weight decay 0) at W1's shape and scene with recorded per-step t / noise, all 266 tensors
Recorded per point: the inputs, e_ref per tensor = max|g32_ref - g64| / max|g64| for the 38 ``pcEmbedding.*`` tensors, every 64th entry of each reference gradient, the
margin figures below; for the trajectory the reference's losses, y_traj = max|theta32 - theta64| over all 11,938,309 parameters and every 64th entry of its final theta.

Asserted BEFORE anything is written, on the reference and the oracle alone (a cloud seed that fails is skipped for the next one; the conditions never move):
  * 4 e_ref <= 1e-4 for all 38 tensors, none of which is exactly zero; the sampled reference entries are within 1.01 e_ref of the oracle;
  * the discontinuities are away from the fixture.  delta_max = the largest |fp32 reference - fp64| over all live pre-activations (those whose ReLU output carries a
    non-zero gradient) and over the candidates of all pools that carry gradient; every live |z| and every gap between a pool's winner and its best candidate from a
    DIFFERENT source point is >= 16 delta_max (ties between copies of one point are exact and harmless: the scatter lands on one address either way);
  * a second fp32 evaluation -- the oracle itself in fp32 with every contraction's channels in reversed order -- picks the same ReLU signs and pool winners and lies
    inside every gate max(4 e_ref, 1e-5) max|g64|;
  * coverage, counted and recorded (``cover`` [4,2]: per grouping SA1 r=0.05, SA1 r=0.1, SA2 r=0.1, SA2 r=0.2 the live balls with fewer / more hits than nsample):
    every point has, at both SA1 radii, a ball with fewer and one with more hits than nsample; N1's two SA2 balls have fewer in every clip (padding slots) -- more
    than nsample there means 16 / 32 further distinct centres, the long live path on which the margin condition cannot hold (``cloud``), so the fixture cloud does
    not allow it; N2's two SA2 balls have more (the repeated FPS positions are hits) and hold the key point in >= 2 slots of ONE scale; every clip has a point FPS skips;
  * W1 shows the feature: the reference's pcEmbedding.Linear.weight gradient is larger than 4 e_ref of its own size.
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
from tests import fixtures as fx                  # noqa: E402
from tests import losses_oracle as lo             # noqa: E402
from tests import mdm_train_oracle as mo          # noqa: E402
from tests import mdm_encoder_train_oracle as meo  # noqa: E402
from tests import pointnet2_train_oracle as po    # noqa: E402
from interdiff_amd import synthetic as syn        # noqa: E402
from interdiff_amd.mdm_train import FULL_PARAM_NAMES  # noqa: E402

np_ = mgt.np_
STRIDE, TRAJ_STEPS, LR, FACTOR = 64, 6, 3e-4, 16.0
PN = po.POINTNET_PARAM_NAMES
ALL = FULL_PARAM_NAMES + PN
NSAMPLE = (16, 32, 16, 32)


RING = (0.07, 0.09, 0.13, 0.16, 0.19)                # distances of the five points placed around the key point
N_IN = 40                                             # points inside |p|^2 <= 1e-3: FPS never samples them, ball queries do find them


def cloud(seed, B, P):
    """A cloud whose LIVE PATH is short, so that the margin condition can hold: with the 41 distinct centres a uniform 2048-point shell gives every key point, some
    300,000 pre-activations carry gradient and the smallest of them is within a few delta_max of zero at every seed (400 tried).  Per clip: the box shell of
    ``synthetic.make_embedding_inputs``; point 0 -- the key point, where FPS starts -- is moved to 0.06 from the origin and every shell point within 0.27 of it is
    pushed out by a factor 1.6; point 1 sits 0.035 from the origin (inside r = 0.1 of the key point), points 2..6 at the distances RING from the key point (two inside
    r = 0.1, all inside r = 0.2: both SA2 balls have fewer hits than nsample, 7 distinct centres); points 7..46 lie inside |p| < 0.03, where FPS skips them, so they
    are never centres, but they give the SA1 balls around point 1 and the key point more hits than nsample, while the balls around the outer points hold a few."""
    pts = syn.make_embedding_inputs(seed=seed, B=B, T=1, n_points=P)['obj_points'].astype(np.float64)
    rs = np.random.RandomState(seed + 50000)
    unit = lambda *shape: (lambda v: v / np.linalg.norm(v, axis=-1, keepdims=True))(rs.standard_normal(shape + (3,)))
    for b in range(B):
        key = 0.06 * unit()
        near = np.linalg.norm(pts[b] - key, axis=1) < 0.27
        pts[b, near] *= 1.6
        pts[b, 0] = key
        pts[b, 1] = 0.035 * unit()
        pts[b, 2:7] = key + np.asarray(RING)[:, None] * unit(5)
        pts[b, 7:7 + N_IN] = 0.03 * rs.uniform(0, 1, (N_IN, 1)) ** (1 / 3) * unit(N_IN)
    return torch.from_numpy(pts.astype(np.float32))


def ref_pc(net, pts):
    """model/diffusion_smpl.py:210-211 on the reference module's own submodule -> [B,256]."""
    B = pts.shape[0]
    pc = torch.cat([pts, pts.norm(dim=2, keepdim=True)], dim=2).unsqueeze(0)
    return net.pcEmbedding(pc).view(1, B, -1)[0]


class BnTaps:
    """Forward hooks on the reference module's twelve BatchNorm2d sites: their outputs (the pre-activations) of the last call, in slot form."""

    def __init__(self, net):
        self.out = []
        for sa in net.pcEmbedding.SA_modules:
            for mlp in sa.mlps:
                for l in range(3):
                    mlp[3 * l + 1].register_forward_hook(lambda m, i, o: self.out.append(o.detach().clone()))       # the ReLU behind it works in place

    def slots(self, idx):
        B = idx['pos'].shape[0]
        z = [o.permute(0, 2, 3, 1)[torch.arange(B)[:, None], idx['pos']] for o in self.out[:6]] + [o.permute(0, 2, 3, 1)[:, 0] for o in self.out[6:12]]
        self.out = []
        return z


def cover(idx):
    h1, h2 = idx['hits1'], idx['hits2']
    rows = [h1[..., 0], h1[..., 1], h2[:, 0], h2[:, 1]]
    return np.asarray([[int((r < ns).sum()), int((r > ns).sum())] for r, ns in zip(rows, NSAMPLE)])


def repeats(idx):
    """The largest number of slots of ONE SA2 scale that hold the same centre."""
    return max(int(torch.unique(row, return_counts=True)[1].max()) for part in (idx['pid'][:, :16], idx['pid'][:, 16:]) for row in part)


def check(name, sd, pts, idx, d_pc, g32, zref):
    """The conditions of the module docstring for one point; returns the record's figures.  g32 {name: reference gradient}, zref: BnTaps.slots()."""
    dist = lambda a, b: float((a.double() - b.double()).abs().max())
    r64 = po.grads(sd, pts, idx, d_pc, taps=True)
    top = {k: float(r64['grads'][k].abs().max()) for k in PN}
    assert all(float(g32[k].abs().max()) > 0 and top[k] > 0 for k in PN), 'an exact-zero gradient tensor'
    e_ref = np.asarray([dist(g32[k], r64['grads'][k]) / top[k] for k in PN])
    assert 4 * e_ref.max() <= 1e-4, 'the reference itself is not within the gate (%.2e, %s)' % (e_ref.max(), PN[int(e_ref.argmax())])
    for k, e in zip(PN, e_ref):
        assert float((g32[k].double() - r64['grads'][k]).abs().reshape(-1)[::STRIDE].max()) <= 1.01 * e * top[k]
    # discontinuity margins
    delta = 0.0
    for i, ((tap, z, a, da), z32) in enumerate(zip(r64['taps'], zref)):
        live = da != 0
        if live.any():
            delta = max(delta, float((z32.double() - z)[live].abs().max()))
        if i % 3 == 2:
            used = (da.abs().sum(dim=a.dim() - 2, keepdim=True) != 0).expand_as(a)
            if used.any():
                delta = max(delta, float((torch.relu(z32).double() - a)[used].abs().max()))
    zmin, gap = po.margins(r64['taps'], idx)
    print('point %s: e_ref median %.2e worst %.2e (%s); delta_max %.2e, min live |z| %.2e (x%.0f), min pool gap %.2e (x%.0f)' % (
        name, np.median(e_ref), e_ref.max(), PN[int(e_ref.argmax())], delta, zmin, zmin / delta, gap, gap / delta))
    assert zmin >= FACTOR * delta and gap >= FACTOR * delta, 'a discontinuity is within 16 delta_max of the fixture'
    # a second fp32 evaluation in another summation order decides the same and lies inside every gate
    r32 = po.grads(sd, pts, idx, d_pc, dtype=torch.float32, reverse=True, taps=True)
    assert po.same_decisions(r32['taps'], r64['taps'], idx), 'the reversed fp32 run decides differently'
    frac = max(dist(r32['grads'][k], r64['grads'][k]) / (max(4 * e, 1e-5) * top[k]) for k, e in zip(PN, e_ref))
    print('point %s: the oracle in fp32, reversed channel order: worst fraction of its gate %.3f' % (name, frac))
    assert frac <= 1.0, 'the reversed fp32 run is outside a gate'
    return dict(e_ref=e_ref, delta_max=np.float64(delta), min_live_z=np.float64(zmin), min_pool_gap=np.float64(gap), fp32_reversed_gate_fraction=np.float64(frac),
                g64_max=np.asarray([top[k] for k in PN]), ref_grad_samples=mgt.sampled([g32[k] for k in PN]))


def leaf_point(name, sd, B, P, seed):
    pts = cloud(seed, B, P)
    idx = po.indices(pts)
    d_pc = fx._randn(np.random.RandomState(seed + 1), B, 256)
    net = mg.ref_mdm(sd)
    assert not net.training
    taps = BnTaps(net)
    pc = ref_pc(net, pts)
    (pc * d_pc).sum().backward()
    params = dict(net.named_parameters())
    assert all(p.grad is None for k, p in params.items() if k not in PN), 'a tensor outside pcEmbedding received a gradient'
    module = {k: tuple(v.shape) for k, v in net.state_dict().items() if k.startswith('pcEmbedding.')}
    rec = check(name, sd, pts, idx, d_pc, {k: params[k].grad for k in PN}, taps.slots(idx))
    cv = cover(idx)
    skipped = int(((pts * pts).sum(-1) <= 1e-3).any(dim=1).sum())
    print('point %s: cover (fewer, more than nsample) %s; slots of one scale on one centre %d; clips with a skipped point %d' % (name, cv.tolist(), repeats(idx), skipped))
    assert skipped == B
    assert (cv[:2] > 0).all(), 'SA1: a ball with fewer and one with more hits than nsample at both radii'
    if name == 'N1':
        assert cv[2, 0] == B and cv[3, 0] == B                                   # SA2: padding slots in every clip (truncation: see the module docstring)
    else:
        assert repeats(idx) >= 2 and cv[2, 1] == B and cv[3, 1] == B             # the repeated FPS positions are hits: the slot lists hold the key point several times
    return dict(rec, points=np_(pts), d_pc=np_(d_pc), ref_pc=np_(pc), cover=cv, slot_repeats=np.int64(repeats(idx)), cloud_seed=np.int64(seed),
                names=np.asarray(PN), stride=np.int64(STRIDE), module_names=np.asarray(list(module)), module_shapes=np.asarray([' '.join(map(str, v)) for v in module.values()]),
                **{k: np_(v).astype(np.int32) for k, v in idx.items()})


def first_seed(make, start, tries=400):
    for seed in range(start, start + tries):
        try:
            return make(seed)
        except AssertionError as e:
            print('  seed %d: %s' % (seed, e))
    raise SystemExit('no seed in %d .. %d holds the conditions' % (start, start + tries - 1))


def main():
    sd = fx.mdm_weights_wc()
    torch.set_grad_enabled(True)
    mgs.save('pointnet2_finetune_N1.npz', **first_seed(lambda s: leaf_point('N1', sd, 3, 2048, s), 9100))
    mgs.save('pointnet2_finetune_N2.npz', **first_seed(lambda s: leaf_point('N2', sd, 2, 700, s), 9200))

    # ---- W1: the whole model, pc_embedding computed from points -------------------------------------------------------------------------------------------
    tds = mgl.trainer()
    gd, diff = mgl.mgs_diffusion()
    betas = gd.get_named_beta_schedule('cosine', 1000, 1.)
    torch.set_grad_enabled(True)
    e2 = mge.POINTS['E2']
    B, T, past = e2['B'], e2['T'], e2['past']
    x0, _, eps = mge.scene(B, T, past, e2['seed'], e2['pc_seed'])
    t = torch.tensor(e2['t'], dtype=torch.int64)

    def whole(seed):
        pts = cloud(seed, B, 2048)
        idx = po.indices(pts)
        net = mg.ref_mdm(sd)
        taps = BnTaps(net)
        params = dict(net.named_parameters())
        lit = mge.lit_for(tds, gd, diff, net, T, past)
        pc = ref_pc(net, pts)
        pc.retain_grad()
        loss = lit.loss(x0, mge.ref_cond(net, x0, pc, past), t, eps)
        loss.backward()
        pr = mgt.pe_rows(net, T, [t])
        sdp = mo.with_pe_rows(sd, (pr['pe_idx'], pr['pe_val']))
        ref = meo.grads(sdp, lit.seen['x_t'], t, po.encode(sd, pts, idx), x0, past)
        print('point W1: loss %.6f (fp64 %.6f); d_pc vs fp64 %.2e' % (float(loss), float(ref['loss']), mgt.rel(pc.grad, ref['d_pc'])))
        rec = check('W1', sd, pts, idx, ref['d_pc'], {k: params[k].grad for k in PN}, taps.slots(idx))
        k = 'pcEmbedding.Linear.weight'
        assert float(params[k].grad.abs().max()) > 4 * rec['e_ref'][PN.index(k)] * rec['g64_max'][PN.index(k)], 'the fixture does not show the feature'
        return dict(rec, points=np_(pts), x0=np_(x0), t=np_(t), eps=np_(eps), past_len=np.int64(past), ref_loss=np_(loss), ref_d_pc=np_(pc.grad), cloud_seed=np.int64(seed),
                    names=np.asarray(PN), stride=np.int64(STRIDE), **pr, **{k: np_(v).astype(np.int32) for k, v in idx.items()}), pts, idx
    w1, pts, idx = first_seed(whole, 9300)
    mgs.save('pointnet2_finetune_W1.npz', **w1)

    # ---- trajectory: 6 AdamW steps at W1's shape and scene, all 266 tensors -----------------------------------------------------------------------------------
    rs = np.random.RandomState(9400)
    ts = [torch.from_numpy(rs.randint(0, 1000, size=B).astype(np.int64)) for _ in range(TRAJ_STEPS)]
    noises = [fx._randn(rs, *x0.shape) for _ in range(TRAJ_STEPS)]
    net = mg.ref_mdm(sd)
    params = dict(net.named_parameters())
    before = {k: v.detach().clone() for k, v in net.state_dict().items()}
    lit = mge.lit_for(tds, gd, diff, net, T, past)
    opt = torch.optim.AdamW(params=list(net.parameters()), lr=LR, weight_decay=0)
    losses = []
    for t_, eps_ in zip(ts, noises):
        opt.zero_grad()
        loss = lit.loss(x0, mge.ref_cond(net, x0, ref_pc(net, pts), past), t_, eps_)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    after = net.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before if k not in ALL), 'a tensor outside the 266 (a running statistic) moved'
    assert all(not torch.equal(before[k], after[k]) for k in PN), 'a pcEmbedding tensor did not move'
    pr = mgt.pe_rows(net, T, ts)
    l64, th64 = po.trajectory(mo.with_pe_rows(sd, (pr['pe_idx'], pr['pe_val'])), betas, x0, pts, idx, ts, noises, past, LR)
    dist = {k: (params[k].detach().double() - th64[k]).abs() for k in ALL}
    y = max(float(d.max()) for d in dist.values())
    ypn = max(float(dist[k].max()) for k in PN)
    move = max(float((th64[k] - sd[k].double()).abs().max()) for k in PN)
    print('trajectory: losses %s (fp64 %s)  y_traj %.3e (pcEmbedding %.3e)  largest pcEmbedding move %.3e' % (['%.6f' % v for v in losses], ['%.6f' % v for v in l64], y, ypn, move))
    assert max(abs(a - b) / b for a, b in zip(losses, l64)) <= 1e-5
    mgs.save('pointnet2_finetune_traj.npz', t=np.stack([np_(t_) for t_ in ts]), noise=np.stack([np_(e) for e in noises]), ref_losses=np.asarray(losses, np.float32),
             y_traj=np.float64(y), y_traj_pointnet=np.float64(ypn), lr=np.float64(LR), stride=np.int64(STRIDE), ref_theta_samples=mgt.sampled([params[k] for k in ALL]), **pr)


if __name__ == '__main__':
    main()
