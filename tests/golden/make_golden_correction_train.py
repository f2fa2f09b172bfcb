"""Generate tests/golden/corr_train.npz and corr_train_traj.npz by running the REFERENCE's own SMPL correction trainer the way it trains:
model/correction_smpl.py ``ObjProjector`` in ``.train()`` -- BatchNorm2d on batch statistics, updating its buffers --, ``LitInteraction.calc_loss`` /
``_common_step`` (train_correction_smpl.py:60-101, :187-189), torch autograd and ``torch.optim.Adam`` (:51-58), imported read-only through refshim.py;
Lightning never runs.  Each ``tcn[2]`` (``nn.Dropout(p, inplace=True)``, model/layers.py:317) is replaced by a module that multiplies by an injected
keep mask times s = fp32(1 / (1 - p)): autograd-equivalent to nn.Dropout, and the mask can be shared with the oracle and the kernels.
``torch.multinomial`` (model/correction_smpl.py:132) is replaced, while the reference runs, by a function that returns the injected nodes.  Run in
the build container only:

    python tests/golden/make_golden_correction_train.py            (--search N: print, per point, the first mask seeds whose assertions hold)

Inputs: tests/corr_fixtures.scene() (T = 35, B = 4) and the real checkpoint (tests/golden/correction_ckpt.npz), rebuilt by the tests -- checksums are
stored.  p = 0.1.  Three gradient points, key prefix in brackets, masks ``masks_for(<prefix>seed_mask, 0, B, p)``:
  [i1_]  B = 4, the checkpoint, ``_common_step(batch, 0, 'train')`` at current_epoch 0 (initialize True; its annealed geometry weights are exactly 0)
  [i0_]  B = 4, the checkpoint, initialize False with injected nodes (i0_nodes: clip 0 without contact -> 0; clip 1 -> body marker 5, not its argmax
         node 11; clip 2 -> a hand marker without any contact label, its weight the 0.5 bonus alone; clip 3 -> its argmax node), the objective
         ``calc_loss + (c * obj_pred).sum()``, c = ``extra_gradient(i0_seed_extra, T, B)`` (the d_obj_pred seam)
  [b1_]  B = 1 (clip 1 of the scene), ``perturbed(ckpt, b1_seed_perturb)``, initialize False, node 21 (marker 20, not the argmax node)
Per point: loss, terms (fp32, the reference's 8 unweighted terms), loss64 (the oracle's), g8 (every 8th entry of the flat fp32 gradient -- one whole
vector is 897 KB; the GPU tests compare against the fp64 oracle, not against a stored vector),
  e_ref            per parameter tensor max|g32 - g64| / max|g64|, g64 from tests/correction_train_oracle.py; NaN for the 24 convolution biases, whose
                   exact gradient is 0 (they cancel inside the batch normalisation)
  bias_ratio       per convolution bias: max|g32 bias| / max|g32 weight of the same convolution|
  stats            mean and biased variance of the batch at the 24 BatchNorm sites (fp32, from the inputs the reference's BatchNorms saw), flat in the
                   layout names_buffers / offsets_buffers; buffers_after: the reference's buffers after this one forward
  e_ref_stats, e_ref_buffers   per buffer tensor max|s32 - s64| / max|s64| of those two
  zeros_A          the number of exact zeros in the reference's gradient of st_gcnns_all.3.gcn.A
corr_train_traj.npz: 10 Adam steps (lr 3e-4, weight decay 0) of ``_common_step`` at epoch 0 from the checkpoint (num_batches_tracked reset to 0), B = 4,
a new mask per step ``masks_for(seed_mask, step, 4, p)``: traj_losses, traj_losses64, theta_final (flat fp32), buffers_final, tracked, y_traj =
max|theta32 - theta64| over the compared tensors (all but the 24 convolution biases), y_stats = max|buffers32 - buffers64|, y_bias.
Asserted here, on the reference and the oracle alone (change a mask seed or the scene until they hold, never the conditions): 4 e_ref <= 1e-4 for every
compared tensor, statistic and buffer at every point; bias_ratio <= 1e-5; trajectory losses within 1e-6 relative; loss[9] < loss[0]; the zero pattern of
the gradient of st_gcnns_all.3.gcn.A is the same in the reference and the oracle (in train() the last layer's batch-normalisation backward spreads the
selected node's gradient over every node: the pattern is empty at the points recorded).
"""
import os
import sys
import warnings
from argparse import Namespace
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, '..', '..'))
warnings.filterwarnings('ignore')
import refshim                                      # noqa: E402,F401
import make_golden as mg                            # noqa: E402
import make_golden_skeleton as mgs                  # noqa: E402
import make_golden_corr_losses as mgc               # noqa: E402
from tests import fixtures as fx                    # noqa: E402
from tests import corr_fixtures as cf               # noqa: E402
from tests import correction_train_oracle as to     # noqa: E402
from interdiff_amd.correction_train import init_state_dict      # noqa: E402

np_ = lambda t: t.detach().cpu().numpy()
SEED_MASK = dict(i1=7601, i0=7601, b1=7604, traj=7606)                 # the first seeds from 7601 whose assertions hold (--search)
SEED_PERTURB, SEED_EXTRA, B1_CLIP, B1_NODE = 7501, 7502, 1, 21
P_DROP, STEPS, LR, WD = 0.1, 10, 3e-4, 0.0
FLAT_GATE, BIAS_GATE = 1e-4, 1e-5
ZERO_TENSOR = 'st_gcnns_all.3.gcn.A'


class InjectedDropout(torch.nn.Module):
    """x * (keep mask * s): what nn.Dropout computes, with the mask given."""
    mask = None

    def forward(self, x):
        return x if self.mask is None else x * self.mask


class injected_nodes:
    """While active, ``torch.multinomial(contact_happen, 1)`` returns the injected nodes of the clips that have contact (marker index = node - 1)."""

    def __init__(self, nodes):
        self.nodes = None if nodes is None else [int(n) for n in nodes]

    def __enter__(self):
        self.saved = torch.multinomial

        def pick(w, n, *a, **k):
            assert n == 1 and self.nodes is not None
            idx = torch.tensor([v - 1 for v in self.nodes if v > 0], dtype=torch.int64)[:, None]
            assert idx.shape[0] == w.shape[0] and bool((w.gather(1, idx) > 0).all()), 'an injected node the reference could not have drawn'
            return idx
        torch.multinomial = pick

    def __exit__(self, *a):
        torch.multinomial = self.saved


def clip_of(sc, b):
    return {k: np.ascontiguousarray(v[b:b + 1] if k == 'obj_points' else v[:, b:b + 1]) for k, v in sc.items()}


def reference(tcs, sd):
    op = mg.ref_objproj(cf.T, cf.PAST)
    missing, unexpected = op.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in sd.items()}, strict=False)
    assert not unexpected and all(k.endswith('num_batches_tracked') for k in missing), (missing, unexpected)
    for m in op.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.num_batches_tracked.zero_()
    op.args.past_len = cf.PAST
    op.train()
    seen = {}
    for prefix, _, _ in to.LAYERS:
        stack, l = prefix.split('.')
        layer = getattr(op, stack)[int(l)]
        assert isinstance(layer.tcn[2], torch.nn.Dropout)
        layer.tcn[2] = InjectedDropout()
        for bn, name in ((layer.tcn[1], prefix + '.tcn.1'), (layer.residual[1], prefix + '.residual.1')):
            bn.register_forward_hook(lambda m, inp, out, name=name: seen.__setitem__(name, inp[0].detach()))
    assert op.training and all(m.training for m in op.modules())
    args = Namespace(past_len=cf.PAST, future_len=cf.T - cf.PAST, render_epoch=10 ** 9, debug=0, **mgc.WEIGHTS)
    return op, mgc.Lit(tcs.LitInteraction, op, args, 0), seen


def set_masks(op, flat, B, p):
    md = to.split_masks(flat, B)
    s = np.float32(to.drop_scale(p))
    for prefix, _, _ in to.LAYERS:
        stack, l = prefix.split('.')
        getattr(op, stack)[int(l)].tcn[2].mask = torch.from_numpy(md[prefix].astype(np.float32) * s)


def buffers_of(op):
    sd = op.state_dict()
    return np.concatenate([np_(sd[k]).ravel() for k in to.BUFFERS])


def rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() / np.abs(np.asarray(b, np.float64)).max())


def point(tcs, sd, sc, how, seed_mask, nodes=None, extra=None, check=True):
    """``how``: 'common_step' (epoch 0: initialize True) or 'calc_loss' (initialize False, ``nodes`` injected).  -> (record, common arrays, passed)."""
    op, lit, seen = reference(tcs, sd)
    B = sc['obj_angle'].shape[1]
    masks = to.masks_for(seed_mask, 0, B, P_DROP)
    set_masks(op, masks, B, P_DROP)
    batch = cf.as_batch(sc, torch)
    names = [n for n, _ in op.named_parameters()]
    assert names == to.param_names(sd)
    before = {k: np.asarray(sd[k], np.float64) for k in to.BUFFERS}
    initialize = how == 'common_step'
    if initialize:
        assert extra is None and nodes is None
        loss, ld, wd = lit._common_step(batch, 0, 'train')
        assert float(wd['contact']) == 0 and float(wd['penetration']) == 0
        ld = {k: ld[k] for k in to.MSE_KEYS}
        obj = loss
    else:
        with injected_nodes(nodes):
            pred, gt = op(batch, False)
        loss, ld, wd = lit.calc_loss(pred, gt, batch)
        obj = loss if extra is None else loss + (torch.from_numpy(extra) * pred).sum()
    assert tuple(ld) == to.MSE_KEYS
    g32 = dict(zip(names, torch.autograd.grad(obj, [p for _, p in op.named_parameters()])))
    stats32 = {}
    for k, x in seen.items():
        stats32[k + '.running_mean'] = x.mean(dim=(0, 2, 3))
        stats32[k + '.running_var'] = x.var(dim=(0, 2, 3), unbiased=False)
    l64, _, g64, s64 = to.loss_and_grads(to.leaves(sd), sc, initialize, nodes, masks, P_DROP, extra)
    b64 = to.updated_buffers({k: torch.from_numpy(v) for k, v in before.items()}, s64, B)
    after = op.state_dict()
    cmp_ = to.compared(names)
    e_ref = np.asarray([rel(np_(g32[n]), np_(g64[n])) if n in cmp_ else np.nan for n in names])
    e_stats = np.asarray([rel(np_(stats32[k]), np_(s64[k])) for k in to.BUFFERS])
    e_buf = np.asarray([rel(np_(after[k]), np_(b64[k])) for k in to.BUFFERS])
    ratio = np.asarray([float(g32[n].abs().max() / g32[n[:-4] + 'weight'].abs().max()) for n in to.CONV_BIASES])
    z32, z64 = np_(g32[ZERO_TENSOR]) == 0, np_(g64[ZERO_TENSOR]) == 0
    worst = int(np.nanargmax(e_ref))
    ok = bool(4 * np.nanmax(e_ref) <= FLAT_GATE and 4 * e_stats.max() <= FLAT_GATE and 4 * e_buf.max() <= FLAT_GATE and ratio.max() <= BIAS_GATE
              and np.array_equal(z32, z64))
    print('%-11s B = %d seed %d%s: loss fp32 %.8f fp64 %.8f; worst e_ref %.3e (%s); e_ref_stats <= %.3e, e_ref_buffers <= %.3e; bias ratio <= %.3e; '
          'zeros of d %s: %d / %d%s' % (how, B, seed_mask, '' if nodes is None else ' nodes %r' % (list(nodes),), float(loss), float(l64), e_ref[worst],
                                        names[worst], e_stats.max(), e_buf.max(), ratio.max(), ZERO_TENSOR, int(z32.sum()), int(z64.sum()),
                                        '' if ok else '   -- MISSES'))
    if check:
        assert 4 * np.nanmax(e_ref) <= FLAT_GATE and 4 * e_stats.max() <= FLAT_GATE and 4 * e_buf.max() <= FLAT_GATE
        assert ratio.max() <= BIAS_GATE, ratio.max()
        assert np.array_equal(z32, z64)
    flat = np.concatenate([np_(g32[n]).ravel() for n in names])
    sizes = [g32[n].numel() for n in names]
    bsizes = [after[k].numel() for k in to.BUFFERS]
    rec = dict(loss=np_(loss), terms=np_(torch.stack([ld[k] for k in to.MSE_KEYS])), loss64=np.float64(float(l64)), g8=flat[::8].copy(), e_ref=e_ref,
               bias_ratio=ratio, stats=np.concatenate([np_(stats32[k]).ravel() for k in to.BUFFERS]), buffers_after=buffers_of(op), e_ref_stats=e_stats,
               e_ref_buffers=e_buf, zeros_A=np.int64(z32.sum()), seed_mask=np.int64(seed_mask))
    if nodes is not None:
        rec['nodes'] = np.asarray(nodes, np.int32)
    common = dict(names=np.asarray(names), offsets=np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64), sizes=np.asarray(sizes, np.int64),
                  names_buffers=np.asarray(to.BUFFERS), offsets_buffers=np.concatenate([[0], np.cumsum(bsizes)[:-1]]).astype(np.int64),
                  sizes_buffers=np.asarray(bsizes, np.int64), names_terms=np.asarray(to.MSE_KEYS), p_drop=np.float64(P_DROP))
    return rec, common, ok


def injected_for(sc):
    """The i0 point's nodes (docstring)."""
    contact = sc['markers'][cf.PAST:, :, :, 6].sum(axis=0)
    arg = to.argmax_nodes(sc)
    assert arg[0] == 0 and arg[1] == 11 and contact[1, 5] > 0, arg
    free = [m for m in to.HAND_MARKERS if contact[2, m] == 0]
    assert contact[2].sum() > 0 and free and contact[3].sum() > 0
    nodes = [0, 6, 1 + free[0], arg[3]]
    assert nodes[1] != arg[1] and nodes[2] != arg[2] and to.node_weights(sc)[2, free[0]] == 0.5
    return nodes


def trajectory(tcs, sd, sc, seed_mask, check=True):
    op, lit, _ = reference(tcs, sd)
    batch = cf.as_batch(sc, torch)
    names = [n for n, _ in op.named_parameters()]
    opt = torch.optim.Adam(params=list(op.parameters()), lr=LR, weight_decay=WD)
    traj = []
    for step in range(STEPS):
        set_masks(op, to.masks_for(seed_mask, step, cf.B, P_DROP), cf.B, P_DROP)
        opt.zero_grad()
        l = lit._common_step(batch, 0, 'train')[0]
        l.backward()
        opt.step()
        traj.append(float(l))
    tracked = sorted({int(v) for k, v in op.state_dict().items() if k.endswith('num_batches_tracked')})
    assert tracked == [STEPS], tracked
    traj64, th64, buf64 = to.adam_trajectory_train(sd, sc, STEPS, seed_mask, P_DROP, True, None, LR, WD)
    cmp_ = to.compared(names)
    th32 = dict(op.named_parameters())
    y_traj = max(float((th32[n].detach().double() - th64[n]).abs().max()) for n in cmp_)
    y_bias = max(float((th32[n].detach().double() - th64[n]).abs().max()) for n in to.CONV_BIASES)
    buf32 = buffers_of(op)
    y_stats = float(np.abs(buf32.astype(np.float64) - np.concatenate([np_(buf64[k]).ravel() for k in to.BUFFERS])).max())
    relv = np.abs(np.asarray(traj) - traj64) / traj64
    ok = bool(traj[-1] < traj[0] and relv.max() <= 1e-6)
    print('trajectory seed %d: losses %s; y_traj %.3e; y_stats %.3e; the reference moved a convolution bias by up to %.3e; loss differences <= %.2e relative%s'
          % (seed_mask, ' '.join('%.6f' % v for v in traj), y_traj, y_stats, y_bias, relv.max(), '' if ok else '   -- MISSES'))
    if check:
        assert traj[-1] < traj[0] and relv.max() <= 1e-6
    return dict(traj_losses=np.asarray(traj, np.float64), traj_losses64=traj64, theta_final=np.concatenate([np_(th32[n]).ravel() for n in names]),
                buffers_final=buf32, tracked=np.int64(STEPS), y_traj=np.float64(y_traj), y_stats=np.float64(y_stats), y_bias=np.float64(y_bias),
                lr=np.float64(LR), weight_decay=np.float64(WD), steps=np.int64(STEPS), p_drop=np.float64(P_DROP), seed_mask=np.int64(seed_mask),
                names=np.asarray(names)), ok


def main():
    torch.set_grad_enabled(True)                                     # (the generators imported above switch it off)
    tcs = mgc.trainer('train_correction_smpl')
    sd = {k: np_(v).astype(np.float32) for k, v in fx.objproj_weights().items() if not k.endswith('num_batches_tracked')}
    sc = cf.scene()
    crc = {'crc_' + k: cf.checksum(v) for k, v in sc.items()}
    nodes = injected_for(sc)
    extra = to.extra_gradient(SEED_EXTRA, cf.T, cf.B)
    sd1, sc1 = to.perturbed(sd, SEED_PERTURB), clip_of(sc, B1_CLIP)
    assert to.argmax_nodes(sc1) != [B1_NODE] and to.node_weights(sc1)[0, B1_NODE - 1] > 0
    # a fresh initialisation must at least load strictly into the reference module: its keys and shapes are the module's
    mg.ref_objproj(cf.T, cf.PAST).load_state_dict(init_state_dict(7503), strict=True)
    runs = dict(i1=lambda s, c: point(tcs, sd, sc, 'common_step', s, check=c), i0=lambda s, c: point(tcs, sd, sc, 'calc_loss', s, nodes, extra, check=c),
                b1=lambda s, c: point(tcs, sd1, sc1, 'calc_loss', s, [B1_NODE], check=c), traj=lambda s, c: trajectory(tcs, sd, sc, s, check=c))
    if '--search' in sys.argv:
        n = int(sys.argv[sys.argv.index('--search') + 1])
        for key, run in runs.items():
            good = [s for s in range(7601, 7601 + n) if run(s, False)[-1]]
            print('==== %s: mask seeds whose assertions hold: %r' % (key, good))
        return
    pts, common = {}, None
    for key in ('i1', 'i0', 'b1'):
        rec, common, _ = runs[key](SEED_MASK[key], True)
        pts.update({key + '_' + k: v for k, v in rec.items()})
    mgs.save('corr_train.npz', i0_seed_extra=np.int64(SEED_EXTRA), b1_seed_perturb=np.int64(SEED_PERTURB), b1_rel=np.float64(0.05), b1_clip=np.int64(B1_CLIP),
             **pts, **common, **crc)
    rec, _ = runs['traj'](SEED_MASK['traj'], True)
    mgs.save('corr_train_traj.npz', **rec, **crc)
    for f in ('corr_train.npz', 'corr_train_traj.npz'):
        assert os.path.getsize(os.path.join(HERE, f)) < 1000000, f


if __name__ == '__main__':
    main()
