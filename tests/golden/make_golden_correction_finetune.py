"""Generate tests/golden/corr_finetune.npz, corr_finetune_points.npz and corr_finetune_traj.npz by running the REFERENCE's own SMPL correction
trainer in the fine-tuning regime: model/correction_smpl.py ``ObjProjector`` in ``.eval()`` with the REAL checkpoint checkpoints/correction.ckpt,
``LitInteraction.calc_loss`` / ``_common_step`` (train_correction_smpl.py:60-101, :187-189), torch autograd and ``torch.optim.Adam`` (:51-58) --
imported read-only through refshim.py, Lightning never runs.  Run in the build container only:

    python tests/golden/make_golden_correction_finetune.py

Inputs: tests/corr_fixtures.scene() (T = 35, B = 4: a no-contact clip, a clip whose argmax lands on hand marker 10 through the bonus only, two further
contact clips), rebuilt by the tests -- their checksums are stored.  Four gradient points, key prefix in brackets:
  [i0_]  initialize False: ``calc_loss`` on ``forward(batch, False)``, the checkpoint as it is
  [i1_]  initialize True: ``_common_step(batch, 0, 'train')`` at current_epoch 0 -- its annealed geometry weights are exactly 0 there
  [b1_]  B = 1 (clip B1_CLIP = 1 of the scene, the hand-bonus clip), initialize False, the trainable parameters perturbed by 5 % relative noise
         (``perturbed(sd, SEED_PERTURB)``, rebuilt by the tests from the seed)
  [x_]   the extra-gradient point: the objective ``loss + (c * obj_pred).sum()``, initialize False, c = ``extra_gradient(SEED_EXTRA, T, B)``
Per point: loss, terms (the 8 unweighted terms, dict order = names_terms), loss64 (the fp64 oracle's), e_ref (per tensor max|g32 - g64| / max|g64|, g32 the
reference's fp32 gradient, g64 from tests/correction_finetune_oracle.py), gmax (per tensor max|g32|), g8 (every 8th entry of the flat fp32 gradient),
zeros (flat indices of its exact zeros).  One fp32 vector of 224,174 values is 897 KB, so the FULL fp32 gradient is stored at i0 only (corr_finetune.npz);
the GPU tests compare against the fp64 oracle, not against a stored vector.
corr_finetune_traj.npz: 10 Adam steps (lr 3e-4, weight_decay 0) of ``_common_step`` at epoch 0 (initialize True) from ``perturbed(sd, SEED_TRAJ)``:
traj_losses, traj_losses64, theta_final (flat fp32), y_traj = max|theta32 - theta64|.  The start is perturbed because of the 1e-6 condition below, not
because the checkpoint's loss fails to fall (0.000300 -> 0.000095): the loss is a mean of squared differences of O(1) values that differ by O(1e-2), so
the reference's own fp32 loss carries ~1e-6 relative rounding noise; from the checkpoint it is 1.3e-6 away from the oracle's at one step, from this
start 8.8e-7 at the worst.
Asserted here, on the reference and the oracle alone (change the seed or the scene until they hold, never the conditions): 4 e_ref <= 1e-4 for every tensor
at every point; the reference's exact zeros are all in the columns of st_gcnns_all.3.gcn.A that no clip selects and the oracle's zeros are the same entries;
no tensor has an all-zero gradient; loss[9] < loss[0]; the oracle's trajectory losses are within 1e-6 relative of the reference's.
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
from tests import correction_finetune_oracle as fo  # noqa: E402

np_ = lambda t: t.detach().cpu().numpy()
SEED_PERTURB, SEED_EXTRA, SEED_TRAJ, B1_CLIP = 7501, 7502, 7506, 1
STEPS, LR, WD = 10, 3e-4, 0.0
FLAT_GATE = 1e-4
ZERO_TENSOR = 'st_gcnns_all.3.gcn.A'


def clip_of(sc, b):
    return {k: np.ascontiguousarray(v[b:b + 1] if k == 'obj_points' else v[:, b:b + 1]) for k, v in sc.items()}


def reference(tcs, sd, epoch=0):
    op = mg.ref_objproj(cf.T, cf.PAST)
    op.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in sd.items()})
    op.args.past_len = cf.PAST
    assert not op.training
    args = Namespace(past_len=cf.PAST, future_len=cf.T - cf.PAST, render_epoch=10 ** 9, debug=0, **mgc.WEIGHTS)
    return op, mgc.Lit(tcs.LitInteraction, op, args, epoch)


def selected_nodes(sc):
    """The node each clip's contact rule selects (model/correction_smpl.py:125-136, eval branch)."""
    contact = sc['markers'][cf.PAST:, :, :, 6].sum(axis=0)
    score = contact.copy()
    score[:, fo.HAND_MARKERS] += 0.5
    return [int(1 + np.argmax(score[b])) if contact[b].sum() > 0 else 0 for b in range(contact.shape[0])]


def point(tcs, sd, sc, how, extra=None):
    """``how``: 'calc_loss' (initialize False) or 'common_step' (epoch 0: initialize True).  -> dict of what is recorded, the fp32 and fp64 gradients."""
    op, lit = reference(tcs, sd)
    batch = cf.as_batch(sc, torch)
    names = [n for n, _ in op.named_parameters()]
    assert names == fo.param_names(sd)
    initialize = how == 'common_step'
    if initialize:
        assert extra is None
        loss, ld, wd = lit._common_step(batch, 0, 'train')
        assert float(wd['contact']) == 0 and float(wd['penetration']) == 0 and float(ld['contact']) > 0
        ld = {k: ld[k] for k in fo.MSE_KEYS}
        obj = loss
    else:
        pred, gt = op(batch, False)
        loss, ld, wd = lit.calc_loss(pred, gt, batch)
        obj = loss if extra is None else loss + (torch.from_numpy(extra) * pred).sum()
    assert tuple(ld) == fo.MSE_KEYS
    g32 = torch.autograd.grad(obj, [p for _, p in op.named_parameters()])
    l64, _, g64 = fo.loss_and_grads(fo.leaves(sd), sc, initialize, extra)
    e_ref = np.asarray([float((a.double() - g64[n]).abs().max() / g64[n].abs().max()) for n, a in zip(names, g32)])
    flat = np.concatenate([np_(a).ravel() for a in g32])
    flat64 = np.concatenate([g64[n].numpy().ravel() for n in names])
    assert np.array_equal(flat == 0, flat64 == 0), 'the oracle\'s exact zeros are not the reference\'s'
    assert all(float(a.abs().max()) > 0 for a in g32), 'a tensor with an all-zero gradient'
    sizes = [a.numel() for a in g32]
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    # exact zeros: only in the columns of the last adjacency that no clip selects
    o = int(offsets[names.index(ZERO_TENSOR)])
    zeros = np.flatnonzero(flat == 0)
    assert ((zeros >= o) & (zeros < o + 10 * 68 * 68)).all(), 'an exact zero outside %s' % ZERO_TENSOR
    A0 = (flat[o:o + 10 * 68 * 68] == 0).reshape(10, 68, 68)                        # [t][v][w]
    picked = sorted(set(range(68) if initialize else selected_nodes(sc)))
    unpicked = [w for w in range(68) if w not in picked]
    assert A0[:, :, unpicked].all() and not A0[:, :, picked].any(), 'zeros of %s are not the unselected columns' % ZERO_TENSOR
    worst = int(np.argmax(e_ref))
    print('%-11s B = %d%s: loss fp32 %.8f fp64 %.8f; worst e_ref %.3e (%s); tensors with e_ref >= 2.5e-6: %d; exact zeros %d (nodes selected: %s)'
          % (how, sc['obj_angle'].shape[1], ' + extra' if extra is not None else '', float(loss), float(l64), e_ref[worst], names[worst], int((e_ref >= 2.5e-6).sum()),
             zeros.size, 'all' if initialize else picked))
    assert 4 * e_ref.max() <= FLAT_GATE
    rec = dict(loss=np_(loss), terms=np_(torch.stack([ld[k] for k in fo.MSE_KEYS])), loss64=np.float64(l64), e_ref=e_ref,
               gmax=np.asarray([float(a.abs().max()) for a in g32], np.float32), g8=flat[::8].copy(), zeros=zeros.astype(np.int32))
    common = dict(names=np.asarray(names), offsets=offsets.astype(np.int64), sizes=np.asarray(sizes, np.int64), names_terms=np.asarray(fo.MSE_KEYS))
    return rec, flat, common


def main():
    torch.set_grad_enabled(True)                                     # (the generators imported above switch it off)
    tcs = mgc.trainer('train_correction_smpl')
    sd = {k: np_(v).astype(np.float32) if v.dtype.is_floating_point else np_(v) for k, v in fx.objproj_weights().items()}
    sc = cf.scene()
    crc = {'crc_' + k: cf.checksum(v) for k, v in sc.items()}
    picks = selected_nodes(sc)
    assert picks[0] == 0 and picks[1] == 11 and all(p > 0 for p in picks[1:]), picks

    i0, g_i0, common = point(tcs, sd, sc, 'calc_loss')
    i1, _, _ = point(tcs, sd, sc, 'common_step')
    sd1 = fo.perturbed(sd, SEED_PERTURB)
    b1, _, _ = point(tcs, sd1, clip_of(sc, B1_CLIP), 'calc_loss')
    extra = fo.extra_gradient(SEED_EXTRA, cf.T, cf.B)
    x, _, _ = point(tcs, sd, sc, 'calc_loss', extra)

    mgs.save('corr_finetune.npz', grads=g_i0, **{'i0_' + k: v for k, v in i0.items()}, **common, **crc)
    pts = {}
    for pre, rec in (('i1_', i1), ('b1_', b1), ('x_', x)):
        pts.update({pre + k: v for k, v in rec.items()})
    mgs.save('corr_finetune_points.npz', b1_seed_perturb=np.int64(SEED_PERTURB), b1_rel=np.float64(0.05), b1_clip=np.int64(B1_CLIP),
             x_seed=np.int64(SEED_EXTRA), **pts, **common, **crc)

    # ---- the Adam trajectory: _common_step at epoch 0 (initialize True), from perturbed parameters (see the docstring)
    sdt = fo.perturbed(sd, SEED_TRAJ)
    op, lit = reference(tcs, sdt)
    batch = cf.as_batch(sc, torch)
    names = [n for n, _ in op.named_parameters()]
    opt = torch.optim.Adam(params=list(op.parameters()), lr=LR, weight_decay=WD)
    before = {k: v.clone() for k, v in op.state_dict().items() if 'running' in k or 'tracked' in k}
    traj = []
    for _ in range(STEPS):
        opt.zero_grad()
        l = lit._common_step(batch, 0, 'train')[0]
        l.backward()
        opt.step()
        traj.append(float(l))
    assert all(torch.equal(v, op.state_dict()[k]) for k, v in before.items())                        # eval(): the BatchNorm buffers never move
    theta32 = torch.cat([p.detach().reshape(-1) for _, p in op.named_parameters()])
    traj64, th64 = fo.adam_trajectory(sdt, sc, STEPS, True, LR, WD)
    theta64 = torch.cat([th64[n].reshape(-1) for n in names])
    y_traj = float((theta32.double() - theta64).abs().max())
    rel = np.abs(np.asarray(traj) - traj64) / traj64
    print('trajectory: losses %s; y_traj %.3e; loss differences <= %.2e relative; parameters beyond 1e-5: %d of %d'
          % (' '.join('%.6f' % v for v in traj), y_traj, rel.max(), int(((theta32.double() - theta64).abs() > 1e-5).sum()), theta32.numel()))
    assert traj[-1] < traj[0] and rel.max() <= 1e-6
    mgs.save('corr_finetune_traj.npz', traj_losses=np.asarray(traj, np.float64), traj_losses64=traj64, theta_final=np_(theta32), y_traj=np.float64(y_traj),
             lr=np.float64(LR), weight_decay=np.float64(WD), traj_seed_perturb=np.int64(SEED_TRAJ), traj_rel=np.float64(0.05), **common, **crc)
    for f in ('corr_finetune.npz', 'corr_finetune_points.npz', 'corr_finetune_traj.npz'):
        assert os.path.getsize(os.path.join(HERE, f)) < 1000000, f


if __name__ == '__main__':
    main()
