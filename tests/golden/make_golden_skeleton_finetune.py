"""Generate tests/golden/skel_finetune.npz (+ skel_finetune_b1.npz) by running the REFERENCE's own skeleton correction trainer in the
fine-tuning regime: model/correction_skeleton.py ``ObjProjector`` in ``.eval()`` with the REAL checkpoint checkpoints/obj_skeleton.ckpt,
``LitObjInteraction._common_step`` (train_correction_skeleton.py:128-154), torch autograd and ``torch.optim.Adam`` (:41-47) -- imported
read-only through refshim.py, Lightning never runs.  Run in the build container only:

    python tests/golden/make_golden_skeleton_finetune.py

Inputs: tests/skeleton_finetune_oracle.make_batch(7400, B = 3) -- unit quaternions from normalised normals, translation = 0.5 N(0,1)
offset + cumulative sum of 0.02 N(0,1) steps, joints likewise (stored).
skel_finetune.npz (B = 3, the checkpoint as it is):
  body, obj, pose, zero_pose_obj   the batch
  loss, terms                      the reference's fp32 loss and its 8 unweighted terms (dict order = names_terms)
  grads                            every gradient tensor of named_parameters(), flat in that order (names, offsets, sizes)
  traj_losses, theta_final         the 10 losses of the Adam trajectory (lr 3e-4, weight_decay 0) and the parameters after it, flat
  e_ref                            per tensor: max|g32 - g64| / max|g64|, g64 from the fp64 oracle (tests/skeleton_finetune_oracle.py)
  y_traj                           max|theta32 - theta64| after the 10 steps, reference against oracle
  loss64, traj_losses64            the oracle's
skel_finetune_b1.npz (B = 1, batch make_batch(7402, 1), the checkpoint's trainable parameters perturbed by 5 % relative noise,
  ``perturbed(sd, 7401)`` -- rebuilt by the tests from the seed): p1_* inputs, p1_loss, p1_terms, p1_grads, p1_e_ref.  A file of its own:
  three fp32 vectors of 96,110 values do not fit one 1 MB file.
Asserted here, on the reference and the oracle alone: 4 e_ref <= 1e-4 for every tensor at both points; the reference's gradient is exactly
0 in 9,240 entries, all of them the columns of st_gcnns_all.3.gcn.A that feed nodes other than node 0, and the oracle's is 0 in the same
entries; loss[9] < loss[0]; the oracle's trajectory losses are within 1e-6 relative of the reference's.
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
import refshim                                    # noqa: E402
import make_golden_skeleton as mgs                # noqa: E402
import make_golden_corr_losses as mgc             # noqa: E402
from tests import skeleton_finetune_oracle as fo  # noqa: E402

np_ = lambda t: t.detach().cpu().numpy()
SEED, SEED_PERTURB, SEED_B1 = 7400, 7401, 7402
STEPS, LR, WD = 10, 3e-4, 0.0
FLAT_GATE = 1e-4


def reference(tsk, hp, sd):
    cm = refshim.load('model.correction_skeleton')
    op = cm.ObjProjector(Namespace(**hp)).eval()
    missing, unexpected = op.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()}, strict=False)
    assert not unexpected and all(k.endswith('num_batches_tracked') for k in missing), (missing, unexpected)
    return op, mgc.Lit(tsk.LitObjInteraction, op, Namespace(**hp), 0)


def point(tsk, hp, sd, batch_np):
    """-> (reference loss, terms, flat fp32 gradient, per-tensor e_ref, fp64 loss, names, sizes)."""
    op, lit = reference(tsk, hp, sd)
    batch = [torch.from_numpy(a) for a in batch_np]
    names = [n for n, _ in op.named_parameters()]
    assert names == fo.param_names(sd)
    loss, ld, _ = lit._common_step(batch, 0, 'train')
    assert tuple(ld) == fo.MSE_KEYS
    g32 = torch.autograd.grad(loss, [p for _, p in op.named_parameters()])
    l64, _, g64 = fo.loss_and_grads(fo.leaves(sd), batch)
    e_ref = np.asarray([float((a.double() - g64[n]).abs().max() / g64[n].abs().max()) for n, a in zip(names, g32)])
    zero32 = {n: int((a == 0).sum()) for n, a in zip(names, g32) if int((a == 0).sum())}
    zero64 = {n: int((g64[n] == 0).sum()) for n in names if int((g64[n] == 0).sum())}
    return (np_(loss), np_(torch.stack([ld[k] for k in fo.MSE_KEYS])), np.concatenate([np_(a).ravel() for a in g32]), e_ref, float(l64), names,
            [a.numel() for a in g32], zero32, zero64, g32, g64)


def main():
    torch.set_grad_enabled(True)                                     # (the generators imported above switch it off)
    tsk = mgc.trainer('train_correction_skeleton')
    _, sd_t = mgs.ref_objprojector()
    sd = {k: np_(v).astype(np.float32) for k, v in sd_t.items() if not k.endswith('num_batches_tracked')}
    ck = torch.load(mgs.CKPT, map_location='cpu', weights_only=False)
    hp = dict(ck['hyper_parameters'])
    hp.update(render=0, debug=0, render_epoch=10 ** 9)
    print('checkpoint hyper-parameters: lr %g, l2_norm %g, dropout %g' % (hp['lr'], hp['l2_norm'], hp['dropout']))
    for k, v in fo.WEIGHTS.items():
        assert float(hp[k]) == v, k

    # ---- B = 3, the checkpoint as it is
    batch_np = fo.make_batch(SEED, 3)
    loss, terms, grads, e_ref, l64, names, sizes, zero32, zero64, g32, g64 = point(tsk, hp, sd, batch_np)
    worst = int(np.argmax(e_ref))
    print('B = 3: loss fp32 %.8f fp64 %.8f; worst e_ref %.3e (%s); tensors with e_ref >= 1e-5: %d' % (float(loss), l64, e_ref[worst], names[worst], int((e_ref >= 1e-5).sum())))
    assert 4 * e_ref.max() <= FLAT_GATE
    assert zero32 == {'st_gcnns_all.3.gcn.A': 9240} and zero64 == zero32, (zero32, zero64)
    A32 = g32[names.index('st_gcnns_all.3.gcn.A')]
    assert int((A32[:, :, 1:] == 0).sum()) == 9240 and int((A32[:, :, 0] == 0).sum()) == 0          # [t][v][w]: the columns w != 0

    # ---- the Adam trajectory
    op, lit = reference(tsk, hp, sd)
    batch = [torch.from_numpy(a) for a in batch_np]
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
    traj64, th64 = fo.adam_trajectory(sd, batch, STEPS, LR, WD)
    theta64 = torch.cat([th64[n].reshape(-1) for n in names])
    y_traj = float((theta32.double() - theta64).abs().max())
    rel = np.abs(np.asarray(traj) - traj64) / traj64
    print('trajectory: losses %s; y_traj %.3e; loss differences <= %.2e relative; parameters beyond 1e-5: %d of %d'
          % (' '.join('%.6f' % v for v in traj), y_traj, rel.max(), int(((theta32.double() - theta64).abs() > 1e-5).sum()), theta32.numel()))
    assert traj[-1] < traj[0] and rel.max() <= 1e-6

    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    common = dict(names=np.asarray(names), offsets=offsets.astype(np.int64), sizes=np.asarray(sizes, np.int64), names_terms=np.asarray(fo.MSE_KEYS))
    mgs.save('skel_finetune.npz', body=batch_np[0], obj=batch_np[1], pose=batch_np[2], zero_pose_obj=batch_np[3], loss=loss, terms=terms, grads=grads,
             e_ref=e_ref, loss64=np.float64(l64), traj_losses=np.asarray(traj, np.float64), traj_losses64=traj64, theta_final=np_(theta32),
             y_traj=np.float64(y_traj), lr=np.float64(LR), weight_decay=np.float64(WD), seed=np.int64(SEED), **common)

    # ---- B = 1, perturbed parameters
    sd1 = fo.perturbed(sd, SEED_PERTURB)
    b1 = fo.make_batch(SEED_B1, 1)
    loss, terms, grads, e_ref, l64, names1, _, zero32, zero64, _, _ = point(tsk, hp, sd1, b1)
    worst = int(np.argmax(e_ref))
    print('B = 1 perturbed: loss fp32 %.8f fp64 %.8f; worst e_ref %.3e (%s)' % (float(loss), l64, e_ref[worst], names[worst]))
    assert names1 == names and 4 * e_ref.max() <= FLAT_GATE and zero32 == {'st_gcnns_all.3.gcn.A': 9240} and zero64 == zero32
    mgs.save('skel_finetune_b1.npz', p1_body=b1[0], p1_obj=b1[1], p1_pose=b1[2], p1_zero_pose_obj=b1[3], p1_loss=loss, p1_terms=terms, p1_grads=grads,
             p1_e_ref=e_ref, p1_loss64=np.float64(l64), p1_seed_perturb=np.int64(SEED_PERTURB), p1_seed=np.int64(SEED_B1), p1_rel=np.float64(0.05), **common)
    for f in ('skel_finetune.npz', 'skel_finetune_b1.npz'):
        assert os.path.getsize(os.path.join(HERE, f)) < 1000000, f


if __name__ == '__main__':
    main()
