"""Generate tests/golden/corr_contact_grad.npz, corr_contact_grad_train.npz, corr_contact_grad_traj.npz and corr_contact_grad_traj_train.npz by running the
REFERENCE's own SMPL correction trainer on its FULL loss: ``LitInteraction.calc_loss_contact`` (train_correction_smpl.py:103-185) on
``ObjProjector.forward`` (model/correction_smpl.py:69-138) with the REAL checkpoint (tests/golden/correction_ckpt.npz), torch autograd and
``torch.optim.Adam`` -- imported read-only through refshim.py, which restates the chamfer op (exact argmin, lowest index wins); Lightning never runs.
Run in the build container only:

    python tests/golden/make_golden_corr_contact_grad.py [eval] [train] [traj] [traj_train]

Inputs: tests/corr_fixtures.scene() (T = 35, B = 4, V = 701, P = 300) and its full-size scene (12 x 2 frames, V = 6890, P = 2048; seed FULL_SEED, stored as f_seed), rebuilt by the tests -- their
checksums are stored -- and ``contact_grad_oracle.apart(scene())`` (prefix a_): in scene() every frame has a penetrating point, so this copy moves clip 0's
object out of its body; its frames have none and their penetration gradient must be exactly zero.  Epochs 5 (initialize, a^2 = 1/16), 10 (a^2 = 1/4) and 20 (a^2 = 1).

corr_contact_grad.npz, per scene (prefix s_ / a_ / f_) and epoch (e5_ / e10_ / e20_), the module in eval():
  pred            the reference's fp32 prediction [T,B,9] -- the point the geometry gradient is taken at
  d32, d64        d (weighted penetration + weighted contact) / d obj_pred: the reference's fp32 autograd, and torch autograd in fp64 on a line-by-line
                  restatement of :121-162 at the same prediction; e_ref = max|d32 - d64|, gmax = max|d64|
  frames, terms   per frame (penetration sum, contact sum, penetrating points, contact vertices); the ten raw terms; loss
  s_ only: the full-loss parameter gradients -- e_ref_p (per tensor max|g32 - g64| / max|g64|), gmax_p, g8 (every 8th entry of the flat fp32 gradient),
  pred64 / d64p (the fp64 oracle's prediction and the geometry gradient there: the ``extra`` tests/correction_finetune_oracle.py needs to rebuild g64)
corr_contact_grad_train.npz: one corr_train-style point, the module in train(): injected masks (``masks_for(seed_mask, 0, B, p)``) and nodes, epoch 20.
corr_contact_grad_traj*.npz: 10 Adam steps (lr 3e-4) over the epoch boundary 9 -> 10 (five steps each: ``initialize`` flips and a^2 goes 0.2025 -> 0.25),
eval() from ``perturbed(sd, seed)`` and train() with a new mask per step (``masks_for(seed, step, B, p)``) and injected nodes, the seeds stored: traj_losses, theta_final, y_traj = max|theta32 - theta64|.

Asserted here on the reference alone (change a seed or the scene until they hold, never the conditions): at every prediction used -- the trajectory's
included -- fp32 and fp64 agree on both index arrays, every sign and every 0.02 test on a labelled vertex; e_ref > 0; each geometry term's gradient is at
least 1 % of the total d_obj_pred norm; at least one frame has a penetrating point and at least one has none, and that frame's penetration gradient is
exactly zero; the closed-form oracle (tests/contact_grad_oracle.py) equals the fp64 autograd to rounding.
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
import make_golden_correction_train as mgt          # noqa: E402
from tests import fixtures as fx                    # noqa: E402
from tests import corr_fixtures as cf               # noqa: E402
from tests import correction_finetune_oracle as fo  # noqa: E402
from tests import correction_train_oracle as to     # noqa: E402
from tests import contact_grad_oracle as cgo        # noqa: E402
from oracle import rotations                        # noqa: E402

np_ = lambda t: t.detach().cpu().numpy()
EPOCHS = (5, 10, 20)
TRAJ_EPOCHS = (9,) * 5 + (10,) * 5
SEED_TRAJ, SEED_MASK, SEED_MASK_TRAJ = 7506, 7601, 7606          # where the search for a seed whose assertions hold starts (first_seed)
LR, WD, P_DROP = 3e-4, 0.0, 0.1
W = mgc.WEIGHTS


FULL_SEED = 9803            # cf.FULL_SEED = 9801 holds for the initialize = False prediction only (one fp32 / fp64 index flip at initialize = True); 9803: the first that holds for both


def full_scene():
    return cf.scene(FULL_SEED, cf.FULL_T, cf.FULL_B, cf.FULL_V, cf.FULL_P)


def geo_weights(epoch):
    a = min(1.0, max(float(epoch) / W['second_stage'], 0)) if W['use_annealing'] else 1
    return max(a ** 2, 0) * W['weight_penetration'], max(a ** 2, 0) * W['weight_contact']


def lit_for(tcs, op, T, epoch):
    args = Namespace(past_len=cf.PAST, future_len=T - cf.PAST, render_epoch=10 ** 9, debug=0, **W)
    return mgc.Lit(tcs.LitInteraction, op, args, epoch)


class Spy:
    """Keeps what point2point_signed returned inside calc_loss_contact."""

    def __init__(self, tcs):
        self.tcs, self.real, self.seen = tcs, tcs.point2point_signed, {}

    def __enter__(self):
        def spy(x, y, **kw):
            r = self.real(x, y, **kw)
            self.seen.update(o2h_signed=r[0], h2o_signed=r[1], yidx=r[2], xidx=r[3])
            return r
        self.tcs.point2point_signed = spy
        return self.seen

    def __exit__(self, *a):
        self.tcs.point2point_signed = self.real


def check_decisions(seen, pred, sc):
    """Every discrete decision of the reference's fp32 run against float64 on the same fp32 inputs (make_golden_corr_losses.check_fp64 without that
    fixture's own conditions on the scene) -> per frame (penetration sum, contact sum, penetrating points, contact vertices)."""
    T_, B_, V_ = sc['human_verts'].shape[:3]
    N = T_ * B_
    hv = sc['human_verts'].reshape(N, V_, 7).astype(np.float64)
    x, xn, lab = hv[..., :3], hv[..., 3:6], hv[..., 6]
    y, _ = cgo.pose(np_(pred).astype(np.float64), sc['obj_points'][..., :3].astype(np.float64))
    xidx, yidx = cgo.nn_index(x, y), cgo.nn_index(y, x)
    assert np.array_equal(xidx, np_(seen['xidx']).astype(np.int64)), 'human->object index differs between fp32 and fp64: another seed'
    assert np.array_equal(yidx, np_(seen['yidx']).astype(np.int64)), 'object->human index differs between fp32 and fp64: another seed'
    take = lambda a, i: np.take_along_axis(a, i[..., None], axis=1)
    y2x = y - take(x, yidx)
    sign = np.sign((take(xn, yidx) * y2x).sum(-1))
    assert np.array_equal(sign, np.sign(np_(seen['o2h_signed']).astype(np.float64))), 'a sign differs between fp32 and fp64: another seed'
    h2o = np.sqrt(((x - take(y, xidx)) ** 2).sum(-1))
    far64, far32 = h2o > 0.02, np.abs(np_(seen['h2o_signed'])) > np.float32(0.02)
    assert np.array_equal(far64[lab > 0.5], far32[lab > 0.5]), 'a 0.02 test on a labelled vertex differs between fp32 and fp64: another seed'
    pen = np_(seen['o2h_signed']) < 0
    o2h, h2o32 = np.abs(np_(seen['o2h_signed'])), np.abs(np_(seen['h2o_signed']))
    mask = far32 & (lab > 0.5)
    return np.stack([(20.0 * o2h * pen).astype(np.float32).sum(1, dtype=np.float64), (h2o32 * mask).sum(1, dtype=np.float64),
                     pen.sum(1).astype(np.float64), mask.sum(1).astype(np.float64)], axis=1)


def restated64(pred, sc, w_pen, w_con):
    """torch autograd in fp64 on :121-162 at ``pred`` -> (d penetration share, d contact share, yidx, xidx)."""
    p = torch.from_numpy(np.asarray(pred, np.float64)).requires_grad_(True)
    T, B = p.shape[:2]
    pts = torch.from_numpy(sc['obj_points'][..., :3].astype(np.float64))
    hv = torch.from_numpy(sc['human_verts'].astype(np.float64)).reshape(T * B, -1, 7)
    x, xn, lab = hv[..., :3], hv[..., 3:6], hv[..., 6]
    rot = rotations.rotation_6d_to_matrix(p[..., :6]).permute(0, 1, 3, 2)
    y = (torch.matmul(pts[None], rot) + p[:, :, None, 6:]).reshape(T * B, -1, 3)
    yidx = torch.from_numpy(cgo.nn_index(y.detach().numpy(), x.numpy()))
    xidx = torch.from_numpy(cgo.nn_index(x.numpy(), y.detach().numpy()))
    ex = lambda i: i[..., None].expand(-1, -1, 3)
    y2x, x2y = y - x.gather(1, ex(yidx)), x - y.gather(1, ex(xidx))
    o2h = y2x.norm(dim=2) * (xn.gather(1, ex(yidx)) * y2x).sum(-1).sign()
    h2o = x2y.norm(dim=2)
    v_contact = ((h2o.abs() > 0.02) & (lab > 0.5)).double()
    w = torch.zeros_like(o2h)
    w[o2h < 0] = 20
    pen, con = (o2h.abs() * w).mean(), (h2o.abs() * v_contact).mean()
    gp, = torch.autograd.grad(w_pen * pen, p, retain_graph=True)
    gc, = torch.autograd.grad(w_con * con, p)
    return gp.numpy(), gc.numpy(), yidx.numpy(), xidx.numpy()


def geometry_point(tcs, op, sc, batch, epoch, forward):
    """The reference's full loss at ``epoch`` on ``forward()`` = (pred, gt) -> (record, loss tensor, pred tensor)."""
    T, B = sc['obj_angle'].shape[:2]
    w_pen, w_con = geo_weights(epoch)
    pred, gt = forward()
    with Spy(tcs) as seen:
        loss, ld, wd = lit_for(tcs, op, T, epoch).calc_loss_contact(pred, gt, batch=batch)
    assert tuple(ld) == mgc.KEYS
    frames = check_decisions(seen, pred.detach(), sc)
    dp32, = torch.autograd.grad(wd['penetration'], pred, retain_graph=True)
    dc32, = torch.autograd.grad(wd['contact'], pred, retain_graph=True)
    d32 = np_(dp32 + dc32)
    gp64, gc64, yidx, xidx = restated64(np_(pred), sc, w_pen, w_con)
    assert np.array_equal(yidx, np_(seen['yidx'])) and np.array_equal(xidx, np_(seen['xidx']))
    d64 = gp64 + gc64
    orc = cgo.geometry(np_(pred), sc['obj_points'], sc['human_verts'], w_pen, w_con)
    closed = float(np.abs(orc['grad'] - d64).max() / np.abs(d64).max())
    assert closed <= 1e-12, closed
    assert np.array_equal(orc['frames'][:, 2:], frames[:, 2:])
    e_ref, gmax = float(np.abs(d32.astype(np.float64) - d64).max()), float(np.abs(d64).max())
    tot = np.linalg.norm(d64)
    share = (np.linalg.norm(gp64) / tot, np.linalg.norm(gc64) / tot)
    pen_frames = frames[:, 2].reshape(T, B)
    print('epoch %2d T = %d B = %d V = %d: e_ref %.3e of gmax %.3e (ratio %.2e); shares of |d_obj_pred|: penetration %.3f contact %.3f; frames with / without '
          'a penetrating point %d / %d; closed form vs autograd %.1e' % (epoch, T, B, sc['human_verts'].shape[2], e_ref, gmax, e_ref / gmax, share[0], share[1],
                                                                       int((pen_frames > 0).sum()), int((pen_frames == 0).sum()), closed))
    assert e_ref > 0 and min(share) >= 0.01
    assert not np_(dp32)[pen_frames == 0].any() and not gp64[pen_frames == 0].any(), 'a frame without a penetrating point has a penetration gradient'
    rec = dict(pred=np_(pred), d32=d32, d64=d64, e_ref=np.float64(e_ref), gmax=np.float64(gmax), frames=frames, loss=np_(loss),
               terms=np_(torch.stack([ld[k].float() for k in mgc.KEYS])), w_geo=np.asarray([w_pen, w_con]))
    return rec, loss, pred


def param_record(names, g32, g64):
    e = np.asarray([float((np_(a).astype(np.float64) - np_(g64[n])).__abs__().max() / np_(g64[n]).__abs__().max()) for n, a in zip(names, g32)])
    flat = np.concatenate([np_(a).ravel() for a in g32])
    return dict(e_ref_p=e, gmax_p=np.asarray([float(a.abs().max()) for a in g32], np.float32), g8=flat[::8].copy())


def eval_reference(tcs, sd, T):
    op = mg.ref_objproj(T, cf.PAST)
    op.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in sd.items()})
    op.args.past_len = cf.PAST
    assert not op.training
    return op


def eval_points(tcs, sd, out):
    with_pen = without_pen = 0
    for pre, sc in (('s_', cf.scene()), ('a_', cgo.apart(cf.scene())), ('f_', full_scene())):
        T = sc['obj_angle'].shape[0]
        batch = cf.as_batch(sc, torch)
        out.update({pre + 'crc_' + k: cf.checksum(v) for k, v in sc.items()})
        for e in EPOCHS:
            op = eval_reference(tcs, sd, T)
            rec, loss, _ = geometry_point(tcs, op, sc, batch, e, lambda: op(batch, e < 10))
            if pre == 's_':
                names = [n for n, _ in op.named_parameters()]
                g32 = torch.autograd.grad(loss, [p for _, p in op.named_parameters()])
                P = fo.leaves(sd)
                pred64 = fo.forward(P, sc, e < 10)[0].detach().numpy()
                d64p = cgo.geometry(pred64, sc['obj_points'], sc['human_verts'], *geo_weights(e))
                assert np.array_equal(d64p['frames'][:, 2:], rec['frames'][:, 2:]), 'the fp64 prediction decides a mask differently: another seed'
                _, _, g64 = fo.loss_and_grads(P, sc, e < 10, d64p['grad'])
                pr = param_record(names, g32, g64)
                worst = int(np.argmax(pr['e_ref_p']))
                print('          full-loss parameter gradients: worst e_ref %.3e (%s)' % (pr['e_ref_p'][worst], names[worst]))
                rec.update(pr, pred64=pred64, d64p=d64p['grad'])
                out['names'] = np.asarray(names)
                out['sizes'] = np.asarray([a.numel() for a in g32], np.int64)
            out.update({'%se%d_%s' % (pre, e, k): v for k, v in rec.items()})
            with_pen, without_pen = with_pen + int((rec['frames'][:, 2] > 0).sum()), without_pen + int((rec['frames'][:, 2] == 0).sum())
            if pre == 'a_':
                assert (rec['frames'][:, 2] > 0).any() and (rec['frames'][:, 2] == 0).any(), 'the apart scene must have frames with and without a penetrating point'
    assert with_pen > 0 and without_pen > 0


def train_point(tcs, sd, out, seed_mask):
    sc = cf.scene()
    batch = cf.as_batch(sc, torch)
    nodes = mgt.injected_for(sc)
    op, _, _ = mgt.reference(tcs, sd)
    masks = to.masks_for(seed_mask, 0, cf.B, P_DROP)
    mgt.set_masks(op, masks, cf.B, P_DROP)

    def forward():
        with mgt.injected_nodes(nodes):
            return op(batch, False)
    rec, loss, _ = geometry_point(tcs, op, sc, batch, 20, forward)
    names = [n for n, _ in op.named_parameters()]
    g32 = torch.autograd.grad(loss, [p for _, p in op.named_parameters()])
    P = to.leaves(sd)
    pred64 = to.forward(P, sc, False, nodes, masks, P_DROP)[0].detach().numpy()
    d64p = cgo.geometry(pred64, sc['obj_points'], sc['human_verts'], *geo_weights(20))
    assert np.array_equal(d64p['frames'][:, 2:], rec['frames'][:, 2:])
    _, _, g64, _ = to.loss_and_grads(P, sc, False, nodes, masks, P_DROP, d64p['grad'])
    pr = param_record(names, g32, g64)
    cmp_ = [i for i, n in enumerate(names) if n not in to.CONV_BIASES]
    print('train() point: worst e_ref %.3e over the compared tensors' % pr['e_ref_p'][cmp_].max())
    rec.update(pr, pred64=pred64, d64p=d64p['grad'], nodes=np.asarray(nodes, np.int32), seed_mask=np.int64(seed_mask), p_drop=np.float64(P_DROP))
    out.update(rec, names=np.asarray(names), **{'crc_' + k: cf.checksum(v) for k, v in sc.items()})


def trajectory(tcs, sd, train, seed):
    """``seed``: the mask seed (train()) or the seed of the 5 % perturbation of the start (eval())."""
    if not train:
        sd = fo.perturbed(sd, seed)
    sc = cf.scene()
    batch = cf.as_batch(sc, torch)
    nodes = mgt.injected_for(sc)
    if train:
        op, _, _ = mgt.reference(tcs, sd)
    else:
        op = eval_reference(tcs, sd, cf.T)
    names = [n for n, _ in op.named_parameters()]
    opt = torch.optim.Adam(params=list(op.parameters()), lr=LR, weight_decay=WD)
    traj = []
    for step, e in enumerate(TRAJ_EPOCHS):
        masks = to.masks_for(seed, step, cf.B, P_DROP) if train else None
        if train:
            mgt.set_masks(op, masks, cf.B, P_DROP)
        opt.zero_grad()
        with Spy(tcs) as seen, mgt.injected_nodes(nodes if train and e >= 10 else None):
            pred, gt = op(batch, e < 10)
            l = lit_for(tcs, op, cf.T, e).calc_loss_contact(pred, gt, batch=batch)[0]
        check_decisions(seen, pred.detach(), sc)
        l.backward()
        opt.step()
        traj.append(float(l))
    # the same steps on the fp64 oracles
    P = fo.leaves(sd)
    pn = fo.param_names(P)
    opt64 = torch.optim.Adam([P[n] for n in pn], lr=LR, weight_decay=WD)
    traj64 = []
    for step, e in enumerate(TRAJ_EPOCHS):
        opt64.zero_grad()
        with torch.enable_grad():
            if train:
                pred, gt, _ = to.forward(P, sc, e < 10, nodes, to.masks_for(seed, step, cf.B, P_DROP), P_DROP)
            else:
                pred, gt = fo.forward(P, sc, e < 10)
            l8 = fo.calc_loss(pred, gt, cf.PAST, fo.WEIGHTS)[0]
            geo = cgo.geometry(pred.detach().numpy(), sc['obj_points'], sc['human_verts'], *geo_weights(e))
            (l8 + (torch.from_numpy(geo['grad']) * pred).sum()).backward()
        if train:
            for n in to.CONV_BIASES:
                P[n].grad.zero_()
        opt64.step()
        traj64.append(float(l8.detach()) + geo['loss'])
    th32 = dict(op.named_parameters())
    cmp_ = [n for n in names if not (train and n in to.CONV_BIASES)]
    y_traj = max(float((th32[n].detach().double() - P[n].detach()).abs().max()) for n in cmp_)
    relv = np.abs(np.asarray(traj) - np.asarray(traj64)) / np.asarray(traj64)
    print('trajectory (%s): losses %s; y_traj %.3e; loss differences <= %.2e relative' % ('train()' if train else 'eval()', ' '.join('%.6f' % v for v in traj), y_traj,
                                                                                        relv.max()))
    assert relv.max() <= 1e-4
    rec = dict(traj_losses=np.asarray(traj, np.float64), traj_losses64=np.asarray(traj64), theta_final=np.concatenate([np_(th32[n]).ravel() for n in names]),
               y_traj=np.float64(y_traj), epochs=np.asarray(TRAJ_EPOCHS, np.int64), lr=np.float64(LR), weight_decay=np.float64(WD), names=np.asarray(names))
    if train:
        rec.update(nodes=np.asarray(nodes, np.int32), seed_mask=np.int64(seed), p_drop=np.float64(P_DROP), buffers_final=mgt.buffers_of(op))
    else:
        rec.update(traj_seed_perturb=np.int64(seed), traj_rel=np.float64(0.05))
    return rec


def first_seed(what, start, run, tries=16):
    """The first seed from ``start`` whose assertions hold (they are conditions on the reference alone)."""
    for seed in range(start, start + tries):
        try:
            return run(seed)
        except AssertionError as e:
            print('%s: seed %d fails (%s)' % (what, seed, e))
    raise SystemExit('%s: no seed in %d .. %d holds' % (what, start, start + tries - 1))


def main():
    torch.set_grad_enabled(True)                                     # (the generators imported above switch it off)
    tcs = mgc.trainer('train_correction_smpl')
    sd = {k: np_(v).astype(np.float32) if v.dtype.is_floating_point else np_(v) for k, v in fx.objproj_weights().items()}
    sdt = {k: v for k, v in sd.items() if not k.endswith('num_batches_tracked')}
    parts = [a for a in sys.argv[1:] if not a.startswith('-')] or ['eval', 'train', 'traj', 'traj_train']
    if 'eval' in parts:
        out = {}
        eval_points(tcs, sd, out)
        mgs.save('corr_contact_grad.npz', f_seed=np.int64(FULL_SEED), apart=np.asarray(cgo.APART), **out)
    if 'train' in parts:
        def run(seed):
            out = {}
            train_point(tcs, sdt, out, seed)
            return out
        mgs.save('corr_contact_grad_train.npz', **first_seed('train() point', SEED_MASK, run))
    if 'traj' in parts:
        mgs.save('corr_contact_grad_traj.npz', **first_seed('eval() trajectory', SEED_TRAJ, lambda seed: trajectory(tcs, sd, False, seed)))
    if 'traj_train' in parts:
        mgs.save('corr_contact_grad_traj_train.npz', **first_seed('train() trajectory', SEED_MASK_TRAJ, lambda seed: trajectory(tcs, sdt, True, seed)))
    for f in ('corr_contact_grad.npz', 'corr_contact_grad_train.npz', 'corr_contact_grad_traj.npz', 'corr_contact_grad_traj_train.npz'):
        assert os.path.getsize(os.path.join(HERE, f)) < 1000000, f


if __name__ == '__main__':
    main()
