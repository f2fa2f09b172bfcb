"""Device-event timing of the contact / penetration gradient (interdiff_amd/correction_losses.py ``geometry_gradient``, csrc/corr_geometry_grad.hip) and
of a training step of the SMPL correction predictor on the reference's full loss; not on the product path.

    python tools/contact_grad_time.py [--blocks 7] [--steps 10] [--json profiles/contact_grad_time.json]

At B = 16 and B = 32, T = 35, V = 6890, P = 2048 (``corr_fixtures.scene(9900 + B, ...)``, the inputs of tools/corr_loss_time.py), the real checkpoint:
  geometry_grad / forward_terms   ``interdiff_correction_geometry_grads`` against the forward scoring ``interdiff_correction_losses`` on the same inputs
  <trainer>_full / _pose / _predict   ``training_step(batch, 20)`` with the geometry operands (predict -> contact_gradient -> gradients -> Adam -> re-fold)
                                  against the pose-only step the trainers had before (``training_step(batch, 0)``: one pass, ``initialize``) and the
                                  predict pass alone, for ``CorrectionFineTuner`` (ft) and ``CorrectionTrainer`` (tr)
  torch_full                      torch-ROCm eager autograd + Adam on the plain-torch restatement of tools/correction_finetune_time.py plus the two
                                  geometry terms, their nearest neighbours from ``interdiff_point2point_signed``
Every side is warmed up; a timed block is ``steps`` consecutive calls between two device events; the sides alternate block by block; reported: the
median over the blocks of microseconds per call, with min and max."""
import argparse
import json
import os
import sys
import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from interdiff_amd import correction_losses as cl, correction_finetune as cft, correction_train as ct      # noqa: E402
from interdiff_amd.geometry import point2point_signed                                                    # noqa: E402
from tests import corr_fixtures as cf, fixtures as fx                                                      # noqa: E402
from correction_finetune_time import TorchStep, PAST                                                       # noqa: E402

DEV = 'cuda'
T, V, P, EPOCH = 35, 6890, 2048, 20


class TorchFullStep(TorchStep):
    """TorchStep's pose loss (its weights, the 68-node mean) plus the two geometry terms at epoch 20 weights."""

    def loss(self, d6, trans, hv, pts=None, body=None):
        Tn, Bn, Pn = hv.shape[:3]
        rel = torch.cat([d6[:, :, None].expand(Tn, Bn, Pn, 6), trans[:, :, None] - hv], dim=3)[self.idx]
        rel = torch.einsum('kt,tbpc->bckp', self.dct, rel)
        rel = rel + self.stack(rel, 0)
        multi = torch.cat([rel[:, :6], rel[:, 6:] + torch.einsum('kt,tbpc->bckp', self.dct, hv)], dim=1)
        gt = torch.cat([d6, trans], dim=2)
        o = torch.einsum('kt,tbc->bck', self.dct, gt[self.idx])[..., None]
        o = o + self.stack(o, 1)
        allx = torch.cat([o, multi], dim=3)
        allx = allx + self.stack(allx, 2)
        pred = torch.einsum('tk,bckp->tbpc', self.idct, allx).mean(dim=2)
        mse = lambda a, b: ((a - b) ** 2).mean()
        r, rg, n, ng = pred[..., :6], gt[..., :6], pred[..., 6:], gt[..., 6:]
        vp, vf = (lambda a: a[1:PAST + 1] - a[:PAST]), (lambda a: a[PAST:] - a[PAST - 1:-1])
        pose = (0.05 * (mse(r[:PAST], rg[:PAST]) + mse(n[:PAST], ng[:PAST]) + mse(vp(r), vp(rg)) + mse(vp(n), vp(ng)))
                + 0.1 * (mse(r[PAST:], rg[PAST:]) + mse(n[PAST:], ng[PAST:]) + mse(vf(r), vf(rg)) + mse(vf(n), vf(ng))))
        F = torch.nn.functional
        b1 = F.normalize(pred[..., :3], dim=-1)
        b2 = F.normalize(pred[..., 3:6] - (b1 * pred[..., 3:6]).sum(-1, keepdim=True) * b1, dim=-1)
        M = torch.stack([b1, b2, torch.cross(b1, b2, dim=-1)], dim=-2)
        y = (torch.matmul(pts[None, :, :, :3], M.transpose(-1, -2)) + pred[:, :, None, 6:]).reshape(Tn * Bn, -1, 3)
        x, xn, lab = body[..., :3].reshape(Tn * Bn, -1, 3), body[..., 3:6].reshape(Tn * Bn, -1, 3), body[..., 6].reshape(Tn * Bn, -1)
        with torch.no_grad():
            o2h_s, _, yidx, xidx = point2point_signed(x, y.detach(), x_normals=xn)
        ex = lambda i: i.long()[..., None].expand(-1, -1, 3)
        o2h, h2o = (y - x.gather(1, ex(yidx))).norm(dim=2), (x - y.gather(1, ex(xidx))).norm(dim=2)
        pen = (o2h * 20.0 * (o2h_s < 0)).mean()
        con = (h2o * ((h2o.detach() > 0.02) & (lab > 0.5))).mean()
        return pose + 0.1 * pen + 1.0 * con


def block_us(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--blocks', type=int, default=7)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X'
    sd = {k: v.numpy() for k, v in fx.objproj_weights().items()}
    res = {'blocks': a.blocks, 'steps_per_block': a.steps, 'device': torch.cuda.get_device_name(0), 'T': T, 'V': V, 'P': P, 'epoch': EPOCH}
    for B in (16, 32):
        sc = {k: torch.from_numpy(v).to(DEV) for k, v in cf.scene(9900 + B, T, B, V, P).items()}
        batch = dict(sc)
        bare = {k: sc[k] for k in ('obj_angle', 'obj_trans', 'markers')}
        w = cl.CorrectionLossWeights().vector(EPOCH)
        ft = cft.CorrectionFineTuner(sd, T=T, past_len=PAST, device=DEV)
        tr = ct.CorrectionTrainer(sd, T=T, past_len=PAST, dropout=0.1, seed=82, device=DEV)
        ts = TorchFullStep(sd)
        pred = ft.predict(bare, False)
        d6, trans, mk = cft.rotation_6d_of_axis_angle(sc['obj_angle']), sc['obj_trans'], sc['markers'][..., :3].contiguous()
        sides = {
            'geometry_grad': lambda: cl.geometry_gradient(pred, sc['obj_points'], sc['human_verts'], w[0], w[1]),
            'forward_terms': lambda: cl.correction_terms(pred, pred, sc['obj_points'], sc['human_verts'], PAST),
            'ft_full': lambda: ft.training_step(batch, EPOCH), 'ft_pose': lambda: ft.training_step(bare, 0), 'ft_predict': lambda: ft.predict(bare, False),
            'tr_full': lambda: tr.training_step(batch, EPOCH), 'tr_pose': lambda: tr.training_step(bare, 0), 'tr_predict': lambda: tr.predict(bare, False),
            'torch_full': lambda: ts.opt.zero_grad(set_to_none=True) or ts.loss(d6, trans, mk, sc['obj_points'], sc['human_verts']).backward() or ts.opt.step(),
        }
        for fn in sides.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in sides}
        for _ in range(a.blocks):
            for k, fn in sides.items():
                times[k].append(block_us(fn, a.steps))
        for k, v in times.items():
            res['%s_B%d_us' % (k, B)] = {'median': float(np.median(v)), 'min': float(np.min(v)), 'max': float(np.max(v))}
            print('B = %2d  %-14s median %10.1f us (min %.1f, max %.1f over %d blocks of %d)' % (B, k, np.median(v), np.min(v), np.max(v), a.blocks, a.steps))
        m = lambda k: res['%s_B%d_us' % (k, B)]['median']
        res['ratio_grad_over_forward_B%d' % B] = m('geometry_grad') / m('forward_terms')
        for t in ('ft', 'tr'):
            res['%s_full_over_pose_B%d' % (t, B)] = m(t + '_full') / m(t + '_pose')
            res['%s_predict_share_B%d' % (t, B)] = m(t + '_predict') / m(t + '_full')
            res['%s_geometry_share_B%d' % (t, B)] = m('geometry_grad') / m(t + '_full')
        res['torch_full_over_ft_full_B%d' % B] = m('torch_full') / m('ft_full')
        print({k: round(v, 3) for k, v in res.items() if k.endswith('B%d' % B)})
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(res, open(a.json, 'w'), indent=1, sort_keys=True)


if __name__ == '__main__':
    main()
