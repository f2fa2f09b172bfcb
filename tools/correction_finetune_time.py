"""hip-event timing of one fine-tuning step of the SMPL contact-frame correction predictor (interdiff_amd/correction_finetune.py,
csrc/objproj_train.hip) against torch-ROCm eager autograd + torch.optim.Adam on a plain-torch fp32 restatement of the same step (eval-mode
BatchNorm, ``initialize=True`` as at epoch 0), on the same GPU in the same process; not on the product path.

    python tools/correction_finetune_time.py [--reps 30] [--json profiles/correction_finetune_time.json]

At B = 16, T = 35, past_len 10, on seeded inputs and the checkpoint stand-in below (the timing does not depend on the weights' values).
Warm-up, then medians of per-call hip-event times, milliseconds.  Also prints the two losses of the first step so that a run shows both
sides compute the same thing."""
import argparse
import json
import os
import sys
import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)
from interdiff_amd import correction_finetune as cft                     # noqa: E402
from interdiff_amd.stgcn_pack import STACKS, dct_matrices                # noqa: E402

DEV = 'cuda'
T, PAST, B, NP, NM = 35, 10, 16, 10, 67
WIDTHS = [(9, 32), (32, 16), (16, 32), (32, 9)] * 3


def synthetic_state_dict(seed=8200):
    """A state_dict of ObjProjector's shapes with seeded values of a trained model's scale."""
    rs = np.random.RandomState(seed)
    sd = {}
    for li, (ci, co) in enumerate(WIDTHS):
        p, nodes = '%s.%d.' % (STACKS[li // 4], li % 4), (NM, 1, NM + 1)[li // 4]
        if li // 4 == 2:
            sd[p + 'gcn.A'] = rs.uniform(-1, 1, (NP, nodes, nodes)) / np.sqrt(nodes)
            sd[p + 'gcn.T'] = rs.uniform(-1, 1, (nodes, NP, NP)) / np.sqrt(NP)
        else:
            sd[p + 'gcn.T'] = rs.uniform(-1, 1, (NP, NP)) / np.sqrt(NP)
        for br in ('tcn', 'residual'):
            sd[p + br + '.0.weight'] = rs.standard_normal((co, ci, 1, 1)) / np.sqrt(ci)
            sd[p + br + '.0.bias'] = 0.1 * rs.standard_normal(co)
            sd[p + br + '.1.weight'] = 1 + 0.1 * rs.standard_normal(co)
            sd[p + br + '.1.bias'] = 0.1 * rs.standard_normal(co)
            sd[p + br + '.1.running_mean'] = 0.1 * rs.standard_normal(co)
            sd[p + br + '.1.running_var'] = rs.uniform(0.5, 1.5, co)
        sd[p + 'prelu.weight'] = np.asarray([0.25])
    return {k: np.asarray(v, np.float32) for k, v in sd.items()}


def synthetic_batch(seed=82, B=B):
    rs = np.random.RandomState(seed)
    walk = lambda scale, step, *s: scale * rs.standard_normal((1, B) + s) + np.cumsum(step * rs.standard_normal((T, B) + s), axis=0)
    mk = np.concatenate([walk(0.3, 0.004, NM, 3), rs.standard_normal((T, B, NM, 3)), (rs.uniform(size=(T, B, NM, 1)) < 0.2).astype(np.float64)], axis=3)
    return {k: torch.from_numpy(v.astype(np.float32)).to(DEV) for k, v in dict(obj_angle=walk(0.3, 0.01, 3), obj_trans=walk(0.3, 0.004, 3), markers=mk).items()}


class TorchStep:
    """The same step in plain torch: eval-mode ObjProjector.forward(initialize=True), calc_loss, autograd, Adam."""

    def __init__(self, sd, lr=3e-4):
        self.P = {k: torch.from_numpy(v).to(DEV) for k, v in sd.items()}
        self.names = [n for n, _, _ in cft.param_table(sd)]
        for n in self.names:
            self.P[n].requires_grad_(True)
        self.opt = torch.optim.Adam([self.P[n] for n in self.names], lr=lr)
        d, idct = dct_matrices(T)
        self.dct, self.idct = torch.from_numpy(d[:NP]).float().to(DEV), torch.from_numpy(idct[:, :NP]).float().to(DEV)
        self.idx = list(range(PAST)) + [PAST - 1] * (T - PAST)

    def layer(self, x, p):
        P = self.P

        def conv_bn(h, c, b):
            y = torch.einsum('oc,nctv->notv', P[p + c + '.weight'][:, :, 0, 0], h) + P[p + c + '.bias'].view(1, -1, 1, 1)
            return ((y - P[p + b + '.running_mean'].view(1, -1, 1, 1)) / torch.sqrt(P[p + b + '.running_var'].view(1, -1, 1, 1) + 1e-5)
                    * P[p + b + '.weight'].view(1, -1, 1, 1) + P[p + b + '.bias'].view(1, -1, 1, 1))
        res = conv_bn(x, 'residual.0', 'residual.1')
        Tm = P[p + 'gcn.T']
        if Tm.dim() == 2:
            g = torch.einsum('nctv,tq->ncqv', x, Tm)
        else:
            g = torch.einsum('nctv,tvw->nctw', torch.einsum('nctv,vtq->ncqv', x, Tm), P[p + 'gcn.A'])
        return torch.nn.functional.prelu(conv_bn(g, 'tcn.0', 'tcn.1') + res, P[p + 'prelu.weight'])

    def stack(self, x, s):
        for l in range(4):
            x = self.layer(x, '%s.%d.' % (STACKS[s], l))
        return x

    def loss(self, d6, trans, hv):
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
        P = PAST
        vp, vf = (lambda a: a[1:P + 1] - a[:P]), (lambda a: a[P:] - a[P - 1:-1])
        return (0.05 * (mse(r[:P], rg[:P]) + mse(n[:P], ng[:P]) + mse(vp(r), vp(rg)) + mse(vp(n), vp(ng)))
                + 0.1 * (mse(r[P:], rg[P:]) + mse(n[P:], ng[P:]) + mse(vf(r), vf(rg)) + mse(vf(n), vf(ng))))

    def step(self, d6, trans, hv):
        self.opt.zero_grad(set_to_none=True)
        l = self.loss(d6, trans, hv)
        l.backward()
        self.opt.step()
        return l.detach()


def median_ms(fn, reps, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    sd, batch = synthetic_state_dict(), synthetic_batch()
    ft, ts = cft.CorrectionFineTuner(sd, T=T, past_len=PAST, device=DEV), TorchStep(sd)
    d6, trans, hv = cft.rotation_6d_of_axis_angle(batch['obj_angle']), batch['obj_trans'], batch['markers'][..., :3].contiguous()
    res = dict(B=B, T=T, device=torch.cuda.get_device_name(0))
    res['first_loss_hip'], res['first_loss_torch'] = float(ft.training_step(batch)), float(ts.step(d6, trans, hv))
    print('B = %d, T = %d on %s: first-step loss hip %.6f, torch %.6f' % (B, T, res['device'], res['first_loss_hip'], res['first_loss_torch']))
    res['hip_training_step_ms'] = median_ms(lambda: ft.training_step(batch), a.reps)
    res['hip_loss_and_grads_ms'] = median_ms(lambda: ft._grads(batch, True), a.reps)
    res['torch_eager_training_step_ms'] = median_ms(lambda: ts.step(d6, trans, hv), a.reps)
    for k in ('hip_training_step_ms', 'hip_loss_and_grads_ms', 'torch_eager_training_step_ms'):
        print('%-36s %10.3f' % (k, res[k]))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(res, open(a.json, 'w'), indent=1, sort_keys=True)


if __name__ == '__main__':
    main()
