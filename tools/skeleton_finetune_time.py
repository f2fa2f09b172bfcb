"""hip-event timing of one fine-tuning step of the skeleton correction predictor (interdiff_amd/skeleton_finetune.py,
csrc/skeleton_train.hip) against torch-ROCm eager autograd + torch.optim.Adam on a plain-torch restatement of the same step (fp32, eval-mode
BatchNorm), on the same GPU in the same process; not on the product path.

    python tools/skeleton_finetune_time.py [--reps 30] [--json profiles/skeleton_finetune_time.json]

At B = 32 and B = 64 (T = 20, past_len 10), weights = the seeded synthetic batch of interdiff_amd.synthetic and the checkpoint stand-in
below (the timing does not depend on the weights' values).  Warm-up, then medians of per-call hip-event times, microseconds.  Also prints
the two losses of the first step so that a run shows both sides compute the same thing."""
import argparse
import json
import os
import sys
import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)
from interdiff_amd import skeleton_finetune as sf, synthetic as syn      # noqa: E402
from interdiff_amd.stgcn_pack import STACKS, dct_matrices                # noqa: E402

DEV = 'cuda'
T, PAST = 20, 10
WIDTHS = [(9, 32), (32, 16), (16, 32), (32, 9)] * 2 + [(9, 64), (64, 32), (32, 64), (64, 9)]


def synthetic_state_dict(seed=8100):
    """A state_dict of ObjProjector's shapes with seeded values of a trained model's scale."""
    rs = np.random.RandomState(seed)
    sd = {}
    for li, (ci, co) in enumerate(WIDTHS):
        p, nodes = '%s.%d.' % (STACKS[li // 4], li % 4), (21, 1, 22)[li // 4]
        if li // 4 == 2:
            sd[p + 'gcn.A'] = rs.uniform(-1, 1, (T, nodes, nodes)) / np.sqrt(nodes)
            sd[p + 'gcn.T'] = rs.uniform(-1, 1, (nodes, T, T)) / np.sqrt(T)
        else:
            sd[p + 'gcn.T'] = rs.uniform(-1, 1, (T, T)) / np.sqrt(T)
        for br in ('tcn', 'residual'):
            sd[p + br + '.0.weight'] = rs.standard_normal((co, ci, 1, 1)) / np.sqrt(ci)
            sd[p + br + '.0.bias'] = 0.1 * rs.standard_normal(co)
            sd[p + br + '.1.weight'] = 1 + 0.1 * rs.standard_normal(co)
            sd[p + br + '.1.bias'] = 0.1 * rs.standard_normal(co)
            sd[p + br + '.1.running_mean'] = 0.1 * rs.standard_normal(co)
            sd[p + br + '.1.running_var'] = rs.uniform(0.5, 1.5, co)
        sd[p + 'prelu.weight'] = np.asarray([0.25])
    return {k: np.asarray(v, np.float32) for k, v in sd.items()}


def q2m(q):                                       # (w, x, y, z) -> [.., 9], pytorch3d's un-normalised form
    r, i, j, k = q.unbind(-1)
    s = 2.0 / (q * q).sum(-1)
    return torch.stack([1 - s * (j * j + k * k), s * (i * j - k * r), s * (i * k + j * r), s * (i * j + k * r), 1 - s * (i * i + k * k), s * (j * k - i * r),
                        s * (i * k - j * r), s * (j * k + i * r), 1 - s * (i * i + j * j)], dim=-1)


def d6_to_quat(d6):
    a1, a2 = d6[..., :3], d6[..., 3:]
    b1 = torch.nn.functional.normalize(a1, dim=-1)
    b2 = torch.nn.functional.normalize(a2 - (b1 * a2).sum(-1, keepdim=True) * b1, dim=-1)
    m = torch.cat([b1, b2, torch.cross(b1, b2, dim=-1)], dim=-1)
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = m.unbind(-1)
    tr = torch.stack([1 + m00 + m11 + m22, 1 + m00 - m11 - m22, 1 - m00 + m11 - m22, 1 - m00 - m11 + m22], dim=-1)
    qa = torch.where(tr > 0, torch.sqrt(tr.clamp(min=1e-30)), torch.zeros_like(tr))
    cand = torch.stack([torch.stack([qa[..., 0] ** 2, m21 - m12, m02 - m20, m10 - m01], dim=-1),
                        torch.stack([m21 - m12, qa[..., 1] ** 2, m10 + m01, m02 + m20], dim=-1),
                        torch.stack([m02 - m20, m10 + m01, qa[..., 2] ** 2, m12 + m21], dim=-1),
                        torch.stack([m10 - m01, m20 + m02, m21 + m12, qa[..., 3] ** 2], dim=-1)], dim=-2) / (2.0 * qa.clamp(min=0.1)[..., None])
    idx = qa.argmax(dim=-1)[..., None, None].expand(qa.shape[:-1] + (1, 4))
    return torch.gather(cand, -2, idx).squeeze(-2)


class TorchStep:
    """The same step in plain torch: eval-mode ObjProjector.forward, calc_loss, autograd, Adam."""

    def __init__(self, sd, lr=3e-4):
        self.P = {k: torch.from_numpy(v).to(DEV) for k, v in sd.items()}
        self.names = [n for n, _, _ in sf.param_table(sd)]
        for n in self.names:
            self.P[n].requires_grad_(True)
        self.opt = torch.optim.Adam([self.P[n] for n in self.names], lr=lr)
        d, idct = dct_matrices(T)
        self.dct, self.idct = torch.from_numpy(d).float().to(DEV), torch.from_numpy(idct).float().to(DEV)
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

    def loss(self, body, pose):
        body, pose = body.transpose(0, 1), pose.transpose(0, 1)
        tr, q = pose[..., :3], pose[..., 3:]
        d6 = q2m(torch.cat([q[..., 3:], q[..., :3]], dim=-1))[..., :6]                       # forward's conversion ...
        a6 = q2m(torch.cat([d6[..., 5:6], d6[..., 2:5]], dim=-1))[..., :6]                   # ... and sample's, on the 6-vector's last four
        Tn, B, Pn = body.shape[:3]
        rel = torch.cat([a6[:, :, None].expand(Tn, B, Pn, 6), tr[:, :, None] - body], dim=3)[self.idx]
        rel = torch.einsum('kt,tbpc->bckp', self.dct, rel)
        rel = rel + self.stack(rel, 0)
        multi = torch.cat([rel[:, :6], rel[:, 6:] + torch.einsum('kt,tbpc->bckp', self.dct, body)], dim=1)
        o = torch.einsum('kt,tbc->bck', self.dct, torch.cat([a6, tr], dim=2)[self.idx])[..., None]
        o = o + self.stack(o, 1)
        allx = torch.cat([o, multi], dim=3)
        allx = allx + self.stack(allx, 2)
        res = torch.einsum('tk,bck->tbc', self.idct, allx[..., 0])
        qw = d6_to_quat(res[..., :6])
        pred = torch.cat([res[..., 6:], qw[..., 1:], qw[..., :1]], dim=2)
        mse = lambda a, b: ((a - b) ** 2).mean()
        r, rg, n, ng = pred[..., :4], pose[..., :4], pred[..., 4:], pose[..., 4:]
        P = PAST
        vp, vf = (lambda a: a[1:P + 1] - a[:P]), (lambda a: a[P:] - a[P - 1:-1])
        return (0.05 * (mse(r[:P], rg[:P]) + mse(n[:P], ng[:P]) + mse(vp(r), vp(rg)) + mse(vp(n), vp(ng)))
                + 0.1 * (mse(r[P:], rg[P:]) + mse(n[P:], ng[P:]) + mse(vf(r), vf(rg)) + mse(vf(n), vf(ng))))

    def step(self, body, pose):
        self.opt.zero_grad(set_to_none=True)
        l = self.loss(body, pose)
        l.backward()
        self.opt.step()
        return l.detach()


def median_us(fn, reps, warm=5):
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
        out.append(a.elapsed_time(b) * 1e3)
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    sd = synthetic_state_dict()
    res = {}
    for B in (32, 64):
        bt = {k: torch.from_numpy(v).to(DEV) for k, v in syn.make_skeleton_batch(81, B=B, T=T).items()}
        batch = (bt['body'], bt['obj'], bt['pose'], bt['zero_pose_obj'])
        ft, ts = sf.SkeletonFineTuner(sd, device=DEV), TorchStep(sd)
        l_hip, l_torch = float(ft.training_step(batch)), float(ts.step(bt['body'].float(), bt['pose'].float()))
        print('B = %d: first-step loss hip %.6f, torch %.6f' % (B, l_hip, l_torch))
        res['first_loss_hip_B%d' % B], res['first_loss_torch_B%d' % B] = l_hip, l_torch
        res['hip_training_step_B%d_us' % B] = median_us(lambda: ft.training_step(batch), a.reps)
        res['hip_loss_and_grads_B%d_us' % B] = median_us(lambda: ft._grads(batch), a.reps)
        res['torch_eager_training_step_B%d_us' % B] = median_us(lambda: ts.step(bt['body'].float(), bt['pose'].float()), a.reps)
    for k, v in res.items():
        print('%-44s %12.3f' % (k, v))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(res, open(a.json, 'w'), indent=1, sort_keys=True)


if __name__ == '__main__':
    main()
