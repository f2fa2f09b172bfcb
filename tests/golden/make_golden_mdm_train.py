"""Generate tests/golden/mdm_train_{A,B,traj}.npz by running the REFERENCE's own ``MDM`` (model/diffusion_smpl.py, through refshim.py) under its own
``LitInteraction.forward_backward`` (train_diffusion_smpl.py:60-166) with autograd ON, and ``torch.optim.AdamW`` as ``configure_optimizers`` builds it
(:177-183, lr 3e-4, weight decay 0), next to the fp64 oracle tests/mdm_train_oracle.py.  Run in the build container only, never at test time:

    python tests/golden/make_golden_mdm_train.py

The module is in eval(): with the reference's defaults --dropout 0 --cond_mask_prob 0 and stochastic depth at rate 0, train() and eval() compute the
same function, and the LocalAttention shim is eval-only.  ``y['cond']`` is a leaf, so the gradient of bodyEmbedding / objEmbedding is the decoder path's.

Points (weights ``fixtures.mdm_weights_wc()``):
  A     B = 4, T = 35, t = [37, 412, 655, 999]: the scene and eps of make_golden_losses.py                          (M = 140 token rows)
  B     B = 3, T = 100, t = [0, 500, 999]: self-attention over more than one 64-key tile, t = 0, an odd batch        (M = 300)
Recorded per point: the inputs (x0, cond, t, eps, and the rows of the positional table the run reads), the reference's fp32 loss and 16 weighted per-clip vectors, e_ref per tensor =
max|g32 - g64| / max|g64| of the reference's fp32 gradient against the fp64 oracle (144 tensors, then d_cond, then d_pred), and every 64th entry of each
reference gradient tensor (the full gradients are 28 MB; the oracle recomputes them at test time in about a second).
Trajectory: 6 AdamW steps at A's shape on A's scene with recorded per-step t / noise: the reference's fp32 losses, y_traj = max|theta32 - theta64| over all
7,069,900 parameters against the oracle's fp64 trajectory, every 64th entry of its final theta.

Asserted here, on the reference and the oracle alone (change the seeds until they hold, never the conditions): 4 e_ref <= 1e-4 for every tensor; the sampled
reference entries are within 1.01 e_ref of the oracle; none of the 144 gradient tensors is exactly zero.
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
import make_golden as mg                          # noqa: E402
import make_golden_skeleton as mgs                # noqa: E402
import make_golden_losses as mgl                  # noqa: E402
from tests import fixtures as fx                  # noqa: E402
from tests import losses_oracle as lo             # noqa: E402
from tests import mdm_train_oracle as mo          # noqa: E402
from interdiff_amd import synthetic as syn        # noqa: E402
from interdiff_amd.mdm_train import PARAM_NAMES   # noqa: E402

np_ = lambda t: t.detach().cpu().numpy()
PAST, STRIDE, TRAJ_STEPS, LR = 10, 64, 6, 3e-4
POINTS = dict(A=dict(B=4, T=35, t=[37, 412, 655, 999], seed=mgl.SEED), B=dict(B=3, T=100, t=[0, 500, 999], seed=8900))


def scene(B, T, seed):
    bt = syn.make_clip_batch(seed=seed, B=B, T=T, past_len=PAST, n_points=8)
    return torch.from_numpy(bt['gt']), torch.from_numpy(bt['cond']), fx._randn(np.random.RandomState(seed + 1), B, 1, 144, T)


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def pe_rows(net, T, ts):
    """The rows of the sinusoidal table the run reads (frames 0 .. T-1 and the timesteps), as the reference module holds them: sin / cos / exp of fp32 arguments
    differ in the last bits between CPUs, and a gradient that is linear in pe[t] (time_embed.0.weight) would inherit that at the size of e_ref."""
    idx = np.unique(np.concatenate([np.arange(T)] + [np_(t) for t in ts]))
    return dict(pe_idx=idx.astype(np.int64), pe_val=np_(dict(net.named_buffers())['PositionalEmbedding.pe'][torch.from_numpy(idx), 0]))


def sampled(tensors):
    return np.concatenate([np_(t).reshape(-1)[::STRIDE] for t in tensors])


class Lit:
    """What forward_backward reads of LitInteraction, around the reference module ``net``."""

    def __init__(self, tds, gd, diff, net, T):
        self.tds, self.gd, self.seen = tds, gd, {}
        outer = self

        class Watch(torch.nn.Module):
            def forward(self, x, ts, y=None):
                outer.seen['x_t'] = x.detach().clone()
                out = net(x, ts, y=y)
                out.retain_grad()
                outer.seen['out'] = out
                return out
        self.ns = Namespace(args=Namespace(smpl_dim=132, past_len=PAST, future_len=T - PAST, **lo.WEIGHTS), diffusion=diff, ddp_model=Watch(), model=None,
                            current_epoch=0)
        self.ns.l2 = lambda a, b: tds.LitInteraction.l2(self.ns, a, b)
        self.ns.log = lambda *a, **k: None
        self.ns.log_loss_dict = lambda diffusion, ts, losses, loss: self.seen.__setitem__('weighted', torch.stack([losses[k].detach() for k in lo.LOSS_KEYS]))

    def loss(self, x0, cond, t, eps):
        self.ns.schedule_sampler = Namespace(sample=lambda n, device: (t, torch.ones(n)))
        real = self.gd.th.randn_like
        self.gd.th.randn_like = lambda x: eps.clone()
        try:
            return self.tds.LitInteraction.forward_backward(self.ns, x0, {'y': {'cond': cond}})[0]
        finally:
            self.gd.th.randn_like = real


def main():
    tds = mgl.trainer()
    gd, diff = mgl.mgs_diffusion()
    betas = gd.get_named_beta_schedule('cosine', 1000, 1.)
    sd = fx.mdm_weights_wc()
    torch.set_grad_enabled(True)
    for name, pt in POINTS.items():
        x0, cond, eps = scene(pt['B'], pt['T'], pt['seed'])
        t = torch.tensor(pt['t'], dtype=torch.int64)
        net = mg.ref_mdm(sd)
        params = dict(net.named_parameters())
        lit = Lit(tds, gd, diff, net, pt['T'])
        c = cond.clone().requires_grad_(True)
        loss = lit.loss(x0, c, t, eps)
        loss.backward()
        pr = pe_rows(net, pt['T'], [t])
        ref = mo.grads(mo.with_pe_rows(sd, (pr['pe_idx'], pr['pe_val'])), lit.seen['x_t'], t, cond, x0, PAST)
        assert torch.equal(lit.seen['x_t'], lo.q_sample(betas, x0, t, eps))
        g32 = [params[k].grad for k in PARAM_NAMES] + [c.grad, lit.seen['out'].grad]
        g64 = [ref['grads'][k] for k in PARAM_NAMES] + [ref['d_cond'], ref['d_pred']]
        assert all(g is not None and float(g.abs().max()) > 0 for g in g32[:len(PARAM_NAMES)]), 'an exact-zero gradient tensor'
        assert all(p.grad is None for k, p in params.items() if k not in PARAM_NAMES), 'a tensor outside the 144 received a gradient'
        e_ref = np.asarray([rel(a, b) for a, b in zip(g32, g64)])
        worst = int(e_ref[:len(PARAM_NAMES)].argmax())
        print('point %s: loss %.6f  e_ref median %.2e  worst %.2e (%s)  d_cond %.2e  d_pred %.2e' % (
            name, float(loss), np.median(e_ref[:-2]), e_ref[worst], PARAM_NAMES[worst], e_ref[-2], e_ref[-1]))
        assert 4 * e_ref.max() <= 1e-4, 'the reference itself is not within the gate: change the seed'
        for a, b, e in zip(g32, g64, e_ref):
            d = (a.double() - b).abs().reshape(-1)[::STRIDE].max()
            assert float(d) <= 1.01 * e * float(b.abs().max())
        mgs.save('mdm_train_%s.npz' % name, x0=np_(x0), cond=np_(cond), t=np_(t), eps=np_(eps), past_len=np.int64(PAST), ref_loss=np_(loss),
                 ref_weighted=np_(lit.seen['weighted']), e_ref=e_ref, names=np.asarray(PARAM_NAMES + ('d_cond', 'd_pred')), stride=np.int64(STRIDE),
                 ref_grad_samples=sampled(g32[:len(PARAM_NAMES)]), ref_d_cond_samples=sampled([c.grad]), ref_d_pred_samples=sampled([lit.seen['out'].grad]), **pr)

    # ---- trajectory: 6 AdamW steps at A's shape ---------------------------------------------------------------------------------------------------------
    pt = POINTS['A']
    x0, cond, _ = scene(pt['B'], pt['T'], pt['seed'])
    rs = np.random.RandomState(8850)
    ts = [torch.from_numpy(rs.randint(0, 1000, size=pt['B']).astype(np.int64)) for _ in range(TRAJ_STEPS)]
    noises = [fx._randn(rs, *x0.shape) for _ in range(TRAJ_STEPS)]
    net = mg.ref_mdm(sd)
    params = dict(net.named_parameters())
    lit = Lit(tds, gd, diff, net, pt['T'])
    opt = torch.optim.AdamW(params=list(net.parameters()), lr=LR, weight_decay=0)
    losses = []
    for t, eps in zip(ts, noises):
        opt.zero_grad()
        loss = lit.loss(x0, cond, t, eps)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    pr = pe_rows(net, pt['T'], ts)
    l64, th64 = mo.trajectory(mo.with_pe_rows(sd, (pr['pe_idx'], pr['pe_val'])), betas, x0, cond, ts, noises, PAST, lr=LR)
    y = max(float((params[k].detach().double() - th64[k]).abs().max()) for k in PARAM_NAMES)
    move = max(float((th64[k] - sd[k].double()).abs().max()) for k in PARAM_NAMES)
    print('trajectory: losses %s (fp64 %s)  y_traj %.3e  largest move %.3e' % (['%.6f' % v for v in losses], ['%.6f' % v for v in l64], y, move))
    mgs.save('mdm_train_traj.npz', t=np.stack([np_(t) for t in ts]), noise=np.stack([np_(e) for e in noises]), ref_losses=np.asarray(losses, np.float32),
             y_traj=np.float64(y), lr=np.float64(LR), stride=np.int64(STRIDE), ref_theta_samples=sampled([params[k] for k in PARAM_NAMES]), **pr)


if __name__ == '__main__':
    main()
