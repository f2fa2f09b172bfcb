"""hip-event timing of the denoiser trainer (interdiff_amd/mdm_train.py, csrc/mdm_train.hip) against torch-ROCm eager autograd + torch.optim.AdamW on a
plain-torch fp32 restatement of the same step (oracle/denoiser.py's functions on the GPU, the QaN block restated device-side below), on the same GPU in the
same process; not on the product path.

    python tools/mdm_train_time.py [--blocks 7] [--calls 10] [--json profiles/mdm_train_time.json]

Shapes: B = 16 and 32 at T = 35, B = 16 at T = 100, past_len 10, seeded inputs, the synthetic weights (the timing does not depend on their values).  The two
sides alternate block by block (``--blocks`` blocks of ``--calls`` calls each, after a warm-up block); per quantity the median of the block medians and their
range, milliseconds: the HIP gradient call (forward with saves, 16 terms, backward), the HIP AdamW call, the full HIP step (q_sample + both), the torch step.
Also prints both sides' first-step loss so that a run shows they compute the same thing."""
import argparse
import json
import os
import sys
import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)
from interdiff_amd import synthetic as syn                               # noqa: E402
from interdiff_amd.mdm_train import DenoiserTrainer, PARAM_NAMES        # noqa: E402
from interdiff_amd.mdm import positional_table                          # noqa: E402
from interdiff_amd.losses import LossWeights                            # noqa: E402
from oracle import denoiser as od                                       # noqa: E402

DEV, PAST = 'cuda', 10
SHAPES = ((16, 35), (32, 35), (16, 100))


def qan_block(x, sd, p):
    """oracle.denoiser.qan_block / oracle.local_attn.local_attention (window 1, look +-1, rotary) on the tensors' own device.  x [T,B,D]."""
    T, B, D = x.shape
    q = od.qan_queries(sd, p) * D ** -0.5                                # [Nq, D]
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2, dtype=torch.float32, device=x.device) / D))
    fr = torch.outer(torch.arange(3, dtype=torch.float32, device=x.device), inv)
    fr = torch.cat([fr, fr], dim=-1)                                     # [3, D]: one row per key slot; the query takes the last
    rot = lambda v: torch.cat([-v[..., D // 2:], v[..., :D // 2]], dim=-1)
    q = q * fr[2].cos() + rot(q) * fr[2].sin()
    pad = torch.full((1, B, D), -1.0, dtype=x.dtype, device=x.device)
    xp = torch.cat([pad, x, pad], dim=0)
    keys = torch.stack([xp[j:j + T] for j in range(3)], dim=2)           # [T,B,3,D]
    kr = keys * fr.cos() + rot(keys) * fr.sin()
    sim = torch.einsum('nd,tbjd->tbnj', q, kr)
    pos = torch.arange(T, device=x.device)[:, None] + torch.arange(-1, 2, device=x.device)[None]
    sim = sim.masked_fill(~((pos >= 0) & (pos < T))[:, None, None, :], -torch.finfo(sim.dtype).max)
    o = torch.einsum('tbnj,tbjd->tbnd', torch.softmax(sim, dim=-1), keys)
    return torch.einsum('tbnd,n->tbd', o, sd[p + '.wk'][:, 0])


def forward(sd, x, ts, cond, pe):
    temb = od.time_embedding(sd, ts, pe)
    xt = x.squeeze(1).permute(2, 0, 1)
    h = od._lin(xt[..., :135], sd, 'bodyEmbedding') + od._lin(xt[..., 135:], sd, 'objEmbedding') + temb + pe[:xt.shape[0], None]
    for l in range(od.N_LAYERS):
        p = 'decoder.layers.%d' % l
        if l in od.QAN_LAYERS:
            y = od._ln(h + qan_block(h, sd, p), sd, p + '.norm1')
            y = od._ln(y + od._mha(y, cond, sd, p + '.multihead_attn'), sd, p + '.norm2')
            y = od._ln(y + od._ffn(y, sd, p), sd, p + '.norm3')
            h = h + (y - h)
        else:
            h = od.std_layer(h, cond, sd, p)
    out = torch.cat([od._lin(h, sd, 'bodyFinalLinear'), od._lin(h, sd, 'objFinalLinear')], dim=-1)
    return out.permute(1, 2, 0).unsqueeze(1)


def loss_of(pred, gt, w, P=PAST):
    """mean_b sum_i w_i term_i[b], the terms of train_diffusion_smpl.py:72-134."""
    l2 = lambda a, b: ((a - b) ** 2).mean(dim=[0, 2])
    x, g = pred.squeeze(1).permute(2, 0, 1), gt.squeeze(1).permute(2, 0, 1)
    total = 0.
    for gi, (a, b) in enumerate(((0, 132), (132, 135), (135, 141), (141, 144))):
        xs, gs = x[..., a:b], g[..., a:b]
        total = total + w[gi] * l2(xs[:P], gs[:P]) + w[8 + gi] * l2(xs[P:], gs[P:])
        total = total + w[4 + gi] * (l2(xs[1:P + 1] - xs[:P], 0 * gs[1:P + 1]) + l2(xs[1:P] - xs[:P - 1], xs[2:P + 1] - xs[1:P]))
        total = total + w[12 + gi] * (l2(xs[P:] - xs[P - 1:-1], 0 * gs[P:]) + l2(xs[P - 1:-2] - xs[P:-1], xs[P:-1] - xs[P + 1:]))
    return total.mean()


class TorchStep:
    def __init__(self, sd, lr=3e-4):
        self.sd = {k: torch.as_tensor(v).float().to(DEV) for k, v in sd.items() if k in PARAM_NAMES}
        for v in self.sd.values():
            v.requires_grad_(True)
        self.pe = torch.as_tensor(positional_table()).float().to(DEV)
        self.opt = torch.optim.AdamW(list(self.sd.values()), lr=lr, weight_decay=0.0)
        self.w = LossWeights().vector()

    def step(self, x_t, t, cond, gt):
        self.opt.zero_grad(set_to_none=True)
        loss = loss_of(forward(self.sd, x_t, t, cond, self.pe), gt, self.w)
        loss.backward()
        self.opt.step()
        return loss.detach()


def block_ms(fn, calls):
    out = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def alternate(sides, blocks, calls):
    """The protocol of the trainer timing tools: the ``sides`` {name: callable} alternate block by block, ``blocks`` blocks of ``calls`` calls each after a
    warm-up block that is dropped.  -> {name: dict(median of the block medians, lo, hi)}, milliseconds."""
    meds = {k: [] for k in sides}
    for blk in range(blocks + 1):                                       # block 0 warms every side up and is dropped
        for k, fn in sides.items():
            m = block_ms(fn, calls)
            if blk:
                meds[k].append(m)
    return {k: dict(median=float(np.median(v)), lo=float(min(v)), hi=float(max(v))) for k, v in meds.items()}


def print_sides(row, sides):
    for k in sides:
        print('  %-32s %9.3f  [%.3f, %.3f]' % (k, row[k]['median'], row[k]['lo'], row[k]['hi']))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--blocks', type=int, default=7)
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    sd = {k: torch.from_numpy(v) for k, v in syn.mdm_state_dict(seed=233).items()}
    res = dict(device=torch.cuda.get_device_name(0), blocks=a.blocks, calls=a.calls, shapes=[])
    for B, T in SHAPES:
        bt = syn.make_clip_batch(seed=500 + B + T, B=B, T=T, past_len=PAST, n_points=8)
        gt, cond = torch.from_numpy(bt['gt']).to(DEV), torch.from_numpy(bt['cond']).to(DEV)
        t = torch.from_numpy(np.random.RandomState(B * T).randint(0, 1000, size=B).astype(np.int64)).to(DEV)
        eps = torch.randn(gt.shape, device=DEV, generator=torch.Generator(DEV).manual_seed(1))
        tr, ts = DenoiserTrainer(sd, device=DEV), TorchStep(sd)
        batch = dict(gt=gt, cond=cond)
        x_t = tr.diffusion.q_sample(gt, t, noise=eps)
        first = float(tr.training_step(batch, t=t, noise=eps)[0].mean()), float(ts.step(x_t, t, cond, gt))
        sides = dict(hip_grads_ms=lambda: tr.grads_at(x_t, t, cond, gt), hip_adamw_ms=tr.apply_gradients,
                     hip_training_step_ms=lambda: tr.training_step(batch, t=t, noise=eps), torch_eager_training_step_ms=lambda: ts.step(x_t, t, cond, gt))
        row = dict(B=B, T=T, first_loss_hip=first[0], first_loss_torch=first[1], **alternate(sides, a.blocks, a.calls))
        row['torch_over_hip_step'] = row['torch_eager_training_step_ms']['median'] / row['hip_training_step_ms']['median']
        res['shapes'].append(row)
        print('B = %d, T = %d on %s: first-step loss hip %.6f, torch %.6f' % (B, T, res['device'], first[0], first[1]))
        print_sides(row, sides)
        print('  torch eager step / hip step     %9.2f' % row['torch_over_hip_step'])
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(res, open(a.json, 'w'), indent=1, sort_keys=True)


if __name__ == '__main__':
    main()
