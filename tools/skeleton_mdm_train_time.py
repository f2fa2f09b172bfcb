"""hip-event timing of the skeleton denoiser's trainer (interdiff_amd/skeleton_mdm_train.py, csrc/skeleton_mdm_train.hip) against torch-ROCm eager autograd +
torch.optim.AdamW on a plain-torch fp32 restatement of the same step (oracle/denoiser.py's functions on the GPU, the QaN block of tools/mdm_train_time.py), on the
same GPU in the same process; not on the product path.  Protocol of tools/mdm_train_time.py.

    python tools/skeleton_mdm_train_time.py [--blocks 7] [--calls 10] [--json profiles/skeleton_mdm_train_time.json]

Shapes: B = 32 (the reference's default batch) and B = 16 at T = 35, past_len 10, seeded inputs, the synthetic weights.  The two sides alternate block by block
(``--blocks`` blocks of ``--calls`` calls each, after a warm-up block); per quantity the median of the block medians and their range, milliseconds: the HIP gradient
call (encoder and decoder forward with saves, head, 13 terms, the whole backward), the HIP AdamW call, the full HIP step (q_sample + both), the torch step.
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
from interdiff_amd.skeleton_mdm_train import SkeletonDenoiserTrainer, PARAM_NAMES, tokens_of    # noqa: E402
from interdiff_amd.mdm import positional_table                          # noqa: E402
from interdiff_amd.skeleton_losses import SkeletonLossWeights           # noqa: E402
from oracle import denoiser as od                                       # noqa: E402
from tools.mdm_train_time import alternate, print_sides, qan_block      # noqa: E402

DEV, PAST = 'cuda', 10
SHAPES = ((32, 35), (16, 35))


def quaternion_to_matrix(q):
    r, i, j, k = q.unbind(-1)
    s2 = 2.0 / (q * q).sum(-1)
    rows = [1 - s2 * (j * j + k * k), s2 * (i * j - k * r), s2 * (i * k + j * r), s2 * (i * j + k * r), 1 - s2 * (i * i + k * k), s2 * (j * k - i * r),
            s2 * (i * k - j * r), s2 * (j * k + i * r), 1 - s2 * (i * i + j * j)]
    return torch.stack(rows, dim=-1).reshape(q.shape[:-1] + (3, 3))


def encode(sd, gt, zpo, pe):
    tok = gt.squeeze(1).permute(2, 0, 1)[:PAST]
    h = od._lin(tok[..., :63], sd, 'bodyEmbedding') + od._lin(tok[..., 63:99], sd, 'objEmbedding') + od._lin(zpo.reshape(1, zpo.shape[0], -1), sd, 'shapeEmbedding')
    h = h + pe[:PAST, None]
    for l in range(od.N_LAYERS):
        p = 'encoder.layers.%d' % l
        if l in od.QAN_LAYERS:
            y = od._ln(h + qan_block(h, sd, p), sd, p + '.norm1')
            y = od._ln(y + od._ffn(y, sd, p), sd, p + '.norm2')
            h = h + (y - h)
        else:
            h = od.enc_std_layer(h, sd, p)
    return h


def forward(sd, x, ts, zpo, cond, pe):
    temb = od.time_embedding(sd, ts, pe)
    xt = x.squeeze(1).permute(2, 0, 1)
    T, B, _ = xt.shape
    h = od._lin(xt[..., :63], sd, 'bodyEmbedding') + od._lin(xt[..., 63:99], sd, 'objEmbedding') + temb + pe[:T, None]
    for l in range(od.N_LAYERS):
        p = 'decoder.layers.%d' % l
        if l in od.QAN_LAYERS:
            y = od._ln(h + qan_block(h, sd, p), sd, p + '.norm1')
            y = od._ln(y + od._mha(y, cond, sd, p + '.multihead_attn'), sd, p + '.norm2')
            y = od._ln(y + od._ffn(y, sd, p), sd, p + '.norm3')
            h = h + (y - h)
        else:
            h = od.std_layer(h, cond, sd, p)
    body, pose = od._lin(h, sd, 'bodyFinalLinear'), od._lin(h, sd, 'objFinalLinear')
    R = quaternion_to_matrix(torch.cat([pose[..., -1:], pose[..., -4:-1]], dim=2))[:, :, None]
    obj = (R @ zpo[None, :, :, :, None] + pose[:, :, None, :3, None])[..., 0].reshape(T, B, -1)
    return torch.cat([body, obj, pose], dim=2).permute(1, 2, 0).unsqueeze(1)


def loss_of(pred, gt, w, P=PAST):
    """mean_b sum_i w_i term_i[b], the 13 terms of train_diffusion_skeleton.py:108-127."""
    mse = lambda a, b: ((a - b) ** 2).mean(dim=[0, 2])
    vel = lambda a: a[1:] - a[:-1]
    x, g = pred.squeeze(1).permute(2, 0, 1), gt.squeeze(1).permute(2, 0, 1)
    total = 0.
    for gi, (a, b, iv) in enumerate(((0, 63, 11), (63, 99, 12), (99, 102, 10), (102, 106, 9))):
        xs, gs = x[..., a:b], g[..., a:b]
        total = total + w[2 * gi] * mse(xs[:P], gs[:P]) + w[2 * gi + 1] * mse(xs[P:], gs[P:]) + w[iv] * mse(vel(xs), vel(gs))
    total = total + w[8] * ((x[..., -4:].norm(p=2, dim=-1).square() - 1).square()).mean(dim=0)
    return total.mean()


class TorchStep:
    def __init__(self, sd, lr=3e-4):
        self.sd = {k: torch.as_tensor(v).float().to(DEV) for k, v in sd.items() if k in PARAM_NAMES}
        for v in self.sd.values():
            v.requires_grad_(True)
        self.pe = torch.as_tensor(positional_table()).float().to(DEV)
        self.opt = torch.optim.AdamW(list(self.sd.values()), lr=lr, weight_decay=0.0)
        self.w = SkeletonLossWeights().vector()

    def step(self, x_t, t, zpo, gt):
        self.opt.zero_grad(set_to_none=True)
        loss = loss_of(forward(self.sd, x_t, t, zpo, encode(self.sd, gt, zpo, self.pe), self.pe), gt, self.w)
        loss.backward()
        self.opt.step()
        return loss.detach()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--blocks', type=int, default=7)
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    sd = {k: torch.from_numpy(v) for k, v in syn.skeleton_mdm_state_dict(1106).items()}
    res = dict(device=torch.cuda.get_device_name(0), blocks=a.blocks, calls=a.calls, shapes=[])
    for B, T in SHAPES:
        bt = {k: torch.from_numpy(v) for k, v in syn.make_skeleton_batch(500 + B + T, B=B, T=T).items()}
        batch = (bt['body'], bt['obj'], bt['pose'], bt['zero_pose_obj'])
        gt, zpo = tokens_of(batch, DEV)
        t = torch.from_numpy(np.random.RandomState(B * T).randint(0, 1000, size=B).astype(np.int64)).to(DEV)
        eps = torch.randn(gt.shape, device=DEV, generator=torch.Generator(DEV).manual_seed(1))
        tr, ts = SkeletonDenoiserTrainer(sd, device=DEV), TorchStep(sd)
        clip = dict(gt=gt, zero_pose_obj=zpo)
        x_t = tr.diffusion.q_sample(gt, t, noise=eps)
        first = float(tr.training_step(clip, t=t, noise=eps)[0].mean()), float(ts.step(x_t, t, zpo, gt))
        sides = dict(hip_grads_ms=lambda: tr.grads_at(x_t, t, zpo, gt), hip_adamw_ms=tr.apply_gradients,
                     hip_training_step_ms=lambda: tr.training_step(clip, t=t, noise=eps), torch_eager_training_step_ms=lambda: ts.step(x_t, t, zpo, gt))
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
