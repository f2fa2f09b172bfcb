"""hip-event timing of the denoiser trainer WITH the encoder in the pass (``DenoiserTrainer(train_encoder=True)``, csrc/mdm_train.hip
``interdiff_mdm_train_full_grads``), by the method of tools/mdm_train_time.py: one process, the sides alternating block by block (``--blocks`` blocks of ``--calls``
calls each, after a warm-up block), per side the median of the block medians and their range, milliseconds.  Not on the product path.

    python tools/mdm_encoder_train_time.py [--blocks 7] [--calls 10] [--json profiles/mdm_encoder_train_time.json]

Shapes: B = 16 and 32 at T = 35, B = 16 at T = 100, past_len 10, seeded inputs, the synthetic weights, a seeded pc_embedding.  Sides:
  hip_full_step_ms           q_sample + encoder forward + decoder forward + terms + both backwards + AdamW on the 228 tensors
  hip_decoder_only_step_ms   the step of the same tree with train_encoder=False, fed a fixed cond (what the trainer did before)
  torch_eager_full_step_ms   torch eager autograd + torch.optim.AdamW on the plain-torch restatement of tools/mdm_train_time.py with the encoder in the graph
Reported: the milliseconds the encoder adds to the decoder-only step, and torch / hip for the full step.  Both full sides print their first-step loss."""
import argparse
import json
import os
import sys
import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mdm_train_time as mtt                                             # noqa: E402
from interdiff_amd import synthetic as syn                               # noqa: E402
from interdiff_amd.mdm_train import DenoiserTrainer, FULL_PARAM_NAMES   # noqa: E402
from interdiff_amd.mdm import positional_table                          # noqa: E402
from interdiff_amd.losses import LossWeights                            # noqa: E402
from oracle import denoiser as od                                       # noqa: E402

DEV, PAST, SHAPES = mtt.DEV, mtt.PAST, mtt.SHAPES


def encode(sd, gt, pc, pe):
    """MDM._get_embeddings from pc_embedding on (model/diffusion_smpl.py:217-221) on the tensors' own device."""
    tok = gt.squeeze(1).permute(2, 0, 1)[:PAST]
    h = od._lin(tok[..., :135], sd, 'bodyEmbedding') + od._lin(tok[..., 135:], sd, 'objEmbedding') + pc[None] + pe[:PAST, None]
    for l in range(od.N_LAYERS):
        p = 'encoder.layers.%d' % l
        if l in od.QAN_LAYERS:
            y = od._ln(h + mtt.qan_block(h, sd, p), sd, p + '.norm1')
            y = od._ln(y + od._ffn(y, sd, p), sd, p + '.norm2')
            h = h + (y - h)
        else:
            h = od.enc_std_layer(h, sd, p)
    return h


class TorchFullStep:
    def __init__(self, sd, lr=3e-4):
        self.sd = {k: torch.as_tensor(v).float().to(DEV) for k, v in sd.items() if k in FULL_PARAM_NAMES}
        for v in self.sd.values():
            v.requires_grad_(True)
        self.pe = torch.as_tensor(positional_table()).float().to(DEV)
        self.opt = torch.optim.AdamW(list(self.sd.values()), lr=lr, weight_decay=0.0)
        self.w = LossWeights().vector()

    def step(self, x_t, t, pc, gt):
        self.opt.zero_grad(set_to_none=True)
        loss = mtt.loss_of(mtt.forward(self.sd, x_t, t, encode(self.sd, gt, pc, self.pe), self.pe), gt, self.w)
        loss.backward()
        self.opt.step()
        return loss.detach()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--blocks', type=int, default=7)
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    sd = {k: torch.from_numpy(v) for k, v in syn.mdm_state_dict(seed=233).items()}
    res = dict(device=torch.cuda.get_device_name(0), blocks=a.blocks, calls=a.calls, past_len=PAST, shapes=[])
    for B, T in SHAPES:
        bt = syn.make_clip_batch(seed=500 + B + T, B=B, T=T, past_len=PAST, n_points=8)
        gt, cond = torch.from_numpy(bt['gt']).to(DEV), torch.from_numpy(bt['cond']).to(DEV)
        t = torch.from_numpy(np.random.RandomState(B * T).randint(0, 1000, size=B).astype(np.int64)).to(DEV)
        eps = torch.randn(gt.shape, device=DEV, generator=torch.Generator(DEV).manual_seed(1))
        pc = torch.randn(B, 256, device=DEV, generator=torch.Generator(DEV).manual_seed(2))
        full, dec, ts = DenoiserTrainer(sd, device=DEV, train_encoder=True), DenoiserTrainer(sd, device=DEV), TorchFullStep(sd)
        x_t = full.diffusion.q_sample(gt, t, noise=eps)
        first = float(full.training_step(dict(gt=gt, pc=pc), t=t, noise=eps)[0].mean()), float(ts.step(x_t, t, pc, gt))
        sides = dict(hip_full_step_ms=lambda: full.training_step(dict(gt=gt, pc=pc), t=t, noise=eps),
                     hip_decoder_only_step_ms=lambda: dec.training_step(dict(gt=gt, cond=cond), t=t, noise=eps),
                     torch_eager_full_step_ms=lambda: ts.step(x_t, t, pc, gt))
        row = dict(B=B, T=T, first_loss_hip=first[0], first_loss_torch=first[1], **mtt.alternate(sides, a.blocks, a.calls))
        row['encoder_adds_ms'] = row['hip_full_step_ms']['median'] - row['hip_decoder_only_step_ms']['median']
        row['torch_over_hip_full_step'] = row['torch_eager_full_step_ms']['median'] / row['hip_full_step_ms']['median']
        res['shapes'].append(row)
        print('B = %d, T = %d on %s: first-step loss hip %.6f, torch %.6f' % (B, T, res['device'], first[0], first[1]))
        mtt.print_sides(row, sides)
        print('  the encoder adds (ms)            %9.3f' % row['encoder_adds_ms'])
        print('  torch eager full / hip full step %9.2f' % row['torch_over_hip_full_step'])
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(res, open(a.json, 'w'), indent=1, sort_keys=True)


if __name__ == '__main__':
    main()
