"""hip-event timing of the denoiser trainer with the PointNet++ object encoder under BATCH statistics (``DenoiserTrainer(train_encoder=True, train_pointnet=True,
pointnet_mode='train')``, csrc/pointnet2_bn_train.hip), by the method of tools/mdm_train_time.py: one process, the sides alternating block by block (``--blocks``
blocks of ``--calls`` calls each, after a warm-up block), per side the median of the block medians and their range, milliseconds.  Not on the product path.

    python tools/pointnet2_train_time.py [--blocks 7] [--calls 10] [--json profiles/pointnet2_train_time.json]

Shapes: B = 16 and 32 at T = 35, past_len 10, P = 2048 (the box-shell clouds of synthetic.make_embedding_inputs), seeded inputs, the synthetic weights.  Sides:
  hip_train_step_ms     the train-mode forward + the full pass + the train-mode backward + AdamW on 266 tensors + the statistics update + the re-fold
  hip_eval_step_ms      the same step with pointnet_mode='eval': the parent's code path (frozen statistics)
  forward_ms / grads_ms / stats_ms     interdiff_pointnet2_train_forward, _train_grads, _train_stats alone
  eager_fwd_bwd_ms      the module's structure (Conv2d 1x1 without bias -> BatchNorm2d -> ReLU, three times per scale; max pools; Linear) in torch eager in train(), forward
                        + backward on the same GPU, fed the grouping tables ready-made -- so it does NOT pay the sampling and the 2 x 1024 ball queries per clip that
                        forward_ms includes (the reference runs those in pointnet2_ops' own kernels, which are not available here)
Reported: the milliseconds the batch-statistic regime adds to the parent's step, and (forward + grads) / eager."""
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
from interdiff_amd.mdm_train import DenoiserTrainer                     # noqa: E402
from interdiff_amd.pointnet2_train import PREFIX                         # noqa: E402

DEV, PAST, T, P = mtt.DEV, mtt.PAST, 35, 2048


class Eager(torch.nn.Module):
    """The module structure in torch's own layers, on grouping tables computed once (tests/pointnet2_bn_train_oracle.py ``tables``)."""

    def __init__(self, sd, tb):
        super().__init__()
        ch = ((4, 16, 16, 32), (4, 32, 32, 64), (99, 64, 64, 128), (99, 64, 96, 128))
        self.mlps = torch.nn.ModuleList()
        for g, spec in enumerate(ch):
            q, layers = '%s.SA_modules.%d.mlps.%d' % (PREFIX, g // 2, g % 2), []
            for l in range(3):
                conv, bn = torch.nn.Conv2d(spec[l], spec[l + 1], 1, bias=False), torch.nn.BatchNorm2d(spec[l + 1])
                conv.weight.data.copy_(sd['%s.%d.weight' % (q, 3 * l)])
                bn.weight.data.copy_(sd['%s.%d.weight' % (q, 3 * l + 1)])
                bn.bias.data.copy_(sd['%s.%d.bias' % (q, 3 * l + 1)])
                layers += [conv, bn, torch.nn.ReLU(True)]
            self.mlps.append(torch.nn.Sequential(*layers))
        self.lin = torch.nn.Linear(256, 253)
        self.lin.weight.data.copy_(sd[PREFIX + '.Linear.weight'])
        self.lin.bias.data.copy_(sd[PREFIX + '.Linear.bias'])
        self.tb = {k: v.to(DEV) for k, v in tb.items()}

    def forward(self, pts):
        B, tb = pts.shape[0], self.tb
        bi = torch.arange(B, device=pts.device)[:, None, None]
        nrm = pts.norm(dim=2, keepdim=True)
        centres = pts[torch.arange(B, device=pts.device)[:, None], tb['fidx']]
        f1 = []
        for sc in range(2):
            nb = tb['all%d' % sc]
            g = torch.cat([pts[bi, nb] - centres[:, :, None], nrm[bi, nb]], dim=3).permute(0, 3, 1, 2).contiguous()
            f1.append(self.mlps[sc](g).max(dim=3)[0])
        f1 = torch.cat(f1, dim=1)                                                       # [B,96,1024]
        rows = torch.arange(B, device=pts.device)[:, None]
        slot_f, slot_c = f1.permute(0, 2, 1)[rows, tb['pos']], centres[rows, tb['pos']]
        f2 = []
        for sc, (lo, hi) in enumerate(((0, 16), (16, 48))):
            g = torch.cat([slot_c[:, lo:hi] - pts[:, :1], slot_f[:, lo:hi]], dim=2).permute(0, 2, 1)[:, :, None, :].contiguous()
            f2.append(self.mlps[2 + sc](g).max(dim=3)[0][:, :, 0])
        return torch.cat([pts[:, 0], self.lin(torch.cat(f2, dim=1))], dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--blocks', type=int, default=7)
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    from tests import pointnet2_bn_train_oracle as bo
    sd = {k: torch.from_numpy(v) for k, v in syn.mdm_state_dict(seed=233).items()}
    res = dict(device=torch.cuda.get_device_name(0), blocks=a.blocks, calls=a.calls, past_len=PAST, P=P, shapes=[])
    for B in (16, 32):
        bt = syn.make_clip_batch(seed=500 + B + T, B=B, T=T, past_len=PAST, n_points=8)
        gt = torch.from_numpy(bt['gt']).to(DEV)
        pts_host = torch.from_numpy(syn.make_embedding_inputs(seed=600 + B, B=B, T=1, n_points=P)['obj_points'])
        pts = pts_host.to(DEV)
        t = torch.from_numpy(np.random.RandomState(B * T).randint(0, 1000, size=B).astype(np.int64)).to(DEV)
        eps = torch.randn(gt.shape, device=DEV, generator=torch.Generator(DEV).manual_seed(1))
        d_pc = torch.randn(B, 256, device=DEV, generator=torch.Generator(DEV).manual_seed(2))
        new = DenoiserTrainer(sd, device=DEV, train_encoder=True, train_pointnet=True, pointnet_mode='train')
        old = DenoiserTrainer(sd, device=DEV, train_encoder=True, train_pointnet=True, pointnet_mode='eval')
        batch = dict(gt=gt, obj_points=pts)
        first = float(new.training_step(batch, t=t, noise=eps)[0].mean()), float(old.training_step(batch, t=t, noise=eps)[0].mean())
        pn = DenoiserTrainer(sd, device=DEV, train_encoder=True, train_pointnet=True, pointnet_mode='train').pointnet       # never stepped
        eager = Eager(sd, bo.tables(pts_host)).to(DEV).train()
        pc_hip, pc_eager = pn.forward(pts), eager(pts).detach()
        agree = float((pc_hip - pc_eager).abs().max() / pc_eager.abs().max())

        def eager_step():
            for q in eager.parameters():
                q.grad = None
            (eager(pts) * d_pc).sum().backward()
        sides = dict(hip_train_step_ms=lambda: new.training_step(batch, t=t, noise=eps), hip_eval_step_ms=lambda: old.training_step(batch, t=t, noise=eps),
                     forward_ms=lambda: pn.forward(pts), grads_ms=lambda: pn.grads(d_pc, flat=True), stats_ms=pn.update_running_stats, eager_fwd_bwd_ms=eager_step)
        row = dict(B=B, T=T, first_loss_train=first[0], first_loss_eval=first[1], pc_hip_vs_eager=agree, **mtt.alternate(sides, a.blocks, a.calls))
        row['train_mode_adds_ms'] = row['hip_train_step_ms']['median'] - row['hip_eval_step_ms']['median']
        row['hip_over_eager'] = (row['forward_ms']['median'] + row['grads_ms']['median']) / row['eager_fwd_bwd_ms']['median']
        res['shapes'].append(row)
        print('B = %d, T = %d, P = %d on %s: first-step loss in train mode %.6f, in eval mode %.6f; pc, HIP vs eager: %.2e' % (B, T, P, res['device'], first[0], first[1], agree))
        mtt.print_sides(row, sides)
        print('  train mode adds (ms)             %9.3f' % row['train_mode_adds_ms'])
        print('  (forward + grads) / eager        %9.3f' % row['hip_over_eager'])
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(res, open(a.json, 'w'), indent=1, sort_keys=True)


if __name__ == '__main__':
    main()
