"""Device-event timing of one train-mode training step of the SMPL contact-frame correction predictor (interdiff_amd/correction_train.py: batch
statistics, dropout from the in-kernel generator, running-buffer update, Adam, re-fold; epoch 0, ``initialize=True``) next to one
frozen-statistics step of ``CorrectionFineTuner.training_step`` (one launch per clip for the whole network, no seams) and to torch-ROCm eager
autograd + torch.optim.Adam on a plain-torch fp32 train-mode restatement (``TorchStep`` of tools/correction_finetune_time.py with
``batch_norm(training=True)`` and ``dropout``), on the same GPU in the same process; not on the product path.

    python tools/correction_train_time.py [--blocks 9] [--steps 20] [--sides train,finetune,torch_train] [--json profiles/correction_train_time.json]

At B = 16 and B = 32, T = 35, past_len 10, p = 0.1, on the seeded inputs and the checkpoint stand-in of tools/correction_finetune_time.py (the
timing does not depend on the weights' values).  Every shape and side is warmed up; a timed block is ``steps`` consecutive steps between two
device events; the sides alternate block by block; reported: the median over the blocks of microseconds per step, and the spread (min, max).
The train-mode step is 17 phase launches + masks + fold + statistics + Adam + re-fold = 22 launches against the fine-tuner's 5, so against the
fine-tuner this measures mostly the cost of the seams.  ``--sides finetune`` with INTERDIFF_HIP_LIB set times the fine-tuner's step of another
build of the library (the same-box A/B against the parent commit)."""
import argparse
import json
import os
import sys
import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from interdiff_amd import correction_finetune as cft                                        # noqa: E402
from correction_finetune_time import TorchStep, synthetic_state_dict, synthetic_batch, T, PAST     # noqa: E402

DEV = 'cuda'
P_DROP = 0.1


class TorchTrainStep(TorchStep):
    """The same step with the module in train(): BatchNorm on batch statistics (updating its running buffers), dropout after the tcn BatchNorm."""

    def layer(self, x, p):
        P, F = self.P, torch.nn.functional

        def conv_bn(h, c, b):
            y = torch.einsum('oc,nctv->notv', P[p + c + '.weight'][:, :, 0, 0], h) + P[p + c + '.bias'].view(1, -1, 1, 1)
            return F.batch_norm(y, P[p + b + '.running_mean'], P[p + b + '.running_var'], P[p + b + '.weight'], P[p + b + '.bias'], True, 0.1, 1e-5)
        res = conv_bn(x, 'residual.0', 'residual.1')
        Tm = P[p + 'gcn.T']
        if Tm.dim() == 2:
            g = torch.einsum('nctv,tq->ncqv', x, Tm)
        else:
            g = torch.einsum('nctv,tvw->nctw', torch.einsum('nctv,vtq->ncqv', x, Tm), P[p + 'gcn.A'])
        return F.prelu(F.dropout(conv_bn(g, 'tcn.0', 'tcn.1'), P_DROP, True) + res, P[p + 'prelu.weight'])


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
    ap.add_argument('--blocks', type=int, default=9)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--sides', default='train,finetune,torch_train')
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X'
    want = a.sides.split(',')
    sd = synthetic_state_dict()
    res = {'blocks': a.blocks, 'steps_per_block': a.steps, 'device': torch.cuda.get_device_name(0), 'T': T, 'p_drop': P_DROP}
    for B in (16, 32):
        batch = synthetic_batch(B=B)
        d6, trans, hv = cft.rotation_6d_of_axis_angle(batch['obj_angle']), batch['obj_trans'], batch['markers'][..., :3].contiguous()
        sides = {}
        if 'train' in want:
            from interdiff_amd import correction_train as ct
            tr = ct.CorrectionTrainer(sd, T=T, past_len=PAST, dropout=P_DROP, seed=82, device=DEV)
            sides['train'] = lambda tr=tr: tr.training_step(batch)
        if 'finetune' in want:
            ft = cft.CorrectionFineTuner(sd, T=T, past_len=PAST, device=DEV)
            sides['finetune'] = lambda ft=ft: ft.training_step(batch)
        if 'torch_train' in want:
            ts = TorchTrainStep(sd)
            sides['torch_train'] = lambda ts=ts: ts.step(d6, trans, hv)
        for k, fn in sides.items():
            res['first_loss_%s_B%d' % (k, B)] = float(fn())
        for fn in sides.values():                       # warm-up of every shape and side
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in sides}
        for _ in range(a.blocks):                       # alternate the sides block by block
            for k, fn in sides.items():
                times[k].append(block_us(fn, a.steps))
        for k, v in times.items():
            res['%s_step_B%d_us' % (k, B)] = {'median': float(np.median(v)), 'min': float(np.min(v)), 'max': float(np.max(v))}
            print('B = %2d  %-12s first loss %.6f  median %10.1f us per step (min %.1f, max %.1f over %d blocks of %d steps)'
                  % (B, k, res['first_loss_%s_B%d' % (k, B)], np.median(v), np.min(v), np.max(v), a.blocks, a.steps))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(res, open(a.json, 'w'), indent=1, sort_keys=True)


if __name__ == '__main__':
    main()
