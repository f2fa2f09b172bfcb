"""Fine-tuning of the HO-GCN skeleton correction predictor (``checkpoints/obj_skeleton.ckpt``) on the HIP path, with FROZEN
normalisation statistics: the reference module in ``eval()`` with autograd on.  BatchNorm uses its running statistics and never
updates them, dropout is off, and every one of the 96,110 parameters is trained -- convolutions, BatchNorm affine weights, the
temporal and adjacency matrices, the PReLU slopes.

    loss, grads     LitObjInteraction._common_step + loss.backward()  train_correction_skeleton.py:128-154, :85-126
    training_step   + torch.optim.Adam(lr, weight_decay=l2_norm).step()  :41-47, :182-189

Training from scratch -- the module in ``train()``: batch statistics, running-statistics updates, dropout -- is
``interdiff_amd.skeleton_train.SkeletonTrainer``, built on this class.  The SMPL predictor's fine-tuner is ``interdiff_amd.correction_finetune``.  NOT built: learning-rate
schedules, the Lightning glue and the dataset.

All arithmetic runs in libinterdiff_hip.so (csrc/skeleton_train.h / .hip): one workgroup per clip for forward, loss gradient and
backward, a fixed-order fold over clips, Adam on fp32 master parameters in the reference layout, and the re-fold into the arena
that ``SkeletonObjProjector`` reads.  The flat parameter layout (``param_table``) is documented in include/interdiff_hip.h.
"""
import ctypes as C
from collections import OrderedDict
import numpy as np
import torch
from . import _lib
from .skeleton import SkeletonObjProjector, N_PRE, N_JOINTS, _check, _strip
from .stgcn_pack import STACKS, to_f64
from .correction_losses import CorrectionLossWeights, MSE_KEYS

BN_EPS = 1e-5
LAYER_PARAMS = ('gcn.A', 'gcn.T', 'tcn.0.weight', 'tcn.0.bias', 'tcn.1.weight', 'tcn.1.bias',
                'residual.0.weight', 'residual.0.bias', 'residual.1.weight', 'residual.1.bias', 'prelu.weight')
LAYER_BUFFERS = ('tcn.1.running_mean', 'tcn.1.running_var', 'residual.1.running_mean', 'residual.1.running_var')
TABLE_COLS = 16                                   # interdiff_skeleton_finetune_param_table: 11 offsets, cin, cout, nodes, joint-stack flag, bn offset


def param_table(state_dict):
    """[(name, offset, shape)] of the flat parameter / gradient vector: ``ObjProjector.named_parameters()`` order -- the three stacks,
    four layers each, per layer LAYER_PARAMS (``gcn.A`` in the joint stack only)."""
    sd = _strip(state_dict)
    out, off = [], 0
    for stack in STACKS:
        for l in range(4):
            for suffix in LAYER_PARAMS:
                name = '%s.%d.%s' % (stack, l, suffix)
                if name not in sd:
                    if suffix == 'gcn.A' and stack != STACKS[2]:
                        continue
                    raise KeyError(name)
                shape = tuple(sd[name].shape)
                out.append((name, off, shape))
                off += int(np.prod(shape))
    return out


def buffer_table(state_dict):
    """[(name, offset, shape)] of the flat BatchNorm-buffer vector (read only): per layer LAYER_BUFFERS."""
    sd = _strip(state_dict)
    out, off = [], 0
    for stack in STACKS:
        for l in range(4):
            for suffix in LAYER_BUFFERS:
                name = '%s.%d.%s' % (stack, l, suffix)
                shape = tuple(sd[name].shape)
                out.append((name, off, shape))
                off += int(np.prod(shape))
    return out


def flatten(state_dict, table):
    sd = _strip(state_dict)
    return np.concatenate([to_f64(sd[name]).astype(np.float32).ravel() for name, _, _ in table])


def folded_to_reference_grads(dWf, dbf, W, b, gamma, mean, var, eps=BN_EPS):
    """Gradients of the folded convolution (W s, (b - mean) s + beta), s = gamma / sqrt(var + eps), back to the reference tensors
    -> (dW, db, dgamma, dbeta).  What stgcn_ft_convert_kernel (csrc/stgcn_train.h) evaluates, in numpy."""
    r = 1.0 / np.sqrt(var + eps)
    s = gamma * r
    return dWf * s[:, None], dbf * s, r * ((dWf * W).sum(axis=1) + dbf * (b - mean)), dbf


class FlatParameters:
    """The master copy of a predictor's trained parameters as ONE flat device vector in ``named_parameters()`` order (``self.table``), its Adam moments, and
    the reference-named views of them: what ``SkeletonFineTuner`` and ``correction_finetune.CorrectionFineTuner`` share."""

    def _init_state(self, sd):
        self.params = torch.from_numpy(flatten(sd, self.table)).to(self.device)
        self.bn = torch.from_numpy(flatten(sd, self.btable)).to(self.device)
        self.exp_avg = torch.zeros_like(self.params)
        self.exp_avg_sq = torch.zeros_like(self.params)
        self.step = 0
        trained = {n for n, _, _ in self.table}
        self._keys = list(sd.keys())
        self._fixed = {k: torch.as_tensor(np.asarray(v.detach().cpu() if isinstance(v, torch.Tensor) else v)).clone() for k, v in sd.items() if k not in trained}
        self._dtypes = {k: torch.as_tensor(np.asarray(v.detach().cpu() if isinstance(v, torch.Tensor) else v)).dtype for k, v in sd.items() if k in trained}

    # ---- views
    def unflatten(self, flat):
        """A flat vector -> {reference name: view of its slice, reference shape}."""
        return OrderedDict((n, flat[o:o + int(np.prod(s))].view(s)) for n, o, s in self.table)

    def _flat(self, t):
        if isinstance(t, dict):
            t = torch.cat([t[n].reshape(-1).to(self.device, torch.float32) for n, _, _ in self.table])
        t = t.to(self.device, torch.float32).contiguous()
        if t.numel() != self.n_param:
            raise ValueError('expected %d values, got %d' % (self.n_param, t.numel()))
        return t

    # ---- state
    def named_parameters(self):
        return self.unflatten(self.params)

    def state_dict(self):
        """The reference's keys, shapes and dtypes (CPU tensors): trained parameters from the master copy, buffers as they came in."""
        cur = {n: v.detach().cpu() for n, v in self.unflatten(self.params).items()}
        return OrderedDict((k, cur[k].to(self._dtypes[k]).clone() if k in cur else self._fixed[k].clone()) for k in self._keys)

    def optimizer_state(self):
        return dict(step=self.step, exp_avg={n: v.detach().cpu().clone() for n, v in self.unflatten(self.exp_avg).items()},
                    exp_avg_sq={n: v.detach().cpu().clone() for n, v in self.unflatten(self.exp_avg_sq).items()})

    def load_optimizer_state(self, state):
        self.exp_avg.copy_(self._flat(state['exp_avg']))
        self.exp_avg_sq.copy_(self._flat(state['exp_avg_sq']))
        self.step = int(state['step'])


class SkeletonFineTuner(FlatParameters):
    """Adapts a skeleton predictor to a user's own clips.  ``batch`` is what ``skeleton_validation_step`` takes: (body [B,T,21,3],
    object keypoints [B,T,12,3], pose [B,T,7], zero_pose_obj [B,12,3]); T = past_len + future_len = 20."""

    def __init__(self, state_dict, lr=3e-4, weight_decay=0., betas=(0.9, 0.999), eps=1e-8, weights=None, past_len=10, future_len=10, device='cuda'):
        sd = _strip(state_dict)
        self.lib = _lib.load()
        self.device = torch.device(device)
        self.lr, self.weight_decay, self.betas, self.eps = float(lr), float(weight_decay), (float(betas[0]), float(betas[1])), float(eps)
        self.weights = weights or CorrectionLossWeights()
        self.predictor = SkeletonObjProjector(sd, past_len, future_len, device=device)          # its arena is the live one
        self.past_len, self.T = past_len, past_len + future_len
        self.table, self.btable = param_table(sd), buffer_table(sd)
        self.n_param = self.table[-1][1] + int(np.prod(self.table[-1][2]))
        self._check_table()
        self._init_state(sd)
        self._w8 = (C.c_float * 8)(*self.weights.vector(0)[2:])
        self._ws = {}

    def _check_table(self):
        """The C side derives the same table from the channel widths (csrc/skeleton_train.h ft_plan): they must agree."""
        tab = (C.c_int32 * (12 * TABLE_COLS))()
        n_param, n_bn = C.c_int32(), C.c_int32()
        _check(self.lib.interdiff_skeleton_finetune_param_table(C.byref(self.predictor.cop), tab, C.byref(n_param), C.byref(n_bn)), 'skeleton_finetune_param_table')
        offs = {n: o for n, o, _ in self.table}
        boffs = {n: o for n, o, _ in self.btable}
        for li in range(12):
            p = '%s.%d.' % (STACKS[li // 4], li % 4)
            row = list(tab[li * TABLE_COLS:(li + 1) * TABLE_COLS])
            want = [offs.get(p + s, -1) for s in LAYER_PARAMS] + [self.predictor.cop.cin[li], self.predictor.cop.cout[li], (N_JOINTS, 1, N_JOINTS + 1)[li // 4],
                                                                 int(li // 4 == 2), boffs[p + LAYER_BUFFERS[0]]]
            if row != want:
                raise RuntimeError('parameter table of layer %d: library %r, state_dict %r' % (li, row, want))
        nb = self.btable[-1][1] + int(np.prod(self.btable[-1][2]))
        if n_param.value != self.n_param or n_bn.value != nb:
            raise RuntimeError('parameter count: library %d / %d, state_dict %d / %d' % (n_param.value, n_bn.value, self.n_param, nb))

    def _workspace(self, B):
        if B not in self._ws:
            n = self.lib.interdiff_skeleton_finetune_workspace_bytes(C.byref(self.predictor.cop), B)
            self._ws = {B: torch.empty(n, dtype=torch.uint8, device=self.device)}
        return self._ws[B]

    # ---- the step
    def _inputs(self, batch):
        """-> (B, T, d6_tail, obj_trans, body_gt, pose_gt), frame-major contiguous fp32 device tensors."""
        dev = self.device
        body_gt, pose_gt = batch[0].transpose(0, 1).float().to(dev).contiguous(), batch[2].transpose(0, 1).float().to(dev).contiguous()
        T, B = pose_gt.shape[:2]
        if T != self.T or tuple(body_gt.shape) != (T, B, N_JOINTS, 3) or pose_gt.shape[2] != 7:
            raise ValueError('expected body [B,%d,%d,3] and pose [B,%d,7]' % (self.T, N_JOINTS, self.T))
        obj_trans, q = pose_gt[..., :3].contiguous(), pose_gt[..., 3:]
        qd = q.double()                                                         # ObjProjector.forward's own conversion (SkeletonObjProjector.forward), rounded once
        i, j, k, r = qd.unbind(-1)
        two_s = 2.0 / (qd * qd).sum(-1)
        d6_tail = torch.stack([two_s * (i * k + j * r), two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r)], dim=-1).float().contiguous()
        return B, T, d6_tail, obj_trans, body_gt, pose_gt

    def _grads(self, batch):
        dev = self.device
        B, T, d6_tail, obj_trans, body_gt, pose_gt = self._inputs(batch)
        out9 = torch.empty(9, dtype=torch.float32, device=dev)
        grads = torch.empty(self.n_param, dtype=torch.float32, device=dev)
        ws = self._workspace(B)
        _check(self.lib.interdiff_skeleton_finetune_grads(C.byref(self.predictor.cop), _lib.dptr(self.params), _lib.dptr(self.bn), _lib.dptr(d6_tail),
                                                          _lib.dptr(obj_trans), _lib.dptr(body_gt), _lib.dptr(pose_gt), B, T, self._w8, _lib.dptr(out9),
                                                          _lib.dptr(grads), _lib.dptr(ws), ws.numel(), _lib.stream()), 'skeleton_finetune_grads')
        return out9, grads

    def loss_and_grads(self, batch):
        """-> (loss, loss_dict, weighted_loss_dict, grads): 0-dim device tensors under the reference's 8 keys, ``grads`` = {reference
        parameter name: d loss / d parameter} (views of one flat device tensor)."""
        out9, grads = self._grads(batch)
        w = torch.tensor(self.weights.vector(0)[2:], dtype=torch.float32, device=self.device) * out9[1:]
        return out9[0], {k: out9[1 + n] for n, k in enumerate(MSE_KEYS)}, {k: w[n] for n, k in enumerate(MSE_KEYS)}, self.unflatten(grads)

    def apply_gradients(self, grads):
        """One Adam step on ``grads`` (flat [n_param] or a dict under reference names) and the re-fold of the arena."""
        g = self._flat(grads)
        self.step += 1
        _check(self.lib.interdiff_skeleton_finetune_step(C.byref(self.predictor.cop), _lib.dptr(self.predictor.arena), _lib.dptr(self.params), _lib.dptr(self.bn),
                                                         _lib.dptr(g), _lib.dptr(self.exp_avg), _lib.dptr(self.exp_avg_sq), self.step, self.lr, self.betas[0],
                                                         self.betas[1], self.eps, self.weight_decay, _lib.stream()), 'skeleton_finetune_step')

    def training_step(self, batch):
        """Gradients, Adam, re-fold.  -> the loss BEFORE the step (0-dim device tensor), like ``training_step`` of the reference."""
        out9, grads = self._grads(batch)
        self.apply_gradients(grads)
        return out9[0]
