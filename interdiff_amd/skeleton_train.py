"""Training of the HO-GCN skeleton correction predictor on the HIP path the way the reference trains it: the module in ``train()``.
All 24 ``BatchNorm2d`` sites normalise with the statistics of the BATCH and update ``running_mean`` / ``running_var`` /
``num_batches_tracked``; ``nn.Dropout(p)`` follows the tcn BatchNorm of every ``ST_GCNN_layer`` (model/layers.py:308-318).

    loss, grads     LitObjInteraction._common_step + loss.backward(), module in train()   train_correction_skeleton.py:128-154
    training_step   + the BatchNorm buffer updates + torch.optim.Adam(lr, weight_decay=l2_norm).step()   :41-47, :182-189
    init_state_dict the reference's initial distributions (nn.Conv2d's default, model/sublayers.py:408-410, :494-500)

``SkeletonTrainer`` builds on ``SkeletonFineTuner`` (flat parameter layout, Adam, the re-fold into the arena that
``SkeletonObjProjector`` reads); after a step the live predictor is the ``eval()`` model of the new weights AND the new running statistics.

Departure from the reference: the 24 convolution biases cancel inside a batch normalisation, so their gradient is identically zero.  The
reference computes fp32 rounding noise there, which Adam turns into a +-lr random walk of parameters that cannot influence the
train-mode output; here those gradients are exact 0.0, and with ``weight_decay = 0`` the biases do not move.

The SMPL predictor's trainer is ``interdiff_amd.correction_train``.  NOT built: learning-rate schedules, the Lightning glue, the dataset.

All arithmetic runs in libinterdiff_hip.so (csrc/skeleton_bn_train.h around csrc/skeleton_train.h, the train-mode layer in
csrc/stgcn_bn_train.h; launchers csrc/skeleton_train.hip).
"""
import ctypes as C
import math
from collections import OrderedDict
import numpy as np
import torch
from . import _lib
from .skeleton import N_PRE, N_JOINTS, _check
from .stgcn_pack import STACKS
from .skeleton_finetune import SkeletonFineTuner
from .correction_losses import MSE_KEYS
from .diffusion import fresh_seed

WIDTHS = ((9, 32, 16, 32, 9), (9, 32, 16, 32, 9), (9, 64, 32, 64, 9))        # model/correction_skeleton.py:13-50


def init_state_dict(seed, embedding_dim=128, num_joints=N_JOINTS):
    """A fresh ``ObjProjector`` state_dict -- the checkpoint's keys (plus ``num_batches_tracked``), shapes and dtypes -- drawn from the
    reference's initial DISTRIBUTIONS with a seeded torch generator (not torch's bits): convolution weights and biases U(+-1/sqrt(fan_in)),
    ``gcn.T`` / ``gcn.A`` U(+-1/sqrt(size(1))), BatchNorm weight 1, bias 0, running mean 0, running variance 1, PReLU 0.25.
    ``embedding_dim`` is accepted as the reference's constructor accepts it: the channel widths do not depend on it."""
    gen = torch.Generator().manual_seed(int(seed))
    uni = lambda bound, *shape: (torch.rand(*shape, generator=gen, dtype=torch.float64) * 2.0 - 1.0).mul(bound).float()
    sd = OrderedDict()
    for si, stack in enumerate(STACKS):
        nodes = (num_joints, 1, num_joints + 1)[si]
        for l in range(4):
            cin, cout, p = WIDTHS[si][l], WIDTHS[si][l + 1], '%s.%d.' % (stack, l)
            if si == 2:
                sd[p + 'gcn.A'] = uni(1.0 / math.sqrt(nodes), N_PRE, nodes, nodes)
                sd[p + 'gcn.T'] = uni(1.0 / math.sqrt(N_PRE), nodes, N_PRE, N_PRE)
            else:
                sd[p + 'gcn.T'] = uni(1.0 / math.sqrt(N_PRE), N_PRE, N_PRE)
            for conv, bn in (('tcn.0', 'tcn.1'), ('residual.0', 'residual.1')):
                sd[p + conv + '.weight'] = uni(1.0 / math.sqrt(cin), cout, cin, 1, 1)
                sd[p + conv + '.bias'] = uni(1.0 / math.sqrt(cin), cout)
                sd[p + bn + '.weight'] = torch.ones(cout)
                sd[p + bn + '.bias'] = torch.zeros(cout)
                sd[p + bn + '.running_mean'] = torch.zeros(cout)
                sd[p + bn + '.running_var'] = torch.ones(cout)
                sd[p + bn + '.num_batches_tracked'] = torch.zeros((), dtype=torch.int64)
            sd[p + 'prelu.weight'] = torch.full((1,), 0.25)
    return sd


class SkeletonTrainer(SkeletonFineTuner):
    """Trains a skeleton predictor from scratch (``init_state_dict``) or from a checkpoint.  ``batch`` as in ``SkeletonFineTuner``.
    ``masks``: the dropout keep masks, uint8, keep iff nonzero -- one flat buffer, the 12 layers in ``named_parameters()`` layer order, each
    [B, cout, 20, nodes], or a dict as ``dropout_masks`` returns; None: the in-kernel generator's masks for (seed, step)."""

    def __init__(self, state_dict, dropout=0.1, momentum=0.1, lr=3e-4, weight_decay=0., betas=(0.9, 0.999), eps=1e-8, weights=None, past_len=10,
                 future_len=10, seed=None, device='cuda'):
        if not (0.0 <= float(dropout) < 1.0):
            raise ValueError('dropout must lie in [0, 1), got %r' % (dropout,))
        if not (0.0 <= float(momentum) <= 1.0):
            raise ValueError('momentum must lie in [0, 1], got %r' % (momentum,))
        super().__init__(state_dict, lr=lr, weight_decay=weight_decay, betas=betas, eps=eps, weights=weights, past_len=past_len, future_len=future_len,
                         device=device)
        self.dropout, self.momentum = float(dropout), float(momentum)
        self.seed = fresh_seed() if seed is None else int(seed)
        cop = self.predictor.cop
        self.layers = [('%s.%d' % (STACKS[li // 4], li % 4), int(cop.cout[li]), (N_JOINTS, 1, N_JOINTS + 1)[li // 4]) for li in range(12)]
        self.mask_clip = sum(co * N_PRE * nodes for _, co, nodes in self.layers)
        self._tracked = {k: int(v) for k, v in self._fixed.items() if k.endswith('num_batches_tracked')}
        self._tws = {}

    # ---- masks
    def _mask_buffer(self, masks, B):
        if masks is None:
            return None
        if isinstance(masks, dict):
            parts = []
            for name, co, nodes in self.layers:
                m = torch.as_tensor(masks[name])
                if tuple(m.shape) != (B, co, N_PRE, nodes):
                    raise ValueError('mask of %s: expected %r, got %r' % (name, (B, co, N_PRE, nodes), tuple(m.shape)))
                parts.append(m.reshape(-1).to(self.device))
            masks = torch.cat(parts)
        m = torch.as_tensor(masks).reshape(-1)
        if m.numel() != B * self.mask_clip:
            raise ValueError('expected %d mask bytes, got %d' % (B * self.mask_clip, m.numel()))
        return (m != 0).to(self.device, torch.uint8).contiguous()

    def split_masks(self, flat, B):
        """The flat mask buffer -> {layer prefix: view [B, cout, 20, nodes]}."""
        out, off = OrderedDict(), 0
        for name, co, nodes in self.layers:
            n = B * co * N_PRE * nodes
            out[name] = flat[off:off + n].view(B, co, N_PRE, nodes)
            off += n
        return out

    def dropout_masks(self, B, step=None):
        """The keep masks the in-kernel generator draws at training step ``step`` (default: the next one) -> {layer prefix: uint8 [B,cout,20,nodes]}."""
        step = self.step if step is None else int(step)
        flat = torch.empty(B * self.mask_clip, dtype=torch.uint8, device=self.device)
        _check(self.lib.interdiff_skeleton_train_masks(C.byref(self.predictor.cop), B, self.dropout, self.seed, step, _lib.dptr(flat), _lib.stream()),
               'skeleton_train_masks')
        return self.split_masks(flat, B)

    # ---- the step
    def _train_workspace(self, B):
        if B not in self._tws:
            n = self.lib.interdiff_skeleton_train_workspace_bytes(C.byref(self.predictor.cop), B)
            self._tws = {B: torch.empty(n, dtype=torch.uint8, device=self.device)}
        return self._tws[B]

    def _train_grads(self, batch, masks=None, update=False, dropout=None, want_stats=False):
        B, T, d6_tail, obj_trans, body_gt, pose_gt = self._inputs(batch)
        m = self._mask_buffer(masks, B)
        p = self.dropout if dropout is None else dropout
        out9 = torch.empty(9, dtype=torch.float32, device=self.device)
        grads = torch.empty(self.n_param, dtype=torch.float32, device=self.device)
        stats = torch.empty_like(self.bn) if want_stats else None
        ws = self._train_workspace(B)
        _check(self.lib.interdiff_skeleton_train_grads(C.byref(self.predictor.cop), _lib.dptr(self.params), _lib.dptr(self.bn), _lib.dptr(d6_tail),
                                                       _lib.dptr(obj_trans), _lib.dptr(body_gt), _lib.dptr(pose_gt), B, T, self._w8, p,
                                                       _lib.dptr(m) if m is not None else None, self.seed, self.step, self.momentum, int(update),
                                                       _lib.dptr(out9), _lib.dptr(grads), _lib.dptr(stats) if want_stats else None, _lib.dptr(ws),
                                                       ws.numel(), _lib.stream()), 'skeleton_train_grads')
        return out9, grads, stats

    def _grads(self, batch):
        out9, grads, _ = self._train_grads(batch)
        return out9, grads

    def loss_and_grads(self, batch, masks=None):
        """As ``SkeletonFineTuner.loss_and_grads`` with the module in train().  Touches neither the running statistics nor the step counter."""
        out9, grads, _ = self._train_grads(batch, masks)
        w = torch.tensor(self.weights.vector(0)[2:], dtype=torch.float32, device=self.device) * out9[1:]
        return out9[0], {k: out9[1 + n] for n, k in enumerate(MSE_KEYS)}, {k: w[n] for n, k in enumerate(MSE_KEYS)}, self.unflatten(grads)

    def training_step(self, batch, masks=None):
        """Gradients, the running-statistics update, ``num_batches_tracked += 1``, Adam, the re-fold.  -> the loss BEFORE the step."""
        out9, grads, _ = self._train_grads(batch, masks, update=True)
        for k in self._tracked:
            self._tracked[k] += 1
        self.apply_gradients(grads)
        return out9[0]

    def batch_statistics(self, batch):
        """{buffer name: tensor} under the ``running_mean`` / ``running_var`` key names: mean and BIASED variance of this batch at every
        BatchNorm site, without dropout."""
        _, _, stats = self._train_grads(batch, dropout=0.0, want_stats=True)
        return OrderedDict((n, stats[o:o + int(np.prod(s))].view(s)) for n, o, s in self.btable)

    # ---- state
    def buffers(self):
        return OrderedDict((n, self.bn[o:o + int(np.prod(s))].view(s)) for n, o, s in self.btable)

    def state_dict(self):
        """The reference's keys, shapes and dtypes (CPU tensors): parameters from the master copy, the UPDATED running statistics and
        ``num_batches_tracked`` (int64, when the input had those keys)."""
        out = super().state_dict()
        for n, v in self.buffers().items():
            out[n] = v.detach().cpu().to(out[n].dtype).clone()
        for k, v in self._tracked.items():
            out[k] = torch.tensor(v, dtype=torch.int64)
        return out

    def optimizer_state(self):
        st = super().optimizer_state()
        st['seed'] = self.seed
        return st

    def load_optimizer_state(self, state):
        super().load_optimizer_state(state)
        self.seed = int(state['seed'])
