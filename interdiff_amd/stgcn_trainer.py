"""What the trainers of the two ST-GCN correction predictors share on the Python side, independent of the predictor: the flat parameter
and buffer tables in ``named_parameters()`` order, the master copy with its Adam moments (``FlatParameters``), the train-mode state --
dropout masks, running statistics, ``num_batches_tracked`` -- (``TrainMode``), and the reference's initial distributions
(``init_state_dict``).  The predictor-specific modules are ``skeleton_finetune`` / ``skeleton_train`` (HO-GCN skeleton predictor) and
``correction_finetune`` / ``correction_train`` (SMPL contact-frame predictor); the device side is csrc/stgcn_train.h and
csrc/stgcn_bn_train.h.
"""
import ctypes as C
import math
from collections import OrderedDict
import numpy as np
import torch
from . import _lib
from .skeleton import _check, _strip
from .stgcn_pack import STACKS, to_f64
from .correction_losses import MSE_KEYS
from .diffusion import fresh_seed

BN_EPS = 1e-5
LAYER_PARAMS = ('gcn.A', 'gcn.T', 'tcn.0.weight', 'tcn.0.bias', 'tcn.1.weight', 'tcn.1.bias',
                'residual.0.weight', 'residual.0.bias', 'residual.1.weight', 'residual.1.bias', 'prelu.weight')
LAYER_BUFFERS = ('tcn.1.running_mean', 'tcn.1.running_var', 'residual.1.running_mean', 'residual.1.running_var')
TABLE_COLS = 16                                   # interdiff_*_finetune_param_table: 11 offsets, cin, cout, nodes, joint-stack flag, bn offset


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


def init_state_dict(seed, widths, nodes, n_pre):
    """A fresh ``ObjProjector`` state_dict -- the checkpoint's keys (plus ``num_batches_tracked``), shapes and dtypes -- drawn from the
    reference's initial DISTRIBUTIONS with a seeded torch generator (not torch's bits): convolution weights and biases U(+-1/sqrt(fan_in)),
    ``gcn.T`` / ``gcn.A`` U(+-1/sqrt(size(1))), BatchNorm weight 1, bias 0, running mean 0, running variance 1, PReLU 0.25.
    ``widths``: the channel widths of the three stacks, 5 each; ``nodes``: nodes of the relative stack; ``n_pre``: DCT coefficients."""
    gen = torch.Generator().manual_seed(int(seed))
    uni = lambda bound, *shape: (torch.rand(*shape, generator=gen, dtype=torch.float64) * 2.0 - 1.0).mul(bound).float()
    sd = OrderedDict()
    for si, stack in enumerate(STACKS):
        n = (nodes, 1, nodes + 1)[si]
        for l in range(4):
            cin, cout, p = widths[si][l], widths[si][l + 1], '%s.%d.' % (stack, l)
            if si == 2:
                sd[p + 'gcn.A'] = uni(1.0 / math.sqrt(n), n_pre, n, n)
                sd[p + 'gcn.T'] = uni(1.0 / math.sqrt(n_pre), n, n_pre, n_pre)
            else:
                sd[p + 'gcn.T'] = uni(1.0 / math.sqrt(n_pre), n_pre, n_pre)
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


class FlatParameters:
    """The master copy of a predictor's trained parameters as ONE flat device vector in ``named_parameters()`` order (``self.table``), its Adam moments, the
    reference-named views of them, and the library calls that differ between the predictors only in their name: what ``SkeletonFineTuner`` and
    ``CorrectionFineTuner`` share.  A subclass names its library functions (``interdiff_<PREFIX>_finetune_*`` / ``_train_*``) and its geometry, and sets
    ``lib``, ``device``, ``predictor``, ``weights`` and the Adam hyperparameters before ``_init_state``."""
    PREFIX = None            # 'skeleton' | 'correction'
    NODES = None             # nodes of the relative stack; the object stack has 1, the joint stack NODES + 1
    N_PRE = None             # DCT coefficients

    def _fn(self, name):
        return getattr(self.lib, 'interdiff_%s_%s' % (self.PREFIX, name))

    def _call(self, name, *args):
        _check(self._fn(name)(C.byref(self.predictor.cop), *args), '%s_%s' % (self.PREFIX, name))

    def _init_state(self, sd):
        self.table, self.btable = param_table(sd), buffer_table(sd)
        self.n_param = self.table[-1][1] + int(np.prod(self.table[-1][2]))
        self._check_table()
        self.params = torch.from_numpy(flatten(sd, self.table)).to(self.device)
        self.bn = torch.from_numpy(flatten(sd, self.btable)).to(self.device)
        self.exp_avg = torch.zeros_like(self.params)
        self.exp_avg_sq = torch.zeros_like(self.params)
        self.step = 0
        trained = {n for n, _, _ in self.table}
        self._keys = list(sd.keys())
        self._fixed = {k: torch.as_tensor(np.asarray(v.detach().cpu() if isinstance(v, torch.Tensor) else v)).clone() for k, v in sd.items() if k not in trained}
        self._dtypes = {k: torch.as_tensor(np.asarray(v.detach().cpu() if isinstance(v, torch.Tensor) else v)).dtype for k, v in sd.items() if k in trained}
        self._w8 = (C.c_float * 8)(*self.weights.vector(0)[2:])
        self._ws = {}

    def _check_table(self):
        """The C side derives the same table from the channel widths (csrc/stgcn_train.h ft_plan_for): they must agree."""
        cop = self.predictor.cop
        tab = (C.c_int32 * (12 * TABLE_COLS))()
        n_param, n_bn = C.c_int32(), C.c_int32()
        self._call('finetune_param_table', tab, C.byref(n_param), C.byref(n_bn))
        offs = {n: o for n, o, _ in self.table}
        boffs = {n: o for n, o, _ in self.btable}
        for li in range(12):
            p = '%s.%d.' % (STACKS[li // 4], li % 4)
            row = list(tab[li * TABLE_COLS:(li + 1) * TABLE_COLS])
            want = [offs.get(p + s, -1) for s in LAYER_PARAMS] + [cop.cin[li], cop.cout[li], (self.NODES, 1, self.NODES + 1)[li // 4], int(li // 4 == 2),
                                                                 boffs[p + LAYER_BUFFERS[0]]]
            if row != want:
                raise RuntimeError('parameter table of layer %d: library %r, state_dict %r' % (li, row, want))
        nb = self.btable[-1][1] + int(np.prod(self.btable[-1][2]))
        if n_param.value != self.n_param or n_bn.value != nb:
            raise RuntimeError('parameter count: library %d / %d, state_dict %d / %d' % (n_param.value, n_bn.value, self.n_param, nb))

    def _workspace(self, B):
        if B not in self._ws:
            n = self._fn('finetune_workspace_bytes')(C.byref(self.predictor.cop), B)
            self._ws = {B: torch.empty(n, dtype=torch.uint8, device=self.device)}
        return self._ws[B]

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

    def _outputs(self):
        """-> (out9, grads): the device tensors a gradient call fills."""
        return torch.empty(9, dtype=torch.float32, device=self.device), torch.empty(self.n_param, dtype=torch.float32, device=self.device)

    def _packed(self, out9, grads):
        """-> (loss, loss_dict, weighted_loss_dict, grads) as ``loss_and_grads`` returns them."""
        w = torch.tensor(self.weights.vector(0)[2:], dtype=torch.float32, device=self.device) * out9[1:]
        return out9[0], {k: out9[1 + n] for n, k in enumerate(MSE_KEYS)}, {k: w[n] for n, k in enumerate(MSE_KEYS)}, self.unflatten(grads)

    def apply_gradients(self, grads):
        """One Adam step on ``grads`` (flat [n_param] or a dict under reference names) and the re-fold of the arena."""
        g = self._flat(grads)
        self.step += 1
        self._call('finetune_step', _lib.dptr(self.predictor.arena), _lib.dptr(self.params), _lib.dptr(self.bn), _lib.dptr(g), _lib.dptr(self.exp_avg),
                   _lib.dptr(self.exp_avg_sq), self.step, self.lr, self.betas[0], self.betas[1], self.eps, self.weight_decay, _lib.stream())

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


def check_train_mode(dropout, momentum):
    """A trainer's constructor checks these before it builds anything."""
    if not (0.0 <= float(dropout) < 1.0):
        raise ValueError('dropout must lie in [0, 1), got %r' % (dropout,))
    if not (0.0 <= float(momentum) <= 1.0):
        raise ValueError('momentum must lie in [0, 1], got %r' % (momentum,))


class TrainMode:
    """The module in ``train()`` on top of a fine-tuner (mix in BEFORE it): the dropout keep masks and their flat buffer, the train workspace, the batch
    statistics, the updated running statistics and ``num_batches_tracked`` in ``state_dict``, and the mask seed in the optimizer state.  The trainer
    supplies ``_train_grads(batch, ..., dropout=, want_stats=) -> (out9, grads, stats)``."""

    def _init_train(self, dropout, momentum, seed):
        self.dropout, self.momentum = float(dropout), float(momentum)
        self.seed = fresh_seed() if seed is None else int(seed)
        cop = self.predictor.cop
        self.layers = [('%s.%d' % (STACKS[li // 4], li % 4), int(cop.cout[li]), (self.NODES, 1, self.NODES + 1)[li // 4]) for li in range(12)]
        self.mask_clip = sum(co * self.N_PRE * nodes for _, co, nodes in self.layers)
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
                if tuple(m.shape) != (B, co, self.N_PRE, nodes):
                    raise ValueError('mask of %s: expected %r, got %r' % (name, (B, co, self.N_PRE, nodes), tuple(m.shape)))
                parts.append(m.reshape(-1).to(self.device))
            masks = torch.cat(parts)
        m = torch.as_tensor(masks).reshape(-1)
        if m.numel() != B * self.mask_clip:
            raise ValueError('expected %d mask bytes, got %d' % (B * self.mask_clip, m.numel()))
        return (m != 0).to(self.device, torch.uint8).contiguous()

    def split_masks(self, flat, B):
        """The flat mask buffer -> {layer prefix: view [B, cout, N_PRE, nodes]}."""
        out, off = OrderedDict(), 0
        for name, co, nodes in self.layers:
            n = B * co * self.N_PRE * nodes
            out[name] = flat[off:off + n].view(B, co, self.N_PRE, nodes)
            off += n
        return out

    def dropout_masks(self, B, step=None):
        """The keep masks the in-kernel generator draws at training step ``step`` (default: the next one) -> {layer prefix: uint8 [B,cout,N_PRE,nodes]}."""
        step = self.step if step is None else int(step)
        flat = torch.empty(B * self.mask_clip, dtype=torch.uint8, device=self.device)
        self._call('train_masks', B, self.dropout, self.seed, step, _lib.dptr(flat), _lib.stream())
        return self.split_masks(flat, B)

    # ---- the step
    def _train_workspace(self, B):
        if B not in self._tws:
            n = self._fn('train_workspace_bytes')(C.byref(self.predictor.cop), B)
            self._tws = {B: torch.empty(n, dtype=torch.uint8, device=self.device)}
        return self._tws[B]

    def _count_batch(self):
        for k in self._tracked:
            self._tracked[k] += 1

    def batch_statistics(self, batch, **how):
        """{buffer name: tensor} under the ``running_mean`` / ``running_var`` key names: mean and BIASED variance of this batch at every
        BatchNorm site, without dropout."""
        _, _, stats = self._train_grads(batch, dropout=0.0, want_stats=True, **how)
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
