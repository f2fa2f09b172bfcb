"""Training of the SMPL contact-frame correction predictor on the HIP path the way the reference trains it: the module in ``train()``.
All 24 ``BatchNorm2d`` sites normalise with the statistics of the BATCH and update ``running_mean`` / ``running_var`` /
``num_batches_tracked``; ``nn.Dropout(p)`` follows the tcn BatchNorm of every ``ST_GCNN_layer`` (model/layers.py:308-318); from epoch 10
on (``initialize=False``) the contact node of a clip is DRAWN, ``torch.multinomial(contact + 0.5 hand, 1)`` (model/correction_smpl.py:131-132).

    loss, grads     LitInteraction.calc_loss + loss.backward() on ObjProjector.forward, module in train()   train_correction_smpl.py:60-101
    training_step   + the BatchNorm buffer updates + torch.optim.Adam(lr, weight_decay=l2_norm).step()      :51-58, :263-270
    init_state_dict the reference's initial distributions (nn.Conv2d's default, model/sublayers.py:408-410, :494-500)

``CorrectionTrainer`` builds on ``CorrectionFineTuner`` (flat parameter layout, Adam, the re-fold into the arena that ``ObjProjector`` and
the correction hook read); after a step the live predictor is the ``eval()`` model of the new weights AND the new running statistics.

The node draw runs in torch on the batch's device, from a generator seeded by (seed, step): a resumed run draws the same nodes, and nothing
on that route waits for the device.  Clips without contact read node 0.  The kernels take the drawn nodes as data.

Departure from the reference: the 24 convolution biases cancel inside a batch normalisation, so their gradient is identically zero.  The
reference computes fp32 rounding noise there, which Adam turns into a +-lr random walk of parameters that cannot influence the
train-mode output; here those gradients are exact 0.0, and with ``weight_decay = 0`` the biases do not move.

NOT built: the contact / penetration gradient (``d_obj_pred`` stays its seam, as in the fine-tuner), learning-rate schedules, the
Lightning glue, the dataset.

All arithmetic but the draw runs in libinterdiff_hip.so (csrc/objproj_bn_train.h around csrc/objproj_train.h, the train-mode layer in
csrc/stgcn_bn_train.h; launchers csrc/objproj_bn_train.hip).
"""
import ctypes as C
import math
from collections import OrderedDict
import numpy as np
import torch
from . import _lib
from .objprojector import HAND_MARKERS
from .skeleton import _check
from .stgcn_pack import STACKS
from .correction_finetune import CorrectionFineTuner, N_MARKERS
from .correction_losses import CorrectionLossWeights, MSE_KEYS
from .diffusion import fresh_seed

N_PRE = 10
WIDTHS = ((9, 32, 16, 32, 9),) * 3                                           # model/correction_smpl.py: the three stacks


def init_state_dict(seed, num_verts=N_MARKERS, dct=N_PRE):
    """A fresh ``ObjProjector`` state_dict -- the checkpoint's keys, shapes and dtypes -- drawn from the reference's initial DISTRIBUTIONS
    with a seeded torch generator (not torch's bits): convolution weights and biases U(+-1/sqrt(fan_in)), ``gcn.T`` / ``gcn.A``
    U(+-1/sqrt(size(1))), BatchNorm weight 1, bias 0, running mean 0, running variance 1, PReLU 0.25."""
    gen = torch.Generator().manual_seed(int(seed))
    uni = lambda bound, *shape: (torch.rand(*shape, generator=gen, dtype=torch.float64) * 2.0 - 1.0).mul(bound).float()
    sd = OrderedDict()
    for si, stack in enumerate(STACKS):
        nodes = (num_verts, 1, num_verts + 1)[si]
        for l in range(4):
            cin, cout, p = WIDTHS[si][l], WIDTHS[si][l + 1], '%s.%d.' % (stack, l)
            if si == 2:
                sd[p + 'gcn.A'] = uni(1.0 / math.sqrt(nodes), dct, nodes, nodes)
                sd[p + 'gcn.T'] = uni(1.0 / math.sqrt(dct), nodes, dct, dct)
            else:
                sd[p + 'gcn.T'] = uni(1.0 / math.sqrt(dct), dct, dct)
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


def node_weights(contact):
    """``contact`` [B,67] (summed future labels) -> the weights the reference draws from: contact + 0.5 on the hand markers (float32)."""
    w = contact.to(torch.float32).clone()
    w[:, HAND_MARKERS] += 0.5
    return w


def draw_nodes(contact, seed, step):
    """The node of every clip at training step ``step``: 1 + ``torch.multinomial(contact + 0.5 hand, 1)`` where the clip has contact, 0 where it
    has none -> int32 [B] on ``contact``'s device.  The generator lives on that device and is seeded from (seed, step) alone; no host sync."""
    gen = torch.Generator(device=contact.device)
    gen.manual_seed((int(seed) * 0x9E3779B97F4A7C15 + int(step) * 0xBF58476D1CE4E5B9 + 0x94D049BB133111EB) % (1 << 63))
    idx = torch.multinomial(node_weights(contact), 1, generator=gen)[:, 0]           # every row has its hand bonus: no all-zero row
    return torch.where(contact.sum(dim=1) > 0, idx + 1, torch.zeros_like(idx)).to(torch.int32)


def check_nodes(nodes, contact):
    """Injected nodes [B] against the clips' contact [B,67]: node 0 iff the clip has no contact, otherwise 1..67 with a positive weight.
    One host sync.  -> int32 [B] on ``contact``'s device."""
    n = torch.as_tensor(nodes).to(contact.device)
    if n.dim() != 1 or n.shape[0] != contact.shape[0] or n.dtype.is_floating_point or n.dtype == torch.bool:
        raise ValueError('nodes must be %d integers, got %r %s' % (contact.shape[0], tuple(n.shape), n.dtype))
    n = n.to(torch.int64)
    has = contact.sum(dim=1) > 0
    inside = (n >= 1) & (n <= N_MARKERS)
    w = node_weights(contact).gather(1, (n.clamp(1, N_MARKERS) - 1)[:, None])[:, 0]
    bad = torch.where(has, ~inside | ~(w > 0), n != 0)
    if bool(bad.any()):
        raise ValueError('nodes: 0 exactly for the clips without contact, otherwise 1..%d with a positive weight; clips %r are not'
                         % (N_MARKERS, torch.nonzero(bad)[:, 0].tolist()))
    return n.to(torch.int32).contiguous()


class CorrectionTrainer(CorrectionFineTuner):
    """Trains a contact-frame predictor from scratch (``init_state_dict``) or from a checkpoint.  ``batch`` as in ``CorrectionFineTuner``.
    ``masks``: the dropout keep masks, uint8, keep iff nonzero -- one flat buffer, the 12 layers in ``named_parameters()`` layer order, each
    [B, cout, 10, nodes], or a dict as ``dropout_masks`` returns; None: the in-kernel generator's masks for (seed, step).
    ``nodes`` [B] (``initialize=False`` only): the node each clip reads; None: ``draw_nodes`` for (seed, step)."""

    def __init__(self, state_dict, T=35, past_len=10, dropout=0.1, momentum=0.1, lr=3e-4, weight_decay=0., betas=(0.9, 0.999), eps=1e-8,
                 weights=CorrectionLossWeights(), seed=None, device='cuda'):
        if not (0.0 <= float(dropout) < 1.0):
            raise ValueError('dropout must lie in [0, 1), got %r' % (dropout,))
        if not (0.0 <= float(momentum) <= 1.0):
            raise ValueError('momentum must lie in [0, 1], got %r' % (momentum,))
        super().__init__(state_dict, T=T, past_len=past_len, lr=lr, weight_decay=weight_decay, betas=betas, eps=eps, weights=weights, device=device)
        self.dropout, self.momentum = float(dropout), float(momentum)
        self.seed = fresh_seed() if seed is None else int(seed)
        cop = self.predictor.cop
        self.layers = [('%s.%d' % (STACKS[li // 4], li % 4), int(cop.cout[li]), (N_MARKERS, 1, N_MARKERS + 1)[li // 4]) for li in range(12)]
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
        """The flat mask buffer -> {layer prefix: view [B, cout, 10, nodes]}."""
        out, off = OrderedDict(), 0
        for name, co, nodes in self.layers:
            n = B * co * N_PRE * nodes
            out[name] = flat[off:off + n].view(B, co, N_PRE, nodes)
            off += n
        return out

    def dropout_masks(self, B, step=None):
        """The keep masks the in-kernel generator draws at training step ``step`` (default: the next one) -> {layer prefix: uint8 [B,cout,10,nodes]}."""
        step = self.step if step is None else int(step)
        flat = torch.empty(B * self.mask_clip, dtype=torch.uint8, device=self.device)
        _check(self.lib.interdiff_correction_train_masks(C.byref(self.predictor.cop), B, self.dropout, self.seed, step, _lib.dptr(flat), _lib.stream()),
               'correction_train_masks')
        return self.split_masks(flat, B)

    # ---- the step
    def _train_workspace(self, B):
        if B not in self._tws:
            n = self.lib.interdiff_correction_train_workspace_bytes(C.byref(self.predictor.cop), B)
            self._tws = {B: torch.empty(n, dtype=torch.uint8, device=self.device)}
        return self._tws[B]

    def select_nodes(self, contact, initialize, nodes=None, step=None):
        """The nodes a step at ``step`` (default: the next one) reads -> int32 [B] or None (``initialize``: the 68-node mean, ``nodes`` ignored)."""
        if initialize:
            return None
        if nodes is not None:
            return check_nodes(nodes, contact)
        return draw_nodes(contact, self.seed, self.step if step is None else step).contiguous()

    def _train_grads(self, batch, initialize=False, masks=None, nodes=None, d_obj_pred=None, update=False, dropout=None, want_stats=False):
        B, T, d6, ot, pos, contact, extra = self._inputs(batch, d_obj_pred)
        m = self._mask_buffer(masks, B)
        picked = self.select_nodes(contact, initialize, nodes)
        p = self.dropout if dropout is None else dropout
        out9 = torch.empty(9, dtype=torch.float32, device=self.device)
        grads = torch.empty(self.n_param, dtype=torch.float32, device=self.device)
        stats = torch.empty_like(self.bn) if want_stats else None
        ws = self._train_workspace(B)
        _check(self.lib.interdiff_correction_train_grads(C.byref(self.predictor.cop), _lib.dptr(self.params), _lib.dptr(self.bn), _lib.dptr(d6), _lib.dptr(ot),
                                                         _lib.dptr(pos), _lib.dptr(contact, torch.int32),
                                                         _lib.dptr(picked, torch.int32) if picked is not None else None,
                                                         _lib.dptr(extra, allow_none=True), B, T, int(bool(initialize)), self._w8, p,
                                                         _lib.dptr(m) if m is not None else None, self.seed, self.step, self.momentum, int(update),
                                                         _lib.dptr(out9), _lib.dptr(grads), _lib.dptr(stats) if want_stats else None, _lib.dptr(ws),
                                                         ws.numel(), _lib.stream()), 'correction_train_grads')
        return out9, grads, stats

    def _grads(self, batch, initialize=False, d_obj_pred=None):
        out9, grads, _ = self._train_grads(batch, initialize, d_obj_pred=d_obj_pred)
        return out9, grads

    def loss_and_grads(self, batch, initialize=False, masks=None, nodes=None, d_obj_pred=None):
        """As ``CorrectionFineTuner.loss_and_grads`` with the module in train().  Touches neither the running statistics nor the step counter."""
        out9, grads, _ = self._train_grads(batch, initialize, masks, nodes, d_obj_pred)
        w = torch.tensor(self.weights.vector(0)[2:], dtype=torch.float32, device=self.device) * out9[1:]
        return out9[0], {k: out9[1 + n] for n, k in enumerate(MSE_KEYS)}, {k: w[n] for n, k in enumerate(MSE_KEYS)}, self.unflatten(grads)

    def training_step(self, batch, current_epoch=0, masks=None, nodes=None, d_obj_pred=None):
        """Gradients (``initialize = current_epoch < 10``, like ``_common_step``), the running-statistics update, ``num_batches_tracked += 1``,
        Adam, the re-fold.  -> the loss of the 8 MSE terms BEFORE the step.  At an epoch whose annealed contact / penetration weights are not
        zero their gradient at the prediction must come in as ``d_obj_pred``, as in the fine-tuner: without it this raises."""
        geometry = self.weights.vector(current_epoch)[:2]
        if any(w != 0 for w in geometry) and d_obj_pred is None:
            raise ValueError('epoch %d weighs the penetration / contact terms by %r: pass their gradient at obj_pred as d_obj_pred [T,B,9] '
                             '(their backward is not built here)' % (current_epoch, geometry))
        out9, grads, _ = self._train_grads(batch, current_epoch < 10, masks, nodes, d_obj_pred, update=True)
        for k in self._tracked:
            self._tracked[k] += 1
        self.apply_gradients(grads)
        return out9[0]

    def batch_statistics(self, batch):
        """{buffer name: tensor} under the ``running_mean`` / ``running_var`` key names: mean and BIASED variance of this batch at every
        BatchNorm site, without dropout (the stacks run before the node selection: it does not enter)."""
        _, _, stats = self._train_grads(batch, initialize=True, dropout=0.0, want_stats=True)
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
