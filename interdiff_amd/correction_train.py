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

The contact / penetration terms come in as in the fine-tuner: ``predict`` (the forward launches alone, same masks, nodes and (seed, step)) ->
``correction_losses.contact_gradient`` -> the gradient call; the running statistics are updated once.  NOT built: a single-pass launcher,
learning-rate schedules, the Lightning glue, the dataset.

All arithmetic but the draw runs in libinterdiff_hip.so (csrc/objproj_bn_train.h around csrc/objproj_train.h, the train-mode layer in
csrc/stgcn_bn_train.h; launchers csrc/objproj_bn_train.hip).
"""
import torch
from . import _lib, stgcn_trainer
from .objprojector import HAND_MARKERS
from .correction_finetune import CorrectionFineTuner, N_MARKERS, N_PRE
from .correction_losses import CorrectionLossWeights
from .stgcn_trainer import TrainMode, check_train_mode

WIDTHS = ((9, 32, 16, 32, 9),) * 3                                           # model/correction_smpl.py: the three stacks


def init_state_dict(seed, num_verts=N_MARKERS, dct=N_PRE):
    """A fresh ``ObjProjector`` state_dict -- the checkpoint's keys, shapes and dtypes -- drawn from the reference's initial DISTRIBUTIONS
    with a seeded torch generator (not torch's bits): convolution weights and biases U(+-1/sqrt(fan_in)), ``gcn.T`` / ``gcn.A``
    U(+-1/sqrt(size(1))), BatchNorm weight 1, bias 0, running mean 0, running variance 1, PReLU 0.25."""
    return stgcn_trainer.init_state_dict(seed, WIDTHS, num_verts, dct)


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


class CorrectionTrainer(TrainMode, CorrectionFineTuner):
    """Trains a contact-frame predictor from scratch (``init_state_dict``) or from a checkpoint.  ``batch`` as in ``CorrectionFineTuner``.
    ``masks``: the dropout keep masks, uint8, keep iff nonzero -- one flat buffer, the 12 layers in ``named_parameters()`` layer order, each
    [B, cout, 10, nodes], or a dict as ``dropout_masks`` returns; None: the in-kernel generator's masks for (seed, step).
    ``nodes`` [B] (``initialize=False`` only): the node each clip reads; None: ``draw_nodes`` for (seed, step)."""

    def __init__(self, state_dict, T=35, past_len=10, dropout=0.1, momentum=0.1, lr=3e-4, weight_decay=0., betas=(0.9, 0.999), eps=1e-8,
                 weights=CorrectionLossWeights(), seed=None, device='cuda'):
        check_train_mode(dropout, momentum)
        super().__init__(state_dict, T=T, past_len=past_len, lr=lr, weight_decay=weight_decay, betas=betas, eps=eps, weights=weights, device=device)
        self._init_train(dropout, momentum, seed)

    # ---- the step
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
        out9, grads = self._outputs()
        stats = torch.empty_like(self.bn) if want_stats else None
        ws = self._train_workspace(B)
        self._call('train_grads', _lib.dptr(self.params), _lib.dptr(self.bn), _lib.dptr(d6), _lib.dptr(ot), _lib.dptr(pos), _lib.dptr(contact, torch.int32),
                   _lib.dptr(picked, torch.int32) if picked is not None else None, _lib.dptr(extra, allow_none=True), B, T, int(bool(initialize)),
                   self._w8, p, _lib.dptr(m) if m is not None else None, self.seed, self.step, self.momentum, int(update), _lib.dptr(out9),
                   _lib.dptr(grads), _lib.dptr(stats) if want_stats else None, _lib.dptr(ws), ws.numel(), _lib.stream())
        return out9, grads, stats

    def _grads(self, batch, initialize=False, d_obj_pred=None):
        out9, grads, _ = self._train_grads(batch, initialize, d_obj_pred=d_obj_pred)
        return out9, grads

    def predict(self, batch, initialize=False, masks=None, nodes=None):
        """``obj_pred`` [T,B,9] as the backward of ``loss_and_grads`` with the same ``masks`` / ``nodes`` (None: those of (seed, step)) sees it: the forward
        launches of the gradient call alone (``interdiff_correction_train_predict``).  Touches neither the running statistics nor the step counter."""
        B, T, d6, ot, pos, contact, _ = self._inputs(batch)
        m = self._mask_buffer(masks, B)
        picked = self.select_nodes(contact, initialize, nodes)
        out = torch.empty(T, B, 9, dtype=torch.float32, device=self.device)
        ws = self._train_workspace(B)
        self._call('train_predict', _lib.dptr(self.params), _lib.dptr(d6), _lib.dptr(ot), _lib.dptr(pos), _lib.dptr(contact, torch.int32),
                   _lib.dptr(picked, torch.int32) if picked is not None else None, B, T, int(bool(initialize)), self.dropout,
                   _lib.dptr(m) if m is not None else None, self.seed, self.step, _lib.dptr(out), _lib.dptr(ws), ws.numel(), _lib.stream())
        return out

    def loss_and_grads(self, batch, initialize=None, masks=None, nodes=None, d_obj_pred=None, current_epoch=None):
        """As ``CorrectionFineTuner.loss_and_grads`` with the module in train(); with ``current_epoch`` and the geometry operands in the batch both
        passes read the same masks and nodes.  Touches neither the running statistics nor the step counter."""
        if initialize is None:
            initialize = current_epoch is not None and current_epoch < 10
        d, terms = (d_obj_pred, None) if current_epoch is None else self._seam(batch, current_epoch, initialize, d_obj_pred, masks=masks, nodes=nodes)
        out9, grads, _ = self._train_grads(batch, initialize, masks, nodes, d)
        return self._packed(out9, grads) if terms is None else self._packed10(out9, grads, terms, current_epoch)

    def training_step(self, batch, current_epoch=0, masks=None, nodes=None, d_obj_pred=None):
        """Gradients (``initialize = current_epoch < 10``, like ``_common_step``), the running-statistics update, ``num_batches_tracked += 1``,
        Adam, the re-fold.  -> the loss BEFORE the step.  At an epoch whose annealed contact / penetration weights are not zero a batch that carries
        ``obj_points`` and ``human_verts`` gets those terms here, as in the fine-tuner: the prediction pass and the gradient pass read the same masks,
        nodes and (seed, step), and the running statistics are updated once, by the gradient pass.  An explicit ``d_obj_pred`` wins; with neither this
        raises."""
        initialize = current_epoch < 10
        d, terms = self._seam(batch, current_epoch, initialize, d_obj_pred, masks=masks, nodes=nodes)
        out9, grads, _ = self._train_grads(batch, initialize, masks, nodes, d, update=True)
        self._count_batch()
        self.apply_gradients(grads)
        return out9[0] if terms is None else self._packed10(out9, grads, terms, current_epoch)[0]

    def batch_statistics(self, batch):
        """{buffer name: tensor} under the ``running_mean`` / ``running_var`` key names: mean and BIASED variance of this batch at every
        BatchNorm site, without dropout (the stacks run before the node selection: it does not enter)."""
        return super().batch_statistics(batch, initialize=True)
