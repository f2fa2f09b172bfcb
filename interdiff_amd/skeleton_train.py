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
import torch
from . import _lib, stgcn_trainer
from .skeleton import N_PRE, N_JOINTS
from .skeleton_finetune import SkeletonFineTuner
from .stgcn_trainer import TrainMode, check_train_mode

WIDTHS = ((9, 32, 16, 32, 9), (9, 32, 16, 32, 9), (9, 64, 32, 64, 9))        # model/correction_skeleton.py:13-50


def init_state_dict(seed, embedding_dim=128, num_joints=N_JOINTS):
    """A fresh ``ObjProjector`` state_dict -- the checkpoint's keys (plus ``num_batches_tracked``), shapes and dtypes -- drawn from the
    reference's initial DISTRIBUTIONS with a seeded torch generator (not torch's bits): convolution weights and biases U(+-1/sqrt(fan_in)),
    ``gcn.T`` / ``gcn.A`` U(+-1/sqrt(size(1))), BatchNorm weight 1, bias 0, running mean 0, running variance 1, PReLU 0.25.
    ``embedding_dim`` is accepted as the reference's constructor accepts it: the channel widths do not depend on it."""
    return stgcn_trainer.init_state_dict(seed, WIDTHS, num_joints, N_PRE)


class SkeletonTrainer(TrainMode, SkeletonFineTuner):
    """Trains a skeleton predictor from scratch (``init_state_dict``) or from a checkpoint.  ``batch`` as in ``SkeletonFineTuner``.
    ``masks``: the dropout keep masks, uint8, keep iff nonzero -- one flat buffer, the 12 layers in ``named_parameters()`` layer order, each
    [B, cout, 20, nodes], or a dict as ``dropout_masks`` returns; None: the in-kernel generator's masks for (seed, step)."""

    def __init__(self, state_dict, dropout=0.1, momentum=0.1, lr=3e-4, weight_decay=0., betas=(0.9, 0.999), eps=1e-8, weights=None, past_len=10,
                 future_len=10, seed=None, device='cuda'):
        check_train_mode(dropout, momentum)
        super().__init__(state_dict, lr=lr, weight_decay=weight_decay, betas=betas, eps=eps, weights=weights, past_len=past_len, future_len=future_len,
                         device=device)
        self._init_train(dropout, momentum, seed)

    # ---- the step
    def _train_grads(self, batch, masks=None, update=False, dropout=None, want_stats=False):
        B, T, d6_tail, obj_trans, body_gt, pose_gt = self._inputs(batch)
        m = self._mask_buffer(masks, B)
        p = self.dropout if dropout is None else dropout
        out9, grads = self._outputs()
        stats = torch.empty_like(self.bn) if want_stats else None
        ws = self._train_workspace(B)
        self._call('train_grads', _lib.dptr(self.params), _lib.dptr(self.bn), _lib.dptr(d6_tail), _lib.dptr(obj_trans), _lib.dptr(body_gt), _lib.dptr(pose_gt),
                   B, T, self._w8, p, _lib.dptr(m) if m is not None else None, self.seed, self.step, self.momentum, int(update), _lib.dptr(out9),
                   _lib.dptr(grads), _lib.dptr(stats) if want_stats else None, _lib.dptr(ws), ws.numel(), _lib.stream())
        return out9, grads, stats

    def _grads(self, batch):
        out9, grads, _ = self._train_grads(batch)
        return out9, grads

    def loss_and_grads(self, batch, masks=None):
        """As ``SkeletonFineTuner.loss_and_grads`` with the module in train().  Touches neither the running statistics nor the step counter."""
        out9, grads, _ = self._train_grads(batch, masks)
        return self._packed(out9, grads)

    def training_step(self, batch, masks=None):
        """Gradients, the running-statistics update, ``num_batches_tracked += 1``, Adam, the re-fold.  -> the loss BEFORE the step."""
        out9, grads, _ = self._train_grads(batch, masks, update=True)
        self._count_batch()
        self.apply_gradients(grads)
        return out9[0]
