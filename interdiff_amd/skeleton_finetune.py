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
that ``SkeletonObjProjector`` reads.  The flat parameter layout (``param_table``) is documented in include/interdiff_hip.h; it, the
master copy and the Adam state (``FlatParameters``) are ``interdiff_amd.stgcn_trainer``'s, shared with the SMPL predictor and re-exported here.
"""
import torch
from . import _lib
from .skeleton import SkeletonObjProjector, N_PRE, N_JOINTS, _strip
from .correction_losses import CorrectionLossWeights
from .stgcn_trainer import (BN_EPS, LAYER_PARAMS, LAYER_BUFFERS, TABLE_COLS, FlatParameters, param_table, buffer_table, flatten,        # noqa: F401
                            folded_to_reference_grads)


class SkeletonFineTuner(FlatParameters):
    """Adapts a skeleton predictor to a user's own clips.  ``batch`` is what ``skeleton_validation_step`` takes: (body [B,T,21,3],
    object keypoints [B,T,12,3], pose [B,T,7], zero_pose_obj [B,12,3]); T = past_len + future_len = 20."""

    PREFIX, NODES, N_PRE = 'skeleton', N_JOINTS, N_PRE

    def __init__(self, state_dict, lr=3e-4, weight_decay=0., betas=(0.9, 0.999), eps=1e-8, weights=None, past_len=10, future_len=10, device='cuda'):
        sd = _strip(state_dict)
        self.lib = _lib.load()
        self.device = torch.device(device)
        self.lr, self.weight_decay, self.betas, self.eps = float(lr), float(weight_decay), (float(betas[0]), float(betas[1])), float(eps)
        self.weights = weights or CorrectionLossWeights()
        self.predictor = SkeletonObjProjector(sd, past_len, future_len, device=device)          # its arena is the live one
        self.past_len, self.T = past_len, past_len + future_len
        self._init_state(sd)

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
        B, T, d6_tail, obj_trans, body_gt, pose_gt = self._inputs(batch)
        out9, grads = self._outputs()
        ws = self._workspace(B)
        self._call('finetune_grads', _lib.dptr(self.params), _lib.dptr(self.bn), _lib.dptr(d6_tail), _lib.dptr(obj_trans), _lib.dptr(body_gt),
                   _lib.dptr(pose_gt), B, T, self._w8, _lib.dptr(out9), _lib.dptr(grads), _lib.dptr(ws), ws.numel(), _lib.stream())
        return out9, grads

    def loss_and_grads(self, batch):
        """-> (loss, loss_dict, weighted_loss_dict, grads): 0-dim device tensors under the reference's 8 keys, ``grads`` = {reference
        parameter name: d loss / d parameter} (views of one flat device tensor)."""
        return self._packed(*self._grads(batch))

    def training_step(self, batch):
        """Gradients, Adam, re-fold.  -> the loss BEFORE the step (0-dim device tensor), like ``training_step`` of the reference."""
        out9, grads = self._grads(batch)
        self.apply_gradients(grads)
        return out9[0]
