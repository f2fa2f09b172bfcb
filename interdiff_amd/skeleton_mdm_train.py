"""Training of the HO-GCN skeleton denoiser on the HIP path: one optimiser step of interdiff/train_diffusion_skeleton.py.

    SkeletonDenoiserTrainer(state_dict).training_step(batch)     _get_embeddings, q_sample, forward with saves, the 13 terms, backward, AdamW

What one call replaces: ``LitInteraction._common_step(mode='train')`` (:255-262) -- ``MDM._get_embeddings`` (model/diffusion_skeleton.py:194-215),
``q_sample``, ``MDM.forward(x, timesteps, zero_pose_obj, y)`` (:231-257), the loss of ``forward_backward`` (:89-168) -- its ``loss.backward()`` and
``torch.optim.AdamW`` (:181-184, lr 3e-4, weight decay ``--l2_norm`` = 0).  The model has no PointNet++: the conditioning is
``shapeEmbedding(zero_pose_obj)``, a linear layer, so the pass has no seam: all 230 parameter tensors (``PARAM_NAMES``; 5,499,582 parameters) get
their gradient and their update.  ``PositionalEmbedding.pe`` and any other entry of the constructor's state_dict pass through unchanged.

The reference trains with ``--dropout 0 --cond_mask_prob 0`` and stochastic depth at rate 0, so ``train()`` and ``eval()`` compute the same function;
other settings are refused, as in ``DenoiserTrainer``.  All arithmetic is in libinterdiff_hip.so (csrc/skeleton_mdm_train.hip on the stacks of
csrc/mdm_train.h): exact fp32, no float atomics -- two calls give the same bits.  torch holds the device memory.  The flat vectors, the state-dict
round trip, ``loss_and_grads``, ``apply_gradients`` and ``training_step`` are ``flat_trainer.FlatAdamWTrainer``'s.
"""
import torch
from . import _lib, flat_trainer
from .flat_trainer import MAX_T, MAX_MEM
from .mdm_train import PARAM_NAMES as _DECODER_NAMES, ENCODER_PARAM_NAMES as _ENCODER_NAMES
from .skeleton_losses import KEYS, N_BODY, N_POINTS, SkeletonLossWeights

C_TOK = N_BODY + 3 * N_POINTS + 7
PARAM_NAMES = _DECODER_NAMES + _ENCODER_NAMES + ('shapeEmbedding.weight', 'shapeEmbedding.bias')      # include/interdiff_hip.h, SKELETON PARAMETER TABLE


def param_table():
    """(offsets, sizes, n_param) of the flat vectors as the library lays them out (``interdiff_skeleton_mdm_train_param_table``)."""
    return flat_trainer.param_table('interdiff_skeleton_mdm_train_param_table', len(PARAM_NAMES))


def tokens_of(batch, device):
    """The dataset tuple (body [B,T,21,3], obj [B,T,12,3], pose [B,T,7], zero_pose_obj [B,12,3]) or a dict with ``gt`` [B,1,106,T] and
    ``zero_pose_obj``  ->  (gt [B,1,106,T], zero_pose_obj [B,12,3]) on ``device``: the ``gt`` of ``_get_embeddings`` (:206) as ``_common_step`` permutes it."""
    if isinstance(batch, dict):
        gt, z = batch['gt'], batch['zero_pose_obj']
    else:
        body, obj, pose, z = batch[:4]
        B, T = body.shape[:2]
        gt = torch.cat([body.reshape(B, T, -1), obj.reshape(B, T, -1), pose], dim=2).permute(0, 2, 1).unsqueeze(1)
    return gt.float().to(device).contiguous(), z.float().to(device).contiguous()


class SkeletonDenoiserTrainer(flat_trainer.FlatAdamWTrainer):
    """``loss.backward()`` + ``optimizer.step()`` of the reference's skeleton diffusion trainer, whole model (the scaffold: interdiff_amd/flat_trainer.py).

    ``state_dict``: the reference skeleton ``MDM``'s (tensors or arrays).  ``dropout`` / ``cond_mask_prob``: the configuration the checkpoint was
    made for; anything but 0 raises (not built).  ``weights`` / ``past_len``: the loss of ``forward_backward``; ``n_steps``: the cosine schedule's length.
    ``state_dict()`` returns the 230 trained tensors and every other entry of the constructor's (``PositionalEmbedding.pe``) as it came in.
    """

    PARAM_NAMES, LOSS_KEYS, C_TOK = PARAM_NAMES, KEYS, C_TOK

    def __init__(self, state_dict, device='cuda', lr=3e-4, weight_decay=0.0, betas=(0.9, 0.999), eps=1e-8, weights=SkeletonLossWeights(), past_len=10,
                 n_steps=1000, dropout=0.0, cond_mask_prob=0.0):
        super().__init__(state_dict, PARAM_NAMES, param_table(), device, lr, weight_decay, betas, eps, weights, past_len, n_steps, dropout, cond_mask_prob)

    def param_table(self):
        return self.offsets, self.sizes, self.n_param

    def export_mdm(self):
        """An ``interdiff_amd.skeleton.SkeletonMDM`` packed (on the host) from the current weights: for sampling and ``skeleton_losses.validation_step``.
        No training batch reads it: the trainer computes ``cond`` itself, from the current weights."""
        from .skeleton import SkeletonMDM
        return SkeletonMDM({k: v.cpu() for k, v in self.state_dict().items()}, device=self.device, n_steps=self.n_steps)

    def loss_grad(self, pred, target):
        """``interdiff_skeleton_denoising_loss_grad``: d/d pred of mean_b sum_i w_i term_i[b]."""
        B, T = pred.shape[0], pred.shape[-1]
        if tuple(pred.shape[1:3]) != (1, C_TOK) or target.shape != pred.shape:
            raise ValueError('pred / target [B,1,%d,T]' % C_TOK)
        d = torch.empty_like(pred, memory_format=torch.contiguous_format)
        _lib.check(self.lib.interdiff_skeleton_denoising_loss_grad(_lib.dptr(pred.contiguous(), torch.float32), _lib.dptr(target.contiguous(), torch.float32), B, T,
                                                                   self.past_len, self._wvec, _lib.dptr(d), _lib.stream()), 'skeleton_denoising_loss_grad')
        return d

    def grads_at(self, x_t, t, zero_pose_obj, target, d_pred=None):
        """One forward with saves and the backward on given x_t: (pred [B,1,106,T], terms [13,B]); the flat gradient lands in ``self.grads``,
        ``self.cond`` [past_len,B,256] keeps the encoder's output.  ``target`` is x_start (its past frames are the encoder's tokens);
        ``d_pred`` [B,1,106,T], when given, takes the place of the loss gradient -- the seam for other objectives."""
        x_t, target, d_pred, B, T = self._checked(x_t, target, d_pred)
        z, S = zero_pose_obj.contiguous(), self.past_len
        if tuple(z.shape) != (B, N_POINTS, 3):
            raise ValueError('zero_pose_obj must be [B,%d,3]' % N_POINTS)
        ws = self._workspace(self.lib.interdiff_skeleton_mdm_train_workspace_bytes, B, T, S)       # (needs 2 <= past_len and T >= past_len + 2)
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=self.device)
        pred, terms, cond = torch.empty_like(x_t), new(len(KEYS), B), new(S, B, 256)
        _lib.check(self.lib.interdiff_skeleton_mdm_train_grads(
            _lib.dptr(self.params), _lib.dptr(self.pe), self.pe.shape[0], _lib.dptr(x_t, torch.float32), _lib.dptr(t.to(self.device).contiguous(), torch.int64),
            _lib.dptr(target, torch.float32), _lib.dptr(z, torch.float32), B, T, S, self._wvec, _lib.dptr(d_pred, torch.float32, allow_none=True),
            _lib.dptr(self.grads), _lib.dptr(cond), _lib.dptr(pred), _lib.dptr(terms), _lib.dptr(ws), ws.numel(), _lib.stream()), 'skeleton_mdm_train_grads')
        self.pred, self.cond = pred, cond
        return pred, terms

    _grads = grads_at

    def _inputs(self, batch):
        """``batch`` of ``loss_and_grads`` (``_common_step(mode='train')`` with the backward): the dataset tuple (body [B,T,21,3], obj [B,T,12,3], pose [B,T,7],
        zero_pose_obj [B,12,3]) that ``skeleton_losses.sample_kwargs`` takes, or a dict with ``gt`` [B,1,106,T] and ``zero_pose_obj``.  ``loss_and_grads`` has no
        seam to return: its result is the 4-tuple, and ``self.pred`` / ``self.cond`` keep the model output and the conditioning."""
        return tokens_of(batch, self.device)
