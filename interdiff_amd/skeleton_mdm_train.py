"""Training of the HO-GCN skeleton denoiser on the HIP path: one optimiser step of interdiff/train_diffusion_skeleton.py.

    SkeletonDenoiserTrainer(state_dict).training_step(batch)     _get_embeddings, q_sample, forward with saves, the 13 terms, backward, AdamW

What one call replaces: ``LitInteraction._common_step(mode='train')`` (:255-262) -- ``MDM._get_embeddings`` (model/diffusion_skeleton.py:194-215),
``q_sample``, ``MDM.forward(x, timesteps, zero_pose_obj, y)`` (:231-257), the loss of ``forward_backward`` (:89-168) -- its ``loss.backward()`` and
``torch.optim.AdamW`` (:181-184, lr 3e-4, weight decay ``--l2_norm`` = 0).  The model has no PointNet++: the conditioning is
``shapeEmbedding(zero_pose_obj)``, a linear layer, so the pass has no seam: all 230 parameter tensors (``PARAM_NAMES``; 5,499,582 parameters) get
their gradient and their update.  ``PositionalEmbedding.pe`` and any other entry of the constructor's state_dict pass through unchanged.

The reference trains with ``--dropout 0 --cond_mask_prob 0`` and stochastic depth at rate 0, so ``train()`` and ``eval()`` compute the same function;
other settings are refused, as in ``DenoiserTrainer``.  All arithmetic is in libinterdiff_hip.so (csrc/skeleton_mdm_train.hip on the stacks of
csrc/mdm_train.h): exact fp32, no float atomics -- two calls give the same bits.  torch holds the device memory.
"""
import ctypes as C
import torch
from . import _lib
from .diffusion import create_gaussian_diffusion
from .mdm import positional_table
from .mdm_train import PARAM_NAMES as _DECODER_NAMES, ENCODER_PARAM_NAMES as _ENCODER_NAMES
from .skeleton_losses import KEYS, N_BODY, N_POINTS, SkeletonLossWeights

MAX_T, MAX_MEM, C_TOK = 128, 16, N_BODY + 3 * N_POINTS + 7
PARAM_NAMES = _DECODER_NAMES + _ENCODER_NAMES + ('shapeEmbedding.weight', 'shapeEmbedding.bias')      # include/interdiff_hip.h, SKELETON PARAMETER TABLE


def param_table():
    """(offsets, sizes, n_param) of the flat vectors as the library lays them out (``interdiff_skeleton_mdm_train_param_table``)."""
    n = len(PARAM_NAMES)
    off, size, cnt, total = (C.c_int64 * n)(), (C.c_int64 * n)(), C.c_int32(0), C.c_int64(0)
    _lib.check(_lib.load().interdiff_skeleton_mdm_train_param_table(off, size, C.byref(cnt), C.byref(total)), 'skeleton_mdm_train_param_table')
    if cnt.value != n:
        raise RuntimeError('parameter table: %d tensors, expected %d' % (cnt.value, n))
    return list(off), list(size), int(total.value)


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


class SkeletonDenoiserTrainer:
    """``loss.backward()`` + ``optimizer.step()`` of the reference's skeleton diffusion trainer, whole model.

    ``state_dict``: the reference skeleton ``MDM``'s (tensors or arrays).  ``dropout`` / ``cond_mask_prob``: the configuration the checkpoint was
    made for; anything but 0 raises (not built).  ``weights`` / ``past_len``: the loss of ``forward_backward``; ``n_steps``: the cosine schedule's length.
    """

    PARAM_NAMES = PARAM_NAMES

    def __init__(self, state_dict, device='cuda', lr=3e-4, weight_decay=0.0, betas=(0.9, 0.999), eps=1e-8, weights=SkeletonLossWeights(), past_len=10,
                 n_steps=1000, dropout=0.0, cond_mask_prob=0.0):
        if dropout > 0 or cond_mask_prob > 0:
            raise ValueError('SkeletonDenoiserTrainer implements the reference defaults --dropout 0 --cond_mask_prob 0 only')
        self.lib = _lib.load()
        self.device = torch.device(device)
        self.lr, self.weight_decay, self.betas, self.eps = float(lr), float(weight_decay), (float(betas[0]), float(betas[1])), float(eps)
        self.weights, self.past_len, self.n_steps = weights, int(past_len), int(n_steps)
        self.diffusion = create_gaussian_diffusion('cosine', self.n_steps)
        sd = {k: torch.as_tensor(v).detach().clone() for k, v in state_dict.items()}
        self.names = PARAM_NAMES
        missing = [k for k in self.names if k not in sd]
        if missing:
            raise KeyError('state_dict lacks %s' % missing[:3])
        self.offsets, self.sizes, self.n_param = param_table()
        self.shapes = [tuple(sd[k].shape) for k in self.names]
        for k, s, shp in zip(self.names, self.sizes, self.shapes):
            if sd[k].numel() != s:
                raise ValueError('%s: %s does not match the parameter table (%d floats)' % (k, shp, s))
        self._passthrough = {k: v for k, v in sd.items() if k not in self.names}         # returned by state_dict() with identical bits
        self.params = torch.cat([sd[k].reshape(-1).float() for k in self.names]).to(self.device).contiguous()
        self.exp_avg, self.exp_avg_sq = torch.zeros_like(self.params), torch.zeros_like(self.params)
        self.grads = torch.zeros_like(self.params)
        self.step = 0
        pe = sd['PositionalEmbedding.pe'][:, 0] if 'PositionalEmbedding.pe' in sd else positional_table()
        self.pe = torch.as_tensor(pe).float().to(self.device).contiguous()
        self._w13 = (C.c_float * len(KEYS))(*weights.vector())
        self._wdev = torch.tensor(weights.vector(), dtype=torch.float32, device=self.device)
        self._ws = {}
        self.pred = self.cond = None                                 # the model output and the conditioning of the last gradient call

    # ------------------------------------------------------------------------------------------------------------ state
    def param_table(self):
        return self.offsets, self.sizes, self.n_param

    def named_views(self, flat):
        return {k: flat[o:o + s].view(shp) for k, o, s, shp in zip(self.names, self.offsets, self.sizes, self.shapes)}

    def state_dict(self):
        """The reference's names: the 230 trained tensors (copies, on the trainer's device) and every other entry of the constructor's state_dict
        (``PositionalEmbedding.pe``) exactly as it came in."""
        out = dict(self._passthrough)
        out.update({k: v.clone() for k, v in self.named_views(self.params).items()})
        return out

    def optimizer_state(self):
        return dict(step=self.step, exp_avg=self.exp_avg.clone(), exp_avg_sq=self.exp_avg_sq.clone())

    def load_optimizer_state(self, state):
        self.step = int(state['step'])
        self.exp_avg.copy_(state['exp_avg'])
        self.exp_avg_sq.copy_(state['exp_avg_sq'])

    def export_mdm(self):
        """An ``interdiff_amd.skeleton.SkeletonMDM`` packed (on the host) from the current weights: for sampling and ``skeleton_losses.validation_step``.
        No training batch reads it: the trainer computes ``cond`` itself, from the current weights."""
        from .skeleton import SkeletonMDM
        return SkeletonMDM({k: v.cpu() for k, v in self.state_dict().items()}, device=self.device, n_steps=self.n_steps)

    # ------------------------------------------------------------------------------------------------------------ steps
    def _workspace(self, B, T):
        need = self.lib.interdiff_skeleton_mdm_train_workspace_bytes(B, T, self.past_len)
        if need == 0:
            raise ValueError('unsupported shape B=%d T=%d past_len=%d (T <= %d, 2 <= past_len <= %d, T >= past_len + 2)' % (B, T, self.past_len, MAX_T, MAX_MEM))
        ws = self._ws.get((B, T))
        if ws is None:
            ws = self._ws[(B, T)] = torch.empty(need, dtype=torch.uint8, device=self.device)
        return ws

    def loss_grad(self, pred, target):
        """``interdiff_skeleton_denoising_loss_grad``: d/d pred of mean_b sum_i w_i term_i[b]."""
        B, T = pred.shape[0], pred.shape[-1]
        if tuple(pred.shape[1:3]) != (1, C_TOK) or target.shape != pred.shape:
            raise ValueError('pred / target [B,1,%d,T]' % C_TOK)
        d = torch.empty_like(pred, memory_format=torch.contiguous_format)
        _lib.check(self.lib.interdiff_skeleton_denoising_loss_grad(_lib.dptr(pred.contiguous(), torch.float32), _lib.dptr(target.contiguous(), torch.float32), B, T,
                                                                   self.past_len, self._w13, _lib.dptr(d), _lib.stream()), 'skeleton_denoising_loss_grad')
        return d

    def grads_at(self, x_t, t, zero_pose_obj, target, d_pred=None):
        """One forward with saves and the backward on given x_t: (pred [B,1,106,T], terms [13,B]); the flat gradient lands in ``self.grads``,
        ``self.cond`` [past_len,B,256] keeps the encoder's output.  ``target`` is x_start (its past frames are the encoder's tokens);
        ``d_pred`` [B,1,106,T], when given, takes the place of the loss gradient -- the seam for other objectives."""
        x_t, target, z = x_t.contiguous(), target.contiguous(), zero_pose_obj.contiguous()
        B, T, S = x_t.shape[0], x_t.shape[-1], self.past_len
        if tuple(x_t.shape[1:3]) != (1, C_TOK) or target.shape != x_t.shape or tuple(z.shape) != (B, N_POINTS, 3):
            raise ValueError('x_t / target [B,1,%d,T], zero_pose_obj [B,%d,3]' % (C_TOK, N_POINTS))
        if T > MAX_T:
            raise ValueError('SkeletonDenoiserTrainer supports T <= %d (got %d)' % (MAX_T, T))
        if d_pred is not None:
            if d_pred.shape != x_t.shape:
                raise ValueError('d_pred must be [B,1,%d,T]' % C_TOK)
            d_pred = d_pred.contiguous()
        ws = self._workspace(B, T)
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=self.device)
        pred, terms, cond = torch.empty_like(x_t), new(len(KEYS), B), new(S, B, 256)
        _lib.check(self.lib.interdiff_skeleton_mdm_train_grads(
            _lib.dptr(self.params), _lib.dptr(self.pe), self.pe.shape[0], _lib.dptr(x_t, torch.float32), _lib.dptr(t.to(self.device).contiguous(), torch.int64),
            _lib.dptr(target, torch.float32), _lib.dptr(z, torch.float32), B, T, S, self._w13, _lib.dptr(d_pred, torch.float32, allow_none=True),
            _lib.dptr(self.grads), _lib.dptr(cond), _lib.dptr(pred), _lib.dptr(terms), _lib.dptr(ws), ws.numel(), _lib.stream()), 'skeleton_mdm_train_grads')
        self.pred, self.cond = pred, cond
        return pred, terms

    def loss_and_grads(self, batch, t=None, noise=None, seed=None, d_pred=None, generator=None):
        """``_common_step(mode='train')`` with the backward: ``batch`` is the dataset tuple (body [B,T,21,3], obj [B,T,12,3], pose [B,T,7],
        zero_pose_obj [B,12,3]) that ``skeleton_losses.sample_kwargs`` takes, or a dict with ``gt`` [B,1,106,T] and ``zero_pose_obj``; the timestep draw
        and ``q_sample`` of ``skeleton_losses.denoising_losses``, then one gradient call.  Returns (loss [B], loss_dict {name: [B]}, weighted
        {name: [B]}, grads {name: tensor} -- views of the flat gradient, valid until the next call); the reference's scalar is ``loss.mean()``.
        ``self.pred`` and ``self.cond`` keep the model output and the conditioning."""
        gt, z = tokens_of(batch, self.device)
        B = gt.shape[0]
        if gt.shape[-1] > MAX_T:
            raise ValueError('SkeletonDenoiserTrainer supports T <= %d (got %d)' % (MAX_T, gt.shape[-1]))
        if t is None:
            t, _ = self.diffusion.sample_timesteps(B, gt.device, generator)
        t = t.to(gt.device)
        x_t = self.diffusion.q_sample(gt, t, noise=noise, seed=seed)
        _, terms = self.grads_at(x_t, t, z, gt, d_pred)
        wt = terms * self._wdev[:, None]
        return wt.sum(0), {k: terms[i] for i, k in enumerate(KEYS)}, {k: wt[i] for i, k in enumerate(KEYS)}, self.named_views(self.grads)

    def apply_gradients(self):
        """``optimizer.step()``: AdamW on the flat vectors with the gradient of the last ``loss_and_grads``."""
        self.step += 1
        _lib.check(self.lib.interdiff_mdm_train_step(_lib.dptr(self.params), _lib.dptr(self.grads), _lib.dptr(self.exp_avg), _lib.dptr(self.exp_avg_sq), self.n_param,
                                                     self.step, self.lr, self.betas[0], self.betas[1], self.eps, self.weight_decay, _lib.stream()), 'mdm_train_step')

    def training_step(self, batch, t=None, noise=None, seed=None, d_pred=None, generator=None):
        """``loss_and_grads`` followed by the AdamW entry; returns what ``loss_and_grads`` returns."""
        out = self.loss_and_grads(batch, t=t, noise=noise, seed=seed, d_pred=d_pred, generator=generator)
        self.apply_gradients()
        return out
