"""Checkpoint scoring on the HIP path: the numbers the reference selects checkpoints by (``ModelCheckpoint(monitor='val_loss')``,
interdiff/train_diffusion_smpl.py:635-637) and its teacher-forced denoising objective.  Forward only -- no backward pass, no optimiser.

    denoising_losses   LitInteraction.forward_backward (:60-166) + log_loss_dict (:168-175)
    calc_val_loss      the scoring of validation_step: _common_step(mode='valid') :396-409 + calc_val_loss :185-260
    calc_loss          the scoring of test_step: _common_step(mode='test') :422-443 + calc_loss :262-379 (16 terms + 16 best-of-K ``_min``)
    validation_step / test_step   the existing sampler (x_T drawn in-kernel and inpainted, diffusion.p_sample_loop) + the scoring

The batch is ``eval.py``'s clip batch (gt [B,1,144,T], cond, hand_pose [T,B,90] NOT padded, ...) or the DataLoader's dict of lists
(``eval.as_clip_batch``).  All arithmetic runs in libinterdiff_hip.so (csrc/losses.hip): scoring K samples is two launches whatever K
is, the 16 per-clip denoising terms are one; torch only stacks the samples and applies the 16 weights (two elementwise launches).
``rotvec_to_rotmat`` (tools.py:88-90) calls human_body_prior's ``aa2matrot``, which is not part of the reference tree: the kernel
restates it (parity unpinned -- restatement defines the contract; csrc/rot_math.h).
"""
from dataclasses import dataclass
import numpy as np
import torch
from . import _lib
from .eval import as_clip_batch
from .diffusion import sample_loop

_KINDS, _GROUPS = ('past', 'v_past', 'future', 'v_future'), ('body_rot', 'body_nonrot', 'obj_rot', 'obj_nonrot')
LOSS_KEYS = tuple('%s_%s' % (g, k) for k in _KINDS for g in _GROUPS)        # the reference's dict order (:117-134); kernel index = 4 * kind + group
MIN_KEYS = tuple(k + '_min' for k in LOSS_KEYS)                             # calc_loss only (:340-355)


@dataclass(frozen=True)
class LossWeights:
    """The reference's CLI defaults (train_diffusion_smpl.py:566-570, :573)."""
    weight_smplx_rot: float = 1.0
    weight_smplx_nonrot: float = 0.2
    weight_obj_rot: float = 0.1
    weight_obj_nonrot: float = 0.2
    weight_past: float = 1.0
    weight_v: float = 0.2

    def vector(self):
        """The 16 factors of the weighted dicts (:136-153), in LOSS_KEYS order."""
        g = (self.weight_smplx_rot, self.weight_smplx_nonrot, self.weight_obj_rot, self.weight_obj_nonrot)
        return tuple(g[i % 4] * (self.weight_v if (i // 4) % 2 else 1.0) * (self.weight_past if i // 4 < 2 else 1.0) for i in range(16))


_W_CACHE = {}


def _weights_on(weights, device):
    key = (weights.vector(), str(device))
    if key not in _W_CACHE:
        _W_CACHE[key] = torch.tensor(weights.vector(), dtype=torch.float32, device=device)
    return _W_CACHE[key]


def denoising_losses(model, diffusion, batch, t=None, noise=None, seed=None, weights=LossWeights(), past_len=10, generator=None):
    """``forward_backward`` without the backward: per-clip timestep ``t`` (None: ``diffusion.sample_timesteps``), x_t by ``q_sample``
    (``noise`` given, else the in-kernel generator under ``seed``), ONE denoiser forward, the 16 per-clip terms in rot6d space.
    Returns (loss [B] -- the weighted sum, before the schedule sampler's weights, which are all one --, loss_dict {name: [B]},
    weighted {name: [B]}, quartiles {name_qN: float}: per timestep quartile the mean of the weighted term over the clips in it,
    ``log_loss_dict``).  The quartile split reads ``t`` and the terms back to the host (one synchronisation)."""
    lib = _lib.load()
    batch = as_clip_batch(model, batch, past_len)
    gt = batch['gt'].contiguous()
    B, _, _, T = gt.shape
    if t is None:
        t, _ = diffusion.sample_timesteps(B, gt.device, generator)
    t = t.to(gt.device)
    pred, target = diffusion.training_losses(model, gt, t, model_kwargs={'y': {'cond': batch['cond']}}, noise=noise, seed=seed)
    out = torch.empty(16, B, dtype=torch.float32, device=gt.device)
    _lib.check(lib.interdiff_denoising_losses(_lib.dptr(pred.contiguous(), torch.float32), _lib.dptr(target, torch.float32), B, T, past_len,
                                              _lib.dptr(out), _lib.stream()), 'denoising_losses')
    wt = out * _weights_on(weights, gt.device)[:, None]
    loss = wt.sum(0)
    loss_dict = {k: out[i] for i, k in enumerate(LOSS_KEYS)}
    weighted = {k: wt[i] for i, k in enumerate(LOSS_KEYS)}
    th, wh = t.cpu().numpy(), wt.cpu().numpy()
    quart = (4 * th // diffusion.num_timesteps).astype(np.int64)
    quartiles = {'%s_q%d' % (k, q): float(wh[i][quart == q].mean()) for i, k in enumerate(LOSS_KEYS) for q in sorted(set(quart.tolist()))}
    return loss, loss_dict, weighted, quartiles


def _score(samples, batch, past_len, weights, variant, per_clip=None):
    lib = _lib.load()
    gt = batch['gt'].contiguous()
    K, B, T = samples.shape[0], gt.shape[0], gt.shape[-1]
    if tuple(samples.shape[1:]) != tuple(gt.shape) or gt.shape[1:3] != (1, 144):
        raise ValueError('samples must be [K,B,1,144,T] like gt [B,1,144,T]')
    hands = batch['hand_pose'].contiguous()
    if tuple(hands.shape) != (T, B, 90):
        raise ValueError('hand_pose must be [T,B,90] (ground-truth hands, not padded)')
    terms = torch.empty(32, dtype=torch.float32, device=gt.device)
    if per_clip is None:
        per_clip = torch.empty(K, 16, B, dtype=torch.float32, device=gt.device)
    _lib.check(lib.interdiff_sample_losses(_lib.dptr(samples.contiguous(), torch.float32), _lib.dptr(gt, torch.float32), _lib.dptr(hands, torch.float32),
                                           K, B, T, past_len, variant, _lib.dptr(terms), _lib.dptr(per_clip), None, 0, _lib.stream()), 'sample_losses')
    wt = terms[:16] * _weights_on(weights, gt.device)
    loss = wt.sum()
    loss_dict = {k: terms[i] for i, k in enumerate(LOSS_KEYS)}
    if variant == _lib.LOSS_TEST:
        loss_dict.update({k: terms[16 + i] for i, k in enumerate(MIN_KEYS)})
    return loss, loss_dict, {k: wt[i] for i, k in enumerate(LOSS_KEYS)}, per_clip


def calc_val_loss(sample, batch, past_len=10, weights=LossWeights()):
    """``sample`` [B,1,144,T] (rot6d tokens, what ``p_sample_loop`` returns) -> (loss, loss_dict, weighted_loss_dict), 0-dim device
    tensors under the reference's 16 keys."""
    return _score(sample[None], batch, past_len, weights, _lib.LOSS_VAL)[:3]


def calc_loss(samples, batch, past_len=10, weights=LossWeights(), return_per_clip=False):
    """``samples`` [K,B,1,144,T] or a list of K token tensors -> (loss, loss_dict with the 16 terms over all K samples and the 16
    best-of-K ``_min`` terms, weighted_loss_dict); ``return_per_clip``: also every (sample, term, clip) mean [K,16,B]."""
    if isinstance(samples, (list, tuple)):
        samples = torch.stack(list(samples))
    out = _score(samples, batch, past_len, weights, _lib.LOSS_TEST)
    return out if return_per_clip else out[:3]


def _valid_kwargs(batch, past_len):
    """model_kwargs of mode 'valid' / 'test' (:385-393, :417-420): cond, the ground truth and the past-frames mask."""
    gt = batch['gt']
    mask = torch.ones_like(gt, dtype=torch.bool)
    mask[..., past_len:] = False
    return {'y': dict(cond=batch['cond'], inpainted_motion=gt, inpainting_mask=mask)}


def sample_seeds(seed, K):
    """The per-sample seeds ``test_step`` hands the sampler: ``seed + k`` (None: a fresh one per sample)."""
    return [None if seed is None else int(seed) + k for k in range(K)]


def validation_step(model, diffusion, batch, past_len=10, seed=None, weights=LossWeights(), **loop_kw):
    """``validation_step``: one full sample (x_T drawn in-kernel and inpainted: ``p_sample_loop`` with ``noise=None``), scored by
    ``calc_val_loss``.  ``loop_kw`` goes to ``p_sample_loop`` (n_steps=, use_graph=, ...), or with ``sampler='ddim'`` (+ ``eta=``) to ``ddim_sample_loop``."""
    batch = as_clip_batch(model, batch, past_len)
    sample = sample_loop(diffusion, model, tuple(batch['gt'].shape), clip_denoised=False, model_kwargs=_valid_kwargs(batch, past_len), seed=seed, **loop_kw)
    return calc_val_loss(sample, batch, past_len, weights)


def test_step(model, diffusion, batch, past_len=10, seed=None, diverse_samples=10, weights=LossWeights(), **loop_kw):
    """``test_step``: ``diverse_samples`` samples (seeds ``sample_seeds(seed, K)``), scored by ``calc_loss``."""
    batch = as_clip_batch(model, batch, past_len)
    kw = _valid_kwargs(batch, past_len)
    samples = [sample_loop(diffusion, model, tuple(batch['gt'].shape), clip_denoised=False, model_kwargs=kw, seed=s, **loop_kw)
               for s in sample_seeds(seed, diverse_samples)]
    return calc_loss(samples, batch, past_len, weights)


test_step.__test__ = False          # (a library entry named after the reference's, not a pytest case)
