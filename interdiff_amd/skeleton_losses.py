"""Scoring of a skeleton diffusion checkpoint on the HIP path: the number interdiff/train_diffusion_skeleton.py selects checkpoints by
(``ModelCheckpoint(monitor='val_loss')``, :443-445) and its teacher-forced denoising objective.  Forward only -- no backward pass, no
optimiser, no Lightning, no rendering (the ``visualize`` / ``torch.save`` branches of ``_common_step`` are not built).

    denoising_losses   LitInteraction.forward_backward (:89-175) around GaussianDiffusion.training_losses; log_loss_dict (:177-180)
    calc_val_loss      calc_val_loss (:190-253) on the split of _common_step (:280-283)
    validation_step / test_step   _common_step(mode='valid' / 'test') (:255-295) + what :329-346 log

Tokens are [B,1,106,T]: body 21 x 3 | object keypoints 12 x 3 | object translation 3 | object quaternion xyzw 4.  The keypoint channels
scored are the sample's / the prediction's own -- the denoiser's keypoint head wrote them; nothing is re-posed here.  All arithmetic
runs in libinterdiff_hip.so (csrc/skeleton_losses.hip): scoring K samples is two launches whatever K and B are, the 13 per-clip
denoising terms are one; torch only applies the 13 weights (two elementwise launches).  ``calc_metric`` (:65-87) is evaluated by the
reference in both ``forward_backward`` and ``calc_val_loss`` and its result is thrown away (nothing logs or returns it): not built.
"""
from dataclasses import dataclass
import torch
from . import _lib
from .skeleton import _check
from .diffusion import sample_loop

KEYS = ('body_past', 'body_future', 'obj_past', 'obj_future', 'loss_obj_nonrot_past', 'loss_obj_nonrot_future', 'loss_obj_rot_past',
        'loss_obj_rot_future', 'quaternion_reg_loss', 'loss_obj_rot_v', 'loss_obj_nonrot_v', 'loss_body_v', 'loss_obj_v')      # the reference's dict order (:129-143, :215-229) = the kernel's term index
N_BODY, N_POINTS = 63, 12


@dataclass(frozen=True)
class SkeletonLossWeights:
    """The reference's CLI defaults (train_diffusion_skeleton.py:372-379)."""
    weight_past: float = 0.5
    weight_body: float = 2.0
    weight_obj: float = 1.0
    weight_obj_rot: float = 1.0
    weight_obj_nonrot: float = 1.0
    weight_quat_reg: float = 0.01
    weight_v: float = 1.0

    def vector(self):
        """The 13 factors of the weighted dict (:145-159), in KEYS order."""
        g = (self.weight_body, self.weight_obj, self.weight_obj_nonrot, self.weight_obj_rot)
        value = tuple(g[i // 2] * (1.0 if i % 2 else self.weight_past) for i in range(8))
        return value + (self.weight_quat_reg, self.weight_obj_rot * self.weight_v, self.weight_obj_nonrot * self.weight_v,
                        self.weight_body * self.weight_v, self.weight_obj * self.weight_v)


_W_CACHE = {}


def _weights_on(weights, device):
    key = (weights.vector(), str(device))
    if key not in _W_CACHE:
        _W_CACHE[key] = torch.tensor(weights.vector(), dtype=torch.float32, device=device)
    return _W_CACHE[key]


def score_samples(samples, gt, past_len=10, n_body=N_BODY, n_points=N_POINTS):
    """``samples`` [K,B,1,C,T] (several samples of ONE batch) against ``gt`` [B,1,C,T] -> (terms [K,13]: per sample the 13 unweighted
    means over its clips, per_clip [K,13,B]: every clip's own means).  Two launches (interdiff_skeleton_sample_losses)."""
    lib = _lib.load()
    gt = gt.contiguous()
    if samples.dim() != 5 or tuple(samples.shape[1:]) != tuple(gt.shape) or gt.shape[1] != 1:
        raise ValueError('samples must be [K,B,1,C,T] like gt [B,1,C,T]')
    K, (B, _, Cc, T) = samples.shape[0], gt.shape
    terms = torch.empty(K, len(KEYS), dtype=torch.float32, device=gt.device)
    per_clip = torch.empty(K, len(KEYS), B, dtype=torch.float32, device=gt.device)
    _check(lib.interdiff_skeleton_sample_losses(_lib.dptr(samples.contiguous(), torch.float32), _lib.dptr(gt, torch.float32), K, B, Cc, T, past_len,
                                                n_body, n_points, _lib.dptr(terms), _lib.dptr(per_clip), None, 0, _lib.stream()),
           'skeleton_sample_losses')
    return terms, per_clip


def calc_val_loss(sample, batch_gt, past_len=10, weights=SkeletonLossWeights(), n_body=N_BODY, n_points=N_POINTS):
    """``sample`` [B,1,106,T] (what ``p_sample_loop`` returns) against ``batch_gt`` [B,1,106,T] -> (loss, loss_dict, weighted_loss_dict),
    0-dim device tensors under the reference's 13 keys; ``loss`` is the sum of the weighted terms (:247)."""
    terms = score_samples(sample[None], batch_gt, past_len, n_body, n_points)[0][0]
    wt = terms * _weights_on(weights, terms.device)
    return wt.sum(), {k: terms[i] for i, k in enumerate(KEYS)}, {k: wt[i] for i, k in enumerate(KEYS)}


def denoising_losses(model, diffusion, gt, zero_pose_obj, cond, t=None, noise=None, seed=None, weights=SkeletonLossWeights(), past_len=10,
                     generator=None):
    """``forward_backward`` without the backward: per-clip timestep ``t`` int64 [B] (None: ``diffusion.sample_timesteps``, the uniform
    schedule sampler), x_t by ``q_sample`` (``noise`` given, else the in-kernel generator under ``seed``; the training path sets no
    inpainting mask), ONE ``SkeletonMDM.forward`` with the per-clip timesteps, one loss launch.  ``gt`` [B,1,106,T], ``cond``
    [past_len,B,256] (``_get_embeddings``), ``zero_pose_obj`` [B,12,3].
    Returns (loss, loss_dict {name: [B]}, t): ``loss`` is the reference's scalar -- every term's mean over the batch, weighted and summed,
    times the schedule sampler's weights, which are all one -- and it is ALL the skeleton trainer logs (``log_loss_dict`` :177-180 logs
    ``train_loss`` alone; unlike the SMPL trainer's it makes no per-quartile split, so nothing is read back to the host); ``loss_dict`` is
    the 13 unweighted terms per clip (their mean over the clips is the reference's ``loss_dict``)."""
    lib = _lib.load()
    gt = gt.contiguous()
    B, _, _, T = gt.shape
    if t is None:
        t, _ = diffusion.sample_timesteps(B, gt.device, generator)
    t = t.to(gt.device)
    pred, target = diffusion.training_losses(model, gt, t, model_kwargs={'y': {'cond': cond}, 'zero_pose_obj': zero_pose_obj}, noise=noise, seed=seed)
    out = torch.empty(len(KEYS), B, dtype=torch.float32, device=gt.device)
    _check(lib.interdiff_skeleton_denoising_losses(_lib.dptr(pred.contiguous(), torch.float32), _lib.dptr(target, torch.float32), B, T, past_len,
                                                   model.n_body, model.n_points, _lib.dptr(out), _lib.stream()), 'skeleton_denoising_losses')
    loss = (out.mean(dim=1) * _weights_on(weights, gt.device)).sum()
    return loss, {k: out[i] for i, k in enumerate(KEYS)}, t


def sample_kwargs(model, batch, past_len=10):
    """What ``_common_step`` builds before it samples (:256-277): ``batch`` = (body [B,T,21,3], object keypoints [B,T,12,3], pose [B,T,7],
    zero_pose_obj [B,12,3]) as the dataset yields it -> (gt [B,1,106,T], model_kwargs with cond, the ground truth and the past-frames mask)."""
    dev = model.device
    body_gt, obj_gt, pose_gt = (batch[i].transpose(0, 1).float().to(dev) for i in range(3))
    zero_pose_obj = batch[3].float().to(dev).contiguous()
    cond, gt = model._get_embeddings(body_gt, obj_gt, pose_gt, zero_pose_obj, past_len=past_len)
    gt = gt.permute(1, 2, 0).unsqueeze(1).contiguous()
    mask = torch.ones_like(gt, dtype=torch.bool)
    mask[..., past_len:] = False
    return gt, {'y': {'cond': cond, 'inpainted_motion': gt, 'inpainting_mask': mask}, 'zero_pose_obj': zero_pose_obj}


def validation_step(model, diffusion, batch, past_len=10, seed=None, weights=SkeletonLossWeights(), **loop_kw):
    """``validation_step`` (:329-333): ``_get_embeddings``, one full sample with the past frames inpainted (``p_sample_loop`` on the graph
    route, no hook), scored by ``calc_val_loss``.  -> (val_loss, loss_dict, weighted_loss_dict).  ``loop_kw`` goes to ``p_sample_loop``, or with ``sampler='ddim'`` (+ ``eta=``) to ``ddim_sample_loop``."""
    gt, kw = sample_kwargs(model, batch, past_len)
    sample = sample_loop(diffusion, model, tuple(gt.shape), clip_denoised=False, model_kwargs=kw, seed=seed, **loop_kw)
    return calc_val_loss(sample, gt, past_len, weights, model.n_body, model.n_points)


def test_step(model, diffusion, batch, past_len=10, seed=None, weights=SkeletonLossWeights(), **loop_kw):
    """``test_step`` (:335-346): the same one sample and the same scoring as ``validation_step`` (the skeleton trainer draws no second
    sample and has no best-of-K terms).  -> (test_loss, {'test_' + name: term} -- the names it logs, :344-346 --, weighted_loss_dict)."""
    loss, ld, wd = validation_step(model, diffusion, batch, past_len, seed, weights, **loop_kw)
    return loss, {'test_' + k: v for k, v in ld.items()}, wd


test_step.__test__ = False          # (a library entry named after the reference's, not a pytest case)
