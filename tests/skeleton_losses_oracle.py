"""fp64 numpy restatement of the skeleton diffusion trainer's 13 loss terms and their weighted sum (interdiff/train_diffusion_skeleton.py
``forward_backward`` :100-161 and ``calc_val_loss`` :190-247 -- the same arithmetic on the model output / on a sample).  Used for the
shapes the recorded fixture (tests/golden/skel_losses.npz) does not cover; it shares no code with interdiff_amd or the kernel.

Tokens [B,1,C,T], C = n_body + 3 * n_points + 7: body | object keypoints | translation 3 | quaternion xyzw 4.
"""
import numpy as np

KEYS = ('body_past', 'body_future', 'obj_past', 'obj_future', 'loss_obj_nonrot_past', 'loss_obj_nonrot_future', 'loss_obj_rot_past',
        'loss_obj_rot_future', 'quaternion_reg_loss', 'loss_obj_rot_v', 'loss_obj_nonrot_v', 'loss_body_v', 'loss_obj_v')
# the CLI defaults (:372-379)
WEIGHTS = dict(weight_past=0.5, weight_body=2.0, weight_obj=1.0, weight_obj_rot=1.0, weight_obj_nonrot=1.0, weight_quat_reg=0.01, weight_v=1.0)


def split(x, n_body=63, n_points=12):
    """[B,1,C,T] -> body, obj, pose as [T,B,*] float64 (``squeeze(1).permute(2, 0, 1)`` + ``torch.split``, :101-104)."""
    x = np.asarray(x, np.float64)
    assert x.ndim == 4 and x.shape[1] == 1 and x.shape[2] == n_body + 3 * n_points + 7
    tbc = x[:, 0].transpose(2, 0, 1)
    return tbc[..., :n_body], tbc[..., n_body:n_body + 3 * n_points], tbc[..., n_body + 3 * n_points:]


def per_clip_terms(pred, gt, past_len=10, n_body=63, n_points=12):
    """The 13 unweighted terms of every clip on its own: [13, B] float64, in KEYS order."""
    bp, op, pp = split(pred, n_body, n_points)
    bg, og, pg = split(gt, n_body, n_points)
    P = past_len
    mse = lambda a, b: ((a - b) ** 2).mean(axis=(0, 2))                     # over frames and channels, per clip
    vel = lambda a: a[1:] - a[:-1]
    qq = (pp[..., -4:] ** 2).sum(-1)                                        # [T,B]
    d = {
        'body_past': mse(bp[:P], bg[:P]), 'body_future': mse(bp[P:], bg[P:]),
        'obj_past': mse(op[:P], og[:P]), 'obj_future': mse(op[P:], og[P:]),
        'loss_obj_nonrot_past': mse(pp[:P, :, :3], pg[:P, :, :3]), 'loss_obj_nonrot_future': mse(pp[P:, :, :3], pg[P:, :, :3]),
        'loss_obj_rot_past': mse(pp[:P, :, -4:], pg[:P, :, -4:]), 'loss_obj_rot_future': mse(pp[P:, :, -4:], pg[P:, :, -4:]),
        'quaternion_reg_loss': ((qq - 1.0) ** 2).mean(axis=0),
        'loss_obj_rot_v': mse(vel(pp[..., -4:]), vel(pg[..., -4:])), 'loss_obj_nonrot_v': mse(vel(pp[..., :3]), vel(pg[..., :3])),
        'loss_body_v': mse(vel(bp), vel(bg)), 'loss_obj_v': mse(vel(op), vel(og)),
    }
    return np.stack([d[k] for k in KEYS])


def terms(pred, gt, past_len=10, n_body=63, n_points=12):
    """The 13 batch terms [13] (``MSELoss(reduction='mean')`` over a batch of equal clips = the mean of the per-clip means)."""
    return per_clip_terms(pred, gt, past_len, n_body, n_points).mean(axis=1)


def weight_vector(w=None):
    """The factors of the weighted dict (:145-159) in KEYS order."""
    w = dict(WEIGHTS, **(w or {}))
    return np.asarray([w['weight_body'] * w['weight_past'], w['weight_body'], w['weight_obj'] * w['weight_past'], w['weight_obj'],
                       w['weight_obj_nonrot'] * w['weight_past'], w['weight_obj_nonrot'], w['weight_obj_rot'] * w['weight_past'], w['weight_obj_rot'],
                       w['weight_quat_reg'], w['weight_obj_rot'] * w['weight_v'], w['weight_obj_nonrot'] * w['weight_v'],
                       w['weight_body'] * w['weight_v'], w['weight_obj'] * w['weight_v']], np.float64)


def weighted(t, w=None):
    """terms [13] -> (loss, weighted terms [13])."""
    wt = np.asarray(t, np.float64) * weight_vector(w)
    return wt.sum(), wt


def near_unit_case(seed, B, T, K=None, n_body=63, n_points=12, noise=0.05):
    """Random tokens whose quaternions are near unit: gt with unit quaternions, prediction(s) = gt + ``noise`` x N(0,1).
    -> (pred [B,1,C,T] or [K,B,1,C,T], gt [B,1,C,T]) float32."""
    rs = np.random.RandomState(seed)
    C = n_body + 3 * n_points + 7
    gt = 0.5 * rs.standard_normal((B, 1, C, T))
    q = rs.standard_normal((B, 1, 4, T))
    gt[:, :, -4:] = q / np.linalg.norm(q, axis=2, keepdims=True)
    pred = gt[None] + noise * rs.standard_normal((K or 1, B, 1, C, T))
    return (pred if K else pred[0]).astype(np.float32), gt.astype(np.float32)
