"""CPU restatement (torch, any float dtype -- fp64 for the error budget) of the scoring side of the reference's trainer
(interdiff/train_diffusion_smpl.py), the counterpart of interdiff_amd/losses.py + csrc/losses.hip.  Written from the reference's
behaviour, checked against its OWN output recorded in tests/golden/losses.npz (tests/test_losses.py):

  q_sample            diffusion/gaussian_diffusion.py:233-250 (+ the inpainting of x_t, :1264-1268)
  denoising_terms     LitInteraction.forward_backward :72-134, l2 :54-58 -- 16 per-clip vectors [B], quirks kept
  to_axis_angle       _common_step :396-408 / :422-438 -- rot6d tokens -> axis-angle, hand joints spliced in
  sample_terms        calc_val_loss :185-237 (variant 'val') / calc_loss :262-356 (variant 'test')
  weighted            the weights of :239-256, LossWeights = the argparse defaults :566-573

``aa2matrot`` restates human_body_prior's function of that name (tools.py:78-90 calls it; the package is neither under the reference
tree nor installed): parity unpinned -- restatement defines the contract.  The golden generator puts THIS function into its shim,
so the recorded numbers pin the reference's code around it.
"""
import numpy as np
import torch
from oracle import rotations as rot

LOSS_KEYS = tuple('%s_%s%s' % (g, n, k) for k in ('_past', '_v_past', '_future', '_v_future') for g, n in
                  (('body', 'rot'), ('body', 'nonrot'), ('obj', 'rot'), ('obj', 'nonrot')))
WEIGHTS = dict(weight_smplx_rot=1.0, weight_smplx_nonrot=0.2, weight_obj_rot=0.1, weight_obj_nonrot=0.2, weight_past=1.0, weight_v=0.2)
SMPL_DIM = 132


def aa2matrot(aa):
    """[N,3] -> [N,3,3]: Rodrigues on axis = aa / (theta + 1e-6) where theta^2 > 1e-6, else I + [aa]x (angle_axis_to_rotation_matrix)."""
    theta2 = (aa * aa).sum(1, keepdim=True)
    theta = torch.sqrt(theta2)
    w = aa / (theta + 1e-6)
    wx, wy, wz = w[:, 0:1], w[:, 1:2], w[:, 2:3]
    c, s = torch.cos(theta), torch.sin(theta)
    k = 1.0 - c
    normal = torch.cat([c + wx * wx * k, wx * wy * k - wz * s, wy * s + wx * wz * k,
                        wz * s + wx * wy * k, c + wy * wy * k, -wx * s + wy * wz * k,
                        -wy * s + wx * wz * k, wx * s + wy * wz * k, c + wz * wz * k], dim=1)
    rx, ry, rz = aa[:, 0:1], aa[:, 1:2], aa[:, 2:3]
    one = torch.ones_like(rx)
    taylor = torch.cat([one, -rz, ry, rz, one, -rx, -ry, rx, one], dim=1)
    return torch.where(theta2 > 1e-6, normal, taylor).view(-1, 3, 3)


def rotvec_to_rotmat(rotvec):
    return aa2matrot(rotvec.contiguous().view(-1, 3)).view(-1, 3, 3)


def sqrt_tables(betas):
    """fp64 sqrt(alphas_cumprod), sqrt(1 - alphas_cumprod) (gaussian_diffusion.py:160-161)."""
    ac = np.cumprod(1.0 - np.asarray(betas, dtype=np.float64))
    return np.sqrt(ac), np.sqrt(1.0 - ac)


def q_sample(betas, x0, t, noise, gt=None, mask=None):
    """The tables are cast to the dtype of x0 AFTER the per-clip extraction, like ``_extract_into_tensor(...).float()``."""
    sa, s1 = sqrt_tables(betas)
    tn = t.cpu().numpy()
    shape = (-1,) + (1,) * (x0.dim() - 1)
    a, b = (torch.from_numpy(v[tn]).to(x0.dtype).view(shape) for v in (sa, s1))
    xt = a * x0 + b * noise
    if mask is not None:
        xt = (xt * ~mask) + (gt * mask)
    return xt


def _split(x):
    """[B,1,144,T] -> body [T,B,135], obj [T,B,9]."""
    xt = x.squeeze(1).permute(2, 0, 1).contiguous()
    return xt[..., :SMPL_DIM + 3], xt[..., SMPL_DIM + 3:]


def _l2(a, b):
    return ((a - b) ** 2).mean(dim=[0, 2])


def denoising_terms(pred, gt, past_len):
    """{key: [B]} in LOSS_KEYS order."""
    P = past_len
    (bp, op), (bg, og) = _split(pred), _split(gt)
    groups = [(bp[..., :-3], bg[..., :-3]), (bp[..., -3:], bg[..., -3:]), (op[..., :-3], og[..., :-3]), (op[..., -3:], og[..., -3:])]
    out = []
    for x, g in groups:
        out.append(_l2(x[:P], g[:P]))
    for x, g in groups:
        out.append(_l2(x[1:P + 1] - x[:P], g[1:P + 1] - g[1:P + 1]) + _l2(x[1:P] - x[:P - 1], x[2:P + 1] - x[1:P]))
    for x, g in groups:
        out.append(_l2(x[P:], g[P:]))
    for x, g in groups:
        out.append(_l2(x[P:] - x[P - 1:-1], g[P:] - g[P:]) + _l2(x[P - 1:-2] - x[P:-1], x[P:-1] - x[P + 1:]))
    return dict(zip(LOSS_KEYS, out))


def weight_vector(weights=None):
    w = dict(WEIGHTS, **(weights or {}))
    g = [w['weight_smplx_rot'], w['weight_smplx_nonrot'], w['weight_obj_rot'], w['weight_obj_nonrot']]
    return [g[i % 4] * (w['weight_v'] if (i // 4) % 2 else 1.0) * (w['weight_past'] if i // 4 < 2 else 1.0) for i in range(16)]


def weighted(terms, weights=None):
    """(loss, weighted dict): the weighted sum over the 16 non-``_min`` terms."""
    wd = {k: terms[k] * w for k, w in zip(LOSS_KEYS, weight_vector(weights))}
    return sum(wd.values()), wd


def quartiles(t, wd, num_timesteps):
    """log_loss_dict :168-175: per key and timestep quartile, the mean of the clips that fall into it."""
    out = {}
    for key, values in wd.items():
        acc = {}
        for sub_t, sub_loss in zip(t.cpu().numpy(), values.detach().cpu().numpy()):
            acc.setdefault(int(4 * sub_t / num_timesteps), []).append(float(sub_loss))
        out.update({'%s_q%d' % (key, q): float(np.mean(v)) for q, v in acc.items()})
    return out


def to_axis_angle(sample, hand_pose, past_len, pred):
    """[B,1,144,T] rot6d tokens -> body [T,B,66+90+3], obj [T,B,6]; ``pred``: hands from the padded past frames."""
    body, obj = _split(sample)
    T, B, _ = body.shape
    aa = lambda v: rot.matrix_to_axis_angle(rot.rotation_6d_to_matrix(v.reshape(T, B, -1, 6))).reshape(T, B, -1)
    hands = hand_pose.to(sample.dtype)
    if pred:
        hands = hands[list(range(past_len)) + [past_len - 1] * (T - past_len)]
    return torch.cat([aa(body[..., :-3]), hands, body[..., -3:]], dim=2), torch.cat([aa(obj[..., :-3]), obj[..., -3:]], dim=2)


def sample_terms(samples, gt, hand_pose, past_len, variant):
    """samples [K,B,1,144,T] -> ({key: scalar} with the 16 (+16 ``_min`` for 'test') terms, per_clip [K,16,B])."""
    P, K = past_len, samples.shape[0]
    assert variant in ('val', 'test') and (variant == 'test' or K == 1)
    bg, og = to_axis_angle(gt, hand_pose, P, False)
    T, B, _ = bg.shape
    mat = lambda v: rotvec_to_rotmat(v).reshape(T, B, -1)
    G = [mat(bg[..., :-3]), bg[..., -3:], mat(og[..., :-3]), og[..., -3:]]
    f0 = P + 1 if variant == 'test' else P
    per = torch.zeros(K, 16, B, dtype=samples.dtype, device=samples.device)
    for k in range(K):
        bp, op = to_axis_angle(samples[k], hand_pose, P, True)
        X = [mat(bp[..., :-3]), bp[..., -3:], mat(op[..., :-3]), op[..., -3:]]
        for gi, (x, g) in enumerate(zip(X, G)):
            per[k, gi] = ((x[:P] - g[:P]) ** 2).mean(dim=[0, 2])
            per[k, 4 + gi] = (((x[1:P + 1] - x[:P]) - (g[1:P + 1] - g[:P])) ** 2).mean(dim=[0, 2])
            per[k, 8 + gi] = ((x[P:] - g[P:]) ** 2).mean(dim=[0, 2])
            per[k, 12 + gi] = (((x[f0:] - x[f0 - 1:-1]) - (g[f0:] - g[f0 - 1:-1])) ** 2).mean(dim=[0, 2])
    terms = {key: per[:, i].mean() for i, key in enumerate(LOSS_KEYS)}
    if variant == 'test':
        terms.update({key + '_min': per[:, i].min(dim=0)[0].mean() for i, key in enumerate(LOSS_KEYS)})
    return terms, per
