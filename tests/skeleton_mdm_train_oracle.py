"""CPU oracle of the skeleton denoiser's trainer (interdiff_amd/skeleton_mdm_train.py, csrc/skeleton_mdm_train.hip): torch autograd, any float dtype (fp64 for
the error budget), through the restatements that already pin the forward side -- ``skeleton_mdm_oracle.get_embeddings`` / ``forward``
(model/diffusion_skeleton.py:194-215, :231-257) with the conditioning IN the graph -- plus the 13-term loss of ``forward_backward``
(train_diffusion_skeleton.py:108-168) in torch, a closed-form gradient of that loss with respect to the model output, a closed-form backward of the keypoint head
(``calc_obj_pred`` :218-229 behind ``objFinalLinear``), which the tests check against autograd, and AdamW (``mdm_train_oracle.adamw_step``).

The loss is the reference's scalar: every term an ``MSELoss(reduction='mean')`` over the batch, weighted and summed, times the schedule sampler's weights, which
are all one -- with clips of equal length that is mean_b sum_i w_i term_i[b] of the per-clip terms.
"""
import torch
from tests import losses_oracle as lo
from tests import mdm_train_oracle as mo
from tests import mdm_encoder_train_oracle as meo
from tests import skeleton_losses_oracle as slo
from tests import skeleton_mdm_oracle as smo
from interdiff_amd.skeleton_mdm_train import PARAM_NAMES

N_BODY, N_OBJ, N_POSE = 63, 36, 7
WK_NAMES = tuple(k for k in PARAM_NAMES if k.endswith('.wk'))
assert WK_NAMES == meo.WK_NAMES
KEYS = slo.KEYS
cast, with_pe_rows, adamw_step = mo.cast, mo.with_pe_rows, mo.adamw_step


def tokens(body, obj, pose):
    """The dataset layout (body [B,T,21,3], obj [B,T,12,3], pose [B,T,7]) -> gt [B,1,106,T] (``_get_embeddings`` :206 as ``_common_step`` permutes it)."""
    B, T = body.shape[:2]
    return torch.cat([body.reshape(B, T, -1), obj.reshape(B, T, -1), pose], dim=2).permute(0, 2, 1).unsqueeze(1).contiguous()


def split(x):
    """[B,1,106,T] -> body, obj, pose as [T,B,*] (:101-104)."""
    return torch.split(x[:, 0].permute(2, 0, 1), [N_BODY, N_OBJ, N_POSE], dim=2)


def per_clip_terms(pred, target, past_len):
    """The 13 unweighted terms of every clip: [13,B], KEYS order (skeleton_losses_oracle.per_clip_terms in torch, differentiable)."""
    (bp, op, pp), (bg, og, pg) = split(pred), split(target)
    P = past_len
    mse = lambda a, b: ((a - b) ** 2).mean(dim=(0, 2))
    vel = lambda a: a[1:] - a[:-1]
    qq = (pp[..., -4:] ** 2).sum(-1)
    d = {'body_past': mse(bp[:P], bg[:P]), 'body_future': mse(bp[P:], bg[P:]), 'obj_past': mse(op[:P], og[:P]), 'obj_future': mse(op[P:], og[P:]),
         'loss_obj_nonrot_past': mse(pp[:P, :, :3], pg[:P, :, :3]), 'loss_obj_nonrot_future': mse(pp[P:, :, :3], pg[P:, :, :3]),
         'loss_obj_rot_past': mse(pp[:P, :, -4:], pg[:P, :, -4:]), 'loss_obj_rot_future': mse(pp[P:, :, -4:], pg[P:, :, -4:]),
         'quaternion_reg_loss': ((qq - 1.0) ** 2).mean(dim=0),
         'loss_obj_rot_v': mse(vel(pp[..., -4:]), vel(pg[..., -4:])), 'loss_obj_nonrot_v': mse(vel(pp[..., :3]), vel(pg[..., :3])),
         'loss_body_v': mse(vel(bp), vel(bg)), 'loss_obj_v': mse(vel(op), vel(og))}
    return torch.stack([d[k] for k in KEYS])


def weight_vector(weights=None, dtype=torch.float64):
    return torch.tensor(slo.weight_vector(weights), dtype=dtype)


def loss_of(pred, target, past_len, weights=None):
    """(mean_b sum_i w_i term_i[b], terms [13,B])."""
    terms = per_clip_terms(pred, target, past_len)
    return (terms * weight_vector(weights, pred.dtype)[:, None]).sum(0).mean(), terms


def encode(p, target, zero_pose_obj, past_len):
    """``_get_embeddings`` on the tokens of x_start [B,1,106,T] -> cond [past_len,B,256]."""
    body, obj, pose = split(target)
    return smo.get_embeddings(p, body, obj, pose, zero_pose_obj, past_len)[0]


def grads(sd, x_t, ts, zero_pose_obj, target, past_len=10, weights=None, dtype=torch.float64, d_pred=None):
    """Autograd of the weighted loss (or of <pred, d_pred>) with respect to the 230 tensors; ``cond`` is an interior node, ``zero_pose_obj`` data.
    Returns dict(loss, terms [13,B], pred, cond, d_pred, grads, wk_scale); wk_scale as tests/mdm_encoder_train_oracle.py ``token_shares`` reads it."""
    p = cast(sd, dtype)
    z = zero_pose_obj.to(dtype)
    with torch.enable_grad(), meo.token_shares() as sh:
        leaves = {k: p[k].clone().requires_grad_(True) for k in PARAM_NAMES}
        p.update(leaves)
        cond = encode(p, target.to(dtype), z, past_len)
        pred = smo.forward(p, x_t.to(dtype), ts, z, cond)
        loss, terms = loss_of(pred, target.to(dtype), past_len, weights)
        dp = torch.autograd.grad(loss, pred, retain_graph=True)[0]
        head = dp if d_pred is None else d_pred.to(dtype)
        zs = [sh.z[k] for k in WK_NAMES]
        g = torch.autograd.grad(pred, list(leaves.values()) + zs, grad_outputs=head, allow_unused=True)
        g, gz = g[:-len(zs)], g[-len(zs):]
    zero = lambda v, like: torch.zeros_like(like) if v is None else v.detach()
    return dict(loss=loss.detach(), terms=terms.detach(), pred=pred.detach(), cond=cond.detach(), d_pred=dp.detach(),
                grads={k: zero(v, leaves[k]) for k, v in zip(PARAM_NAMES, g)},
                wk_scale={k: (float(v.abs().sum(dim=(0, 2, 3)).max()) if v is not None else 0.0) for k, v in zip(WK_NAMES, gz)})


# the scale a gradient tensor's error is measured on (the twelve ``wk`` tensors: the sum of magnitudes) and the project's gate as an absolute distance: the SMPL
# encoder trainer's, whose twelve ``wk`` names are this model's
grad_scale, grad_gate_abs = meo.grad_scale, meo.grad_gate_abs


def d_pred_closed_form(pred, target, past_len, weights=None):
    """d/d pred of mean_b sum_i w_i term_i[b], written out: per group (body 63, obj 36, translation 3, quaternion 4) an MSE on the past / future values and an
    MSE of v_t = (x_t - x_{t-1}) - (g_t - g_{t-1}) over all T - 1 differences; on the quaternion channels also mean_t (q.q - 1)^2."""
    B, _, _, T = pred.shape
    P = past_len
    w = [float(v) for v in slo.weight_vector(weights)]
    x, g = pred[:, 0], target[:, 0]
    out = torch.zeros_like(x)
    frames = torch.arange(T)
    on = lambda mask: mask.to(x.dtype)
    groups = ((0, 63, 11), (63, 99, 12), (99, 102, 10), (102, 106, 9))
    for gi, (c0, c1, iv) in enumerate(groups):
        F = float(c1 - c0)
        a_val = on(frames < P) * (w[2 * gi] / (P * F)) + on(frames >= P) * (w[2 * gi + 1] / ((T - P) * F))
        d = out[:, c0:c1]
        d += 2 * a_val * (x[:, c0:c1] - g[:, c0:c1])
        v = (x[:, c0:c1, 1:] - x[:, c0:c1, :-1]) - (g[:, c0:c1, 1:] - g[:, c0:c1, :-1])
        a_v = w[iv] / ((T - 1) * F)
        d[..., 1:] += 2 * a_v * v
        d[..., :-1] -= 2 * a_v * v
    q = x[:, 102:106]
    out[:, 102:106] += (4 * w[8] / T) * ((q * q).sum(1, keepdim=True) - 1.0) * q
    return (out / B)[:, None]


def head(rows, zero_pose_obj):
    """The keypoint head on rows [T,B,70] = bodyFinalLinear | objFinalLinear -> pred [B,1,106,T] (:244-257)."""
    T, B, _ = rows.shape
    body, pose = rows[..., :N_BODY], rows[..., N_BODY:]
    obj = smo.calc_obj_pred(pose, zero_pose_obj).reshape(T, B, -1)
    return torch.cat([body, obj, pose], dim=2).permute(1, 2, 0).unsqueeze(1)


def head_backward_closed_form(d_pred, rows, zero_pose_obj):
    """d rows [T,B,70] of <head(rows), d_pred>: d body passes through, d pose = d_pred[pose] + J^T d_pred[obj].  The translation takes the sum over the 12
    points; with R = I + two_s N(q), two_s = 2 / (q . q) (pytorch3d's quaternion_to_matrix does not normalise), dR[a][c] = sum_p d obj[p][a] z[p][c]:
    d q_m = two_s <dR, dN/dq_m> - two_s^2 q_m <dR, N>."""
    T, B, _ = rows.shape
    g = d_pred[:, 0].permute(2, 0, 1)                                             # [T,B,106]
    gb, go, gp = g[..., :N_BODY], g[..., N_BODY:N_BODY + N_OBJ].reshape(T, B, -1, 3), g[..., N_BODY + N_OBJ:]
    pose = rows[..., N_BODY:]
    i, j, k, r = pose[..., 3], pose[..., 4], pose[..., 5], pose[..., 6]
    s2 = 2.0 / (i * i + j * j + k * k + r * r)
    dR = torch.einsum('tbpa,bpc->tbac', go, zero_pose_obj)
    o = torch.zeros_like(i)
    st = lambda rows_: torch.stack([torch.stack(r_, dim=-1) for r_ in rows_], dim=-2)
    N = st([[-(j * j + k * k), i * j - k * r, i * k + j * r], [i * j + k * r, -(i * i + k * k), j * k - i * r], [i * k - j * r, j * k + i * r, -(i * i + j * j)]])
    dN = {'r': st([[o, -k, j], [k, o, -i], [-j, i, o]]), 'i': st([[o, j, k], [j, -2 * i, -r], [k, r, -2 * i]]),
          'j': st([[-2 * j, i, r], [i, o, k], [-r, k, -2 * j]]), 'k': st([[-2 * k, -r, i], [r, -2 * k, j], [i, j, o]])}
    dn = (dR * N).sum(dim=(-1, -2))
    dq = {m: s2 * (dR * dN[m]).sum(dim=(-1, -2)) - s2 * s2 * qm * dn for m, qm in (('r', r), ('i', i), ('j', j), ('k', k))}
    d_pose = gp + torch.cat([go.sum(dim=2), torch.stack([dq['i'], dq['j'], dq['k'], dq['r']], dim=-1)], dim=-1)
    return torch.cat([gb, d_pose], dim=-1)


def trajectory(sd, betas, x0, zero_pose_obj, ts, noises, past_len=10, weights=None, dtype=torch.float64, **opt):
    """``len(ts)`` AdamW steps on the 230 tensors: step k draws x_t = q_sample(x0, ts[k], noises[k]).  Returns (losses, final {name: tensor})."""
    cur = {k: v.clone() for k, v in cast(sd, dtype).items()}
    m = {k: torch.zeros_like(cur[k]) for k in PARAM_NAMES}
    v = {k: torch.zeros_like(cur[k]) for k in PARAM_NAMES}
    losses = []
    for k, (t, eps) in enumerate(zip(ts, noises)):
        x_t = lo.q_sample(betas, x0.to(dtype), t, eps.to(dtype))
        r = grads(cur, x_t, t, zero_pose_obj, x0, past_len, weights, dtype)
        losses.append(float(r['loss']))
        for name in PARAM_NAMES:
            adamw_step(cur[name], r['grads'][name], m[name], v[name], k + 1, **opt)
    return losses, {k: cur[k] for k in PARAM_NAMES}
