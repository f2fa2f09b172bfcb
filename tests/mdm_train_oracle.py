"""CPU oracle of the denoiser trainer (interdiff_amd/mdm_train.py, csrc/mdm_train.h): torch autograd, any float dtype (fp64 for the error budget),
through the restatements that already pin the forward side -- ``oracle.denoiser.mdm_forward`` (model/diffusion_smpl.py:226-246) and
``losses_oracle.denoising_terms`` / ``weight_vector`` (train_diffusion_smpl.py:72-153) -- plus AdamW as torch.optim.AdamW writes it and a closed-form
gradient of the weighted loss with respect to the model output, which the tests check against autograd.

The loss is the reference's: ``loss = sum_i w_i term_i`` per clip, ``(loss * weights).mean()`` with the schedule sampler's weights all one, so
mean_b sum_i w_i term_i[b].  ``cond`` is a leaf (the reference's autograd with ``y['cond']`` detached); its gradient is returned.
"""
import numpy as np
import torch
from oracle import denoiser as od
from tests import losses_oracle as lo
from interdiff_amd.mdm_train import PARAM_NAMES

GROUPS = ((0, 132), (132, 135), (135, 141), (141, 144))


def cast(sd, dtype):
    return {k: (torch.as_tensor(v).to(dtype) if torch.as_tensor(v).is_floating_point() else torch.as_tensor(v)) for k, v in sd.items()}


def with_pe_rows(sd, *recorded):
    """A copy of ``sd`` whose 'PositionalEmbedding.pe' [5000,1,256] is the sinusoidal table with the recorded rows (pairs of index array, values) written over it.
    sin / cos / exp of fp32 arguments differ in the last bits between CPUs, and the gradient of time_embed.0.weight is linear in pe[t]: the oracle, the trainer and
    the sampler model of a test all read the rows the reference run read."""
    pe = od.positional_table()
    for idx, val in recorded:
        pe[torch.as_tensor(np.asarray(idx))] = torch.as_tensor(np.asarray(val))
    return dict(sd, **{'PositionalEmbedding.pe': pe[:, None].contiguous()})


def loss_of(pred, target, past_len, weights=None):
    """(mean_b sum_i w_i term_i[b], terms [16,B])."""
    terms = lo.denoising_terms(pred, target, past_len)
    stack = torch.stack([terms[k] for k in lo.LOSS_KEYS])
    w = torch.tensor(lo.weight_vector(weights), dtype=pred.dtype)
    return (stack * w[:, None]).sum(0).mean(), stack


WK_NAMES = tuple(k for k in PARAM_NAMES if k.endswith('.wk'))


class token_shares:
    """While active, ``oracle.denoiser.qan_block`` computes what it computes with ``wk[n] + z[b,n,t,c]`` in the place of ``wk[n]``, z a zero leaf per layer: the gradient
    of z is the share of token (b, t) and channel c in d wk[n] = sum_{b,t,c} d block[t,b,c] o_n[b,t,c], so the sum of the products' magnitudes -- the scale on which that
    near-cancelling sum is well conditioned (the post-norm LayerNorm behind the block makes d block orthogonal to the row it normalises, so already one token's
    256 products cancel) -- can be read off autograd.  ``self.z``: {'<layer prefix>.wk': leaf}."""

    def __enter__(self):
        self.z, self.real = {}, od.qan_block

        def qan_block(x, sd, p, rotary=od.ROTARY_DEFAULT):
            T, B, D = x.shape
            q = od.qan_queries(sd, p)
            nq = q.shape[0]
            qq = q[None, :, None, :].expand(B, nq, T, D).reshape(B * nq, T, D)
            xx = x.permute(1, 0, 2)[:, None].expand(B, nq, T, D).reshape(B * nq, T, D)
            o = od.local_attention(qq, xx, xx, rotary=rotary).reshape(B, nq, T, D)
            z = torch.zeros(B, nq, T, D, dtype=x.dtype, requires_grad=True)
            self.z[p + '.wk'] = z
            return (o * (sd[p + '.wk'][None, :, None, :] + z)).sum(1).permute(1, 0, 2)
        od.qan_block = qan_block
        return self

    def __exit__(self, *exc):
        od.qan_block = self.real


def grads(sd, x_t, ts, cond, target, past_len=10, weights=None, dtype=torch.float64, d_pred=None):
    """Autograd of the weighted loss (or of <pred, d_pred> when ``d_pred`` is given) with respect to the 144 tensors and ``cond``.
    Returns dict(loss, terms [16,B], pred, d_pred, d_cond, grads {name: tensor}, wk_scale), everything in ``dtype``; wk_scale
    {name: max_n sum_{b,t,c} |d block[t,b,c] o_n[b,t,c]|} for the six decoder ``wk`` tensors (``token_shares``)."""
    p = cast(sd, dtype)
    with torch.enable_grad(), token_shares() as ts_:               # (other test modules switch autograd off process-wide)
        leaves = {k: p[k].clone().requires_grad_(True) for k in PARAM_NAMES}
        p.update(leaves)
        c = cond.to(dtype).clone().requires_grad_(True)
        pred = od.mdm_forward(p, x_t.to(dtype), ts, c)
        loss, terms = loss_of(pred, target.to(dtype), past_len, weights)
        dp = torch.autograd.grad(loss, pred, retain_graph=True)[0]
        head = dp if d_pred is None else d_pred.to(dtype)
        zs = [ts_.z[k] for k in WK_NAMES]
        g = torch.autograd.grad(pred, list(leaves.values()) + [c] + zs, grad_outputs=head, allow_unused=True)
        g, gz = g[:-len(zs)], g[-len(zs):]
    assert all(v is not None for v in g)
    return dict(loss=loss.detach(), terms=terms.detach(), pred=pred.detach(), d_pred=dp.detach(), d_cond=g[-1].detach(),
                grads={k: v.detach() for k, v in zip(PARAM_NAMES, g[:-1])},
                wk_scale={k: (float(v.abs().sum(dim=(0, 2, 3)).max()) if v is not None else 0.0) for k, v in zip(WK_NAMES, gz)})


def d_pred_closed_form(pred, target, past_len, weights=None):
    """d/d pred of mean_b sum_i w_i term_i[b], written out: per group an MSE on the values, and per velocity term an MSE of first differences
    (frames 1..P | P..T-1) plus an MSE of e_u = 2 x_u - x_{u-1} - x_{u+1} (u = 1..P-1 | P..T-2); the ground-truth velocity operand is zero."""
    B, _, _, T = pred.shape
    P = past_len
    w = lo.weight_vector(weights)
    x, g = pred[:, 0], target[:, 0]
    out = torch.zeros_like(x)
    frames = torch.arange(T)
    for gi, (c0, c1) in enumerate(GROUPS):
        F = float(c1 - c0)
        xs, d = x[:, c0:c1], out[:, c0:c1]
        on = lambda mask: mask.to(x.dtype)                         # (a mask times a Python float would be fp32)
        a_val = on(frames < P) * (w[gi] / (P * F)) + on(frames >= P) * (w[8 + gi] / ((T - P) * F))
        d += 2 * a_val * (xs - g[:, c0:c1])
        tt = frames[1:]                                            # a first difference v_t = x_t - x_{t-1}, t = 1 .. T-1
        a1 = on(tt <= P) * (w[4 + gi] / (P * F)) + on(tt >= P) * (w[12 + gi] / ((T - P) * F))
        v = xs[..., 1:] - xs[..., :-1]
        d[..., 1:] += 2 * a1 * v
        d[..., :-1] -= 2 * a1 * v
        uu = frames[1:-1]                                          # e_u, u = 1 .. T-2
        a2 = on((uu >= 1) & (uu <= P - 1)) * (w[4 + gi] / ((P - 1) * F)) + on((uu >= P) & (uu <= T - 2)) * (w[12 + gi] / ((T - P - 1) * F))
        e = 2 * xs[..., 1:-1] - xs[..., :-2] - xs[..., 2:]
        d[..., 1:-1] += 4 * a2 * e
        d[..., :-2] -= 2 * a2 * e
        d[..., 2:] -= 2 * a2 * e
    return (out / B)[:, None]


def adamw_step(p, g, m, v, step, lr=3e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
    """torch.optim.AdamW (_single_tensor_adamw), in place on tensors of any float dtype."""
    p.mul_(1 - lr * weight_decay)
    m.lerp_(g, 1 - betas[0])
    v.mul_(betas[1]).addcmul_(g, g, value=1 - betas[1])
    bc1, bc2 = 1 - betas[0] ** step, 1 - betas[1] ** step
    p.addcdiv_(m, (v.sqrt() / np.sqrt(bc2)).add_(eps), value=-lr / bc1)


def trajectory(sd, betas, x0, cond, ts, noises, past_len=10, weights=None, dtype=torch.float64, **opt):
    """``len(ts)`` AdamW steps on the 144 tensors: step k draws x_t = q_sample(x0, ts[k], noises[k]).  Returns (losses, final {name: tensor})."""
    cur = {k: v.clone() for k, v in cast(sd, dtype).items()}        # (updated in place below: never the caller's tensors)
    m = {k: torch.zeros_like(cur[k]) for k in PARAM_NAMES}
    v = {k: torch.zeros_like(cur[k]) for k in PARAM_NAMES}
    losses = []
    for k, (t, eps) in enumerate(zip(ts, noises)):
        x_t = lo.q_sample(betas, x0.to(dtype), t, eps.to(dtype))
        r = grads(cur, x_t, t, cond, x0, past_len, weights, dtype)
        losses.append(float(r['loss']))
        for name in PARAM_NAMES:
            adamw_step(cur[name], r['grads'][name], m[name], v[name], k + 1, **opt)
    return losses, {k: cur[k] for k in PARAM_NAMES}
