"""CPU oracle of the denoiser trainer with the encoder in the graph (``DenoiserTrainer(train_encoder=True)``, csrc/mdm_train.h): torch autograd, any float
dtype (fp64 for the error budget), composed of the restatements that already pin the forward side -- ``oracle.denoiser.enc_std_layer`` / ``enc_qan_layer`` (the
layers of ``get_embeddings``, model/diffusion_smpl.py:217-221) and ``mdm_forward`` (:226-246) -- and of tests/mdm_train_oracle.py (``loss_of``, ``adamw_step``,
``cast``).  ``pc`` (pc_embedding [B,256]) is a leaf; ``cond`` is NOT detached, so bodyEmbedding / objEmbedding receive both paths' gradient.
"""
import torch
from oracle import denoiser as od
from tests import losses_oracle as lo
from tests import mdm_train_oracle as mo
from tests.mdm_train_oracle import token_shares
from interdiff_amd.mdm_train import PARAM_NAMES, ENCODER_PARAM_NAMES, FULL_PARAM_NAMES


def encode(p, x0, pc, past_len, n_body=135):
    """``_get_embeddings`` from pc_embedding on: x0 [B,1,144,T] (its past frames are the encoder's tokens), pc [B,256]  ->  cond [past_len,B,256]."""
    pe = (p['PositionalEmbedding.pe'][:, 0] if 'PositionalEmbedding.pe' in p else od.positional_table()).to(x0.dtype)
    tok = x0.squeeze(1).permute(2, 0, 1)[:past_len]                                   # [S,B,144]
    h = od._lin(tok[..., :n_body], p, 'bodyEmbedding') + od._lin(tok[..., n_body:], p, 'objEmbedding') + pc[None]
    h = h + pe[:past_len, None]
    for l in range(od.N_LAYERS):
        name = 'encoder.layers.%d' % l
        h = od.enc_qan_layer(h, p, name) if l in od.QAN_LAYERS else od.enc_std_layer(h, p, name)
    return h


WK_NAMES = tuple(k for k in FULL_PARAM_NAMES if k.endswith('.wk'))


def grads(sd, x_t, ts, pc, target, past_len=10, weights=None, dtype=torch.float64, d_pred=None, detach_cond=False):
    """Autograd of the weighted loss (or of <pred, d_pred>) with respect to the 228 tensors, ``pc`` and ``cond`` (an interior node).  ``detach_cond``: the
    decoder-only gradient (tests/mdm_train_oracle.py's) on the same ``cond``.  Returns dict(loss, terms, pred, cond, d_pred, d_cond, d_pc, grads, wk_scale);
    wk_scale {name: max_n sum_{b,t,c} |d block[t,b,c] o_n[b,t,c]|} for the twelve ``wk`` tensors (``token_shares``)."""
    p = mo.cast(sd, dtype)
    with torch.enable_grad(), token_shares() as ts_:
        leaves = {k: p[k].clone().requires_grad_(True) for k in FULL_PARAM_NAMES}
        p.update(leaves)
        pcl = pc.to(dtype).clone().requires_grad_(True)
        cond = encode(p, target.to(dtype), pcl, past_len)
        c = cond.detach().requires_grad_(True) if detach_cond else cond
        pred = od.mdm_forward(p, x_t.to(dtype), ts, c)
        loss, terms = mo.loss_of(pred, target.to(dtype), past_len, weights)
        dp = torch.autograd.grad(loss, pred, retain_graph=True)[0]
        head = dp if d_pred is None else d_pred.to(dtype)
        zs = [ts_.z[k] for k in WK_NAMES]
        g = torch.autograd.grad(pred, list(leaves.values()) + [pcl, c] + zs, grad_outputs=head, allow_unused=True)
        g, gz = g[:-len(zs)], g[-len(zs):]
    zero = lambda v, like: torch.zeros_like(like) if v is None else v.detach()
    return dict(loss=loss.detach(), terms=terms.detach(), pred=pred.detach(), cond=cond.detach(), d_pred=dp.detach(), d_cond=g[-1].detach(), d_pc=zero(g[-2], pcl),
                grads={k: zero(v, leaves[k]) for k, v in zip(FULL_PARAM_NAMES, g[:-2])},
                wk_scale={k: (float(v.abs().sum(dim=(0, 2, 3)).max()) if v is not None else 0.0) for k, v in zip(WK_NAMES, gz)})


def grad_scale(ref, k):
    """The scale a gradient tensor's error is measured on: max|g64|, and for the ``wk`` tensors the sum of the magnitudes of the products d wk[n] adds up (``wk_scale``)."""
    return ref['wk_scale'][k] if k in WK_NAMES else float(ref['grads'][k].abs().max())


def grad_gate_abs(ref, k, e_ref, floor=1e-5):
    """The project's gate as an absolute distance: max(4 e_ref, floor) of the tensor's scale.  For ``wk`` the floor stays on max|g64| (on the sum-of-magnitudes scale, 1e4
    to 1e5 times larger, it would admit a gradient wrong by half its size), so its gate is max(4 e_ref wk_scale, floor max|g64|)."""
    top = float(ref['grads'][k].abs().max())
    return max(4.0 * float(e_ref) * grad_scale(ref, k), floor * top)


def trajectory(sd, betas, x0, pc, ts, noises, past_len=10, weights=None, dtype=torch.float64, **opt):
    """``len(ts)`` AdamW steps on the 228 tensors: step k draws x_t = q_sample(x0, ts[k], noises[k]).  Returns (losses, final {name: tensor})."""
    cur = {k: v.clone() for k, v in mo.cast(sd, dtype).items()}
    m = {k: torch.zeros_like(cur[k]) for k in FULL_PARAM_NAMES}
    v = {k: torch.zeros_like(cur[k]) for k in FULL_PARAM_NAMES}
    losses = []
    for k, (t, eps) in enumerate(zip(ts, noises)):
        x_t = lo.q_sample(betas, x0.to(dtype), t, eps.to(dtype))
        r = grads(cur, x_t, t, pc, x0, past_len, weights, dtype)
        losses.append(float(r['loss']))
        for name in FULL_PARAM_NAMES:
            mo.adamw_step(cur[name], r['grads'][name], m[name], v[name], k + 1, **opt)
    return losses, {k: cur[k] for k in FULL_PARAM_NAMES}


__all__ = ['encode', 'grads', 'trajectory', 'token_shares', 'grad_scale', 'grad_gate_abs', 'WK_NAMES', 'PARAM_NAMES', 'ENCODER_PARAM_NAMES', 'FULL_PARAM_NAMES']
