"""CPU oracle of the PointNet++ fine-tuner (``interdiff_amd.pointnet2_train``, csrc/pointnet2_train.hip): ``PointNet2Encoder.forward`` (model/layers.py:141-175) with ONE
key point as ``MDM._get_embeddings`` calls it (model/diffusion_smpl.py:210-211), BatchNorm in eval mode, restated in the RAW form (1x1 conv without bias -> BatchNorm
with running statistics -> ReLU) on torch autograd in any float dtype (fp64 for the error budget).

The sampling / grouping indices are INPUTS (``indices``: oracle/pointnet2.py's restatement, computed once in fp32), so a ball membership cannot differ between an fp32
run and the fp64 one.  Only the live path is evaluated: the 48 SA1 centres the key point groups ("slots": 16 of the r = 0.1 ball, then 32 of the r = 0.2 ball; a centre
held by several slots is evaluated once per slot and autograd adds the slots' gradients).  ``forward`` exposes every pre-activation and pooled activation of that path
(``taps``), which is what the golden recorder measures its discontinuity margins on.
"""
import torch
from oracle import pointnet2 as opn
from interdiff_amd.pointnet2_train import POINTNET_PARAM_NAMES, POINTNET_STAT_NAMES, PREFIX

NS = (16, 32)
GROUPS = tuple('%s.SA_modules.%d.mlps.%d' % (PREFIX, si, sc) for si in range(2) for sc in range(2))


def indices(points):
    """points [B,P,3] fp32 -> dict of int64 tensors: pos [B,48] FPS position of each slot's centre, pid [B,48] its point id, nb0 [B,48,16] / nb1 [B,48,32] the point ids
    each centre groups, hits2 [B,2] / hits1 [B,48,2] the number of points inside each ball (not clipped to nsample)."""
    xyz = points.float().contiguous()
    B = xyz.shape[0]
    fidx = opn.furthest_point_sample(xyz, opn.SA1['npoint'])
    new_xyz = torch.gather(xyz, 1, fidx[:, :, None].expand(B, fidx.shape[1], 3))
    key = new_xyz[:, :1]
    pos = torch.cat([opn.ball_query(r, ns, new_xyz, key)[:, 0] for r, ns in zip(opn.SA2['radii'], opn.SA2['nsamples'])], dim=1)
    pid = torch.gather(fidx, 1, pos)
    centres = xyz[torch.arange(B)[:, None], pid]
    nb = [opn.ball_query(r, ns, xyz, centres) for r, ns in zip(opn.SA1['radii'], opn.SA1['nsamples'])]
    inside = lambda src, q, r: (opn._d2(src[:, None], q[:, :, None]) < r * r).sum(dim=2)
    hits2 = torch.stack([inside(new_xyz, key, r)[:, 0] for r in opn.SA2['radii']], dim=1)
    hits1 = torch.stack([inside(xyz, centres, r) for r in opn.SA1['radii']], dim=2)
    return dict(pos=pos, pid=pid, nb0=nb[0], nb1=nb[1], hits2=hits2, hits1=hits1)


def _mlp(x, p, q, taps, reverse, eps=1e-5):
    """x [..., ns, cin] -> post-ReLU [..., ns, cout] of the three conv + BatchNorm + ReLU layers of group ``q``; taps gets (z, a) per layer."""
    for l in range(3):
        W = p['%s.%d.weight' % (q, 3 * l)][:, :, 0, 0]
        bn = '%s.%d' % (q, 3 * l + 1)
        z = (x.flip(-1) @ W.flip(1).T) if reverse else x @ W.T
        z = (z - p[bn + '.running_mean']) / torch.sqrt(p[bn + '.running_var'] + eps) * p[bn + '.weight'] + p[bn + '.bias']
        x = torch.relu(z)
        if taps is not None:
            x.retain_grad()
            taps.append(('%s.%d' % (q, l), z, x))
    return x


def forward(p, points, idx, taps=None, reverse=False):
    """p: ``pcEmbedding.*`` in the working dtype (leaves for a gradient); points [B,P,3] in the same dtype -> pc [B,256].  ``taps``: a list that receives
    (name, pre-activation z, post-ReLU a) of the twelve layers -- SA1 [B,48,ns,C], SA2 [B,ns,C].  ``reverse``: every contraction sums its channels in reversed order."""
    B = points.shape[0]
    bi = torch.arange(B)[:, None, None]
    nrm = torch.sqrt((points * points).sum(dim=2, keepdim=True))
    centres = points[torch.arange(B)[:, None], idx['pid']]                       # [B,48,3]
    f1 = []
    for sc in range(2):
        nb = idx['nb%d' % sc]
        g = torch.cat([points[bi, nb] - centres[:, :, None], nrm[bi, nb]], dim=3)  # [B,48,ns,4]
        f1.append(_mlp(g, p, GROUPS[sc], taps, reverse).max(dim=2)[0])
    f1 = torch.cat(f1, dim=2)                                                    # [B,48,96]
    key = points[:, :1]                                                          # FPS starts at point 0
    f2 = []
    for sc, (lo, hi) in enumerate(((0, 16), (16, 48))):
        g = torch.cat([centres[:, lo:hi] - key, f1[:, lo:hi]], dim=2)            # [B,ns,99]
        f2.append(_mlp(g, p, GROUPS[2 + sc], taps, reverse).max(dim=1)[0])
    f2 = torch.cat(f2, dim=1)                                                    # [B,256]
    W, b = p[PREFIX + '.Linear.weight'], p[PREFIX + '.Linear.bias']
    lin = (f2.flip(-1) @ W.flip(1).T if reverse else f2 @ W.T) + b
    return torch.cat([key[:, 0], lin], dim=1)


def cast(sd, dtype):
    return {k: (torch.as_tensor(v).to(dtype) if torch.as_tensor(v).is_floating_point() else torch.as_tensor(v)) for k, v in sd.items() if k.startswith(PREFIX + '.')}


def grads(sd, points, idx, d_pc, dtype=torch.float64, reverse=False, taps=False):
    """Gradient of sum(d_pc * pc) with respect to the 38 raw tensors.  Returns dict(pc, grads {name: tensor}, taps [(name, z, a, da)] if asked)."""
    p = cast(sd, dtype)
    with torch.enable_grad():
        leaves = {k: p[k].clone().requires_grad_(True) for k in POINTNET_PARAM_NAMES}
        p.update(leaves)
        tp = [] if taps else None
        pc = forward(p, points.to(dtype), idx, tp, reverse)
        g = torch.autograd.grad((pc * d_pc.to(dtype)).sum(), list(leaves.values()) + ([a for _, _, a in tp] if taps else []), allow_unused=True)
    n = len(leaves)
    out = dict(pc=pc.detach(), grads={k: (torch.zeros_like(leaves[k]) if v is None else v.detach()) for k, v in zip(POINTNET_PARAM_NAMES, g[:n])})
    if taps:
        out['taps'] = [(name, z.detach(), a.detach(), (torch.zeros_like(a) if da is None else da.detach())) for (name, z, a), da in zip(tp, g[n:])]
    return out


def sources(idx):
    """Per layer group the source point id of every pool candidate: SA1 [B,48,ns], SA2 [B,ns]."""
    return [idx['nb0'], idx['nb1'], idx['pid'][:, :16], idx['pid'][:, 16:]]


def margins(taps, idx):
    """The discontinuity margins of a run: (min |z| over the live pre-activations -- those whose ReLU output carries a non-zero gradient --, min pool gap between a
    positive winner that carries gradient and the best candidate FROM A DIFFERENT SOURCE POINT).  Ties between copies of one point are exact and harmless."""
    zmin, gap = float('inf'), float('inf')
    src = sources(idx)
    for i, (name, z, a, da) in enumerate(taps):
        live = da != 0
        if live.any():
            zmin = min(zmin, float(z[live].abs().min()))
        if i % 3 != 2:
            continue
        dim = a.dim() - 2                                                        # the sample axis
        s = src[i // 3].unsqueeze(-1).expand_as(a)
        win, arg = a.max(dim=dim, keepdim=True)
        other = torch.where(s != torch.gather(s, dim, arg), a, torch.full_like(a, -float('inf'))).max(dim=dim, keepdim=True)[0]
        used = (win > 0) & (da.abs().sum(dim=dim, keepdim=True) != 0)
        if used.any():
            gap = min(gap, float((win - other)[used].min()))
    return zmin, gap


def same_decisions(taps, ref, idx):
    """Whether a run decides what ``ref`` (the fp64 run) decides, where a decision reaches the gradient: the ReLU sign of every live pre-activation and, for every pool
    that carries gradient, a winner from the SOURCE POINT of ref's winner (copies of one point tie up to the rounding of a blocked matrix product, and either
    copy scatters to the same address)."""
    src = sources(idx)
    for i, ((_, z, a, _), (_, zr, ar, dar)) in enumerate(zip(taps, ref)):
        live = dar != 0
        if not torch.equal((z > 0)[live], (zr > 0)[live]):
            return False
        if i % 3 == 2:
            dim = a.dim() - 2
            s = src[i // 3].unsqueeze(-1).expand_as(a)
            used = (dar.abs().sum(dim=dim, keepdim=True) != 0) & (ar.max(dim=dim, keepdim=True)[0] > 0)
            same = torch.gather(s, dim, a.max(dim=dim, keepdim=True)[1]) == torch.gather(s, dim, ar.max(dim=dim, keepdim=True)[1])
            if not bool(same[used].all()):
                return False
    return True


def encode(sd, points, idx, dtype=torch.float64):
    """pc [B,256] of the raw state_dict ``sd`` in ``dtype``."""
    return forward(cast(sd, dtype), points.to(dtype), idx)


def trajectory(sd, betas, x0, points, idx, ts, noises, past_len, lr, dtype=torch.float64):
    """AdamW on all 266 tensors of the whole model with ``pc_embedding`` computed from the points: per step tests/mdm_encoder_train_oracle.py's gradient for the 228
    tensors and d_pc, this module's for the 38.  Returns (losses, {name: final tensor})."""
    from tests import losses_oracle as lo
    from tests import mdm_train_oracle as mo
    from tests import mdm_encoder_train_oracle as meo
    names = meo.FULL_PARAM_NAMES + POINTNET_PARAM_NAMES
    cur = {k: v.clone() for k, v in mo.cast(sd, dtype).items()}
    m, v = ({k: torch.zeros_like(cur[k]) for k in names} for _ in range(2))
    losses = []
    for k, (t, eps) in enumerate(zip(ts, noises)):
        r = meo.grads(cur, lo.q_sample(betas, x0.to(dtype), t, eps.to(dtype)), t, encode(cur, points, idx, dtype), x0, past_len, dtype=dtype)
        g = dict(r['grads'], **grads(cur, points, idx, r['d_pc'], dtype)['grads'])
        losses.append(float(r['loss']))
        for name in names:
            mo.adamw_step(cur[name], g[name], m[name], v[name], k + 1, lr=lr)
    return losses, {k: cur[k] for k in names}


__all__ = ['encode', 'trajectory', 'indices', 'forward', 'grads', 'margins', 'same_decisions', 'sources', 'cast', 'POINTNET_PARAM_NAMES', 'POINTNET_STAT_NAMES', 'GROUPS']
