"""CPU oracle of the PointNet++ batch-statistic trainer (``interdiff_amd.pointnet2_train.PointNetTrainer``, csrc/pointnet2_bn_train.hip): ``PointNet2Encoder.forward``
(model/layers.py:141-175) with ONE key point as ``MDM._get_embeddings`` calls it (model/diffusion_smpl.py:210-211), the module in ``train()``: every one of the twelve
BatchNorm2d sites normalises with the mean and biased variance of its own tensor, autograd runs through those statistics, and the running statistics move
(momentum 0.1, unbiased variance).  Restated on torch autograd in any float dtype (fp64 for the error budget).

Unlike the fine-tuner's oracle (tests/pointnet2_train_oracle.py, imported for what it offers) SA1 is evaluated for ALL 1024 FPS positions -- their rows are what the
statistics run over; padding slots and repeated positions count as often as they occur.  The sampling / grouping tables are INPUTS (``tables``: oracle/pointnet2.py's
restatement, computed once in fp32), so a ball membership cannot differ between an fp32 run and the fp64 one.

The DIRECT path (the slot rows whose gradient arrives through a pool, and those pools' candidates) is what the golden recorder measures its discontinuity margins
on: ``direct`` evaluates it with the fine-tuner oracle's own ``grads`` on a state dict whose running statistics are replaced by the batch statistics, which is the
same function of the live rows.
"""
import torch
from oracle import pointnet2 as opn
from tests import pointnet2_train_oracle as po
from interdiff_amd.pointnet2_train import POINTNET_PARAM_NAMES, POINTNET_STAT_NAMES, PREFIX

GROUPS, NS = po.GROUPS, po.NS
SITES = tuple('%s.%d' % (q, 3 * l + 1) for q in GROUPS for l in range(3))
MOMENTUM, EPS = 0.1, 1e-5


def tables(points):
    """points [B,P,3] fp32 -> the fine-tuner oracle's ``indices`` (the 48 slots) plus fidx [B,1024] (FPS point ids) and nb0 / nb1 of ALL positions
    (``all0`` [B,1024,16], ``all1`` [B,1024,32])."""
    xyz = points.float().contiguous()
    B = xyz.shape[0]
    tb = po.indices(xyz)
    fidx = opn.furthest_point_sample(xyz, opn.SA1['npoint'])
    new_xyz = torch.gather(xyz, 1, fidx[:, :, None].expand(B, fidx.shape[1], 3))
    tb['fidx'] = fidx
    for sc, (r, ns) in enumerate(zip(opn.SA1['radii'], opn.SA1['nsamples'])):
        tb['all%d' % sc] = opn.ball_query(r, ns, xyz, new_xyz)
    return tb


def _mlp(x, p, q, stats, reverse):
    """x [..., cin] -> post-ReLU [..., cout] of the three conv + train-mode BatchNorm + ReLU layers of group ``q``; stats gets (site, mean, biased var, rows)."""
    for l in range(3):
        W = p['%s.%d.weight' % (q, 3 * l)][:, :, 0, 0]
        bn = '%s.%d' % (q, 3 * l + 1)
        z = (x.flip(-1) @ W.flip(1).T) if reverse else x @ W.T
        rows = z.reshape(-1, z.shape[-1])
        mean = rows.mean(dim=0)
        var = ((rows - mean) ** 2).mean(dim=0)
        stats.append((bn, mean, var, rows.shape[0]))
        x = torch.relu((z - mean) / torch.sqrt(var + EPS) * p[bn + '.weight'] + p[bn + '.bias'])
    return x


def forward(p, points, tb, reverse=False):
    """p: ``pcEmbedding.*`` in the working dtype; points [B,P,3] in the same dtype -> (pc [B,256], [(site, batch mean, biased batch variance, rows)] x 12 in
    the order of ``SITES``).  ``reverse``: every contraction sums its channels in reversed order."""
    B = points.shape[0]
    bi = torch.arange(B)[:, None, None]
    nrm = torch.sqrt((points * points).sum(dim=2, keepdim=True))
    centres = points[torch.arange(B)[:, None], tb['fidx']]                       # [B,1024,3]
    stats, f1 = [], []
    for sc in range(2):
        nb = tb['all%d' % sc]
        g = torch.cat([points[bi, nb] - centres[:, :, None], nrm[bi, nb]], dim=3)  # [B,1024,ns,4]
        f1.append(_mlp(g, p, GROUPS[sc], stats, reverse).max(dim=2)[0])
    f1 = torch.cat(f1, dim=2)                                                    # [B,1024,96]
    rows = torch.arange(B)[:, None]
    slot_f, slot_c = f1[rows, tb['pos']], centres[rows, tb['pos']]               # [B,48,96], [B,48,3]
    key = points[:, :1]
    f2 = []
    for sc, (lo, hi) in enumerate(((0, 16), (16, 48))):
        g = torch.cat([slot_c[:, lo:hi] - key, slot_f[:, lo:hi]], dim=2)         # [B,ns,99]
        f2.append(_mlp(g, p, GROUPS[2 + sc], stats, reverse).max(dim=1)[0])
    f2 = torch.cat(f2, dim=1)
    W, b = p[PREFIX + '.Linear.weight'], p[PREFIX + '.Linear.bias']
    lin = (f2.flip(-1) @ W.flip(1).T if reverse else f2 @ W.T) + b
    return torch.cat([key[:, 0], lin], dim=1), stats


def updated_stats(p, stats, momentum=MOMENTUM):
    """{running_mean / running_var name: value after one train-mode forward} in the dtype of ``stats``."""
    out = {}
    for bn, mean, var, n in stats:
        out[bn + '.running_mean'] = (1 - momentum) * p[bn + '.running_mean'].to(mean.dtype) + momentum * mean.detach()
        out[bn + '.running_var'] = (1 - momentum) * p[bn + '.running_var'].to(mean.dtype) + momentum * var.detach() * (n / (n - 1.0))
    return out


def grads(sd, points, tb, d_pc, dtype=torch.float64, reverse=False):
    """Gradient of sum(d_pc * pc) with respect to the 38 raw tensors, through the batch statistics.  Returns dict(pc, grads {name: tensor}, stats {name: updated
    running statistic}, batch {site: (mean, biased var)})."""
    p = po.cast(sd, dtype)
    with torch.enable_grad():
        leaves = {k: p[k].clone().requires_grad_(True) for k in POINTNET_PARAM_NAMES}
        p.update(leaves)
        pc, stats = forward(p, points.to(dtype), tb, reverse)
        g = torch.autograd.grad((pc * d_pc.to(dtype)).sum(), list(leaves.values()), allow_unused=True)
    return dict(pc=pc.detach(), grads={k: (torch.zeros_like(leaves[k]) if v is None else v.detach()) for k, v in zip(POINTNET_PARAM_NAMES, g)},
                stats=updated_stats(p, stats), batch={bn: (m.detach(), v.detach()) for bn, m, v, _ in stats})


def direct(sd, batch, points, tb, d_pc, dtype=torch.float64, reverse=False):
    """The direct path of a run with batch statistics ``batch``: the fine-tuner oracle's ``grads(..., taps=True)`` on ``sd`` with those statistics in the place of the
    running ones -- the same function of the live rows, with the statistics held fixed."""
    fixed = dict(sd)
    for bn, (m, v) in batch.items():
        fixed[bn + '.running_mean'], fixed[bn + '.running_var'] = m, v
    return po.grads(fixed, points, tb, d_pc, dtype=dtype, reverse=reverse, taps=True)


def with_stats(sd, stats, steps=1):
    """``sd`` with the running statistics ``stats`` and every ``num_batches_tracked`` of pcEmbedding advanced by ``steps``."""
    out = dict(sd)
    out.update({k: v.to(torch.as_tensor(sd[k]).dtype) for k, v in stats.items()})
    for bn in SITES:
        out[bn + '.num_batches_tracked'] = torch.as_tensor(sd[bn + '.num_batches_tracked']) + steps
    return out


def stat_error(got, ref):
    """Per site the largest |got - ref| of running_mean and running_var relative to the largest |ref| entry of that tensor: {name: error}."""
    return {k: float((torch.as_tensor(got[k]).double() - ref[k].double()).abs().max() / max(float(ref[k].double().abs().max()), 1e-300)) for k in POINTNET_STAT_NAMES}


def trajectory(sd, betas, x0, points, tb, ts, noises, past_len, lr, dtype=torch.float64):
    """AdamW on all 266 tensors of the whole model with ``pc_embedding`` computed from the points under batch statistics: per step
    tests/mdm_encoder_train_oracle.py's gradient for the 228 tensors and d_pc, this module's for the 38; the running statistics move once per step.
    Returns (losses, {name: final tensor}, {name: final running statistic})."""
    from tests import losses_oracle as lo
    from tests import mdm_train_oracle as mo
    from tests import mdm_encoder_train_oracle as meo
    names = meo.FULL_PARAM_NAMES + POINTNET_PARAM_NAMES
    cur = {k: v.clone() for k, v in mo.cast(sd, dtype).items()}
    m, v = ({k: torch.zeros_like(cur[k]) for k in names} for _ in range(2))
    losses = []
    for k, (t, eps) in enumerate(zip(ts, noises)):
        with torch.no_grad():
            pc = forward(po.cast(cur, dtype), points.to(dtype), tb)[0]
        r = meo.grads(cur, lo.q_sample(betas, x0.to(dtype), t, eps.to(dtype)), t, pc, x0, past_len, dtype=dtype)
        pn = grads(cur, points, tb, r['d_pc'], dtype)
        g = dict(r['grads'], **pn['grads'])
        losses.append(float(r['loss']))
        for name in names:
            mo.adamw_step(cur[name], g[name], m[name], v[name], k + 1, lr=lr)
        cur.update(pn['stats'])
    return losses, {k: cur[k] for k in names}, {k: cur[k] for k in POINTNET_STAT_NAMES}


__all__ = ['trajectory', 'tables', 'forward', 'grads', 'direct', 'updated_stats', 'with_stats', 'stat_error', 'SITES', 'POINTNET_PARAM_NAMES', 'POINTNET_STAT_NAMES']
