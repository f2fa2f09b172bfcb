"""fp64 torch restatement, with autograd, of what interdiff_amd.correction_finetune computes: the loss of ``LitInteraction.calc_loss``
(train_correction_smpl.py:60-101) on ``ObjProjector.forward(data, initialize)`` (model/correction_smpl.py:69-138) in eval mode -- BatchNorm
on its running statistics, no dropout, ``argmax`` node selection -- with every entry of ``named_parameters()`` a leaf, an optional linear
term ``(c * obj_pred).sum()`` on the prediction, and ``torch.optim.Adam`` on those leaves.  Built on oracle/objprojector.py
(``st_gcnn_layer``, ``dct_matrices``) and oracle/rotations.py; pinned to the reference's own autograd by tests/golden/corr_finetune*.npz.
"""
import numpy as np
import torch
from oracle.objprojector import st_gcnn_layer, dct_matrices, HAND_MARKERS
from oracle import rotations as R
from tests import skeleton_finetune_oracle as sfo

STACKS, MSE_KEYS, WEIGHTS = sfo.STACKS, sfo.MSE_KEYS, sfo.WEIGHTS
param_names, leaves, perturbed, calc_loss = sfo.param_names, sfo.leaves, sfo.perturbed, sfo.calc_loss
N_PRE = 10


def _stack(x, P, name):
    for l in range(4):
        x = st_gcnn_layer(x, P, '%s.%d' % (name, l))
    return x


def forward(P, sc, initialize, past_len=10):
    """``P`` = leaves(sd); ``sc`` = the scene's arrays (obj_angle [T,B,3], obj_trans [T,B,3], markers [T,B,67,7], numpy or tensors)
    -> (obj_pred [T,B,9], obj_gt [T,B,9])."""
    dt = next(iter(P.values())).dtype
    t = lambda a: torch.as_tensor(np.asarray(a)).float().to(dt)
    aa, trans, mk = t(sc['obj_angle']), t(sc['obj_trans']), t(sc['markers'])
    d6 = R.matrix_to_rotation_6d(R.axis_angle_to_matrix(aa))
    hv, contact = mk[..., :3], mk[past_len:, :, :, 6].sum(dim=0)
    T, B, Pn, _ = hv.shape
    dct64, idct64 = dct_matrices(T)
    dct, idct = torch.from_numpy(dct64).to(dt)[:N_PRE], torch.from_numpy(idct64).to(dt)[:, :N_PRE]
    idx_pad = list(range(past_len)) + [past_len - 1] * (T - past_len)
    rel = torch.cat([d6[:, :, None, :].expand(T, B, Pn, 6), trans[:, :, None, :] - hv], dim=3)[idx_pad]
    rel = torch.einsum('kt,tbpc->bckp', dct, rel)
    rel = rel + _stack(rel, P, 'st_gcnns_relative')
    multi = torch.cat([rel[:, :6], rel[:, 6:9] + torch.einsum('kt,tbpc->bckp', dct, hv)], dim=1)
    og = torch.cat([d6, trans], dim=2)
    o = torch.einsum('kt,tbc->bck', dct, og[idx_pad])[..., None]
    o = o + _stack(o, P, 'st_gcnns')
    allx = torch.cat([o, multi], dim=3)
    allx = allx + _stack(allx, P, 'st_gcnns_all')
    res = torch.einsum('tk,bckp->tbpc', idct, allx)                              # [T,B,68,9]
    if initialize:
        return res.mean(dim=2), og
    score = contact.clone()
    score[:, HAND_MARKERS] = score[:, HAND_MARKERS] + 0.5
    pick = torch.where(contact.sum(dim=1) > 0, 1 + torch.argmax(score, dim=1), torch.zeros(B, dtype=torch.int64))
    return res[:, torch.arange(B), pick, :], og


def loss(P, sc, initialize, extra=None, past_len=10, w=WEIGHTS):
    """-> (objective, loss of the 8 terms, loss_dict, weighted): objective = loss + (extra * obj_pred).sum() when ``extra`` [T,B,9] is given."""
    pred, gt = forward(P, sc, initialize, past_len)
    l, ld, wd = calc_loss(pred, gt, past_len, w)
    obj = l if extra is None else l + (torch.as_tensor(np.asarray(extra)).to(pred.dtype) * pred).sum()
    return obj, l, ld, wd


def loss_and_grads(P, sc, initialize, extra=None, past_len=10, w=WEIGHTS):
    names = param_names(P)
    with torch.enable_grad():                                  # (other test modules switch autograd off process-wide)
        obj, l, ld, _ = loss(P, sc, initialize, extra, past_len, w)
        g = torch.autograd.grad(obj, [P[n] for n in names])
    return l.detach(), {k: v.detach() for k, v in ld.items()}, dict(zip(names, g))


def adam_trajectory(sd, sc, steps, initialize, lr=3e-4, weight_decay=0., dtype=torch.float64, past_len=10):
    """``steps`` training steps with torch.optim.Adam on the leaves -> (losses [steps], final {name: tensor})."""
    P = leaves(sd, dtype)
    names = param_names(P)
    opt = torch.optim.Adam([P[n] for n in names], lr=lr, weight_decay=weight_decay)
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        with torch.enable_grad():
            l = loss(P, sc, initialize, None, past_len)[1]
            l.backward()
        opt.step()
        losses.append(float(l.detach()))
    return np.asarray(losses), {n: P[n].detach() for n in names}


def extra_gradient(seed, T, B, scale=2e-5):
    """The seeded c [T,B,9] of the extra-gradient point: ``scale`` * N(0,1), float32 -- the size of the loss gradient at the prediction (its rms on the scene is 1.6e-5)."""
    return (scale * np.random.RandomState(seed).standard_normal((T, B, 9))).astype(np.float32)
