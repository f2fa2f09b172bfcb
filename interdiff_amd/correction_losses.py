"""Scoring of a correction-predictor checkpoint on the HIP path: the number ``ModelCheckpoint(monitor='val_loss')`` selects
``correction.ckpt`` by (interdiff/train_correction_smpl.py), and the backward of its two geometry terms (``contact_gradient``, what the
correction trainers feed their ``d_obj_pred`` seam with).  No optimiser, no rendering.

    calc_loss_contact   LitInteraction.calc_loss_contact :103-185  (8 object MSE terms + contact + penetration)
    calc_loss           LitInteraction.calc_loss :60-101           (the 8 MSE terms; rotation width 6, or 4 for the skeleton trainer)
    validation_step     _common_step(mode='valid') :187-189 + validation_step :272-277: ObjProjector.forward with
                        ``initialize = current_epoch < 10``, then calc_loss_contact; the ``visualize`` branch is not built
    contact_gradient    d (annealed penetration + contact) / d obj_pred :121-162 (csrc/corr_geometry_grad.hip)
    body_records        the ``human_verts`` [T,B,6890,7] / ``markers`` [T,B,67,7] records of a batch from a body model

The batch is the DataLoader's dict of lists (``frames[t]['human_verts']`` [B,V,7] = position | normal | contact label,
``obj_points`` [B,P,6]) or the stacked tensors (``human_verts`` [T,B,V,7]).  All arithmetic runs in libinterdiff_hip.so
(csrc/corr_losses.hip): a launch count that does not depend on T * B (the rotation entry, the fused geometry pass, the reduction);
torch only applies the ten weights.  The contact labels are an input; ``contact_labels.generate_contact``
(prepare_behave.py) writes them.
"""
from dataclasses import dataclass
import torch
from . import _lib

GEOMETRY_KEYS = ('penetration', 'contact')
MSE_KEYS = ('obj_rot_past', 'obj_nonrot_past', 'obj_rot_future', 'obj_nonrot_future',
            'obj_rot_v_past', 'obj_nonrot_v_past', 'obj_rot_v_future', 'obj_nonrot_v_future')
LOSS_KEYS = GEOMETRY_KEYS + MSE_KEYS                     # the reference's loss_dict order (:155-172) = the kernel's term index
WEIGHTED_KEYS = ('contact', 'penetration') + MSE_KEYS    # the order of its weighted_loss_dict (:159-181)


@dataclass(frozen=True)
class CorrectionLossWeights:
    """The reference's CLI defaults (train_correction_smpl.py:308-321, :333)."""
    weight_obj_rot: float = 0.1
    weight_obj_nonrot: float = 0.1
    weight_past: float = 0.5
    weight_v: float = 1.0
    weight_contact: float = 1.0
    weight_penetration: float = 0.1
    use_annealing: int = 1
    second_stage: int = 20

    def annealing_factor(self, current_epoch):
        """min(1, max(epoch / second_stage, 0)) (:158); squared where it is applied (:160-161)."""
        return min(1.0, max(float(current_epoch) / self.second_stage, 0)) if self.use_annealing else 1

    def vector(self, current_epoch=0):
        """The ten factors of the weighted dict, in LOSS_KEYS order."""
        a2 = max(self.annealing_factor(current_epoch) ** 2, 0)
        mse = []
        for k in MSE_KEYS:
            w = self.weight_obj_rot if '_rot' in k else self.weight_obj_nonrot
            if '_v_' in k:
                w = w * self.weight_v
            if k.endswith('past'):
                w = w * self.weight_past
            mse.append(w)
        return (a2 * self.weight_penetration, a2 * self.weight_contact) + tuple(mse)


def _stack_frames(batch, key, device):
    if key in batch:
        return batch[key].to(device)
    return torch.stack([f[key] for f in batch['frames']]).to(device)


def correction_terms(obj_pred, obj_gt, obj_points=None, human_verts=None, past_len=10, return_frames=False):
    """The raw terms on ``interdiff_correction_losses``: f32 [10] in LOSS_KEYS order (terms 0, 1 are zero without the geometry
    operands).  ``obj_points`` [B,P,>=3] canonical (xyz leading), ``human_verts`` [T,B,V,7].  ``return_frames``: also the per-frame
    partials [T*B,4] = (penetration sum, contact sum, penetrating points, contact vertices)."""
    lib = _lib.load()
    x, g = obj_pred.contiguous().float(), obj_gt.contiguous().float()
    if x.dim() != 3 or x.shape != g.shape or x.shape[2] < 4:
        raise ValueError('obj_pred and obj_gt must both be [T,B,rot_width + 3]')
    T, B, C = x.shape
    out = torch.empty(10, dtype=torch.float32, device=x.device)
    if obj_points is None and human_verts is None:
        if return_frames:
            raise ValueError('per-frame partials need the geometry operands')
        _lib.check(lib.interdiff_correction_losses(_lib.dptr(x), _lib.dptr(g), None, 0, None, T, B, 0, 0, C - 3, past_len, _lib.dptr(out), None,
                                                   None, 0, _lib.stream()), 'correction_losses')
        return out
    pts, hv = obj_points.float(), human_verts.float()
    if not pts.is_contiguous():
        pts = pts.contiguous()
    if not hv.is_contiguous():
        hv = hv.contiguous()
    if pts.dim() != 3 or pts.shape[0] != B or pts.shape[2] < 3 or hv.dim() != 4 or tuple(hv.shape[:2]) != (T, B) or hv.shape[3] != 7:
        raise ValueError('obj_points must be [B,P,>=3] and human_verts [T,B,V,7] (position | normal | contact label)')
    P, V = pts.shape[1], hv.shape[2]
    ws = torch.empty(lib.interdiff_correction_losses_workspace_bytes(T, B, V, P), dtype=torch.uint8, device=x.device)
    frames = torch.empty(T * B, 4, dtype=torch.float32, device=x.device) if return_frames else None
    _lib.check(lib.interdiff_correction_losses(_lib.dptr(x), _lib.dptr(g), _lib.dptr(pts), pts.shape[2], _lib.dptr(hv), T, B, V, P, C - 3, past_len,
                                               _lib.dptr(out), _lib.dptr(frames, allow_none=True), _lib.dptr(ws), ws.numel(), _lib.stream()),
               'correction_losses')
    return (out, frames) if return_frames else out


def _dicts(terms, keys, first, vec):
    wt = terms[first:] * torch.tensor(vec[first:], dtype=torch.float32, device=terms.device)
    loss_dict = {k: terms[first + i] for i, k in enumerate(keys)}
    weighted = {k: wt[i] for i, k in enumerate(keys)}
    return wt.sum(), loss_dict, weighted


def calc_loss_contact(obj_pred, obj_gt, batch, past_len=10, weights=CorrectionLossWeights(), current_epoch=0):
    """``obj_pred``, ``obj_gt`` [T,B,9] (rot6d | translation) -> (loss, loss_dict, weighted_loss_dict): 0-dim device tensors under the
    reference's ten keys, the two geometry terms annealed by ``min(1, max(epoch / second_stage, 0)) ** 2``."""
    dev = obj_pred.device
    terms = correction_terms(obj_pred, obj_gt, batch['obj_points'].to(dev), _stack_frames(batch, 'human_verts', dev), past_len)
    loss, loss_dict, weighted = _dicts(terms, LOSS_KEYS, 0, weights.vector(current_epoch))
    return loss, loss_dict, {k: weighted[k] for k in WEIGHTED_KEYS}


def has_geometry(batch):
    """Whether ``batch`` carries what the two geometry terms read: ``obj_points`` and ``human_verts`` (stacked, or in every ``frames[t]``)."""
    if not isinstance(batch, dict) or 'obj_points' not in batch:
        return False
    return 'human_verts' in batch or ('frames' in batch and all('human_verts' in f for f in batch['frames']))


def geometry_gradient(obj_pred, obj_points, human_verts, w_penetration, w_contact, return_frames=False):
    """``interdiff_correction_geometry_grads``: d (w_penetration * penetration + w_contact * contact) / d obj_pred -> (f32 [T,B,9], f32 [2] the two raw
    terms[, per-frame partials [T*B,4] as ``correction_terms`` returns them]).  The weights are the already annealed factors."""
    lib = _lib.load()
    x = obj_pred.contiguous().float()
    if x.dim() != 3 or x.shape[2] != 9:
        raise ValueError('obj_pred must be [T,B,9] (rot6d | translation)')
    T, B = x.shape[:2]
    pts, hv = obj_points.to(x.device).float(), human_verts.to(x.device).float()
    if not pts.is_contiguous():
        pts = pts.contiguous()
    if not hv.is_contiguous():
        hv = hv.contiguous()
    if pts.dim() != 3 or pts.shape[0] != B or pts.shape[2] < 3 or hv.dim() != 4 or tuple(hv.shape[:2]) != (T, B) or hv.shape[3] != 7:
        raise ValueError('obj_points must be [B,P,>=3] and human_verts [T,B,V,7] (position | normal | contact label)')
    P, V = pts.shape[1], hv.shape[2]
    ws = torch.empty(lib.interdiff_correction_geometry_grads_workspace_bytes(T, B, V, P), dtype=torch.uint8, device=x.device)
    out, terms = torch.empty_like(x), torch.empty(2, dtype=torch.float32, device=x.device)
    frames = torch.empty(T * B, 4, dtype=torch.float32, device=x.device) if return_frames else None
    _lib.check(lib.interdiff_correction_geometry_grads(_lib.dptr(x), _lib.dptr(pts), pts.shape[2], _lib.dptr(hv), T, B, V, P, float(w_penetration),
                                                       float(w_contact), _lib.dptr(out), _lib.dptr(terms), _lib.dptr(frames, allow_none=True), _lib.dptr(ws),
                                                       ws.numel(), _lib.stream()), 'correction_geometry_grads')
    return (out, terms, frames) if return_frames else (out, terms)


def contact_gradient(obj_pred, batch, weights=CorrectionLossWeights(), current_epoch=0):
    """The gradient at ``obj_pred`` [T,B,9] of the two annealed geometry terms of ``calc_loss_contact`` (what ``loss.backward()`` sends into the
    prediction from train_correction_smpl.py:121-162) -> (d_obj_pred [T,B,9], {'penetration', 'contact'}: the raw terms, 0-dim device tensors).
    ``batch`` as ``calc_loss_contact`` takes it.  This is the ``d_obj_pred`` of the trainers' gradient calls."""
    dev = obj_pred.device
    w = weights.vector(current_epoch)
    d, terms = geometry_gradient(obj_pred, batch['obj_points'].to(dev), _stack_frames(batch, 'human_verts', dev), w[0], w[1])
    return d, {k: terms[i] for i, k in enumerate(GEOMETRY_KEYS)}


def calc_loss(obj_pred, obj_gt, batch=None, past_len=10, weights=CorrectionLossWeights()):
    """The eight MSE terms only (``calc_loss``); [T,B,W+3] with rot = the leading W channels (6: the SMPL trainer, 4: the skeleton
    trainer's pose).  ``batch`` is accepted and unused, like upstream."""
    terms = correction_terms(obj_pred, obj_gt, past_len=past_len)
    return _dicts(terms, MSE_KEYS, 2, weights.vector(0))


def validation_step(objprojector, batch, current_epoch=0, weights=CorrectionLossWeights()):
    """-> (val_loss, {'val_<term>': value}): ``ObjProjector.forward(batch, initialize=current_epoch < 10)`` + ``calc_loss_contact``."""
    obj_pred, obj_gt = objprojector.forward(batch, current_epoch < 10)
    loss, loss_dict, _ = calc_loss_contact(obj_pred, obj_gt, batch, objprojector.past_len, weights, current_epoch)
    return loss, {'val_' + k: v for k, v in loss_dict.items()}


def body_records(smpl_layer, pose, betas, trans, contact_labels, markers_idx=None, topology=None):
    """The two per-frame body records of a batch (data/dataset_smpl.py) from a body model, on the HIP SMPL forward and
    ``vertex_normals``: ``human_verts`` [T,B,V,7] = vertex | normal | contact label and ``markers`` [T,B,67,7] = its rows
    ``markerset_ssm67_smplh``.  ``pose`` [T,B,3J] axis-angle, ``betas`` [T,B,nb], ``trans`` [T,B,3], ``contact_labels`` [T,B,V]
    (``data.clip_labels`` of a ``contact.npz`` that ``contact_labels.generate_contact`` wrote).  ``topology``: a ``geometry.MeshTopology`` to reuse."""
    from .correction import MARKERS67
    from .geometry import vertex_normals
    T, B = pose.shape[:2]
    verts = smpl_layer(pose.reshape(T * B, -1), th_betas=betas.reshape(T * B, -1), th_trans=trans.reshape(T * B, 3))[0]
    V = verts.shape[1]
    if tuple(contact_labels.shape) != (T, B, V):
        raise ValueError('contact_labels must be [T,B,%d]' % V)
    normals = vertex_normals(verts, topology if topology is not None else smpl_layer.th_faces)
    hv = torch.cat([verts, normals, contact_labels.to(verts.device).float().reshape(T * B, V, 1)], dim=2).view(T, B, V, 7)
    idx = torch.as_tensor(list(MARKERS67 if markers_idx is None else markers_idx), dtype=torch.long, device=hv.device)
    return hv, hv[:, :, idx].contiguous()
