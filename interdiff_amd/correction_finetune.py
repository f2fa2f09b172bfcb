"""Fine-tuning of the SMPL contact-frame correction predictor (``checkpoints/correction.ckpt``) on the HIP path under the object-pose loss,
with FROZEN normalisation statistics: the reference module in ``eval()`` with autograd on.  BatchNorm uses its running statistics and
never updates them, dropout is off, contact clips take the ``argmax`` node, and every one of the 224,174 parameters is trained --
convolutions, BatchNorm affine weights, the temporal and adjacency matrices, the PReLU slopes.

    loss, grads     LitInteraction.calc_loss + loss.backward() on ObjProjector.forward   train_correction_smpl.py:60-101, model/correction_smpl.py:69-138
    training_step   + torch.optim.Adam(lr, weight_decay=l2_norm).step()                  :51-58, :263-270

That is the reference's own regime where its schedule starts: ``_common_step`` anneals the contact and penetration terms by
``min(1, epoch / second_stage) ** 2``, exactly 0 at epoch 0, so there it trains on the eight MSE terms alone.  From epoch 1 on those two
terms add a gradient that reaches the network only through ``obj_pred`` [T,B,9]: ``d_obj_pred`` is the seam through which it comes in.
A batch that also carries ``obj_points`` and ``human_verts`` gets it in the same call -- ``predict`` (this object's own prediction, the forward half
of the gradient call) -> ``correction_losses.contact_gradient`` (csrc/corr_geometry_grad.hip) -> the gradient call with that ``d_obj_pred`` -- so
``training_step(batch, current_epoch)`` trains on the reference's full loss at every epoch; the forward runs twice.
Training the way the reference trains -- the module in ``train()``: batch statistics, running-statistics updates, dropout, ``multinomial``
node selection -- is ``interdiff_amd.correction_train.CorrectionTrainer``, built on this class.  NOT built: a single-pass
launcher that splits at the head, learning-rate schedules, the Lightning glue and the dataset.

All arithmetic runs in libinterdiff_hip.so (csrc/objproj_train.h / .hip, csrc/stgcn_train.h): one workgroup per clip for forward, loss
gradient and backward, a fixed-order fold over clips, Adam on fp32 master parameters in the reference layout, and the re-fold into the
arena that ``ObjProjector``, the correction hook and ``correction_losses.validation_step`` read.  The flat parameter layout
(``param_table``) is documented in include/interdiff_hip.h; it, the master copy and the Adam state (``FlatParameters``) are
``interdiff_amd.stgcn_trainer``'s, shared with the skeleton predictor.
"""
import torch
from . import _lib
from .objprojector import ObjProjector
from .skeleton import _strip
from .correction_losses import CorrectionLossWeights, GEOMETRY_KEYS, contact_gradient, has_geometry
from .stgcn_trainer import FlatParameters, param_table            # noqa: F401

N_MARKERS = 67
N_PRE = 10


def rotation_6d_of_axis_angle(aa):
    """``matrix_to_rotation_6d(axis_angle_to_matrix(aa))`` (ObjProjector.forward, model/correction_smpl.py:71; pytorch3d 0.7.2: through the
    quaternion) evaluated in float64 and rounded once: the loss gradient is proportional to prediction - target, and the target is this."""
    a = aa.double()
    angle = a.norm(dim=-1, keepdim=True)
    small = angle.abs() < 1e-6
    safe = torch.where(small, torch.ones_like(angle), angle)
    sinc_half = torch.where(small, 0.5 - angle * angle / 48.0, torch.sin(safe * 0.5) / safe)
    r, (i, j, k) = torch.cos(angle * 0.5)[..., 0], (a * sinc_half).unbind(-1)
    two_s = 2.0 / (r * r + i * i + j * j + k * k)
    return torch.stack([1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
                        two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r)], dim=-1).float().contiguous()


class CorrectionFineTuner(FlatParameters):
    """Adapts a contact-frame predictor to a user's own clips.  ``batch`` is what ``ObjProjector.forward`` takes: the reference's
    dict-of-lists (``frames[t]['objfit_params']['angle' | 'trans']`` [B,3], ``frames[t]['markers']`` [B,67,7]) or the stacked tensors
    ``dict(obj_angle [T,B,3], obj_trans [T,B,3], markers [T,B,67,7])``."""

    PREFIX, NODES, N_PRE = 'correction', N_MARKERS, N_PRE

    def __init__(self, state_dict, T=35, past_len=10, lr=3e-4, weight_decay=0., betas=(0.9, 0.999), eps=1e-8, weights=CorrectionLossWeights(), device='cuda'):
        sd = _strip(state_dict)
        self.lib = _lib.load()
        self.device = torch.device(device)
        self.lr, self.weight_decay, self.betas, self.eps = float(lr), float(weight_decay), (float(betas[0]), float(betas[1])), float(eps)
        self.weights = weights
        self.predictor = ObjProjector(sd, T, past_len, device=device)          # its arena is the live one
        self.past_len, self.T = past_len, T
        self._init_state(sd)

    # ---- the step
    def _inputs(self, batch, d_obj_pred=None):
        """-> (B, T, d6, obj_trans, marker positions, contact int32 [B,67], d_obj_pred or None): contiguous device tensors, what the library takes."""
        dev = self.device
        aa, ot, mk = self.predictor.batch_tensors(batch)
        T, B = aa.shape[:2]
        if T != self.T or tuple(aa.shape) != (T, B, 3) or tuple(ot.shape) != (T, B, 3) or tuple(mk.shape[:3]) != (T, B, N_MARKERS):
            raise ValueError('expected obj_angle, obj_trans [%d,B,3] and markers [%d,B,%d,7]' % (self.T, self.T, N_MARKERS))
        d6, ot = rotation_6d_of_axis_angle(aa), ot.contiguous()
        pos = mk[..., :3].contiguous()
        contact = mk[self.past_len:, :, :, 6].sum(dim=0).to(torch.int32).contiguous()
        extra = None
        if d_obj_pred is not None:
            extra = d_obj_pred.to(dev, torch.float32).contiguous()
            if tuple(extra.shape) != (T, B, 9):
                raise ValueError('d_obj_pred must be [%d,%d,9]' % (T, B))
        return B, T, d6, ot, pos, contact, extra

    def _grads(self, batch, initialize=False, d_obj_pred=None):
        B, T, d6, ot, pos, contact, extra = self._inputs(batch, d_obj_pred)
        out9, grads = self._outputs()
        ws = self._workspace(B)
        self._call('finetune_grads', _lib.dptr(self.params), _lib.dptr(self.bn), _lib.dptr(d6), _lib.dptr(ot), _lib.dptr(pos),
                   _lib.dptr(contact, torch.int32), _lib.dptr(extra, allow_none=True), B, T, int(bool(initialize)), self._w8, _lib.dptr(out9),
                   _lib.dptr(grads), _lib.dptr(ws), ws.numel(), _lib.stream())
        return out9, grads

    def predict(self, batch, initialize=False):
        """``obj_pred`` [T,B,9] (rot6d | translation) as the backward of ``loss_and_grads`` sees it: the forward half of the gradient call alone
        (``interdiff_correction_finetune_predict``), the head's double rounded once."""
        B, T, d6, ot, pos, contact, _ = self._inputs(batch)
        out = torch.empty(T, B, 9, dtype=torch.float32, device=self.device)
        ws = self._workspace(B)
        self._call('finetune_predict', _lib.dptr(self.params), _lib.dptr(self.bn), _lib.dptr(d6), _lib.dptr(ot), _lib.dptr(pos),
                   _lib.dptr(contact, torch.int32), B, T, int(bool(initialize)), _lib.dptr(out), _lib.dptr(ws), ws.numel(), _lib.stream())
        return out

    def _seam(self, batch, current_epoch, initialize, d_obj_pred, **how):
        """What the gradient call gets as ``d_obj_pred`` at ``current_epoch`` -> (d_obj_pred or None, the two raw geometry terms or None).  An explicit
        ``d_obj_pred`` wins; an epoch whose annealed geometry weights are zero needs none; otherwise the batch must carry ``obj_points`` and
        ``human_verts`` and the gradient is taken at this object's own prediction: predict -> ``correction_losses.contact_gradient``.  ``how``:
        what the subclass's ``predict`` takes beyond ``initialize``."""
        geometry = self.weights.vector(current_epoch)[:2]
        if d_obj_pred is not None or not any(w != 0 for w in geometry):
            return d_obj_pred, None
        if not has_geometry(batch):
            raise ValueError('epoch %d weighs the penetration / contact terms by %r: the batch must carry obj_points [B,P,>=3] and human_verts '
                             '[T,B,V,7], or their gradient at obj_pred must come in as d_obj_pred [T,B,9]' % (current_epoch, geometry))
        return contact_gradient(self.predict(batch, initialize, **how), batch, self.weights, current_epoch)

    def _packed10(self, out9, grads, terms, current_epoch):
        """-> (loss, loss_dict, weighted_loss_dict, grads) with all ten terms under the reference's keys, as ``calc_loss_contact`` orders them."""
        loss8, ld8, wd8, g = self._packed(out9, grads)
        w = self.weights.vector(current_epoch)
        ld = {k: terms[k] for k in GEOMETRY_KEYS}
        ld.update(ld8)
        wd = {'contact': terms['contact'] * w[1], 'penetration': terms['penetration'] * w[0]}
        wd.update(wd8)
        return loss8 + wd['contact'] + wd['penetration'], ld, wd, g

    def loss_and_grads(self, batch, initialize=None, d_obj_pred=None, current_epoch=None):
        """-> (loss, loss_dict, weighted_loss_dict, grads): 0-dim device tensors under the reference's 8 MSE keys, ``grads`` = {reference
        parameter name: d (loss + <d_obj_pred, obj_pred>) / d parameter} (views of one flat device tensor).  ``d_obj_pred`` [T,B,9]: the gradient
        at the prediction of any further term of the caller's objective; the returned loss stays that of the 8 terms.
        ``current_epoch`` (``initialize`` then defaults to ``current_epoch < 10``, like ``_common_step``): the reference's full objective at that epoch.
        Where its annealed geometry weights are not zero and no ``d_obj_pred`` is given, the batch must also carry ``obj_points`` and ``human_verts``;
        the call then runs predict -> ``contact_gradient`` -> gradients and returns all ten terms and the full loss, as ``calc_loss_contact`` does."""
        if initialize is None:
            initialize = current_epoch is not None and current_epoch < 10
        if current_epoch is None:
            return self._packed(*self._grads(batch, initialize, d_obj_pred))
        d, terms = self._seam(batch, current_epoch, initialize, d_obj_pred)
        out9, grads = self._grads(batch, initialize, d)
        return self._packed(out9, grads) if terms is None else self._packed10(out9, grads, terms, current_epoch)

    def training_step(self, batch, current_epoch=0, d_obj_pred=None):
        """Gradients (``initialize = current_epoch < 10``, like ``_common_step``), Adam, re-fold.  -> the loss BEFORE the step (0-dim device tensor).
        At an epoch whose annealed contact / penetration weights are not zero the reference trains on those terms too.  A batch that carries
        ``obj_points`` and ``human_verts`` gets them here in one call: predict -> ``contact_gradient`` -> gradients with that ``d_obj_pred`` (the
        forward runs twice), and the returned loss is the full one.  An explicit ``d_obj_pred`` wins (the returned loss is then that of the 8 MSE
        terms); with neither this raises instead of training on another loss."""
        initialize = current_epoch < 10
        d, terms = self._seam(batch, current_epoch, initialize, d_obj_pred)
        out9, grads = self._grads(batch, initialize, d)
        self.apply_gradients(grads)
        return out9[0] if terms is None else self._packed10(out9, grads, terms, current_epoch)[0]
