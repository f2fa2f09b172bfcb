"""Corrector seam: ``ObjProjector.sample(obj_angles, obj_trans, human_verts, contact)``
(model/correction_smpl.py:79-138, eval branch) on ``interdiff_objprojector_sample``, and the trainer's teacher-forced
``ObjProjector.forward(data, initialize)`` (:69-77) on ``interdiff_objprojector_forward``.

``pack_objprojector`` takes the reference module's state_dict (``checkpoints/correction.ckpt`` keys with
the ``model.`` prefix stripped); what it folds and the arena it writes: ``stgcn_pack.py``, csrc/stgcn.h.
"""
import ctypes as C
import numpy as np
import torch
from . import _lib
from .stgcn_pack import ArenaBuilder, dct_matrices, pack_dct, pack_stgcn_layers     # noqa: F401  (dct_matrices: the tests read it here)

HAND_MARKERS = [10, 11, 14, 31, 13, 17, 23, 28, 27] + [60, 43, 44, 47, 62, 46, 51, 57]   # data/utils.py:249-260
VP = 80                                  # nodes padded to 5 MFMA tiles (csrc/objproj.h)


def pack_objprojector(sd, T, past_len, device, n_pre=10, P=67):
    ab = ArenaBuilder()
    op = _lib.ObjProj()
    op.T, op.past_len, op.P, op.n_pre = T, past_len, P, n_pre
    op.dct_pad, op.dct, op.idct = pack_dct(ab, T, n_pre, past_len)
    bonus = np.zeros(P)
    bonus[HAND_MARKERS] = 0.5
    op.hand_bonus = ab.add(bonus)
    pack_stgcn_layers(ab, sd, op, n_pre, VP)
    arena = torch.from_numpy(ab.arena()).to(device)
    op.arena = arena.data_ptr()
    return op, arena


class ObjProjector:
    def __init__(self, state_dict, T, past_len=10, device='cuda', n_pre=10):
        self.lib = _lib.load()
        self.device = torch.device(device)
        self.T, self.past_len = T, past_len
        self.cop, self.arena = pack_objprojector(state_dict, T, past_len, self.device, n_pre=n_pre)

    def eval(self):
        return self

    def batch_tensors(self, data):
        """Either batch form of ``forward`` -> (obj_angle [T,B,3], obj_trans [T,B,3], markers [T,B,67,7]), float32 on the device."""
        if 'frames' in data:
            fr = data['frames']
            aa = torch.stack([f['objfit_params']['angle'] for f in fr])
            ot = torch.stack([f['objfit_params']['trans'] for f in fr])
            mk = torch.stack([f['markers'] for f in fr])
        else:
            aa, ot, mk = data['obj_angle'], data['obj_trans'], data['markers']
        aa, ot, mk = (a.to(self.device).float() for a in (aa, ot, mk))
        if mk.dim() != 4 or mk.shape[-1] != 7:
            raise ValueError('markers must be [T,B,67,7] (position | normal | contact label)')
        return aa, ot, mk

    def forward(self, data, initialize=False):
        """``ObjProjector.forward`` (model/correction_smpl.py:69-77): ``data`` is the reference's dict-of-lists batch
        (``frames[t]['objfit_params']['angle' | 'trans']`` [B,3], ``frames[t]['markers']`` [B,67,7]) or the stacked tensors
        ``dict(obj_angle [T,B,3], obj_trans [T,B,3], markers [T,B,67,7])``.  Axis-angle -> 6D on the rotation kernels, contact =
        the future frames' marker labels summed, then ``sample``.  Returns (final_results [T,B,9], obj_gt [T,B,9])."""
        from . import transforms
        aa, ot, mk = self.batch_tensors(data)
        d6 = transforms.matrix_to_rotation_6d(transforms.axis_angle_to_matrix(aa))
        contact = mk[self.past_len:, :, :, 6].sum(dim=0)
        return self.sample(d6, ot, mk, contact, initialize), torch.cat([d6, ot], dim=2)

    __call__ = forward

    def sample(self, obj_angles, obj_trans, human_verts, contact, initialize=False):
        """``initialize=True``: the mean over the 68 output nodes (:122-123, what the trainer asks for while current_epoch < 10);
        ``contact`` is then not read."""
        T, B = obj_angles.shape[:2]
        if T != self.T:
            raise ValueError('ObjProjector was packed for T=%d' % self.T)
        hv = human_verts[..., :3].contiguous().float()
        oa, ot = obj_angles.contiguous().float(), obj_trans.contiguous().float()
        out = torch.empty(T, B, 9, dtype=torch.float32, device=self.device)
        if initialize:
            ws = torch.empty(self.lib.interdiff_objprojector_forward_workspace_bytes(B), dtype=torch.uint8, device=self.device)
            _lib.check(self.lib.interdiff_objprojector_forward(C.byref(self.cop), _lib.dptr(oa), _lib.dptr(ot), _lib.dptr(hv), None, B, 1,
                                                               _lib.dptr(out), _lib.dptr(ws), ws.numel(), _lib.stream()), 'objprojector_forward')
            return out
        ct = contact.to(torch.int32).contiguous()
        _lib.check(self.lib.interdiff_objprojector_sample(C.byref(self.cop), _lib.dptr(oa), _lib.dptr(ot), _lib.dptr(hv),
                                                          _lib.dptr(ct, torch.int32), B, _lib.dptr(out), _lib.stream()),
                   'objprojector_sample')
        return out
