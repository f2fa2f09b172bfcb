"""HO-GCN skeleton mode (eval_skeleton.py): the correction predictor ``ObjProjector.sample``
(model/correction_skeleton.py:84-137), the correction hook ``denoised_fn`` (eval_skeleton.py:82-111) and the metrics
``calc_metric_single`` (:46-68) on ``interdiff_skeleton_*`` (csrc/skeleton.hip).

Tokens are C = 106 channels: body 21 x 3 | object keypoints 12 x 3 | pose [translation 3, quaternion xyzw 4].

``pack_skeleton_objprojector`` takes the skeleton checkpoint's state_dict (``checkpoints/obj_skeleton.ckpt``, with or without
the ``model.`` prefix) and folds, on the host in float64:
  * eval-mode BatchNorm into the preceding 1x1 convolution (tcn.0/tcn.1 and residual.0/residual.1);
  * the idx_pad frame repetition into ``dct_pad`` [n_pre, past_len];
  * DCT / IDCT matrices as get_dct_matrix builds them (fp64, inverse by numpy) -> fp32.
Arena layer block (csrc/skeleton.h): Tm | (A^T padded to 32 x 32 per coefficient, joint stack) | Wt bt Wr br (zero-padded to
multiples of 16 channels: MFMA operands) | prelu.
"""
import ctypes as C
import itertools
import numpy as np
import torch
from . import _lib
from .correction import correction_gate
from .objprojector import dct_matrices, _fold, _np

STACKS = ('st_gcnns_relative', 'st_gcnns', 'st_gcnns_all')
N_PRE, N_JOINTS, N_OBJ = 20, 21, 12
C_TOKENS = 3 * N_JOINTS + 3 * N_OBJ + 7          # 106
VP = 32                                          # joint-stack nodes (22) padded to 2 MFMA tiles (csrc/skeleton.h)
METRIC_FROM = 10                                 # calc_metric_single scores frames 10.. (a literal in eval_skeleton.py:55-62)

_UID = itertools.count(1)


def _check(rc, what):
    """IDF_E_INVAL (a shape the kernel was not built for: T != past_len + future_len, channel counts) -> ValueError."""
    if rc == -22:
        raise ValueError('interdiff_hip %s: IDF_E_INVAL (bad shape / pointer / unsupported size)' % what)
    _lib.check(rc, what)


def _strip(sd):
    return {(k[6:] if k.startswith('model.') else k): v for k, v in sd.items()}


def pack_skeleton_objprojector(state_dict, past_len=10, future_len=10):
    """-> (idf_skel_objproj with arena = NULL, float32 numpy arena).  The caller puts the arena on the device and sets ``arena``."""
    sd = _strip(state_dict)
    T = past_len + future_len
    if T != N_PRE:
        raise ValueError('the skeleton predictor keeps all %d DCT coefficients: past_len + future_len must be %d' % (N_PRE, N_PRE))
    parts, n = [], [0]

    def add(a):
        a = np.ascontiguousarray(a, dtype=np.float32).ravel()
        off = n[0]
        pad = (-a.size) % 16
        parts.append(a)
        if pad:
            parts.append(np.zeros(pad, np.float32))
        n[0] += a.size + pad
        return off
    op = _lib.SkelObjProj()
    op.T, op.past_len, op.J, op.n_pre = T, past_len, N_JOINTS, N_PRE
    dct, idct = dct_matrices(T)
    d = dct[:N_PRE]
    dpad = d[:, :past_len].copy()
    dpad[:, past_len - 1] = d[:, past_len - 1:].sum(axis=1)
    op.dct_pad, op.dct, op.idct = add(dpad), add(d), add(idct[:, :N_PRE])
    for s, name in enumerate(STACKS):
        for l in range(4):
            p = '%s.%d' % (name, l)
            Wt, bt = _fold(sd, p + '.tcn.0', p + '.tcn.1')
            Wr, br = _fold(sd, p + '.residual.0', p + '.residual.1')
            cout, cin = Wt.shape
            cinp, coutp = -(-cin // 16) * 16, -(-cout // 16) * 16

            def padw(W):
                out = np.zeros((coutp, cinp))
                out[:cout, :cin] = W
                return out.ravel()

            def padb(b):
                out = np.zeros(coutp)
                out[:cout] = b
                return out
            blk = [_np(sd[p + '.gcn.T']).ravel()]
            if s == 2:
                A = _np(sd[p + '.gcn.A'])                                  # [n_pre, nodes, nodes] : y[w] = sum_v x[v] A[t][v][w]
                AT = np.zeros((N_PRE, VP, VP))
                AT[:, :A.shape[2], :A.shape[1]] = A.transpose(0, 2, 1)     # [t][w][v], zero padded to 32 x 32
                blk.append(AT.ravel())
            blk += [padw(Wt), padb(bt), padw(Wr), padb(br), _np(sd[p + '.prelu.weight']).ravel()]
            op.layer[s * 4 + l] = add(np.concatenate(blk))
            op.cout[s * 4 + l], op.cin[s * 4 + l] = cout, cin
    return op, np.concatenate(parts)


def packed_layers(op, arena):
    """The 12 folded layers back out of a packed arena (numpy, float32), as dicts Tm, A (joint stack), Wt, bt, Wr, br, prelu --
    what the CPU restatement (tests/skeleton_oracle.py) evaluates to check the packer."""
    out = []
    for li in range(12):
        s, cin, cout = li // 4, op.cin[li], op.cout[li]
        cinp, coutp = -(-cin // 16) * 16, -(-cout // 16) * 16
        nodes = N_JOINTS + 1
        o = op.layer[li]
        L = {}
        nT = nodes * N_PRE * N_PRE if s == 2 else N_PRE * N_PRE
        L['Tm'] = arena[o:o + nT].reshape((nodes, N_PRE, N_PRE) if s == 2 else (N_PRE, N_PRE))
        o += nT
        if s == 2:
            AT = arena[o:o + N_PRE * VP * VP].reshape(N_PRE, VP, VP)
            L['A'] = AT[:, :nodes, :nodes].transpose(0, 2, 1)
            o += N_PRE * VP * VP
        L['Wt'] = arena[o:o + coutp * cinp].reshape(coutp, cinp)[:cout, :cin]; o += coutp * cinp
        L['bt'] = arena[o:o + cout]; o += coutp
        L['Wr'] = arena[o:o + coutp * cinp].reshape(coutp, cinp)[:cout, :cin]; o += coutp * cinp
        L['br'] = arena[o:o + cout]; o += coutp
        L['prelu'] = arena[o]
        out.append(L)
    return out


class SkeletonObjProjector:
    """``ObjProjector`` of model/correction_skeleton.py in eval mode, on one fused launch per call."""

    def __init__(self, state_dict, past_len=10, future_len=10, device='cuda'):
        self.lib = _lib.load()
        self.device = torch.device(device)
        self.past_len, self.T = past_len, past_len + future_len
        self.cop, arena = pack_skeleton_objprojector(state_dict, past_len, future_len)
        self.arena = torch.from_numpy(arena).to(self.device)
        self.cop.arena = self.arena.data_ptr()

    def eval(self):
        return self

    def sample(self, obj_angles, obj_trans, human_points):
        """obj_angles [T,B,4] quaternion xyzw, obj_trans [T,B,3], human_points [T,B,21,3] -> (quaternion xyzw [T,B,4], translation [T,B,3])."""
        T, B = obj_angles.shape[:2]
        if T != self.T or human_points.shape[:3] != (T, B, N_JOINTS):
            raise ValueError('expected T=%d frames and %d joints' % (self.T, N_JOINTS))
        oa, ot, hp = (a.contiguous().float() for a in (obj_angles, obj_trans, human_points))
        q = torch.empty(T, B, 4, dtype=torch.float32, device=self.device)
        tr = torch.empty(T, B, 3, dtype=torch.float32, device=self.device)
        _check(self.lib.interdiff_skeleton_objprojector_sample(C.byref(self.cop), _lib.dptr(oa), _lib.dptr(ot), _lib.dptr(hp), B,
                                                               _lib.dptr(q), _lib.dptr(tr), _lib.stream()), 'skeleton_objprojector_sample')
        return q, tr


class HipSkeletonCorrection:
    """Drop-in ``denoised_fn(x, t, model_kwargs)`` of eval_skeleton.py:82-111 on ``interdiff_skeleton_correction``.

    Gated like the SMPL hook (t <= 500 and t % 50 == 0, ``correction_gate``); when it acts it returns a NEW tensor
    t/1000 * x + (1 - t/1000) * [body, calc_obj_pred(pose'), pose'] and leaves x untouched, like the reference.  Reads the past pose
    rows of ``model_kwargs['y']['inpainted_motion']`` and ``model_kwargs['zero_pose_obj']`` [B,12,3] -- top level, where the reference
    puts it; ``model_kwargs['y']['zero_pose_obj']`` is taken when the top level has none (a sampler that hands every top-level key to
    the denoiser needs it there).  The reference's contact labels (``body_obj_to_contact``, :99) are computed and never read: not built.
    Not graph-capturable: the sampler calls it eagerly on both of its routes."""

    graph_capturable = False

    def __init__(self, objprojector, device='cuda'):
        self.lib = _lib.load()
        self.objproj = objprojector
        self.device = torch.device(device)
        self._uid = next(_UID)

    def is_active(self, t0):
        return correction_gate(int(t0))

    @staticmethod
    def zero_pose_obj(model_kwargs):
        z = model_kwargs.get('zero_pose_obj')
        return model_kwargs['y']['zero_pose_obj'] if z is None else z

    def apply(self, x, t0, y, zero_pose_obj):
        """Run the correction unconditionally for timestep value t0 (host int); x [B,1,106,T] -> new tensor."""
        B, _, Cc, T = x.shape
        if Cc != C_TOKENS:
            raise ValueError('skeleton tokens have %d channels, got %d' % (C_TOKENS, Cc))
        if tuple(zero_pose_obj.shape) != (B, N_OBJ, 3):
            raise ValueError('zero_pose_obj must be [B, %d, 3]' % N_OBJ)
        xc, gt = x.contiguous().float(), y['inpainted_motion'].contiguous().float()
        if gt.shape != xc.shape:
            raise ValueError('inpainted_motion must have the shape of x')
        z = zero_pose_obj.contiguous().float()
        out = torch.empty_like(xc)
        blend_t = float(np.float32(t0) / np.float32(1000))                      # hard-coded 1000, eval_skeleton.py:111
        _check(self.lib.interdiff_skeleton_correction(C.byref(self.objproj.cop), _lib.dptr(xc), _lib.dptr(gt), _lib.dptr(z), B, T, blend_t,
                                                      _lib.dptr(out), _lib.stream()), 'skeleton_correction')
        return out

    def __call__(self, x, t, model_kwargs):
        t0 = getattr(t, 'host_value', None)
        if t0 is None:
            t0 = int(t[0])                      # device sync, like the reference's `t[0] > 500`
        if not correction_gate(t0):
            return x
        return self.apply(x, t0, model_kwargs['y'], self.zero_pose_obj(model_kwargs))


def skeleton_metrics(body_pred, body_gt, obj_pred, obj_gt, pose_pred, pose_gt, from_frame=METRIC_FROM):
    """calc_metric_single (eval_skeleton.py:46-68): body [T,B,21,3], obj [T,B,12,3], pose [T,B,7] (pred and gt) ->
    dict(mpjpe_h, mpjpe_o, translation_error, rotation_error) over frames from_frame.. (Python floats, like .item())."""
    T, B = body_pred.shape[:2]
    args = [a.contiguous().float() for a in (body_pred, body_gt, obj_pred, obj_gt, pose_pred, pose_gt)]
    if args[0].numel() != T * B * 3 * N_JOINTS or args[2].numel() != T * B * 3 * N_OBJ or args[4].numel() != T * B * 7:
        raise ValueError('expected body [T,B,21,3], obj [T,B,12,3], pose [T,B,7]')
    if any(a.shape != b.shape for a, b in zip(args[::2], args[1::2])):
        raise ValueError('pred and gt shapes differ')
    out = torch.empty(4, dtype=torch.float32, device=args[0].device)
    lib = _lib.load()
    _check(lib.interdiff_skeleton_metrics(*[_lib.dptr(a) for a in args], T, B, from_frame, _lib.dptr(out), _lib.stream()), 'skeleton_metrics')
    v = out.cpu().tolist()
    return dict(mpjpe_h=v[0], mpjpe_o=v[1], translation_error=v[2], rotation_error=v[3])
