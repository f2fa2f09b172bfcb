"""HO-GCN skeleton mode (eval_skeleton.py): the denoiser ``MDM`` of model/diffusion_skeleton.py (``SkeletonMDM``: conditioning
encoder with the shape embedding, feed-forward width 256, keypoint head ``calc_obj_pred`` inside the heads GEMM; csrc/skel_head.h),
the sampling glue ``sample_once_proj`` (eval_skeleton.py:114-142), the correction predictor ``ObjProjector.sample``
(model/correction_skeleton.py:84-137), the correction hook ``denoised_fn`` (eval_skeleton.py:82-111) and the metrics
``calc_metric_single`` (:46-68) on ``interdiff_skeleton_*`` (csrc/skeleton.hip).

Tokens are C = 106 channels: body 21 x 3 | object keypoints 12 x 3 | pose [translation 3, quaternion xyzw 4].

``pack_skeleton_objprojector`` takes the skeleton checkpoint's state_dict (``checkpoints/obj_skeleton.ckpt``, with or without
the ``model.`` prefix); what it folds and the arena it writes: ``stgcn_pack.py``, csrc/stgcn.h.
"""
import ctypes as C
import itertools
import numpy as np
import torch
from . import _lib
from .correction import correction_gate
from .stgcn_pack import ArenaBuilder, pack_dct, pack_stgcn_layers, unpack_stgcn_layers, to_f64
from . import mdm as _mdm
from .diffusion import sample_loop

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
    ab = ArenaBuilder()
    op = _lib.SkelObjProj()
    op.T, op.past_len, op.J, op.n_pre = T, past_len, N_JOINTS, N_PRE
    op.dct_pad, op.dct, op.idct = pack_dct(ab, T, N_PRE, past_len)
    pack_stgcn_layers(ab, sd, op, N_PRE, VP)
    return op, ab.arena()


def packed_layers(op, arena):
    """The 12 folded layers back out of a packed arena (numpy, float32): what the CPU restatement (tests/skeleton_oracle.py)
    evaluates to check the packer."""
    return unpack_stgcn_layers(op, arena, N_PRE, VP, N_JOINTS + 1)


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


    def forward(self, obj_angles, obj_trans, human_points):
        """``ObjProjector.forward`` of the trainer (model/correction_skeleton.py:68-80) AS WRITTEN: it converts the xyzw quaternion to 6D
        and hands the 6-vector to ``sample``, which converts again -- reading the 6-vector's trailing four values [r02, r10, r11, r12]
        as a quaternion xyzw.  The checkpoint was trained and selected through this double conversion, so it is kept: the first
        conversion runs here on the host side (elementwise torch on the device tensors), the rest is ``sample``.
        Returns (obj_angles_p [T,B,4], obj_trans_p [T,B,3], obj_angles_gt, obj_trans_gt)."""
        q = obj_angles.to(self.device).float()
        i, j, k, r = q.unbind(-1)                                               # xyzw -> (r, i, j, k) = quat_correct (:74)
        two_s = 2.0 / (q * q).sum(-1)                                           # quaternion_to_matrix, rows 0 and 1 = rotation 6D
        d6_tail = torch.stack([two_s * (i * k + j * r), two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r)], dim=-1)
        qp, tp = self.sample(d6_tail, obj_trans, human_points)
        return qp, tp, obj_angles.clone(), obj_trans.clone()


def skeleton_calc_loss(pose_pred, pose_gt, past_len=10, weights=None):
    """``calc_loss`` of train_correction_skeleton.py:85-126 on pose [T,B,7] = translation | quaternion xyzw, split as that trainer splits
    it: "rot" = the leading four channels, "nonrot" = the trailing three.  -> (loss, loss_dict, weighted_loss_dict)."""
    from . import correction_losses as cl
    return cl.calc_loss(pose_pred, pose_gt, past_len=past_len, weights=weights or cl.CorrectionLossWeights())


def skeleton_validation_step(objprojector, batch, weights=None):
    """``_common_step`` + ``validation_step`` of train_correction_skeleton.py:128-154, :191-196: ``batch`` = (body [B,T,21,3], object
    keypoints [B,T,12,3], pose [B,T,7], zero_pose_obj [B,12,3]).  -> (val_loss, loss_dict, weighted_loss_dict).  The reference also
    computes ``calc_obj_pred`` and ``calc_metric`` there and discards both (nothing logs them): neither is evaluated."""
    dev = objprojector.device
    body_gt, pose_gt = batch[0].transpose(0, 1).float().to(dev), batch[2].transpose(0, 1).float().to(dev)
    obj_trans, obj_angles = torch.split(pose_gt, [3, 4], dim=2)
    qp, tp, _, _ = objprojector.forward(obj_angles, obj_trans, body_gt)
    return skeleton_calc_loss(torch.cat([tp, qp], dim=2), pose_gt, objprojector.past_len, weights)


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


# ---------------------------------------------------------------------------------------------------------------
# the skeleton denoiser (model/diffusion_skeleton.py MDM)
# ---------------------------------------------------------------------------------------------------------------
HEAD_POSE, HEAD_BODY = 7, 25                     # rows of a 32-row column tile of the packed head: pose first, then body (csrc/skel_head.h)


def pad_ffn_width(w1, b1, w2, width=_mdm.FF):
    """linear1 [ff,256] / [ff], linear2 [256,ff] of a narrower feed-forward block -> the 1024-wide matrices the packed streams are built
    from: the added hidden units have zero weight and zero bias, gelu(0) = 0, and they meet zero columns of linear2 -- they contribute
    exactly nothing (csrc/ffn.h relies on the same for units 1024..1039), so every kernel and range proof of the 1024-wide block holds."""
    w1, b1, w2 = (np.asarray(a, np.float32) for a in (w1, b1, w2))
    ff = w1.shape[0]
    if ff > width or ff % 16 or ff < 16 or w1.shape != (ff, _mdm.D) or w2.shape != (_mdm.D, ff) or b1.shape != (ff,):
        raise ValueError('feed-forward width %d: need a multiple of 16, at most %d, with linear1 [ff,%d] and linear2 [%d,ff]' % (ff, width, _mdm.D, _mdm.D))
    w1p, b1p, w2p = np.zeros((width, _mdm.D), np.float32), np.zeros(width, np.float32), np.zeros((_mdm.D, width), np.float32)
    w1p[:ff], b1p[:ff], w2p[:, :ff] = w1, b1, w2
    return w1p, b1p, w2p


def pack_skeleton_head(body_w, body_b, obj_w, obj_b):
    """bodyFinalLinear [n_body,256] / [n_body], objFinalLinear [7,256] / [7] -> (W [32 tiles][256], b [32 tiles], tiles): every 32-row
    column tile of the heads GEMM starts with the 7 pose rows and carries 25 body rows (zero past n_body), so that the workgroup of any
    tile holds the pose of its token rows (csrc/skel_head.h)."""
    body_w, body_b, obj_w, obj_b = (np.asarray(a, np.float32) for a in (body_w, body_b, obj_w, obj_b))
    n_body = body_w.shape[0]
    if obj_w.shape != (HEAD_POSE, _mdm.D) or body_w.shape[1] != _mdm.D:
        raise ValueError('objFinalLinear must be [7,%d] (translation | quaternion xyzw)' % _mdm.D)
    tiles = -(-n_body // HEAD_BODY)
    W, b = np.zeros((32 * tiles, _mdm.D), np.float32), np.zeros(32 * tiles, np.float32)
    for t in range(tiles):
        W[32 * t:32 * t + HEAD_POSE], b[32 * t:32 * t + HEAD_POSE] = obj_w, obj_b
        n = min(HEAD_BODY, n_body - HEAD_BODY * t)
        W[32 * t + HEAD_POSE:32 * t + HEAD_POSE + n] = body_w[HEAD_BODY * t:HEAD_BODY * t + n]
        b[32 * t + HEAD_POSE:32 * t + HEAD_POSE + n] = body_b[HEAD_BODY * t:HEAD_BODY * t + n]
    return W, b, tiles


def skeleton_state_dict_for_pack(state_dict):
    """The skeleton model's state_dict in the shape ``mdm.pack_mdm_weights`` packs: feed-forward blocks zero-padded to width 1024
    (``pad_ffn_width``), objEmbedding with 7 zero columns for the pose channels the model does not embed (diffusion_skeleton.py:236-238).
    The two head matrices stay as they are (their packed form is ``pack_skeleton_head``).  Returns (dict, ff_size)."""
    sd = {k: to_f64(v).astype(np.float32) for k, v in _strip(state_dict).items() if not k.endswith('.pe')}
    ff = sd['decoder.layers.0.linear1.weight'].shape[0]
    for k in [k for k in sd if k.endswith('.linear1.weight')]:
        p = k[:-len('linear1.weight')]
        sd[p + 'linear1.weight'], sd[p + 'linear1.bias'], sd[p + 'linear2.weight'] = pad_ffn_width(sd[p + 'linear1.weight'], sd[p + 'linear1.bias'], sd[p + 'linear2.weight'])
    sd['objEmbedding.weight'] = np.concatenate([sd['objEmbedding.weight'], np.zeros((_mdm.D, HEAD_POSE), np.float32)], axis=1)
    return sd, ff


class SkeletonMDM(_mdm.MDM):
    """Drop-in for model/diffusion_skeleton.py ``MDM`` at the sampler seam: ``model(x, t, **{'y': {'cond': ...}, 'zero_pose_obj': z})``
    with x [B,1,106,T].  ``MDM``'s decoder, encoder, memory and workspace machinery on the padded weights; the last launch of a forward
    carries the keypoint head (``interdiff_skeleton_mdm_forward`` / ``_forward_step``)."""

    def __init__(self, state_dict, device='cuda', n_steps=1000, rotary=_mdm.ROTARY_DEFAULT):
        sd, self.ff_size = skeleton_state_dict_for_pack(state_dict)
        self.n_body, self.n_points = sd['bodyEmbedding.weight'].shape[1], sd['shapeEmbedding.weight'].shape[1] // 3
        hw, hb, tiles = pack_skeleton_head(sd['bodyFinalLinear.weight'], sd['bodyFinalLinear.bias'], sd['objFinalLinear.weight'], sd['objFinalLinear.bias'])
        extra = dict(out_w=hw, out_b=hb, shape_w=sd['shapeEmbedding.weight'], shape_b=sd['shapeEmbedding.bias'])
        super().__init__(sd, device=device, n_steps=n_steps, rotary=rotary, extra=extra)
        self.w.C = self.n_body + 3 * self.n_points + HEAD_POSE          # (the packer counted the embedding's columns: the same number)
        self.head = _lib.SkelHead(n_body=self.n_body, n_points=self.n_points, n_tiles=tiles, reserved=0, **extra)
        self._zero = None

    def _zpo(self, zero_pose_obj, B):
        if zero_pose_obj is None:
            raise ValueError("the skeleton denoiser needs model_kwargs['zero_pose_obj'] [B,%d,3]" % self.n_points)
        if tuple(zero_pose_obj.shape) != (B, self.n_points, 3):
            raise ValueError('zero_pose_obj must be [%d,%d,3]' % (B, self.n_points))
        return zero_pose_obj if (zero_pose_obj.dtype == torch.float32 and zero_pose_obj.is_contiguous()) else zero_pose_obj.contiguous().float()

    def forward(self, x, timesteps, zero_pose_obj=None, y=None, out=None, memctx=None, ws=None, batch_rows=None):
        """``MDM.forward(x, timesteps, zero_pose_obj, y=)`` (diffusion_skeleton.py:250-257); the other operands as ``mdm.MDM.forward``."""
        return self._forward(x, timesteps, y, out, memctx, ws, batch_rows, z=self._zpo(zero_pose_obj, x.shape[0]))

    __call__ = forward

    def _launch_forward(self, memctx, x, ts, B, T, out, ws, z):
        _check(self.lib.interdiff_skeleton_mdm_forward(C.byref(self.w), C.byref(self.head), _lib.dptr(memctx), _lib.dptr(x, torch.float32),
                                                       _lib.dptr(ts, torch.int64), _lib.dptr(z), B, T, _lib.dptr(out, torch.float32),
                                                       _lib.dptr(ws), ws.numel(), _lib.stream()), 'skeleton_mdm_forward')

    @property
    def step_chaining(self):
        return False                              # the chained step tail is the split-f16 kernel of the 144-channel model (csrc/tail_h2.h)

    def forward_step(self, x, timesteps, table, state, gt=None, mask=None, y=None, zero_pose_obj=None, memctx=None, ws=None, batch_rows=None, tmap=None):
        """One plain reverse step with the update over all 106 channels inside the heads GEMM (interdiff_skeleton_mdm_forward_step);
        operands as ``mdm.MDM.forward_step``."""
        return self._forward_step(x, timesteps, table, state, gt, mask, y, memctx, ws, batch_rows, 0, z=self._zpo(zero_pose_obj, x.shape[0]), tmap=tmap)

    def _launch_step(self, memctx, x, timesteps, B, T, gt, mask, table, state, ws, flags, z, tmap=None):
        _check(self.lib.interdiff_skeleton_mdm_forward_step_map(C.byref(self.w), C.byref(self.head), _lib.dptr(memctx), _lib.dptr(x, torch.float32),
                                                                _lib.dptr(timesteps, torch.int64), _lib.dptr(z), B, T, _lib.dptr(gt, allow_none=True),
                                                                _lib.dptr(mask, allow_none=True), _lib.dptr(table), _lib.dptr(tmap, torch.int64, allow_none=True),
                                                                _lib.dptr(state), _lib.dptr(ws), ws.numel(), _lib.stream()), 'skeleton_mdm_forward_step')

    def arithmetic_report(self, device_verdicts=True):
        rep = super().arithmetic_report(device_verdicts)
        rep['ff_size'] = self.ff_size
        return rep

    def _get_embeddings(self, body_gt, obj_gt, pose_gt, zero_pose_obj, past_len=10, batch_clips=None):
        """``MDM._get_embeddings`` (model/diffusion_skeleton.py:194-215): body_gt [T,B,21,3], obj_gt [T,B,12,3], pose_gt [T,B,7],
        zero_pose_obj [B,12,3] -> (cond [past_len,B,256], gt [T,B,106])."""
        if not self.w.has_encoder:
            raise RuntimeError('this state_dict has no encoder weights')
        T, B = body_gt.shape[:2]
        z = self._zpo(zero_pose_obj, B)
        gt = torch.cat([body_gt.reshape(T, B, -1).float(), obj_gt.reshape(T, B, -1).float(), pose_gt.float()], dim=2)      # [T,B,106]
        if gt.shape[2] != self.w.C:
            raise ValueError('expected body [T,B,%d,3], obj [T,B,%d,3], pose [T,B,7]' % (self.n_body // 3, self.n_points))
        x_past = gt[:past_len].permute(1, 2, 0).unsqueeze(1).contiguous()                                # [B,1,106,past]
        self._pick_ffn_tile((batch_clips or B) * past_len, B * past_len)
        ws = torch.empty(self.lib.interdiff_skeleton_mdm_encode_workspace_bytes(B, past_len), dtype=torch.uint8, device=self.device)
        cond = torch.empty(past_len, B, _mdm.D, dtype=torch.float32, device=self.device)
        _check(self.lib.interdiff_skeleton_mdm_encode(C.byref(self.w), C.byref(self.head), _lib.dptr(z), _lib.dptr(x_past), B, past_len,
                                                      _lib.dptr(cond), _lib.dptr(ws), ws.numel(), _lib.stream()), 'skeleton_mdm_encode')
        return cond, gt


def sample_once_proj(batch, model, diffusion, obj_model=None, seed=None, past_len=10, device=None, **loop_kw):
    """``sample_once_proj`` of eval_skeleton.py:114-142 (``obj_model=None``: eval_skeleton_no_correction.py's, identity hook).  ``batch``
    = (body [B,T,21,3], obj keypoints [B,T,12,3], pose [B,T,7], zero_pose_obj [B,12,3]) as the dataset yields it; ``obj_model``: a
    ``SkeletonObjProjector`` (or a ready ``HipSkeletonCorrection``).  Returns (obj_pred, body_pred, pose_pred, obj_gt, body_gt, pose_gt),
    each [T,B,*] -- what ``skeleton_metrics`` takes.  ``loop_kw`` goes to ``p_sample_loop`` (``noise=``, ``step_noise=``, ``use_graph=``), or with ``sampler='ddim'`` (+ ``eta=``) to ``ddim_sample_loop``."""
    dev = torch.device(device) if device is not None else model.device
    body_gt, obj_gt, pose_gt = (batch[i].transpose(0, 1).float().to(dev) for i in range(3))
    zero_pose_obj = batch[3].float().to(dev).contiguous()
    cond, gt = model._get_embeddings(body_gt, obj_gt, pose_gt, zero_pose_obj, past_len=past_len)
    gt = gt.permute(1, 2, 0).unsqueeze(1).contiguous()                                                   # [B,1,106,T]
    mask = torch.ones_like(gt, dtype=torch.bool)
    mask[..., past_len:] = False
    kw = {'y': {'cond': cond, 'inpainted_motion': gt, 'inpainting_mask': mask}, 'zero_pose_obj': zero_pose_obj}
    hook = None
    if obj_model is not None:
        hook = obj_model if isinstance(obj_model, HipSkeletonCorrection) else HipSkeletonCorrection(obj_model, device=dev)
    sample = sample_loop(diffusion, model, tuple(gt.shape), clip_denoised=False, model_kwargs=kw, denoised_fn=hook, seed=seed, **loop_kw)
    nb, no = model.n_body, 3 * model.n_points
    body_pred, obj_pred, pose_pred = torch.split(sample.squeeze(1).permute(2, 0, 1).contiguous(), [nb, no, HEAD_POSE], dim=2)
    body_g, obj_g, pose_g = torch.split(gt.squeeze(1).permute(2, 0, 1).contiguous(), [nb, no, HEAD_POSE], dim=2)
    return obj_pred, body_pred, pose_pred, obj_g, body_g, pose_g
