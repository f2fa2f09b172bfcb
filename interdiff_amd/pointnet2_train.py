"""Fine-tuning of the SMPL denoiser's PointNet++ object encoder on the HIP path: the backward of ``PointNet2Encoder.forward`` (model/layers.py:141-175) as
``MDM._get_embeddings`` calls it (model/diffusion_smpl.py:210-211), with ``pcEmbedding`` in ``eval()`` and autograd on -- frozen running statistics, the
regime of ``SkeletonFineTuner`` and ``CorrectionFineTuner``.

    ft = PointNetFineTuner(state_dict)
    pc = ft.encode_saved(obj_points)          # [B,256], the bits of interdiff_pointnet2_encode; keeps the sampling / grouping decisions
    g = ft.grads(d_pc)                        # {reference name: gradient of sum(d_pc * pc)} for the 38 raw tensors (views of ft.grad)
    ...update ft.params...; ft.refold()       # the folded arena the encoder reads, rewritten on the device

The 38 tensors (``POINTNET_PARAM_NAMES``, 113,917 parameters): twelve bias-free 1x1 convolutions, their BatchNorm ``weight`` / ``bias``, and the Linear.
``running_mean`` / ``running_var`` are read and never written; ``num_batches_tracked`` is carried through.  The ``train()`` regime (batch statistics over all 1024
SA1 centres, the backward through them, running-statistic updates) is ``PointNetTrainer`` below (csrc/pointnet2_bn_train.hip):

    tr = PointNetTrainer(state_dict)
    pc = tr.forward(obj_points)               # [B,256] under batch statistics; keeps the grouping of every centre and the statistics
    g = tr.grads(d_pc)                        # the 38 gradients THROUGH the statistics
    ...update tr.params...; tr.update_running_stats(); tr.refold()     # the eval pack then carries the moved statistics, as the reference's eval() does

NOT built: a gradient with respect to ``obj_points``, caching FPS results across steps, parity with the real ``pointnet2_ops`` (oracle/pointnet2.py).  All
arithmetic is in libinterdiff_hip.so (csrc/pointnet2.hip, csrc/pointnet2_train.hip, csrc/pointnet2_bn_train.hip); torch holds the memory.
"""
import ctypes as C
import torch
from . import _lib, flat_trainer
from .mdm import pack_pointnet2

PREFIX = 'pcEmbedding'


def _layers(prefix=PREFIX):
    return ['%s.SA_modules.%d.mlps.%d' % (prefix, si, sc) for si in range(2) for sc in range(2)]


def pointnet_param_names(prefix=PREFIX):
    """The 38 trained names in the order of the flat vectors (include/interdiff_hip.h, interdiff_pointnet2_finetune_param_table)."""
    names = []
    for q in _layers(prefix):
        for l in range(3):
            names += ['%s.%d.weight' % (q, 3 * l), '%s.%d.weight' % (q, 3 * l + 1), '%s.%d.bias' % (q, 3 * l + 1)]
    return names + [prefix + '.Linear.weight', prefix + '.Linear.bias']


def pointnet_stat_names(prefix=PREFIX):
    """running_mean / running_var of the twelve BatchNorm sites in the order of the ``stats`` vector."""
    return [n for q in _layers(prefix) for l in range(3) for n in ('%s.%d.running_mean' % (q, 3 * l + 1), '%s.%d.running_var' % (q, 3 * l + 1))]


POINTNET_PARAM_NAMES = tuple(pointnet_param_names())
POINTNET_STAT_NAMES = tuple(pointnet_stat_names())


def param_table():
    """(offsets, sizes, n_param) of the 38 tensors as the library lays them out."""
    return flat_trainer.param_table('interdiff_pointnet2_finetune_param_table', len(POINTNET_PARAM_NAMES))


class PointNetFineTuner(flat_trainer.FlatParams):
    """``state_dict``: any dict that holds the reference's ``pcEmbedding.*``.  ``params`` / ``grad``: views of a larger flat master / gradient vector to work on
    (``DenoiserTrainer`` passes the tail of its own); by default the tuner owns both.  ``state_dict()`` gives ``pcEmbedding.*`` under the reference's names: the
    38 trained tensors (copies) and every other entry (running statistics, ``num_batches_tracked``) with the bits it came in with."""

    def __init__(self, state_dict, device='cuda', params=None, grad=None):
        self.lib = _lib.load()
        self.device = torch.device(device)
        sd = {k: torch.as_tensor(v).detach().clone() for k, v in state_dict.items() if k.startswith(PREFIX + '.')}
        flat = self._intake(sd, POINTNET_PARAM_NAMES, param_table(), also=POINTNET_STAT_NAMES)
        if params is None:
            self.params = flat.contiguous()
        else:
            self.params = params
            self.params.copy_(flat)
        self.grad = torch.zeros_like(self.params) if grad is None else grad
        if self.params.numel() != self.n_param or self.grad.numel() != self.n_param or not (self.params.is_contiguous() and self.grad.is_contiguous()):
            raise ValueError('params / grad must be contiguous vectors of %d floats' % self.n_param)
        self.stats = torch.cat([sd[k].reshape(-1).float() for k in POINTNET_STAT_NAMES]).to(self.device).contiguous()
        self.pn, self.arena = pack_pointnet2(sd, self.device)
        self._saves = self._points = None
        self._ws = {}

    def encode_saved(self, obj_points):
        """``pc_embedding`` [B,256] of ``obj_points`` [B,P,3] (P <= 2048) with the record the backward reads (``interdiff_pointnet2_encode_saved``)."""
        pts = obj_points.to(self.device).contiguous().float()
        if pts.dim() != 3 or pts.shape[2] != 3:
            raise ValueError('obj_points must be [B,P,3]')
        B = pts.shape[0]
        need = self.lib.interdiff_pointnet2_saves_bytes(B)
        if self._saves is None or self._saves.numel() != need:
            self._saves = torch.empty(need, dtype=torch.uint8, device=self.device)
        pc = torch.empty(B, 256, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.interdiff_pointnet2_encode_saved(C.byref(self.pn), _lib.dptr(pts), B, pts.shape[1], _lib.dptr(pc), _lib.dptr(self._saves), need, _lib.stream()),
                   'pointnet2_encode_saved')
        self._points = pts
        return pc

    def saves(self):
        """The last record as int32 [B,7156] (layout: csrc/pointnet2_train.h); its last 48 x 96 words are floats."""
        return self._saves.view(torch.int32).view(self._points.shape[0], -1)

    def grads(self, d_pc, flat=False):
        """Gradient of ``sum(d_pc * pc)`` of the last ``encode_saved`` with respect to the 38 raw tensors: a dict by reference name (views of ``self.grad``, valid
        until the next call), or the flat vector itself."""
        if self._points is None:
            raise RuntimeError('grads() follows encode_saved()')
        B = self._points.shape[0]
        d_pc = d_pc.to(self.device).contiguous().float()
        if tuple(d_pc.shape) != (B, 256):
            raise ValueError('d_pc must be [B,256] of the last encode_saved')
        ws = self._ws.get(B)
        if ws is None:
            ws = self._ws[B] = torch.empty(self.lib.interdiff_pointnet2_finetune_workspace_bytes(B), dtype=torch.uint8, device=self.device)
        _lib.check(self.lib.interdiff_pointnet2_finetune_grads(C.byref(self.pn), _lib.dptr(self.params), _lib.dptr(self.stats), _lib.dptr(self._points), B, self._points.shape[1],
                                                               _lib.dptr(self._saves), _lib.dptr(d_pc), _lib.dptr(self.grad), _lib.dptr(ws), ws.numel(), _lib.stream()),
                   'pointnet2_finetune_grads')
        return self.grad if flat else self.named_views(self.grad)

    def refold(self):
        """Rewrite the folded arena ``encode_saved`` reads from the current ``params`` (``interdiff_pointnet2_refold``: on the stream, no host round trip)."""
        _lib.check(self.lib.interdiff_pointnet2_refold(C.byref(self.pn), _lib.dptr(self.params), _lib.dptr(self.stats), _lib.stream()), 'pointnet2_refold')


MAX_POINTS, MAX_CLIPS, MOMENTUM = 2048, 256, 0.1


class PointNetTrainer(PointNetFineTuner):
    """``pcEmbedding`` in ``train()``: the twelve BatchNorm2d sites normalise with the statistics of the batch, the backward runs through those statistics, and
    ``update_running_stats`` moves ``running_mean`` / ``running_var`` / ``num_batches_tracked`` (momentum 0.1, unbiased variance).  Intake, views and the eval pack
    (``encode_saved``, ``refold``) are the fine-tuner's; ``state_dict()`` returns the 38 tensors, the 24 moved statistics and the twelve counters (int64) under the
    reference's names."""

    def __init__(self, state_dict, device='cuda', params=None, grad=None):
        super().__init__(state_dict, device, params, grad)
        self._tracked = [k[:-len('running_mean')] + 'num_batches_tracked' for k in POINTNET_STAT_NAMES[::2]]
        self.num_batches_tracked = [int(self._passthrough[k]) if k in self._passthrough else 0 for k in self._tracked]
        self._train_points = self._train_ws = None

    def forward(self, obj_points):
        """``pc_embedding`` [B,256] of ``obj_points`` [B,P,3] (P <= 2048, B <= 256) under batch statistics (``interdiff_pointnet2_train_forward``)."""
        pts = obj_points.to(self.device).contiguous().float()
        if pts.dim() != 3 or pts.shape[2] != 3:
            raise ValueError('obj_points must be [B,P,3]')
        B, P = pts.shape[0], pts.shape[1]
        if not (1 <= P <= MAX_POINTS and 1 <= B <= MAX_CLIPS):
            raise ValueError('PointNetTrainer supports 1 <= P <= %d points and 1 <= B <= %d clips (got P=%d, B=%d)' % (MAX_POINTS, MAX_CLIPS, P, B))
        ws = self._ws.get(('train', B))
        if ws is None:
            ws = self._ws[('train', B)] = torch.empty(self.lib.interdiff_pointnet2_train_workspace_bytes(B), dtype=torch.uint8, device=self.device)
        pc = torch.empty(B, 256, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.interdiff_pointnet2_train_forward(_lib.dptr(self.params), _lib.dptr(pts), B, P, _lib.dptr(pc), _lib.dptr(ws), ws.numel(), _lib.stream()),
                   'pointnet2_train_forward')
        self._train_points, self._train_ws = pts, ws
        return pc

    def grads(self, d_pc, flat=False):
        """Gradient of ``sum(d_pc * pc)`` of the last ``forward`` with respect to the 38 raw tensors, through the batch statistics."""
        if self._train_points is None:
            raise RuntimeError('grads() follows forward()')
        pts, ws = self._train_points, self._train_ws
        d_pc = d_pc.to(self.device).contiguous().float()
        if tuple(d_pc.shape) != (pts.shape[0], 256):
            raise ValueError('d_pc must be [B,256] of the last forward')
        _lib.check(self.lib.interdiff_pointnet2_train_grads(_lib.dptr(self.params), _lib.dptr(pts), pts.shape[0], pts.shape[1], _lib.dptr(d_pc), _lib.dptr(self.grad),
                                                            _lib.dptr(ws), ws.numel(), _lib.stream()), 'pointnet2_train_grads')
        return self.grad if flat else self.named_views(self.grad)

    def update_running_stats(self, momentum=MOMENTUM):
        """What one train-mode forward does to the 24 running statistics and the twelve counters (``interdiff_pointnet2_train_stats``), from the last ``forward``."""
        if self._train_points is None:
            raise RuntimeError('update_running_stats() follows forward()')
        _lib.check(self.lib.interdiff_pointnet2_train_stats(_lib.dptr(self._train_ws), self._train_points.shape[0], float(momentum), _lib.dptr(self.stats), _lib.stream()),
                   'pointnet2_train_stats')
        self.num_batches_tracked = [n + 1 for n in self.num_batches_tracked]

    def state_dict(self):
        out = super().state_dict()
        at = 0
        for k in POINTNET_STAT_NAMES:
            n = out[k].numel()
            out[k] = self.stats[at:at + n].clone().view(out[k].shape)
            at += n
        out.update({k: torch.tensor(n, dtype=torch.int64) for k, n in zip(self._tracked, self.num_batches_tracked)})
        return out
