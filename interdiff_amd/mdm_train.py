"""Training of the SMPL denoiser's decoder on the HIP path: the backward of ``MDM.forward(x, timesteps, y)`` (model/diffusion_smpl.py:226-246)
under the loss of ``LitInteraction.forward_backward`` (train_diffusion_smpl.py:60-166), and AdamW (:177-183).

    DenoiserTrainer(state_dict).training_step(batch)      one optimiser step: q_sample, forward with saves, the 16 terms, backward, AdamW

Scope: the 144 tensors ``MDM.forward`` reads (``PARAM_NAMES``: bodyEmbedding, objEmbedding, the timestep MLP, the eight decoder layers, the two
output heads; 7,069,900 parameters).  ``finalLinear.*``, ``bodyFutureEmbedding`` / ``objFutureEmbedding``, ``PositionalEmbedding.pe`` and every
``encoder.*`` / ``pcEmbedding.*`` tensor are carried through unchanged and get no gradient.  ``cond`` is an INPUT of this pass: its gradient
``d_cond [mem_len,B,256]`` is returned as the seam a later backward of ``MDM._get_embeddings`` (encoder, PointNet++) will take.  bodyEmbedding /
objEmbedding are shared with the encoder; their gradient here is the decoder path's alone, which equals the reference's autograd with
``y['cond']`` detached.

The reference trains with ``--dropout 0`` and ``--cond_mask_prob 0`` and runs ``stochastic_depth`` at rate 0, so ``train()`` and ``eval()`` compute
the same function; a configuration with dropout or condition masking is refused.  All arithmetic is in libinterdiff_hip.so (csrc/mdm_train.h):
exact fp32, no float atomics -- two calls give the same bits.  torch holds the device memory.  The flat vectors, the state-dict round trip, the workspace
cache and the model-independent half of a step are ``flat_trainer.FlatAdamWTrainer``'s; this module supplies the names, the three modes' batch handling and
gradient calls, and ``export_mdm``.

``DenoiserTrainer(state_dict, train_encoder=True)`` closes the ``d_cond`` seam: the pass then covers ``MDM._get_embeddings`` from ``pc_embedding`` on
(model/diffusion_smpl.py:217-221: the shared input embeddings on the past frames, ``pc_embedding``, the positional rows, the eight ``encoder.layers.*``), as
``LitInteraction._common_step`` (train_diffusion_smpl.py:381-388) has it with autograd on.  The 84 encoder tensors (``ENCODER_PARAM_NAMES``; 4,754,492
parameters) follow the 144 in the flat vectors, bodyEmbedding / objEmbedding receive the sum of both paths, and a batch carries ``pc`` [B,256] or raw
``obj_points`` [B,P,3] instead of ``cond``.  ``pc_embedding`` is the new input seam: ``d_pc`` [B,256] is returned, ``pcEmbedding.*`` is carried through.

``DenoiserTrainer(state_dict, train_encoder=True, train_pointnet=True)`` closes the ``d_pc`` seam too: ``pcEmbedding`` (the PointNet++ object encoder,
model/diffusion_smpl.py:210-211) is trained with frozen normalisation statistics -- the module in ``eval()`` with autograd on (interdiff_amd/pointnet2_train.py says
what that regime is and what is not built).  Its 38 tensors (``POINTNET_PARAM_NAMES``; 113,917 parameters) follow the 228 in the flat vectors, a batch carries raw
``obj_points`` [B,P,3] (never ``pc`` or ``cond``: their gradient could not reach the points), and one ``training_step`` is: encode with saves, the full pass, the
PointNet++ backward on its ``d_pc``, AdamW over all 266 tensors, the device re-fold of eval BatchNorm -- so the encoder's pack is never stale.

``pointnet_mode='train'`` (with ``train_pointnet``) is the reference's own regime: Lightning puts the whole model in ``train()``, so ``pcEmbedding`` normalises with
batch statistics, back-propagates through them and moves its running statistics (``PointNetTrainer``).  One ``training_step`` is then: the train-mode forward, the
full pass, the train-mode backward, AdamW over all 266 tensors, the statistics update, the re-fold.  ``encode_points`` (validation, the sampler, ``export_mdm``) goes
on reading the eval pack, which now carries the moved statistics, as the reference's ``eval()`` does; ``state_dict()`` carries them too.  The default ``'eval'`` is
the frozen regime above, bit for bit.
"""
import ctypes as C
import torch
from . import _lib, flat_trainer
from .eval import as_clip_batch
from .flat_trainer import MAX_T, MAX_MEM
from .losses import LOSS_KEYS, LossWeights
from .mdm import MDM
from .pointnet2_train import POINTNET_PARAM_NAMES, PointNetFineTuner, PointNetTrainer, param_table as pointnet_param_table

QAN_LAYERS = (1, 2, 3, 4, 5, 6)


def param_names():
    """The 144 state_dict names in the order of the flat master vector (include/interdiff_hip.h, PARAMETER TABLE)."""
    wb = lambda p: [p + '.weight', p + '.bias']
    names = wb('bodyEmbedding') + wb('objEmbedding') + wb('embedTimeStep.time_embed.0') + wb('embedTimeStep.time_embed.2')
    for l in range(8):
        p = 'decoder.layers.%d.' % l
        if l in QAN_LAYERS:
            names += [p + 'queries', p + 'wk']
        else:
            names += [p + 'self_attn.in_proj_weight', p + 'self_attn.in_proj_bias'] + wb(p + 'self_attn.out_proj')
        names += [p + 'multihead_attn.in_proj_weight', p + 'multihead_attn.in_proj_bias'] + wb(p + 'multihead_attn.out_proj')
        names += wb(p + 'linear1') + wb(p + 'linear2') + wb(p + 'norm1') + wb(p + 'norm2') + wb(p + 'norm3')
    return names + wb('bodyFinalLinear') + wb('objFinalLinear')


PARAM_NAMES = tuple(param_names())


def encoder_param_names():
    """The 84 ``encoder.layers.*`` names in the order they follow the 144 in the flat vectors (include/interdiff_hip.h, FULL PARAMETER TABLE)."""
    wb = lambda p: [p + '.weight', p + '.bias']
    names = []
    for l in range(8):
        p = 'encoder.layers.%d.' % l
        if l in QAN_LAYERS:
            names += [p + 'queries', p + 'wk']
        else:
            names += [p + 'self_attn.in_proj_weight', p + 'self_attn.in_proj_bias'] + wb(p + 'self_attn.out_proj')
        names += wb(p + 'linear1') + wb(p + 'linear2') + wb(p + 'norm1') + wb(p + 'norm2')
    return names


ENCODER_PARAM_NAMES = tuple(encoder_param_names())
FULL_PARAM_NAMES = PARAM_NAMES + ENCODER_PARAM_NAMES


def param_table(full=False):
    """(offsets, sizes, n_param) of the flat vectors as the library lays them out (``interdiff_mdm_train_param_table``; ``full``: the 228 tensors of
    ``interdiff_mdm_train_full_param_table``)."""
    return flat_trainer.param_table('interdiff_mdm_train_full_param_table' if full else 'interdiff_mdm_train_param_table', len(FULL_PARAM_NAMES if full else PARAM_NAMES))


class DenoiserTrainer(flat_trainer.FlatAdamWTrainer):
    """``loss.backward()`` + ``optimizer.step()`` of the reference's diffusion trainer for the SMPL denoiser (the scaffold: interdiff_amd/flat_trainer.py).

    ``state_dict``: the reference ``MDM``'s (tensors or arrays).  ``dropout`` / ``cond_mask_prob``: the configuration the checkpoint was made
    for; anything but 0 raises (not built).  ``weights`` / ``past_len``: the loss of ``forward_backward``; ``n_steps``: the cosine schedule's length.
    ``train_encoder``: the 84 encoder tensors are trained too (module docstring); a batch then carries ``pc`` or ``obj_points``, never ``cond``.
    ``train_pointnet`` (needs ``train_encoder``): the 38 ``pcEmbedding.*`` tensors are trained too, running statistics frozen; a batch carries ``obj_points``.
    ``pointnet_mode``: ``'eval'`` (that frozen regime) or ``'train'`` (needs ``train_pointnet``): batch statistics, the backward through them, running statistics moved.
    ``state_dict()`` returns the trained tensors (144, 228 or 266) and every other tensor of the constructor's state_dict exactly as it came in.

    ``loss_and_grads`` returns, behind the four common elements, ``d_cond`` [mem_len,B,256] and, with ``train_encoder``, ``d_pc`` [B,256]; ``self.cond`` then
    keeps the conditioning the step computed.
    """

    LOSS_KEYS, C_TOK = LOSS_KEYS, 144
    # per mode (train_encoder, train_pointnet): the one argument of cond / pc / obj_points that grads_at takes, its form for the refusal, and the names of the
    # methods that turn a batch into (gt, that argument) and that compute the gradients from it
    MODES = {
        (False, False): (('cond',), 'grads_at(x_t, t, cond, target)', '_decoder_inputs', '_decoder_grads'),
        (True, False): (('cond', 'pc'), 'train_encoder=True: grads_at(x_t, t, pc [B,256], target)', '_encoder_inputs', '_full_grads'),
        (True, True): (('obj_points',), 'train_pointnet=True: grads_at(x_t, t, target=target, obj_points=obj_points [B,P,3])', '_pointnet_inputs', '_pointnet_grads'),
    }

    def __init__(self, state_dict, device='cuda', lr=3e-4, weight_decay=0.0, betas=(0.9, 0.999), eps=1e-8, weights=LossWeights(), past_len=10, n_steps=1000,
                 dropout=0.0, cond_mask_prob=0.0, train_encoder=False, train_pointnet=False, pointnet_mode='eval'):
        if train_pointnet and not train_encoder:
            raise ValueError('train_pointnet=True needs train_encoder=True: the gradient reaches pcEmbedding through the encoder')
        if pointnet_mode not in ('eval', 'train'):
            raise ValueError("pointnet_mode must be 'eval' or 'train'")
        if pointnet_mode == 'train' and not train_pointnet:
            raise ValueError("pointnet_mode='train' needs train_pointnet=True: batch statistics are the regime of a trained pcEmbedding")
        self.train_encoder, self.train_pointnet, self.pointnet_mode = bool(train_encoder), bool(train_pointnet), pointnet_mode
        self._takes, self._form, inputs, grads = self.MODES[self.train_encoder, self.train_pointnet]
        self._inputs, self._grads = getattr(self, inputs), getattr(self, grads)
        names, table = (FULL_PARAM_NAMES if self.train_encoder else PARAM_NAMES), param_table(self.train_encoder)
        n_mdm = table[2]
        if self.train_pointnet:                                      # the 38 follow the 228
            names, table = names + POINTNET_PARAM_NAMES, flat_trainer.append_table(table, pointnet_param_table())
        super().__init__(state_dict, names, table, device, lr, weight_decay, betas, eps, weights, past_len, n_steps, dropout, cond_mask_prob)
        self._mdm, self._pn, self.pointnet = None, None, None
        if self.train_pointnet:
            tuner = PointNetTrainer if pointnet_mode == 'train' else PointNetFineTuner
            self.pointnet = tuner(state_dict, self.device, params=self.params[n_mdm:], grad=self.grads[n_mdm:])
            self.after_step = self._after_train_step if pointnet_mode == 'train' else self.pointnet.refold       # so the encoder's pack is never stale

    def export_mdm(self):
        """An ``interdiff_amd.mdm.MDM`` packed (on the host, ``pack_mdm_weights``) from the current weights: for sampling and ``validation_step``.
        Without ``train_encoder`` it is also the model a batch WITHOUT ``cond`` gets its conditioning from, so that conditioning lags the shared
        embeddings (and the untrained encoder stays what it was) until the next ``export_mdm()``.  With ``train_encoder`` the trained encoder is
        re-packed too, and no training batch reads this model: the trainer computes ``cond`` itself, from the current weights."""
        self._mdm = MDM({k: v.cpu() for k, v in self.state_dict().items()}, device=self.device, n_steps=self.n_steps)
        return self._mdm

    def loss_grad(self, pred, target):
        """``interdiff_denoising_loss_grad``: d/d pred of mean_b sum_i w_i term_i[b]."""
        B, T = pred.shape[0], pred.shape[-1]
        d = torch.empty_like(pred)
        _lib.check(self.lib.interdiff_denoising_loss_grad(_lib.dptr(pred.contiguous(), torch.float32), _lib.dptr(target.contiguous(), torch.float32), B, T, self.past_len,
                                                          self._wvec, _lib.dptr(d), _lib.stream()), 'denoising_loss_grad')
        return d

    def grads_at(self, x_t, t, cond=None, target=None, d_pred=None, pc=None, obj_points=None):
        """One forward with saves and the backward on given x_t: (pred, terms [16,B], d_cond); the flat gradient lands in ``self.grads``.
        With ``train_encoder`` it is ``grads_at(x_t, t, pc, target, d_pred=None)``: the third argument (or ``pc=``) is ``pc`` [B,256] and the result is
        (pred, terms, d_cond, d_pc [B,256]); ``self.cond`` [past_len,B,256] keeps the encoder's output.  With ``train_pointnet`` it is
        ``grads_at(x_t, t, target=target, obj_points=obj_points)``: ``pc`` is encoded from the raw points with saves, and the PointNet++ backward fills the
        last 113,917 entries of ``self.grads`` from ``d_pc``; the result is the same 4-tuple."""
        given = [(k, v) for k, v in (('cond', cond), ('pc', pc), ('obj_points', obj_points)) if v is not None]
        if target is None or len(given) != 1 or given[0][0] not in self._takes:
            raise ValueError(self._form)
        return self._grads(x_t, t, given[0][1], target, d_pred)

    # ---- decoder only: cond [mem_len,B,256] is an input
    def _decoder_inputs(self, batch):
        if not (isinstance(batch, dict) and 'cond' in batch):        # the conditioning of the lazily exported model (export_mdm)
            if self._mdm is None:
                self.export_mdm()
            batch = as_clip_batch(self._mdm, batch, self.past_len)
        return batch['gt'], batch['cond']

    def _decoder_grads(self, x_t, t, cond, target, d_pred):
        x_t, target, d_pred, B, T = self._checked(x_t, target, d_pred)
        cond, S = cond.contiguous(), cond.shape[0]
        if tuple(cond.shape[1:]) != (B, 256):
            raise ValueError('cond must be [mem_len,B,256]')
        if S > MAX_MEM:
            raise ValueError('DenoiserTrainer supports mem_len <= %d (got %d)' % (MAX_MEM, S))
        ws = self._workspace(self.lib.interdiff_mdm_train_workspace_bytes, B, T, S)
        pred, terms, d_cond = torch.empty_like(x_t), torch.empty(16, B, dtype=torch.float32, device=self.device), torch.empty_like(cond)
        _lib.check(self.lib.interdiff_mdm_train_grads(
            _lib.dptr(self.params), _lib.dptr(self.pe), self.pe.shape[0], _lib.dptr(x_t, torch.float32), _lib.dptr(t.to(self.device).contiguous(), torch.int64),
            _lib.dptr(cond, torch.float32), _lib.dptr(target, torch.float32), B, T, S, self.past_len, self._wvec, _lib.dptr(d_pred, torch.float32, allow_none=True),
            _lib.dptr(self.grads), _lib.dptr(d_cond), _lib.dptr(pred), _lib.dptr(terms), _lib.dptr(ws), ws.numel(), _lib.stream()), 'mdm_train_grads')
        return pred, terms, d_cond

    # ---- train_encoder: pc [B,256] is the input, cond is computed
    def _encoder_inputs(self, batch):
        if isinstance(batch, dict) and 'cond' in batch:
            raise ValueError('train_encoder=True: a batch that carries cond cannot reach the encoder; pass pc [B,256] or obj_points [B,P,3]')
        if not isinstance(batch, dict) or 'gt' not in batch or not ('pc' in batch or 'obj_points' in batch):
            raise ValueError('train_encoder=True takes a clip batch with gt [B,1,144,T] and pc [B,256] or obj_points [B,P,3]')
        return batch['gt'], (batch['pc'] if 'pc' in batch else self.encode_points(batch['obj_points']))

    def _full_grads(self, x_t, t, pc, target, d_pred):
        x_t, target, d_pred, B, T = self._checked(x_t, target, d_pred)
        pc, S = pc.contiguous(), self.past_len
        if tuple(pc.shape) != (B, 256):
            raise ValueError('pc must be [B,256]')
        ws = self._workspace(self.lib.interdiff_mdm_train_full_workspace_bytes, B, T, S)
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=self.device)
        pred, terms, cond, d_cond, d_pc = torch.empty_like(x_t), new(16, B), new(S, B, 256), new(S, B, 256), new(B, 256)
        _lib.check(self.lib.interdiff_mdm_train_full_grads(
            _lib.dptr(self.params), _lib.dptr(self.pe), self.pe.shape[0], _lib.dptr(x_t, torch.float32), _lib.dptr(t.to(self.device).contiguous(), torch.int64),
            _lib.dptr(pc, torch.float32), _lib.dptr(target, torch.float32), B, T, S, self._wvec, _lib.dptr(d_pred, torch.float32, allow_none=True),
            _lib.dptr(self.grads), _lib.dptr(cond), _lib.dptr(d_cond), _lib.dptr(d_pc), _lib.dptr(pred), _lib.dptr(terms), _lib.dptr(ws), ws.numel(), _lib.stream()),
            'mdm_train_full_grads')
        self.cond = cond
        return pred, terms, d_cond, d_pc

    # ---- train_pointnet: raw obj_points [B,P,3] are the input (pc or cond could not carry a gradient to the points)
    def _pointnet_inputs(self, batch):
        if isinstance(batch, dict) and ('cond' in batch or 'pc' in batch):
            raise ValueError('train_pointnet=True: a batch that carries cond or pc cannot reach the points; pass raw obj_points [B,P,3]')
        if not isinstance(batch, dict) or 'gt' not in batch or 'obj_points' not in batch:
            raise ValueError('train_pointnet=True takes a clip batch with gt [B,1,144,T] and obj_points [B,P,3]')
        return batch['gt'], batch['obj_points']

    def _after_train_step(self):
        self.pointnet.update_running_stats()
        self.pointnet.refold()

    def state_dict(self):
        out = super().state_dict()
        if self.pointnet_mode == 'train':                            # the moved statistics and counters
            moved = self.pointnet.state_dict()
            out.update({k: moved[k] for k in moved if k not in self.names})
        return out

    def _pointnet_grads(self, x_t, t, obj_points, target, d_pred):
        pc = self.pointnet.forward(obj_points) if self.pointnet_mode == 'train' else self.pointnet.encode_saved(obj_points)
        out = self._full_grads(x_t, t, pc, target, d_pred)
        self.pointnet.grads(out[3], flat=True)
        return out

    def encode_points(self, obj_points):
        """``pc_embedding`` [B,256] of raw ``obj_points`` [B,P,3]: ``interdiff_pointnet2_encode`` on a pack made once from the constructor's
        ``pcEmbedding.*`` (frozen, so the pack is never stale).  With ``train_pointnet``: on the trained tensors' pack, which every optimiser step re-folds."""
        from .mdm import pack_pointnet2
        if self.train_pointnet:
            return self._encode(self.pointnet.pn, obj_points)
        if self._pn is None:
            if 'pcEmbedding.Linear.weight' not in self._passthrough:
                raise KeyError('state_dict lacks pcEmbedding.*: pass pc [B,256] instead of obj_points')
            self._pn = pack_pointnet2(self._passthrough, self.device)
        return self._encode(self._pn[0], obj_points)

    def _encode(self, pn, obj_points):
        pts = obj_points.to(self.device).contiguous().float()
        pc = torch.empty(pts.shape[0], 256, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.interdiff_pointnet2_encode(C.byref(pn), _lib.dptr(pts), pts.shape[0], pts.shape[1], _lib.dptr(pc), _lib.stream()), 'pointnet2_encode')
        return pc
