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
exact fp32, no float atomics -- two calls give the same bits.  torch holds the device memory.

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
"""
import ctypes as C
import torch
from . import _lib
from .diffusion import create_gaussian_diffusion
from .eval import as_clip_batch
from .losses import LOSS_KEYS, LossWeights
from .mdm import MDM, positional_table
from .pointnet2_train import POINTNET_PARAM_NAMES, PointNetFineTuner, param_table as pointnet_param_table

MAX_T, MAX_MEM = 128, 16
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
    n = len(FULL_PARAM_NAMES if full else PARAM_NAMES)
    off, size, cnt, total = (C.c_int64 * n)(), (C.c_int64 * n)(), C.c_int32(0), C.c_int64(0)
    entry = _lib.load().interdiff_mdm_train_full_param_table if full else _lib.load().interdiff_mdm_train_param_table
    _lib.check(entry(off, size, C.byref(cnt), C.byref(total)), 'mdm_train_param_table')
    if cnt.value != n:
        raise RuntimeError('parameter table: %d tensors, expected %d' % (cnt.value, n))
    return list(off), list(size), int(total.value)


class DenoiserTrainer:
    """``loss.backward()`` + ``optimizer.step()`` of the reference's diffusion trainer for the decoder side of the SMPL denoiser.

    ``state_dict``: the reference ``MDM``'s (tensors or arrays).  ``dropout`` / ``cond_mask_prob``: the configuration the checkpoint was made
    for; anything but 0 raises (not built).  ``weights`` / ``past_len``: the loss of ``forward_backward``; ``n_steps``: the cosine schedule's length.
    ``train_encoder``: the 84 encoder tensors are trained too (module docstring); a batch then carries ``pc`` or ``obj_points``, never ``cond``.
    ``train_pointnet`` (needs ``train_encoder``): the 38 ``pcEmbedding.*`` tensors are trained too, running statistics frozen; a batch carries ``obj_points``.
    """

    def __init__(self, state_dict, device='cuda', lr=3e-4, weight_decay=0.0, betas=(0.9, 0.999), eps=1e-8, weights=LossWeights(), past_len=10, n_steps=1000,
                 dropout=0.0, cond_mask_prob=0.0, train_encoder=False, train_pointnet=False):
        if dropout > 0 or cond_mask_prob > 0:
            raise ValueError('DenoiserTrainer implements the reference defaults --dropout 0 --cond_mask_prob 0 only')
        if train_pointnet and not train_encoder:
            raise ValueError('train_pointnet=True needs train_encoder=True: the gradient reaches pcEmbedding through the encoder')
        self.lib = _lib.load()
        self.device = torch.device(device)
        self.lr, self.weight_decay, self.betas, self.eps = float(lr), float(weight_decay), (float(betas[0]), float(betas[1])), float(eps)
        self.weights, self.past_len, self.n_steps = weights, int(past_len), int(n_steps)
        self.diffusion = create_gaussian_diffusion('cosine', self.n_steps)
        sd = {k: torch.as_tensor(v).detach().clone() for k, v in state_dict.items()}
        self.train_encoder, self.train_pointnet = bool(train_encoder), bool(train_pointnet)
        self.names = FULL_PARAM_NAMES if self.train_encoder else PARAM_NAMES
        if self.train_pointnet:
            self.names = self.names + POINTNET_PARAM_NAMES
        missing = [k for k in self.names if k not in sd]
        if missing:
            raise KeyError('state_dict lacks %s' % missing[:3])
        self.offsets, self.sizes, self.n_param = param_table(self.train_encoder)
        if self.train_pointnet:                                      # the 38 follow the 228
            off, size, n = pointnet_param_table()
            self.offsets, self.sizes, self.n_param, self._n_mdm = self.offsets + [self.n_param + o for o in off], self.sizes + size, self.n_param + n, self.n_param
        self.shapes = [tuple(sd[k].shape) for k in self.names]
        for k, s, shp in zip(self.names, self.sizes, self.shapes):
            if sd[k].numel() != s:
                raise ValueError('%s: %s does not match the parameter table (%d floats)' % (k, shp, s))
        self._passthrough = {k: v for k, v in sd.items() if k not in self.names}         # returned by state_dict() with identical bits
        self.params = torch.cat([sd[k].reshape(-1).float() for k in self.names]).to(self.device).contiguous()
        self.exp_avg, self.exp_avg_sq = torch.zeros_like(self.params), torch.zeros_like(self.params)
        self.grads = torch.zeros_like(self.params)
        self.step = 0
        pe = sd['PositionalEmbedding.pe'][:, 0] if 'PositionalEmbedding.pe' in sd else positional_table()
        self.pe = torch.as_tensor(pe).float().to(self.device).contiguous()
        self._w16 = (C.c_float * 16)(*weights.vector())
        self._wdev = torch.tensor(weights.vector(), dtype=torch.float32, device=self.device)
        self._ws, self._mdm, self._pn = {}, None, None
        self.cond = None                                             # encoder mode: the conditioning the last gradient call computed
        self.pointnet = PointNetFineTuner(sd, self.device, params=self.params[self._n_mdm:], grad=self.grads[self._n_mdm:]) if self.train_pointnet else None

    # ------------------------------------------------------------------------------------------------------------ state
    def named_views(self, flat):
        return {k: flat[o:o + s].view(shp) for k, o, s, shp in zip(self.names, self.offsets, self.sizes, self.shapes)}

    def state_dict(self):
        """The reference's names: the trained tensors (144, or 228 with ``train_encoder``; copies, on the trainer's device) and every other tensor of
        the constructor's state_dict exactly as it came in."""
        out = dict(self._passthrough)
        out.update({k: v.clone() for k, v in self.named_views(self.params).items()})
        return out

    def optimizer_state(self):
        return dict(step=self.step, exp_avg=self.exp_avg.clone(), exp_avg_sq=self.exp_avg_sq.clone())

    def load_optimizer_state(self, state):
        self.step = int(state['step'])
        self.exp_avg.copy_(state['exp_avg'])
        self.exp_avg_sq.copy_(state['exp_avg_sq'])

    def export_mdm(self):
        """An ``interdiff_amd.mdm.MDM`` packed (on the host, ``pack_mdm_weights``) from the current weights: for sampling and ``validation_step``.
        Without ``train_encoder`` it is also the model a batch WITHOUT ``cond`` gets its conditioning from, so that conditioning lags the shared
        embeddings (and the untrained encoder stays what it was) until the next ``export_mdm()``.  With ``train_encoder`` the trained encoder is
        re-packed too, and no training batch reads this model: the trainer computes ``cond`` itself, from the current weights."""
        self._mdm = MDM({k: v.cpu() for k, v in self.state_dict().items()}, device=self.device, n_steps=self.n_steps)
        return self._mdm

    # ------------------------------------------------------------------------------------------------------------ steps
    def _workspace(self, B, T, S):
        need = (self.lib.interdiff_mdm_train_full_workspace_bytes if self.train_encoder else self.lib.interdiff_mdm_train_workspace_bytes)(B, T, S)
        if need == 0:
            raise ValueError('unsupported shape B=%d T=%d mem_len=%d' % (B, T, S))
        ws = self._ws.get((B, T, S))
        if ws is None:
            ws = self._ws[(B, T, S)] = torch.empty(need, dtype=torch.uint8, device=self.device)
        return ws

    def loss_grad(self, pred, target):
        """``interdiff_denoising_loss_grad``: d/d pred of mean_b sum_i w_i term_i[b]."""
        B, T = pred.shape[0], pred.shape[-1]
        d = torch.empty_like(pred)
        _lib.check(self.lib.interdiff_denoising_loss_grad(_lib.dptr(pred.contiguous(), torch.float32), _lib.dptr(target.contiguous(), torch.float32), B, T, self.past_len,
                                                          self._w16, _lib.dptr(d), _lib.stream()), 'denoising_loss_grad')
        return d

    def grads_at(self, x_t, t, cond=None, target=None, d_pred=None, pc=None, obj_points=None):
        """One forward with saves and the backward on given x_t: (pred, terms [16,B], d_cond); the flat gradient lands in ``self.grads``.
        With ``train_encoder`` it is ``grads_at(x_t, t, pc, target, d_pred=None)``: the third argument (or ``pc=``) is ``pc`` [B,256] and the result is
        (pred, terms, d_cond, d_pc [B,256]); ``self.cond`` [past_len,B,256] keeps the encoder's output.  With ``train_pointnet`` it is
        ``grads_at(x_t, t, target=target, obj_points=obj_points)``: ``pc`` is encoded from the raw points with saves, and the PointNet++ backward fills the
        last 113,917 entries of ``self.grads`` from ``d_pc``; the result is the same 4-tuple."""
        if self.train_pointnet:
            if target is None or obj_points is None or cond is not None or pc is not None:
                raise ValueError('train_pointnet=True: grads_at(x_t, t, target=target, obj_points=obj_points [B,P,3])')
            out = self._full_grads_at(x_t, t, self.pointnet.encode_saved(obj_points), target, d_pred)
            self.pointnet.grads(out[3], flat=True)
            return out
        if obj_points is not None:
            raise ValueError('obj_points= is the train_pointnet form of grads_at')
        if target is None or (cond is None) == (pc is None) or (pc is not None and not self.train_encoder):
            raise ValueError('grads_at(x_t, t, cond, target) or, with train_encoder, grads_at(x_t, t, pc, target)')
        if self.train_encoder:
            return self._full_grads_at(x_t, t, cond if pc is None else pc, target, d_pred)
        x_t, target, cond = x_t.contiguous(), target.contiguous(), cond.contiguous()
        B, T, S = x_t.shape[0], x_t.shape[-1], cond.shape[0]
        if tuple(x_t.shape[1:3]) != (1, 144) or tuple(cond.shape[1:]) != (B, 256) or target.shape != x_t.shape:
            raise ValueError('x_t / target [B,1,144,T], cond [mem_len,B,256]')
        if T > MAX_T:
            raise ValueError('DenoiserTrainer supports T <= %d (got %d)' % (MAX_T, T))
        if S > MAX_MEM:
            raise ValueError('DenoiserTrainer supports mem_len <= %d (got %d)' % (MAX_MEM, S))
        if d_pred is not None:
            if d_pred.shape != x_t.shape:
                raise ValueError('d_pred must be [B,1,144,T]')
            d_pred = d_pred.contiguous()
        ws = self._workspace(B, T, S)
        pred, terms, d_cond = torch.empty_like(x_t), torch.empty(16, B, dtype=torch.float32, device=self.device), torch.empty_like(cond)
        _lib.check(self.lib.interdiff_mdm_train_grads(
            _lib.dptr(self.params), _lib.dptr(self.pe), self.pe.shape[0], _lib.dptr(x_t, torch.float32), _lib.dptr(t.to(self.device).contiguous(), torch.int64),
            _lib.dptr(cond, torch.float32), _lib.dptr(target, torch.float32), B, T, S, self.past_len, self._w16, _lib.dptr(d_pred, torch.float32, allow_none=True),
            _lib.dptr(self.grads), _lib.dptr(d_cond), _lib.dptr(pred), _lib.dptr(terms), _lib.dptr(ws), ws.numel(), _lib.stream()), 'mdm_train_grads')
        return pred, terms, d_cond

    def _full_grads_at(self, x_t, t, pc, target, d_pred):
        x_t, target, pc = x_t.contiguous(), target.contiguous(), pc.contiguous()
        B, T, S = x_t.shape[0], x_t.shape[-1], self.past_len
        if tuple(x_t.shape[1:3]) != (1, 144) or tuple(pc.shape) != (B, 256) or target.shape != x_t.shape:
            raise ValueError('x_t / target [B,1,144,T], pc [B,256]')
        if T > MAX_T:
            raise ValueError('DenoiserTrainer supports T <= %d (got %d)' % (MAX_T, T))
        if d_pred is not None:
            if d_pred.shape != x_t.shape:
                raise ValueError('d_pred must be [B,1,144,T]')
            d_pred = d_pred.contiguous()
        ws = self._workspace(B, T, S)
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=self.device)
        pred, terms, cond, d_cond, d_pc = torch.empty_like(x_t), new(16, B), new(S, B, 256), new(S, B, 256), new(B, 256)
        _lib.check(self.lib.interdiff_mdm_train_full_grads(
            _lib.dptr(self.params), _lib.dptr(self.pe), self.pe.shape[0], _lib.dptr(x_t, torch.float32), _lib.dptr(t.to(self.device).contiguous(), torch.int64),
            _lib.dptr(pc, torch.float32), _lib.dptr(target, torch.float32), B, T, S, self._w16, _lib.dptr(d_pred, torch.float32, allow_none=True),
            _lib.dptr(self.grads), _lib.dptr(cond), _lib.dptr(d_cond), _lib.dptr(d_pc), _lib.dptr(pred), _lib.dptr(terms), _lib.dptr(ws), ws.numel(), _lib.stream()),
            'mdm_train_full_grads')
        self.cond = cond
        return pred, terms, d_cond, d_pc

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

    def _full_batch(self, batch):
        """Encoder mode: (gt [B,1,144,T], pc [B,256]) of a clip batch that carries ``pc`` or raw ``obj_points``; with ``train_pointnet`` (gt, obj_points)."""
        if self.train_pointnet:
            if isinstance(batch, dict) and ('cond' in batch or 'pc' in batch):
                raise ValueError('train_pointnet=True: a batch that carries cond or pc cannot reach the points; pass raw obj_points [B,P,3]')
            if not isinstance(batch, dict) or 'gt' not in batch or 'obj_points' not in batch:
                raise ValueError('train_pointnet=True takes a clip batch with gt [B,1,144,T] and obj_points [B,P,3]')
            return batch['gt'], batch['obj_points']
        if isinstance(batch, dict) and 'cond' in batch:
            raise ValueError('train_encoder=True: a batch that carries cond cannot reach the encoder; pass pc [B,256] or obj_points [B,P,3]')
        if not isinstance(batch, dict) or 'gt' not in batch or not ('pc' in batch or 'obj_points' in batch):
            raise ValueError('train_encoder=True takes a clip batch with gt [B,1,144,T] and pc [B,256] or obj_points [B,P,3]')
        return batch['gt'], (batch['pc'] if 'pc' in batch else self.encode_points(batch['obj_points']))

    def _batch(self, batch):
        if not (isinstance(batch, dict) and 'cond' in batch):
            if self._mdm is None:
                self.export_mdm()
            batch = as_clip_batch(self._mdm, batch, self.past_len)
        return batch

    def loss_and_grads(self, batch, t=None, noise=None, seed=None, d_pred=None, generator=None):
        """``forward_backward`` with the backward: the batch handling, timestep draw and ``q_sample`` of ``losses.denoising_losses``, then one
        forward with saves, the 16 terms, the loss gradient (or ``d_pred`` [B,1,144,T] in its place -- the seam for other objectives) and the
        backward.  Returns (loss [B], loss_dict {name: [B]}, weighted {name: [B]}, grads {name: tensor} -- views of the flat gradient, valid until
        the next call --, d_cond [mem_len,B,256]); ``self.pred`` keeps the model output.  With ``train_encoder``: ``d_pc`` [B,256] as a further
        last element, and ``self.cond`` keeps the conditioning the step computed."""
        if self.train_encoder:
            gt, third = self._full_batch(batch)
        else:
            batch = self._batch(batch)
            gt, third = batch['gt'], batch['cond']
        gt = gt.contiguous()
        B = gt.shape[0]
        if gt.shape[-1] > MAX_T:
            raise ValueError('DenoiserTrainer supports T <= %d (got %d)' % (MAX_T, gt.shape[-1]))
        if t is None:
            t, _ = self.diffusion.sample_timesteps(B, gt.device, generator)
        t = t.to(gt.device)
        x_t = self.diffusion.q_sample(gt, t, noise=noise, seed=seed)
        if self.train_pointnet:
            self.pred, terms, *seams = self.grads_at(x_t, t, target=gt, d_pred=d_pred, obj_points=third)
        else:
            self.pred, terms, *seams = self.grads_at(x_t, t, third, gt, d_pred)
        wt = terms * self._wdev[:, None]
        return (wt.sum(0), {k: terms[i] for i, k in enumerate(LOSS_KEYS)}, {k: wt[i] for i, k in enumerate(LOSS_KEYS)}, self.named_views(self.grads), *seams)

    def apply_gradients(self):
        """``optimizer.step()``: AdamW on the flat vectors with the gradient of the last ``loss_and_grads``; with ``train_pointnet`` the re-fold follows."""
        self.step += 1
        _lib.check(self.lib.interdiff_mdm_train_step(_lib.dptr(self.params), _lib.dptr(self.grads), _lib.dptr(self.exp_avg), _lib.dptr(self.exp_avg_sq), self.n_param,
                                                     self.step, self.lr, self.betas[0], self.betas[1], self.eps, self.weight_decay, _lib.stream()), 'mdm_train_step')
        if self.train_pointnet:
            self.pointnet.refold()

    def training_step(self, batch, t=None, noise=None, seed=None, d_pred=None, generator=None):
        """``loss_and_grads`` followed by the AdamW entry; returns what ``loss_and_grads`` returns."""
        out = self.loss_and_grads(batch, t=t, noise=noise, seed=seed, d_pred=d_pred, generator=generator)
        self.apply_gradients()
        return out
