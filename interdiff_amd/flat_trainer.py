"""The scaffold the denoiser trainers share: a model's trained tensors as ONE flat fp32 vector laid out by a table the library gives, and AdamW on it.

    param_table(entry, n)       (offsets, sizes, n_param) of a ``*_param_table`` entry of libinterdiff_hip.so
    FlatParams                  state-dict intake against such a table, views of a flat vector by reference name, ``state_dict()``
    FlatAdamWTrainer            + moments, gradient vector, positional table, workspace cache, the model-independent half of a training step

``DenoiserTrainer`` (mdm_train.py) and ``SkeletonDenoiserTrainer`` (skeleton_mdm_train.py) subclass ``FlatAdamWTrainer`` and supply their names and table, their loss
keys and weight vector, how a batch becomes (gt, conditioning input), the one ctypes call that computes the gradients, and ``export_mdm``.  ``PointNetFineTuner``
(pointnet2_train.py) is a ``FlatParams``: it has no optimiser of its own.  All arithmetic is in the library; torch holds the device memory.
"""
import ctypes as C
import torch
from . import _lib
from .diffusion import create_gaussian_diffusion
from .mdm import positional_table

MAX_T, MAX_MEM = 128, 16


def param_table(entry, n):
    """(offsets, sizes, n_param) of the flat vectors as the library entry ``entry`` (a name) lays them out; ``n``: the tensor count the caller's names expect."""
    off, size, cnt, total = (C.c_int64 * n)(), (C.c_int64 * n)(), C.c_int32(0), C.c_int64(0)
    _lib.check(getattr(_lib.load(), entry)(off, size, C.byref(cnt), C.byref(total)), entry[len('interdiff_'):])
    if cnt.value != n:
        raise RuntimeError('parameter table: %d tensors, expected %d' % (cnt.value, n))
    return list(off), list(size), int(total.value)


def append_table(head, tail):
    """The table of ``tail``'s tensors following ``head``'s in one flat vector."""
    return head[0] + [head[2] + o for o in tail[0]], head[1] + tail[1], head[2] + tail[2]


class FlatParams:
    """``names`` / ``offsets`` / ``sizes`` / ``shapes`` / ``n_param`` of the trained tensors and the pass-through of everything else."""

    def _intake(self, sd, names, table, also=()):
        """``sd``: the caller's own copy of a state_dict ({name: tensor}).  Every name of ``names`` (and ``also``) must be there (KeyError) with the table's size
        (ValueError).  Returns the trained tensors as one fp32 vector on ``self.device``; the rest of ``sd`` is what ``state_dict()`` returns with identical bits."""
        missing = [k for k in tuple(names) + tuple(also) if k not in sd]
        if missing:
            raise KeyError('state_dict lacks %s' % missing[:3])
        self.names, (self.offsets, self.sizes, self.n_param) = names, table
        self.shapes = [tuple(sd[k].shape) for k in names]
        for k, s, shp in zip(names, self.sizes, self.shapes):
            if sd[k].numel() != s:
                raise ValueError('%s: %s does not match the parameter table (%d floats)' % (k, shp, s))
        self._passthrough = {k: v for k, v in sd.items() if k not in names}
        return torch.cat([sd[k].reshape(-1).float() for k in names]).to(self.device)

    def named_views(self, flat):
        return {k: flat[o:o + s].view(shp) for k, o, s, shp in zip(self.names, self.offsets, self.sizes, self.shapes)}

    def state_dict(self):
        """The reference's names: the trained tensors (copies, on the trainer's device) and every other entry of the constructor's state_dict exactly as it came in."""
        out = dict(self._passthrough)
        out.update({k: v.clone() for k, v in self.named_views(self.params).items()})
        return out


class FlatAdamWTrainer(FlatParams):
    """``loss.backward()`` + ``optimizer.step()`` of a reference diffusion trainer on flat vectors: ``params``, ``exp_avg``, ``exp_avg_sq``, ``grads``, ``step``.

    A subclass sets ``LOSS_KEYS`` and ``C_TOK`` (channels of a token) and defines ``_inputs(batch) -> (gt [B,1,C_TOK,T], conditioning input)`` and
    ``_grads(x_t, t, conditioning input, target, d_pred) -> (pred, terms [len(LOSS_KEYS),B], *seams)``, which leaves the flat gradient in ``self.grads``.
    ``after_step``, when set, is called after every AdamW step.  ``dropout`` / ``cond_mask_prob``: the configuration the checkpoint was made for; the reference
    trains at 0, where ``train()`` and ``eval()`` compute the same function, and anything else raises (not built).
    """

    LOSS_KEYS = C_TOK = after_step = None

    def __init__(self, state_dict, names, table, device, lr, weight_decay, betas, eps, weights, past_len, n_steps, dropout, cond_mask_prob):
        if dropout > 0 or cond_mask_prob > 0:
            raise ValueError('%s implements the reference defaults --dropout 0 --cond_mask_prob 0 only' % type(self).__name__)
        self.lib = _lib.load()
        self.device = torch.device(device)
        self.lr, self.weight_decay, self.betas, self.eps = float(lr), float(weight_decay), (float(betas[0]), float(betas[1])), float(eps)
        self.weights, self.past_len, self.n_steps = weights, int(past_len), int(n_steps)
        self.diffusion = create_gaussian_diffusion('cosine', self.n_steps)
        sd = {k: torch.as_tensor(v).detach().clone() for k, v in state_dict.items()}
        self.params = self._intake(sd, names, table).contiguous()
        self.exp_avg, self.exp_avg_sq = torch.zeros_like(self.params), torch.zeros_like(self.params)
        self.grads = torch.zeros_like(self.params)
        self.step = 0
        pe = sd['PositionalEmbedding.pe'][:, 0] if 'PositionalEmbedding.pe' in sd else positional_table()
        self.pe = torch.as_tensor(pe).float().to(self.device).contiguous()
        self._wvec = (C.c_float * len(self.LOSS_KEYS))(*weights.vector())
        self._wdev = torch.tensor(weights.vector(), dtype=torch.float32, device=self.device)
        self._ws = {}
        self.pred = self.cond = None                                 # the model output of the last step; the conditioning the last gradient call computed

    # ------------------------------------------------------------------------------------------------------------ state
    def optimizer_state(self):
        return dict(step=self.step, exp_avg=self.exp_avg.clone(), exp_avg_sq=self.exp_avg_sq.clone())

    def load_optimizer_state(self, state):
        self.step = int(state['step'])
        self.exp_avg.copy_(state['exp_avg'])
        self.exp_avg_sq.copy_(state['exp_avg_sq'])

    # ------------------------------------------------------------------------------------------------------------ steps
    def _workspace(self, bytes_entry, B, T, S):
        """The workspace of a (B, T, memory length) shape, sized by the library and kept for the next call at that shape."""
        need = bytes_entry(B, T, S)
        if need == 0:
            raise ValueError('unsupported shape B=%d T=%d mem_len=%d (T <= %d, mem_len <= %d)' % (B, T, S, MAX_T, MAX_MEM))
        ws = self._ws.get((B, T, S))
        if ws is None:
            ws = self._ws[(B, T, S)] = torch.empty(need, dtype=torch.uint8, device=self.device)
        return ws

    def _checked(self, x_t, target, d_pred):
        """What every gradient call checks: contiguous x_t / target [B,1,C_TOK,T], T <= MAX_T, d_pred (or None) of x_t's shape.  -> (x_t, target, d_pred, B, T)"""
        x_t, target = x_t.contiguous(), target.contiguous()
        if tuple(x_t.shape[1:3]) != (1, self.C_TOK) or target.shape != x_t.shape:
            raise ValueError('x_t / target must be [B,1,%d,T]' % self.C_TOK)
        if x_t.shape[-1] > MAX_T:
            raise ValueError('%s supports T <= %d (got %d)' % (type(self).__name__, MAX_T, x_t.shape[-1]))
        if d_pred is not None:
            if d_pred.shape != x_t.shape:
                raise ValueError('d_pred must be [B,1,%d,T]' % self.C_TOK)
            d_pred = d_pred.contiguous()
        return x_t, target, d_pred, x_t.shape[0], x_t.shape[-1]

    def loss_and_grads(self, batch, t=None, noise=None, seed=None, d_pred=None, generator=None):
        """``forward_backward`` with the backward: the subclass's batch handling, the timestep draw and ``q_sample`` of the reference's ``denoising_losses``, then
        one forward with saves, the terms, the loss gradient (or ``d_pred`` [B,1,C_TOK,T] in its place -- the seam for other objectives) and the backward.
        Returns (loss [B], loss_dict {name: [B]}, weighted {name: [B]}, grads {name: tensor} -- views of the flat gradient, valid until the next call --,
        *the subclass's seams); the reference's scalar is ``loss.mean()``.  ``self.pred`` keeps the model output."""
        gt, inp = self._inputs(batch)
        gt = gt.contiguous()
        B = gt.shape[0]
        if gt.shape[-1] > MAX_T:
            raise ValueError('%s supports T <= %d (got %d)' % (type(self).__name__, MAX_T, gt.shape[-1]))
        if t is None:
            t, _ = self.diffusion.sample_timesteps(B, gt.device, generator)
        t = t.to(gt.device)
        x_t = self.diffusion.q_sample(gt, t, noise=noise, seed=seed)
        self.pred, terms, *seams = self._grads(x_t, t, inp, gt, d_pred)
        wt = terms * self._wdev[:, None]
        return (wt.sum(0), {k: terms[i] for i, k in enumerate(self.LOSS_KEYS)}, {k: wt[i] for i, k in enumerate(self.LOSS_KEYS)}, self.named_views(self.grads), *seams)

    def apply_gradients(self):
        """``optimizer.step()``: AdamW on the flat vectors with the gradient of the last ``loss_and_grads``, then ``after_step`` if there is one."""
        self.step += 1
        _lib.check(self.lib.interdiff_mdm_train_step(_lib.dptr(self.params), _lib.dptr(self.grads), _lib.dptr(self.exp_avg), _lib.dptr(self.exp_avg_sq), self.n_param,
                                                     self.step, self.lr, self.betas[0], self.betas[1], self.eps, self.weight_decay, _lib.stream()), 'mdm_train_step')
        if self.after_step:
            self.after_step()

    def training_step(self, batch, t=None, noise=None, seed=None, d_pred=None, generator=None):
        """``loss_and_grads`` followed by the AdamW entry; returns what ``loss_and_grads`` returns."""
        out = self.loss_and_grads(batch, t=t, noise=noise, seed=seed, d_pred=d_pred, generator=generator)
        self.apply_gradients()
        return out
