"""Sampler seam: ``p_sample_loop(model, shape, noise=, clip_denoised=False, model_kwargs=, denoised_fn=)``
(diffusion/gaussian_diffusion.py:598-736) with the step update on ``interdiff_inpaint`` /
``interdiff_posterior_step``.

Host-side design (not a translation of the reference loop):
  * the seven fp64 coefficient tables are built once (numpy) and only the three per-step SCALARS the
    START_X / FIXED_SMALL path needs -- c1[t], c2[t], sigma[t] = exp(.5 logvar[t]) -- are handed to the
    kernel as fp32 arguments; the reference re-uploads whole tables 6x per step (:1620);
  * ``t`` tensors for all steps are materialised once; each carries ``host_value`` so the correction hook
    never syncs on ``t[0]``;
  * x0-inpainting, the posterior mean and the noise add are two elementwise launches (one when no hook);
  * per-step noise: ``step_noise`` = tensor [steps,...] / callable(i, x) for deterministic parity, else the
    in-kernel Philox generator keyed by (seed, loop index);
  * with the in-kernel generator and a graph-safe denoiser the sample runs on captured hipGraphs (graph_sampler.py): blocks of
    plain steps [denoiser forward -> inpaint+posterior -> advance] whose per-step scalars (c1, c2, sigma, t, loop index, seed)
    live in HBM, batches that do not fill the chip as two half-batch chains forked and joined inside every block, and a hook
    step that can be captured riding in the block before it -- a corrected 1000-step sample is 23 replays.  Other hook steps run
    eagerly between replays.  The routes are bit-identical (tests/test_hip_parity.py).  A third form, chains staggered on their own
    streams through the whole loop, lost its A/B and is gone (profiles/NOTES.md, profiles/r03_stagger_ab.txt).
Sharding: ``shard=(first_clip, total_clips)`` says that the batch handed in is clips [first, first + B) of a
larger batch that other ranks (or other calls) hold the rest of.  The in-kernel noise is then drawn at the WHOLE batch's Philox
counters (element offset first * C * T: the reference fills one ``randn_like`` tensor for the whole batch, :532) and the
feed-forward tile is picked from the whole batch's token rows, so the shard's result is bit-identical to the same clips of an
unsharded run -- whatever the route (eager, graph, chains).
Only the configuration the eval path uses is implemented (ModelMeanType.START_X, ModelVarType.FIXED_SMALL,
clip_denoised=False, identity timestep map); anything else raises NotImplementedError.
"""
import itertools
import math
import os
import numpy as np
import torch
from . import _lib
from . import graph_sampler


def get_named_beta_schedule(schedule_name, num_diffusion_timesteps, scale_betas=1.):
    """gaussian_diffusion.py:20-64."""
    n = num_diffusion_timesteps
    if schedule_name == 'linear':
        scale = scale_betas * 1000 / n
        return np.linspace(scale * 0.0001, scale * 0.02, n, dtype=np.float64)
    if schedule_name == 'cosine':
        abar = lambda t: math.cos((t + 0.008) / 1.008 * math.pi / 2) ** 2
        return np.array([min(1 - abar((i + 1) / n) / abar(i / n), 0.999) for i in range(n)], dtype=np.float64)
    raise NotImplementedError('unknown beta schedule: %s' % schedule_name)


GRAPH_BLOCKS = (49, 7, 1)          # plain steps per captured hipGraph (49 = the gap between two correction steps)
SPLIT_MAX_BATCH = int(os.environ.get('INTERDIFF_SPLIT_MAX_BATCH', 128))     # plain steps of a batch of up to this many clips run as N_CHAINS independent chains (graph_sampler.sample); measured up to 128 (two chains 6 - 15 % faster than one at 40 .. 128 clips, tools/small_batch_ab.py)
N_CHAINS = int(os.environ.get('INTERDIFF_CHAINS', 2))
MAX_GRAPH_SHAPES = 8               # captured (shape, mask, cond) entries kept per denoiser before the cache is dropped wholesale
_UID = itertools.count(1)


def fresh_seed():
    """A 62-bit seed from torch's global CPU generator: what a caller who passes no ``seed`` gets, so that every sampling call
    draws its own per-step noise stream (the reference calls ``randn_like`` afresh in every step of every call,
    gaussian_diffusion.py:532) while ``torch.manual_seed`` still makes a whole run reproducible."""
    return int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())


def mask_operands(mask, gt, like):
    """What the inpainting kernels take: (uint8 view of the bool / uint8 ``mask``, contiguous ``gt``), both shaped like ``like``; (None, None) unless both are given."""
    if mask is None or gt is None:
        return None, None
    assert like.shape == mask.shape == gt.shape
    return (mask if mask.dtype == torch.uint8 else mask.view(torch.uint8)).contiguous(), gt.contiguous()


def inpaint(x, gt, mask_u8):
    """x <- gt where the mask is set, in place."""
    _lib.check(_lib.load().interdiff_inpaint(_lib.dptr(x, torch.float32), _lib.dptr(gt, torch.float32), _lib.dptr(mask_u8), x.numel(), _lib.stream()), 'inpaint')


def seeded_state(t_start, seed, elem0):
    """The eight int64 words of the device-side sampler state (host tensor) at the start of a sample: timestep, loop index, seed, three
    reserved words, the Philox element counter of x[0], one reserved word."""
    return torch.tensor([t_start, 0, int(seed) & 0x7FFFFFFFFFFFFFFF, 0, 0, 0, elem0, 0], dtype=torch.int64)


class GaussianDiffusion:
    """START_X / FIXED_SMALL diffusion (the reference's create_gaussian_diffusion configuration)."""

    def __init__(self, betas):
        betas = np.array(betas, dtype=np.float64)
        assert betas.ndim == 1 and (betas > 0).all() and (betas <= 1).all()
        self.betas = betas
        self.num_timesteps = int(betas.shape[0])
        alphas = 1.0 - betas
        self.alphas_cumprod = np.cumprod(alphas, axis=0)
        self.alphas_cumprod_prev = np.append(1.0, self.alphas_cumprod[:-1])
        self.posterior_variance = betas * (1.0 - self.alphas_cumprod_prev) / (1.0 - self.alphas_cumprod)
        self.posterior_log_variance_clipped = np.log(np.append(self.posterior_variance[1], self.posterior_variance[1:]))
        self.posterior_mean_coef1 = betas * np.sqrt(self.alphas_cumprod_prev) / (1.0 - self.alphas_cumprod)
        self.posterior_mean_coef2 = (1.0 - self.alphas_cumprod_prev) * np.sqrt(alphas) / (1.0 - self.alphas_cumprod)
        # fp32 per-step scalars exactly as `_extract_into_tensor(...).float()` then fp32 math would give them
        self._c1 = self.posterior_mean_coef1.astype(np.float32)
        self._c2 = self.posterior_mean_coef2.astype(np.float32)
        self._sigma = np.exp(np.float32(0.5) * self.posterior_log_variance_clipped.astype(np.float32)).astype(np.float32)
        # forward-diffusion tables (gaussian_diffusion.py:160-161), fp64; q_sample hands the kernel their fp32 casts
        self.sqrt_alphas_cumprod = np.sqrt(self.alphas_cumprod)
        self.sqrt_one_minus_alphas_cumprod = np.sqrt(1.0 - self.alphas_cumprod)
        self._t_cache = {}
        self._tables = {}
        self._q_tables = {}
        self.fuse_plain_step = True          # plain steps of the graph route: posterior update inside the denoiser's last GEMM
        self.chain_plain_steps = os.environ.get('INTERDIFF_CHAIN_STEPS', '1') != '0'      # ... and, inside a captured run of plain steps, the next step's embedding in the same launch (csrc/tail_h2.h)
        self.split_chains = True             # ... and, for batches that do not fill the chip, as two independent half-batch chains
        self.split_min_rows = None           # ... when the batch has more token rows than this (None: the denoiser's one_chain_max_rows(), see graph_sampler.sample)
        self._uid = next(_UID)               # names this schedule in the per-denoiser graph cache (never reused, unlike id())

    # ------------------------------------------------------------------ helpers
    def _timesteps(self, B, device):
        key = (B, str(device))
        if key not in self._t_cache:
            self._t_cache[key] = torch.arange(self.num_timesteps, device=device, dtype=torch.int64)[:, None].repeat(1, B).contiguous()
        return self._t_cache[key]

    def _table(self, device):
        """[steps,4] fp32 rows {c1, c2, sigma (0 at t=0), t/1000} for the device-parameterised step kernels."""
        key = str(device)
        if key not in self._tables:
            sig = self._sigma.copy()
            sig[0] = 0.0
            blend = (np.arange(self.num_timesteps, dtype=np.float32) / np.float32(1000)).astype(np.float32)
            self._tables[key] = torch.from_numpy(np.stack([self._c1, self._c2, sig, blend], axis=1).astype(np.float32)).contiguous().to(device)
        return self._tables[key]

    def _step(self, model, img, x0_buf, i, it, t, model_kwargs, denoised_fn, noise_i, seed, elem0=0, rows_kw={}):
        lib = _lib.load()
        y = model_kwargs.get('y', {})
        x0 = model(img, t, **model_kwargs, **rows_kw)
        mu8, gc = mask_operands(y.get('inpainting_mask'), y.get('inpainted_motion'), x0)
        if mu8 is not None:
            inpaint(x0, gc, mu8)
        if denoised_fn is not None:
            x0 = denoised_fn(x0, t, model_kwargs)
        sigma = 0.0 if i == 0 else float(self._sigma[i])
        _lib.check(lib.interdiff_posterior_step_at(_lib.dptr(img, torch.float32), _lib.dptr(x0, torch.float32),
                                                   _lib.dptr(noise_i, torch.float32, allow_none=True), img.numel(),
                                                   float(self._c1[i]), float(self._c2[i]), sigma, seed, it, elem0, _lib.stream()),
                   'posterior_step')
        return x0

    # ------------------------------------------------------------------ public surface
    def p_sample_loop(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None, model_kwargs=None,
                      device=None, progress=False, skip_timesteps=0, init_image=None, randomize_class=False,
                      cond_fn_with_grad=False, dump_steps=None, const_noise=False, step_noise=None, seed=None, n_steps=None,
                      use_graph=True, first_t=None, shard=None):
        """Same keyword surface as the reference (:598-614).  Extra: ``step_noise`` (tensor [n,...] or callable
        (loop_index, x) -> tensor) for deterministic parity, ``seed`` for the in-kernel generator (None: a fresh one per call
        from torch's global generator, see ``fresh_seed``), ``n_steps`` to
        run only the first n iterations (t = T-1 .. T-n) -- used by the bench / short-chain parity tests, ``use_graph=False``
        to force the eager route, ``first_t`` to enter the schedule at that timestep with ``noise`` taken as x_{first_t}
        (a window of the loop for measurements; default T-1), ``shard=(first_clip, total_clips)``: the batch is clips
        [first, first + B) of a larger one -- noise counters and the feed-forward tile are the larger batch's (module docstring);
        ``noise`` / ``step_noise`` tensors, when given, are this shard's slices."""
        if clip_denoised:
            raise NotImplementedError('clip_denoised=True is not used on the eval path (eval_smpl_short.py:153)')
        if cond_fn is not None or skip_timesteps or init_image is not None or randomize_class or cond_fn_with_grad or const_noise:
            raise NotImplementedError('only noise=, denoised_fn=, model_kwargs=, dump_steps= are live (SURVEY.md §8(b))')
        if model_kwargs is None:
            model_kwargs = {}
        if seed is None:
            seed = fresh_seed()
        if device is None:
            device = next(model.parameters()).device
        assert isinstance(shape, (tuple, list))
        if shard is not None:
            shard = (int(shard[0]), int(shard[1]))
            if not 0 <= shard[0] <= shard[0] + shape[0] <= shard[1]:
                raise ValueError('shard=(first_clip, total_clips) must contain this batch of %d clips' % shape[0])
        first, total = (0, shape[0]) if shard is None else shard
        per_clip = int(np.prod(shape[1:]))
        elem0 = first * per_clip
        if shard is not None and elem0 % 4:
            raise ValueError('a shard must start at a multiple of 4 elements (C * T = %d per clip)' % per_clip)
        if noise is not None:
            img = noise.clone().contiguous().float()             # NOT inpainted when given (:691-692)
        else:
            img = torch.empty(*shape, dtype=torch.float32, device=device)
            _lib.check(_lib.load().interdiff_randn_at(_lib.dptr(img), img.numel(), seed, 0xFFFFFFFF, elem0, _lib.stream()), 'randn')
            y = model_kwargs.get('y', {})
            mu8, gc = mask_operands(y.get('inpainting_mask'), y.get('inpainted_motion'), img)
            if mu8 is not None:
                inpaint(img, gc, mu8)
        t_first = self.num_timesteps - 1 if first_t is None else int(first_t)
        if not 0 <= t_first < self.num_timesteps:
            raise ValueError('first_t outside the schedule')
        todo = t_first + 1 if n_steps is None else min(int(n_steps), t_first + 1)
        if (step_noise is None and use_graph and getattr(model, 'graph_safe', False) and img.is_cuda
                and 'cond' in model_kwargs.get('y', {}) and os.environ.get('INTERDIFF_NO_GRAPH') != '1'):
            return graph_sampler.sample(self, model, img, model_kwargs, denoised_fn, seed, todo, dump_steps, t_first, shard)
        rows_kw = {'batch_rows': total * shape[-1]} if shard is not None and getattr(model, 'accepts_batch_rows', False) else {}
        ts = self._timesteps(shape[0], device)
        dump = []
        cond = model_kwargs.get('y', {}).get('cond') if isinstance(model_kwargs.get('y', None), dict) else None
        if cond is not None and hasattr(model, 'prepare_memory'):
            model.prepare_memory(cond)                  # once per sample, like the graph route (never trust a cached fold across samples)
        for it, i in enumerate(range(t_first, t_first - todo, -1)):
            t = ts[i]
            t.host_value = i
            if step_noise is None:
                nz = None
            elif callable(step_noise):
                nz = step_noise(it, img).contiguous()
            else:
                nz = step_noise[it]
            self._step(model, img, None, i, it, t, model_kwargs, denoised_fn, nz, seed, elem0, rows_kw)
            if dump_steps is not None and it in dump_steps:
                dump.append(img.clone())
        return dump if dump_steps is not None else img

    # ------------------------------------------------------------------ forward diffusion / teacher-forced objective (forward only)
    def sample_timesteps(self, B, device, generator=None):
        """``UniformSampler.sample`` (diffusion/resample.py:61-77): ``t`` int64 [B] uniform over the schedule and the importance
        weights, all one.  ``generator``: a torch generator (of any device) for a reproducible draw; default torch's global one."""
        gdev = generator.device if generator is not None else device
        t = torch.randint(0, self.num_timesteps, (B,), dtype=torch.int64, device=gdev, generator=generator).to(device)
        return t, torch.ones(B, dtype=torch.float32, device=device)

    def q_sample(self, x_start, t, noise=None, seed=None, inpainted_motion=None, inpainting_mask=None, elem0=0):
        """``q_sample`` (gaussian_diffusion.py:233-250) with a per-clip timestep ``t`` int64 [B]: one launch of ``interdiff_q_sample``.
        ``noise`` None: eps comes from the in-kernel Philox generator under ``seed`` (None: a fresh one, see ``fresh_seed``) at the
        step index reserved for q_sample (include/interdiff_hip.h), element counter ``elem0`` + e -- a clip shard of a batch passes
        first_clip * C * T and draws what the whole batch would.  ``inpainted_motion`` / ``inpainting_mask``: the inpainting of x_t
        that ``training_losses`` applies when both keys are present (:1264-1268)."""
        lib = _lib.load()
        x0 = x_start.contiguous()
        if x0.dtype != torch.float32:
            raise ValueError('x_start must be float32')
        B = x0.shape[0]
        if tuple(t.shape) != (B,):
            raise ValueError('t must be [B]')
        if not t.is_cuda:
            if int(t.min()) < 0 or int(t.max()) >= self.num_timesteps:
                raise ValueError('t outside the schedule')
            t = t.to(x0.device)
        key = str(x0.device)
        if key not in self._q_tables:
            self._q_tables[key] = tuple(torch.from_numpy(v.astype(np.float32)).to(x0.device) for v in (self.sqrt_alphas_cumprod, self.sqrt_one_minus_alphas_cumprod))
        sa, s1 = self._q_tables[key]
        if (inpainted_motion is None) != (inpainting_mask is None):
            raise ValueError('inpainted_motion and inpainting_mask go together')
        mu8, gc = mask_operands(inpainting_mask, inpainted_motion, x0)
        if noise is not None:
            assert noise.shape == x0.shape
            noise = noise.contiguous()
        elif seed is None:
            seed = fresh_seed()
        x_t = torch.empty_like(x0)
        _lib.check(lib.interdiff_q_sample(_lib.dptr(x_t), _lib.dptr(x0), _lib.dptr(noise, torch.float32, allow_none=True),
                                          _lib.dptr(t.contiguous(), torch.int64), _lib.dptr(sa), _lib.dptr(s1), self.num_timesteps,
                                          _lib.dptr(gc, torch.float32, allow_none=True), _lib.dptr(mu8, allow_none=True), B, x0.numel() // B,
                                          int(seed or 0) & 0xFFFFFFFFFFFFFFFF, int(elem0), _lib.stream()), 'q_sample')
        return x_t

    def training_losses(self, model, x_start, t, model_kwargs=None, noise=None, seed=None):
        """``training_losses`` (gaussian_diffusion.py:1233-1368) for the configuration this module implements (START_X, MSE): x_t by
        ``q_sample`` (inpainted when model_kwargs['y'] carries both mask keys), ONE denoiser forward with the per-clip ``t``, and
        ``(model_output, target)`` with target = x_start, as the reference returns them (:1368).  No backward pass."""
        if model_kwargs is None:
            model_kwargs = {}
        y = model_kwargs.get('y', {})
        both = 'inpainting_mask' in y and 'inpainted_motion' in y
        x_t = self.q_sample(x_start, t, noise=noise, seed=seed, inpainted_motion=y['inpainted_motion'] if both else None,
                            inpainting_mask=y['inpainting_mask'] if both else None)
        model_output = model(x_t, t.to(x_t.device), **model_kwargs)
        assert model_output.shape == x_start.shape
        return model_output, x_start


class SpacedDiffusion(GaussianDiffusion):
    """respace.py:64-114.  Betas are re-derived from the kept alphas_cumprod; the timestep map is the
    identity when every step is kept (the only configuration the eval path builds)."""

    def __init__(self, use_timesteps, betas):
        base = GaussianDiffusion(betas)
        use = set(use_timesteps)
        last, new_betas, self.timestep_map = 1.0, [], []
        for i, ac in enumerate(base.alphas_cumprod):
            if i in use:
                new_betas.append(1 - ac / last)
                last = ac
                self.timestep_map.append(i)
        if self.timestep_map != list(range(len(betas))):
            raise NotImplementedError('timestep respacing is not used by the reference eval path')
        super().__init__(np.array(new_betas))


def create_gaussian_diffusion(noise_schedule='cosine', diffusion_steps=1000):
    """model/diffusion_smpl.py:251-284 with its fixed defaults (predict x_start, sigma_small, no respacing)."""
    betas = get_named_beta_schedule(noise_schedule, diffusion_steps, 1.)
    return SpacedDiffusion(range(diffusion_steps), betas)
