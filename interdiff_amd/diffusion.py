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
Respacing and DDIM: ``space_timesteps`` / ``SpacedDiffusion`` (diffusion/respace.py) keep a subset of the base
process's timesteps; ``ddim_sample_loop`` (gaussian_diffusion.py:738-788, :885-1000) is the same loop on other table rows -- for an
x0-predicting model the DDIM update is linear in (x0, x_t, noise), so it is folded on the host, in fp64, into the three per-step
scalars {c1, c2, sigma} the kernels already take.  Two indices then exist per step: the loop-side (spaced) index i -- table row,
Philox step counter, what ``denoised_fn`` is told and what its gate and blend weight act on -- and the model's timestep
``timestep_map[i]``, which only the denoiser's embedding sees (respace.py:124-126); on the device, ``state[0]`` holds the former and
``ts`` the latter (``_tmap``).
PLMS and partial schedules: ``plms_sample_loop`` (gaussian_diffusion.py:1001-1196) is not a table row -- every step combines the
current eps with up to three earlier ones, and its first step calls the denoiser twice, the second time at t - 1 -- so it has step kernels of its
own (csrc/plms.hip: an eps ring f32[3][n], a table of four square roots per step, state-driven like the posterior step) and runs the two-call
form on every route.  ``skip_timesteps`` / ``init_image`` on all three loops start from ``q_sample(init_image, first index, x_T)``.
Only the configuration the eval path uses is implemented (ModelMeanType.START_X, ModelVarType.FIXED_SMALL, clip_denoised=False,
rescale_timesteps=False); anything else raises NotImplementedError.
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


def space_timesteps(num_timesteps, section_counts):
    """respace.py:8-61: the set of base timesteps to keep.  ``section_counts``: a list of ints or a comma string -- that many evenly
    strided steps from each of len(section_counts) equal portions of the base process -- or 'ddimN': the fixed integer stride of the
    DDIM paper that yields exactly N steps.  ValueError when no integer stride does, or a portion has fewer steps than asked of it."""
    if isinstance(section_counts, str):
        if section_counts.startswith('ddim'):
            want = int(section_counts[len('ddim'):])
            for stride in range(1, num_timesteps):
                if len(range(0, num_timesteps, stride)) == want:
                    return set(range(0, num_timesteps, stride))
            raise ValueError('cannot create exactly %d steps with an integer stride' % num_timesteps)
        section_counts = [int(c) for c in section_counts.split(',')]
    size_per, extra = divmod(num_timesteps, len(section_counts))
    start, kept = 0, []
    for k, count in enumerate(section_counts):
        size = size_per + (1 if k < extra else 0)
        if size < count:
            raise ValueError('cannot divide section of %d steps into %d' % (size, count))
        stride = 1 if count <= 1 else (size - 1) / (count - 1)
        kept += [start + round(cur) for cur in _strided(stride, count)]
        start += size
    return set(kept)


def _strided(stride, count):
    """0, stride, 2 stride, ... accumulated the way the reference does (repeated addition: the rounding of the sum is part of the result)."""
    cur = 0.0
    for _ in range(count):
        yield cur
        cur += stride


def ddim_coefficients(alphas_cumprod, alphas_cumprod_prev, eta):
    """The DDIM step of an x0-predicting model (gaussian_diffusion.py:769-787) as x_prev = c1 x0 + c2 x_t + sigma noise, fp64 [steps] each:
        eps    = (sqrt(1/ab) x - x0) / sqrt(1/ab - 1)
        sigma  = eta sqrt((1 - ab_prev) / (1 - ab)) sqrt(1 - ab / ab_prev)
        x_prev = x0 sqrt(ab_prev) + sqrt(1 - ab_prev - sigma^2) eps + sigma noise
    so with k = sqrt(1 - ab_prev - sigma^2) / sqrt(1/ab - 1):  c1 = sqrt(ab_prev) - k,  c2 = k sqrt(1/ab)."""
    ab, abp = np.asarray(alphas_cumprod, np.float64), np.asarray(alphas_cumprod_prev, np.float64)
    sigma = float(eta) * np.sqrt((1.0 - abp) / (1.0 - ab)) * np.sqrt(1.0 - ab / abp)
    k = np.sqrt(np.maximum(1.0 - abp - sigma ** 2, 0.0)) / np.sqrt(1.0 / ab - 1.0)     # (eta = 1: 1 - ab_prev - sigma^2 is >= 0 up to rounding)
    return np.sqrt(abp) - k, k * np.sqrt(1.0 / ab), sigma


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
        self.timestep_map = list(range(self.num_timesteps))       # a SpacedDiffusion overwrites both (respace.py:75-76)
        self.original_num_steps = self.num_timesteps
        self.identity_tmap_is_null = True    # an identity timestep map goes to the kernels as NULL (the route of the un-suffixed C entries); False: as an array, for the A/B test of the _map entries
        self._t_cache = {}
        self._tables = {}
        self._rows_cache = {}
        self._tmaps = {}
        self._q_tables = {}
        self.fuse_plain_step = True          # plain steps of the graph route: posterior update inside the denoiser's last GEMM
        self.chain_plain_steps = os.environ.get('INTERDIFF_CHAIN_STEPS', '1') != '0'      # ... and, inside a captured run of plain steps, the next step's embedding in the same launch (csrc/tail_h2.h)
        self.split_chains = True             # ... and, for batches that do not fill the chip, as two independent half-batch chains
        self.split_min_rows = None           # ... when the batch has more token rows than this (None: the denoiser's one_chain_max_rows(), see graph_sampler.sample)
        self._uid = next(_UID)               # names this schedule in the per-denoiser graph cache (never reused, unlike id())

    # ------------------------------------------------------------------ helpers
    @property
    def is_respaced(self):
        return self.timestep_map != list(range(self.num_timesteps))

    def _timesteps(self, B, device, loop_side=False):
        """int64 [steps, B]: row i is the ``t`` of loop-side step i -- the MODEL's timestep ``timestep_map[i]`` (respace.py:124-126), or with
        ``loop_side`` the spaced index i itself, which is what ``denoised_fn`` is handed (gaussian_diffusion.py:356 passes the unmapped t).
        The same tensor when the map is the identity."""
        key = (B, str(device), bool(loop_side) and self.is_respaced)
        if key not in self._t_cache:
            vals = torch.tensor(self.timestep_map, dtype=torch.int64) if not key[2] and self.is_respaced else torch.arange(self.num_timesteps, dtype=torch.int64)
            self._t_cache[key] = vals.to(device)[:, None].repeat(1, B).contiguous()
        return self._t_cache[key]

    def _tmap(self, device):
        """The device array the step kernels map ``ts`` through (int64 [steps] = timestep_map), None for the identity."""
        if not self.is_respaced and self.identity_tmap_is_null:
            return None
        key = str(device)
        if key not in self._tmaps:
            self._tmaps[key] = torch.tensor(self.timestep_map, dtype=torch.int64).to(device)
        return self._tmaps[key]

    def _rows(self, sampler=('ddpm',)):
        """Host [steps,4] fp32 rows {c1, c2, sigma (0 at step 0), step/1000} of a sampler: ('ddpm',) -- posterior mean coefficients and
        exp(.5 logvar) -- or ('ddim', eta) -- ``ddim_coefficients``.  ``step`` is the loop-side index: the blend weight of the correction
        hook acts on it (module docstring)."""
        if sampler not in self._rows_cache:
            if sampler[0] == 'ddpm':
                c1, c2, sig = self._c1, self._c2, self._sigma.copy()
            else:
                c1, c2, sig = (v.astype(np.float32) for v in ddim_coefficients(self.alphas_cumprod, self.alphas_cumprod_prev, sampler[1]))
            sig[0] = 0.0
            blend = (np.arange(self.num_timesteps, dtype=np.float32) / np.float32(1000)).astype(np.float32)
            self._rows_cache[sampler] = np.ascontiguousarray(np.stack([c1, c2, sig, blend], axis=1).astype(np.float32))
        return self._rows_cache[sampler]

    def _table(self, device, sampler=('ddpm',)):
        """``_rows`` on the device, for the device-parameterised step kernels."""
        key = (str(device), sampler)
        if key not in self._tables:
            self._tables[key] = torch.from_numpy(self._rows(sampler)).to(device)
        return self._tables[key]

    def _plms_rows(self):
        """Host [steps,4] fp32 rows {sqrt(1/ab), sqrt(1/ab - 1), sqrt(ab_prev), sqrt(1 - ab_prev)} of the PLMS step kernels (csrc/plms.hip): what
        ``plms_sample`` reads or forms per step (gaussian_diffusion.py:1044, :1054), each rounded ONCE from the fp64 tables, as ``_rows`` does."""
        if 'plms' not in self._rows_cache:
            ab, abp = self.alphas_cumprod, self.alphas_cumprod_prev
            self._rows_cache['plms'] = np.ascontiguousarray(np.stack([np.sqrt(1.0 / ab), np.sqrt(1.0 / ab - 1.0), np.sqrt(abp), np.sqrt(1.0 - abp)], axis=1).astype(np.float32))
        return self._rows_cache['plms']

    def _plms_table(self, device):
        """``_plms_rows`` on the device."""
        key = (str(device), 'plms')
        if key not in self._tables:
            self._tables[key] = torch.from_numpy(self._plms_rows()).to(device)
        return self._tables[key]

    def _predict_x0(self, model, x, t, t_hook, model_kwargs, denoised_fn, rows_kw):
        """The x0 a step works on: model(x, t) -> inpainting -> ``denoised_fn`` told ``t_hook`` (p_mean_variance, gaussian_diffusion.py:277-388)."""
        y = model_kwargs.get('y', {})
        x0 = model(x, t, **model_kwargs, **rows_kw)
        mu8, gc = mask_operands(y.get('inpainting_mask'), y.get('inpainted_motion'), x0)
        if mu8 is not None:
            inpaint(x0, gc, mu8)
        if denoised_fn is not None:
            x0 = denoised_fn(x0, t_hook, model_kwargs).contiguous()
        return x0

    def _step(self, model, img, x0_buf, i, it, t, model_kwargs, denoised_fn, noise_i, seed, elem0=0, rows_kw={}, t_hook=None, rows=None):
        """``t``: what the model is called with; ``t_hook`` (default ``t``): what ``denoised_fn`` is; ``rows``: the sampler's ``_rows``."""
        lib = _lib.load()
        y = model_kwargs.get('y', {})
        x0 = model(img, t, **model_kwargs, **rows_kw)
        mu8, gc = mask_operands(y.get('inpainting_mask'), y.get('inpainted_motion'), x0)
        if mu8 is not None:
            inpaint(x0, gc, mu8)
        if denoised_fn is not None:
            x0 = denoised_fn(x0, t if t_hook is None else t_hook, model_kwargs)
        c1, c2, sigma = (float(v) for v in (self._rows() if rows is None else rows)[i, :3])
        _lib.check(lib.interdiff_posterior_step_at(_lib.dptr(img, torch.float32), _lib.dptr(x0, torch.float32),
                                                   _lib.dptr(noise_i, torch.float32, allow_none=True), img.numel(),
                                                   c1, c2, sigma, seed, it, elem0, _lib.stream()),
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
        ``noise`` / ``step_noise`` tensors, when given, are this shard's slices.  On a respaced schedule ``first_t``, ``n_steps`` and
        ``dump_steps`` count spaced steps.  ``skip_timesteps`` / ``init_image`` (:701-709): x starts as ``q_sample(init_image, N - 1, x)`` -- after
        the inpainting of a drawn x_T -- and the loop runs the spaced indices N - 1 ... skip_timesteps: the reference slices the FRONT of the index
        list off (:705), so the last step still draws noise unless skip_timesteps == 0.  That quirk is kept."""
        return self._sample_loop(('ddpm',), model, shape, noise, clip_denoised, denoised_fn, cond_fn, model_kwargs, device, skip_timesteps,
                                 init_image, randomize_class, cond_fn_with_grad, dump_steps, const_noise, step_noise, seed, n_steps, use_graph,
                                 first_t, shard)

    def ddim_sample_loop(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None, model_kwargs=None,
                         device=None, progress=False, eta=0.0, skip_timesteps=0, init_image=None, randomize_class=False,
                         cond_fn_with_grad=False, dump_steps=None, const_noise=False, step_noise=None, seed=None, n_steps=None,
                         use_graph=True, first_t=None, shard=None):
        """``ddim_sample_loop`` (gaussian_diffusion.py:885-1000): ``p_sample_loop``'s keyword surface and extras, plus ``eta``.  The same
        loop on the table rows of ``ddim_coefficients``; inpainting and ``denoised_fn`` act on x0 before the update, and x_T drawn here
        (``noise=None``) is NOT inpainted (:960-963, unlike :695-699).  With ``eta = 0`` every sigma is 0: the noise is still drawn and
        multiplied, so that the eager and the graph route stay one arithmetic (the result does not depend on ``seed``).  ``skip_timesteps`` /
        ``init_image`` (:965-972): x starts as ``q_sample(init_image, N - 1 - skip, x)`` and the loop runs N - 1 - skip ... 0."""
        return self._sample_loop(('ddim', float(eta)), model, shape, noise, clip_denoised, denoised_fn, cond_fn, model_kwargs, device,
                                 skip_timesteps, init_image, randomize_class, cond_fn_with_grad, dump_steps, const_noise, step_noise, seed,
                                 n_steps, use_graph, first_t, shard)

    def plms_sample_loop(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None, model_kwargs=None, device=None,
                         progress=False, skip_timesteps=0, init_image=None, randomize_class=False, cond_fn_with_grad=False, order=2,
                         dump_steps=None, seed=None, n_steps=None, use_graph=True, shard=None):
        """``plms_sample_loop`` (gaussian_diffusion.py:1085-1196), the pseudo linear multistep sampler: the reference's keywords plus ``seed`` (for
        a drawn x_T only: the steps draw nothing), ``n_steps``, ``use_graph``, ``shard`` and ``dump_steps`` as in ``p_sample_loop``.  Every step
        re-derives eps from the inpainted, ``denoised_fn``-corrected x0 and combines it with up to ``order`` - 1 earlier ones (csrc/plms.hip);
        the first step calls the model twice, the second time on the half-way point and with t - 1 (:1051-1058) -- ``denoised_fn`` is told
        t - 1 there too.  x_T drawn here is not inpainted (:1153-1156).  ``order`` 2, 3 or 4: the reference's ``order=1`` dies on its first
        step (``old_out`` is None at :1061), so it is refused here.  ``skip_timesteps`` / ``init_image`` as in ``ddim_sample_loop`` (:1158-1165)."""
        if isinstance(order, bool) or not isinstance(order, (int, np.integer)) or not 1 <= order <= 4:
            raise ValueError('order must be 2, 3 or 4')
        if order == 1:
            raise ValueError('order=1 is not a sampler: the reference fails there too (TypeError on its first step, old_out is None)')
        return self._sample_loop(('plms', int(order)), model, shape, noise, clip_denoised, denoised_fn, cond_fn, model_kwargs, device, skip_timesteps,
                                 init_image, randomize_class, cond_fn_with_grad, dump_steps, False, None, seed, n_steps, use_graph, None, shard)

    def _sample_loop(self, sampler, model, shape, noise, clip_denoised, denoised_fn, cond_fn, model_kwargs, device, skip_timesteps, init_image,
                     randomize_class, cond_fn_with_grad, dump_steps, const_noise, step_noise, seed, n_steps, use_graph, first_t, shard):
        if clip_denoised:
            raise NotImplementedError('clip_denoised=True is not used on the eval path (eval_smpl_short.py:153)')
        if cond_fn is not None or randomize_class or cond_fn_with_grad or const_noise:
            raise NotImplementedError('only noise=, denoised_fn=, model_kwargs=, dump_steps=, skip_timesteps=, init_image= are live (SURVEY.md §8(b))')
        skip, N = int(skip_timesteps or 0), self.num_timesteps
        started = bool(skip) or init_image is not None
        if started and first_t is not None:
            raise ValueError('first_t enters the schedule with noise taken as x_t; skip_timesteps / init_image start it from a noised motion: give one')
        if not 0 <= skip < N:
            raise ValueError('skip_timesteps must leave a step of the %d to run' % N)
        if init_image is not None and (tuple(init_image.shape) != tuple(shape) or init_image.dtype != torch.float32):
            raise ValueError('init_image must be float32 of shape %s' % (tuple(shape),))
        if sampler[0] == 'plms' and N - skip < 2:
            raise ValueError('PLMS needs two steps: its first step calls the model at t - 1 (the reference would index step -1)')
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
            mu8, gc = mask_operands(y.get('inpainting_mask'), y.get('inpainted_motion'), img) if sampler[0] == 'ddpm' else (None, None)
            if mu8 is not None:
                inpaint(img, gc, mu8)
        # p_sample_loop slices the skipped steps off the FRONT of the ascending index list (:705: N - 1 ... skip), the other two off its end (:967, :1161)
        t_first = (N - 1 if sampler[0] == 'ddpm' else N - 1 - skip) if first_t is None else int(first_t)
        if not 0 <= t_first < self.num_timesteps:
            raise ValueError('first_t outside the schedule')
        left = t_first + 1 - (skip if sampler[0] == 'ddpm' else 0)
        todo = left if n_steps is None else min(int(n_steps), left)
        if started:                                     # x = q_sample(init_image, first index, x): the drawn or given noise serves as eps (:707-709)
            x_start = torch.zeros_like(img) if init_image is None else init_image.to(device).contiguous()
            img = self.q_sample(x_start, torch.full((shape[0],), t_first, dtype=torch.int64, device=device), noise=img)
        if (step_noise is None and use_graph and getattr(model, 'graph_safe', False) and img.is_cuda
                and 'cond' in model_kwargs.get('y', {}) and os.environ.get('INTERDIFF_NO_GRAPH') != '1'):
            return graph_sampler.sample(self, model, img, model_kwargs, denoised_fn, seed, todo, dump_steps, t_first, shard, sampler)
        rows_kw = {'batch_rows': total * shape[-1]} if shard is not None and getattr(model, 'accepts_batch_rows', False) else {}
        ts, ts_hook = self._timesteps(shape[0], device), self._timesteps(shape[0], device, loop_side=True)
        dump = []
        cond = model_kwargs.get('y', {}).get('cond') if isinstance(model_kwargs.get('y', None), dict) else None
        if cond is not None and hasattr(model, 'prepare_memory'):
            model.prepare_memory(cond)                  # once per sample, like the graph route (never trust a cached fold across samples)
        if sampler[0] == 'plms':
            return self._plms_loop(sampler[1], model, img, ts, ts_hook, t_first, todo, model_kwargs, denoised_fn, rows_kw, dump_steps, seed, elem0)
        rows = self._rows(sampler)
        for it, i in enumerate(range(t_first, t_first - todo, -1)):
            t, th = ts[i], ts_hook[i]
            t.host_value = th.host_value = i
            if step_noise is None:
                nz = None
            elif callable(step_noise):
                nz = step_noise(it, img).contiguous()
            else:
                nz = step_noise[it]
            self._step(model, img, None, i, it, t, model_kwargs, denoised_fn, nz, seed, elem0, rows_kw, th, rows)
            if dump_steps is not None and it in dump_steps:
                dump.append(img.clone())
        return dump if dump_steps is not None else img

    def _plms_loop(self, order, model, img, ts, ts_hook, t_first, todo, model_kwargs, denoised_fn, rows_kw, dump_steps, seed, elem0):
        """The eager PLMS loop on the entries the graph route captures (graph_sampler.plms_*): sampler state, model timesteps, eps ring and
        the half-way point live on the device; the model and ``denoised_fn`` are handed the host-known rows of ``ts`` / ``ts_hook``."""
        dev, B = img.device, img.shape[0]
        ptable, tmap = self._plms_table(dev), self._tmap(dev)
        state = seeded_state(t_first, seed, elem0).to(dev)
        ts_dev = torch.full((B,), self.timestep_map[t_first], dtype=torch.int64, device=dev)
        ring, x_mid = torch.empty(3, img.numel(), dtype=torch.float32, device=dev), torch.empty_like(img)

        def x0_at(x, i):
            t, th = ts[i], ts_hook[i]
            t.host_value = th.host_value = i
            return self._predict_x0(model, x, t, th, model_kwargs, denoised_fn, rows_kw)
        dump = []
        for it, i in enumerate(range(t_first, t_first - todo, -1)):
            x0 = x0_at(img, i)
            if it == 0:                                 # pseudo improved Euler: the second call sees (x_mid, i - 1)
                graph_sampler.plms_first_half(img, x0, None, None, ring, x_mid, ptable, state, ts_dev, tmap)
                graph_sampler.plms_second_half(img, x0_at(x_mid, i - 1), None, None, ring, x_mid, ptable, state)
            else:
                graph_sampler.plms_step(img, x0, None, None, ring, order, ptable, state, ts_dev, tmap)
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
        t = t.to(x_t.device)
        if self.is_respaced:                   # the model is told the base process's timestep (respace.py:94-97, :124-126)
            t = torch.tensor(self.timestep_map, dtype=torch.int64, device=x_t.device)[t]
        model_output = model(x_t, t, **model_kwargs)
        assert model_output.shape == x_start.shape
        return model_output, x_start


def sample_loop(diffusion, model, shape, sampler='ddpm', eta=0.0, order=None, **kw):
    """``diffusion.p_sample_loop`` (sampler='ddpm', the default everywhere), ``diffusion.ddim_sample_loop`` (sampler='ddim', with ``eta``) or
    ``diffusion.plms_sample_loop`` (sampler='plms', with ``order``, which has no default here): what the eval and scoring entry points call, so that
    their ``loop_kw`` can choose the sampler; ``skip_timesteps`` / ``init_image`` pass through ``kw``."""
    if sampler == 'ddpm':
        return diffusion.p_sample_loop(model, shape, **kw)
    if sampler == 'ddim':
        return diffusion.ddim_sample_loop(model, shape, eta=eta, **kw)
    if sampler == 'plms':
        if order is None:
            raise ValueError("sampler='plms' needs order=2, 3 or 4")
        return diffusion.plms_sample_loop(model, shape, order=order, **kw)
    raise ValueError("sampler must be 'ddpm', 'ddim' or 'plms'")


class SpacedDiffusion(GaussianDiffusion):
    """respace.py:64-114: the steps ``use_timesteps`` of the base process ``betas``.  The betas are re-derived (fp64) from the kept
    alphas_cumprod, so every table of ``GaussianDiffusion`` is the spaced process's; ``timestep_map[i]`` is the base timestep of spaced
    step i -- what the model is called with -- and ``original_num_steps`` the base length.  ``rescale_timesteps=True`` is not built."""

    def __init__(self, use_timesteps, betas, rescale_timesteps=False):
        if rescale_timesteps:
            raise NotImplementedError('rescale_timesteps=True is not built (the reference configuration is False: model/diffusion_smpl.py:258)')
        base = GaussianDiffusion(betas)
        self.use_timesteps = set(use_timesteps)
        last, new_betas, tmap = 1.0, [], []
        for i, ac in enumerate(base.alphas_cumprod):
            if i in self.use_timesteps:
                new_betas.append(1 - ac / last)
                last = ac
                tmap.append(i)
        super().__init__(np.array(new_betas))
        self.timestep_map, self.original_num_steps, self.rescale_timesteps = tmap, len(base.betas), False


def create_gaussian_diffusion(noise_schedule='cosine', diffusion_steps=1000, timestep_respacing=''):
    """model/diffusion_smpl.py:251-284 with its fixed defaults (predict x_start, sigma_small); ``timestep_respacing``: '' (every step, the
    reference's setting) or what ``space_timesteps`` takes -- '100', [4, 3, 2], 'ddim50'."""
    betas = get_named_beta_schedule(noise_schedule, diffusion_steps, 1.)
    if not timestep_respacing:
        timestep_respacing = [diffusion_steps]
    return SpacedDiffusion(space_timesteps(diffusion_steps, timestep_respacing), betas)
