"""The captured-graph route of ``GaussianDiffusion.p_sample_loop`` (diffusion.py): taken with the in-kernel noise generator and a
graph-safe denoiser (``MDM`` and its subclasses), so the denoiser's methods are called here without probing for them.

  * ``plan_steps`` cuts a sample into ops -- captured blocks of plain steps, hook steps, dump points: pure integer logic;
  * ``Entry`` is what one (schedule, shape, mask, cond shape, feed-forward choice) of a denoiser keeps between samples: the buffers the
    captured graphs read the sample's inputs from, and the graphs.  The entries live ON the denoiser object (``model._graph_cache``):
    the captured graphs bake in the addresses of its arena, workspace and memory context, so they must die with it (a cache keyed by
    id(model) would replay freed memory once the id is recycled);
  * ``Run`` is one sample on an entry: it captures what the plan needs and is not there yet, and replays;
  * ``sample`` is the route: entry, this sample's inputs, warm-up, chains, hook buffers, plan, one replay or eager hook step per op.
  * ``PlmsRun`` is a ``Run`` whose update is the PLMS step (``plms_step`` ... on csrc/plms.hip): one chain of two-call steps, the eps ring and the
    half-way point on the entry, and the two-call first step as an op of its own in front of the plan (captured unless it takes an eager hook).
The module constants that tools rebind (``GRAPH_BLOCKS`` ...) stay in diffusion.py and are read from there at call time.
"""
import os
import torch
from . import _lib, diffusion

HOOK_KEYS = ('hand_pose', 'beta', 'obj_points')          # what a captured hook step reads from ``y`` beside inpainted_motion


def plan_steps(t_start, todo, active, dump_steps, fuse_hook, it0=0):
    """The ops of the ``todo`` steps t_start, t_start - 1, ... (loop index it = ``it0``, ``it0`` + 1, ...), ``active(t)`` telling the hook steps:
      ('plain', k)      one captured graph of k plain steps
      ('hook', k)       one captured graph of k plain steps and the hook step after them (k = 0: a lone hook step); ``fuse_hook`` only
      ('eager_hook',)   the two-call hook step
      ('dump', it)      x after loop index ``it`` is wanted
    A plain run reaches up to the next hook step, dump point or the end and is replayed in the largest of ``diffusion.GRAPH_BLOCKS``
    that fits: the 989 plain steps of a corrected 1000-step sample take 23 graphs with the hook fused."""
    blocks = diffusion.GRAPH_BLOCKS
    dumps = () if dump_steps is None else dump_steps
    ops, i, it, end = [], t_start, it0, t_start - todo
    while i > end:
        if active(i):
            ops.append(('hook', 0) if fuse_hook else ('eager_hook',))
            k = 1
        else:
            run = 1
            while i - run > end and not active(i - run) and (it + run - 1) not in dumps:
                run += 1
            k = next(b for b in blocks if b <= run)
            if fuse_hook and k == run and i - run > end and active(i - run) and (it + k - 1) not in dumps:
                ops.append(('hook', k))             # the run ends right at a hook step: one graph for both
                k += 1
            else:
                ops.append(('plain', k))
        i -= k
        it += k
        if (it - 1) in dumps:
            ops.append(('dump', it - 1))
    return ops


def capture(enqueue, *args):
    """hipGraph of what ``enqueue(*args)`` launches on the capturing stream."""
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        enqueue(*args)
    return g


def posterior_update(x, x0, gt, mask, table, state, ts, tmap=None):
    """x_t -> x_{t-1} from x0 (inpainted first when gt / mask are given), every per-step scalar read from ``table[state[0]]``; advances ``state`` and
    ``ts`` (to ``tmap[state[0]]``, the model's timestep under a respaced schedule; None: the identity)."""
    _lib.check(_lib.load().interdiff_posterior_step_dev_map(_lib.dptr(x), _lib.dptr(x0), _lib.dptr(gt, allow_none=True), _lib.dptr(mask, allow_none=True),
                                                            x.numel(), _lib.dptr(table), _lib.dptr(tmap, torch.int64, allow_none=True), _lib.dptr(state),
                                                            _lib.dptr(ts), ts.numel(), _lib.stream()),
               'posterior_step_dev')


def plms_step(x, x0, gt, mask, ring, order, ptable, state, ts, tmap=None):
    """One multistep PLMS update of x from x0 (inpainted in the kernel when gt / mask are given): eps into ``ring`` f32[3][n], its Adams-Bashforth
    combination with the earlier ones, the update; advances ``state`` and ``ts`` like ``posterior_update`` (interdiff_plms_step_dev)."""
    _lib.check(_lib.load().interdiff_plms_step_dev(_lib.dptr(x), _lib.dptr(x0), _lib.dptr(gt, allow_none=True), _lib.dptr(mask, allow_none=True), _lib.dptr(ring),
                                                   x.numel(), int(order), _lib.dptr(ptable), _lib.dptr(tmap, torch.int64, allow_none=True), _lib.dptr(state),
                                                   _lib.dptr(ts), ts.numel(), _lib.stream()), 'plms_step_dev')


def plms_first_half(x, x0, gt, mask, ring, x_mid, ptable, state, ts, tmap=None):
    """First half of the first PLMS step: eps into the ring, the half-way point into ``x_mid``, ``state[0]`` / ``ts`` to t - 1 for the second
    denoiser call; the loop index stays (interdiff_plms_first_half_dev)."""
    _lib.check(_lib.load().interdiff_plms_first_half_dev(_lib.dptr(x), _lib.dptr(x0), _lib.dptr(gt, allow_none=True), _lib.dptr(mask, allow_none=True), _lib.dptr(ring),
                                                         _lib.dptr(x_mid), x.numel(), _lib.dptr(ptable), _lib.dptr(tmap, torch.int64, allow_none=True),
                                                         _lib.dptr(state), _lib.dptr(ts), ts.numel(), _lib.stream()), 'plms_first_half_dev')


def plms_second_half(x, x0, gt, mask, ring, x_mid, ptable, state):
    """Second half: the update of the ORIGINAL x from the mean of the two eps; advances the loop index (interdiff_plms_second_half_dev)."""
    _lib.check(_lib.load().interdiff_plms_second_half_dev(_lib.dptr(x), _lib.dptr(x0), _lib.dptr(gt, allow_none=True), _lib.dptr(mask, allow_none=True), _lib.dptr(ring),
                                                          _lib.dptr(x_mid), x.numel(), _lib.dptr(ptable), _lib.dptr(state), _lib.stream()), 'plms_second_half_dev')


class Chain:
    """One part of a split batch: its slices of the entry's x / ts / gt / mask / zero_pose_obj and its own sampler state, cond, folded
    memory, workspace and stream (chain 0 steps on the entry's state: the whole-batch hook steps advance that one)."""

    def __init__(self, model, entry, sl, own_state):
        dev, h, mem_len = entry.x.device, sl.stop - sl.start, entry.cond.shape[0]
        self.sl = sl
        self.x, self.ts = entry.x[sl], entry.ts[sl]
        self.gt = None if entry.gt is None else entry.gt[sl]
        self.mask = None if entry.mask is None else entry.mask[sl]
        self.kwargs = {} if entry.zpo is None else {'zero_pose_obj': entry.zpo[sl]}
        self.state = torch.zeros(8, dtype=torch.int64, device=dev) if own_state else entry.state
        self.cond = torch.empty(mem_len, h, entry.cond.shape[2], device=dev)
        self.memctx = torch.empty(model.memctx_floats(h, mem_len), dtype=torch.float32, device=dev)
        self.ws = torch.empty(model.workspace_bytes(h, entry.x.shape[-1]), dtype=torch.uint8, device=dev)
        self.stream = torch.cuda.Stream(dev)


class HookBuffers:
    """What the captured hook steps of one hook read: its workspace and this sample's hook inputs, at addresses the graphs know."""

    def __init__(self, hook, entry, y, shapes):
        B, T = entry.x.shape[0], entry.x.shape[-1]
        self.shapes = shapes
        self.ws = hook.workspace_for(B, T)
        self.y = {k: torch.empty(y[k].shape, dtype=torch.float32, device=entry.x.device) for k in HOOK_KEYS}
        self.y['inpainted_motion'] = entry.gt if entry.gt is not None else torch.empty_like(entry.x)
        self.fresh = True            # until the hook's kernels have been launched once outside a capture


class Entry:
    """The buffers the captured graphs read a sample's inputs from (x, gt, mask, cond, zero_pose_obj) and the graphs themselves: one
    capture per (denoiser, shape) then serves every sample -- an eval loop or an autoregressive rollout feeds a new cond / gt per sample
    and must not pay a re-capture (57 denoiser forwards) each time."""

    def __init__(self, img, cond, has_mask, zpo):
        dev = img.device
        self.x, self.x0 = torch.zeros_like(img), torch.empty_like(img)
        self.ts = torch.zeros(img.shape[0], dtype=torch.int64, device=dev)
        self.state = torch.zeros(8, dtype=torch.int64, device=dev)       # the sampler state of csrc: see ``diffusion.seeded_state``
        self.cond = torch.empty_like(cond, memory_format=torch.contiguous_format)
        self.gt = torch.empty_like(img) if has_mask else None
        self.mask = torch.empty(img.shape, dtype=torch.uint8, device=dev) if has_mask else None
        # a denoiser that takes a per-clip constant beside y (the skeleton model's zero_pose_obj [B,12,3], a TOP-LEVEL model_kwargs entry: eval_skeleton.py:126)
        self.zpo = None if zpo is None else torch.empty(zpo.shape, dtype=torch.float32, device=dev)
        self.kwargs = {'y': {'cond': self.cond}}            # what the captured denoiser calls see
        if zpo is not None:
            self.kwargs['zero_pose_obj'] = self.zpo
        self.graphs = {}             # (k, fused, split): k plain steps; ('hook', hook uid, k, fused, split): and a hook step; 'fwd': the denoiser forward of an eager hook step; PLMS: ('first', hook uid or None, hooked at t, hooked at t - 1): the first step, 'fwd_mid': the forward on x_mid
        self.chains = []             # empty until the split route is first taken
        self.hooks = {}              # hook uid -> HookBuffers
        self.chain_steps = None      # whether the captured plain steps carry the next step's embedding (baked into the graphs)
        self.pool_keys = ()          # the denoiser's per-shape buffers that were allocated FOR this entry (``MDM.shape_buffer_keys``)
        self.ring = self.x_mid = None            # a PLMS entry's eps ring f32[3][n] and the half-way point of its first step

    @staticmethod
    def of(model, key, img, cond, has_mask, zpo):
        """(the denoiser's entry under ``key``, whether it is new).  A new entry beyond ``diffusion.MAX_GRAPH_SHAPES`` drops the cache wholesale:
        its graphs, the buffers the entries allocated (x, x0, cond, chain and hook workspaces) and the entries of the denoiser's per-shape
        pools that were created FOR these graphs (``pool_keys``); pool entries that existed before -- a graph captured elsewhere (bench.py,
        an integrator following INTEGRATION.md) may have baked their addresses in -- stay."""
        cache = model.__dict__.setdefault('_graph_cache', {})
        entry = cache.get(key)
        if entry is not None:
            return entry, False
        entry = Entry(img, cond, has_mask, zpo)
        if len(cache) >= diffusion.MAX_GRAPH_SHAPES:
            evicted = list(cache.values())
            cache.clear()
            for old in evicted:
                model.forget_shape_buffers(old.pool_keys)
        cache[key] = entry
        return entry, True

    def load(self, cond, zpo, gt, mask):
        """This sample's inputs, into the buffers the graphs know."""
        self.cond.copy_(cond)
        if zpo is not None:
            self.zpo.copy_(zpo)
        if mask is not None:
            self.gt.copy_(gt)
            self.mask.copy_(mask)

    def warm_up_plms(self, model, ptable, rows, tmap=None):
        """``warm_up`` of a PLMS entry: the forward and the three step kernels, on copies of x / ts and a state of their own."""
        model(self.x, self.ts, out=self.x0, **self.kwargs, batch_rows=rows)
        t0 = min(2, ptable.shape[0] - 1)
        x, ts, state = self.x.clone(), self.ts.clone(), diffusion.seeded_state(t0, 1, 0).to(self.x.device)
        plms_first_half(x, self.x0, self.gt, self.mask, self.ring, self.x_mid, ptable, state, ts, tmap)
        plms_second_half(x, self.x0, self.gt, self.mask, self.ring, self.x_mid, ptable, state)
        state.copy_(diffusion.seeded_state(t0, 1, 0))
        plms_step(x, self.x0, self.gt, self.mask, self.ring, 2, ptable, state, ts, tmap)
        torch.cuda.synchronize(self.x.device)

    def warm_up(self, model, table, rows, tmap=None):
        """First launches of everything a plain step can consist of, outside a capture (where a launch error cannot be reported): the
        forward (workspaces, kernel attributes), the fused step's own instantiations (last GEMM with the update in its epilogue, QKV kernel
        with the sampler bookkeeping) and the chained forms of the step tail (csrc/tail_h2.h).  The steps run on copies of x / ts."""
        model(self.x, self.ts, out=self.x0, **self.kwargs, batch_rows=rows)
        if model.supports_forward_step:
            t0 = min(2, table.shape[0] - 1)              # (a row every schedule has: respaced ones can be shorter than three steps)
            x, ts, state = self.x.clone(), self.ts.clone(), diffusion.seeded_state(t0, 1, 0).to(self.x.device)
            model.forward_step(x, ts, table, state, gt=self.gt, mask=self.mask, tmap=tmap, **self.kwargs, batch_rows=rows)
            if model.step_chaining:
                state.copy_(diffusion.seeded_state(t0, 1, 0))
                ts.copy_(self.ts)
                model.forward_step(x, ts, table, state, gt=self.gt, mask=self.mask, tmap=tmap, embed_next=True, **self.kwargs, batch_rows=rows)
                model.forward_step(x, ts, table, state, gt=self.gt, mask=self.mask, tmap=tmap, embed_ready=True, **self.kwargs, batch_rows=rows)
        torch.cuda.synchronize(self.x.device)

    def split_into_chains(self, model, n):
        """Balanced contiguous parts of the batch (sizes differ by at most one clip)."""
        B = self.x.shape[0]
        for c in range(n):
            start = c * (B // n) + min(c, B % n)
            self.chains.append(Chain(model, self, slice(start, start + B // n + (1 if c < B % n else 0)), own_state=c > 0))

    def hook_buffers(self, hook, y, table):
        """The entry's ``HookBuffers`` of ``hook`` holding this sample's hook inputs, the hook's kernels launched once before any capture."""
        shapes = tuple(tuple(y[k].shape) for k in HOOK_KEYS)
        hk = self.hooks.get(hook._uid)
        if hk is None or hk.shapes != shapes:
            hk = self.hooks[hook._uid] = HookBuffers(hook, self, y, shapes)
            for stale in [gk for gk in self.graphs if isinstance(gk, tuple) and gk[0] in ('hook', 'first') and gk[1] == hook._uid]:
                del self.graphs[stale]
        for k in HOOK_KEYS + (() if self.gt is not None else ('inpainted_motion',)):
            hk.y[k].copy_(y[k])
        if hk.fresh:
            hook.apply_dev(hk.y['inpainted_motion'].clone(), table, torch.zeros(8, dtype=torch.int64, device=self.x.device), hk.y, hk.ws)
            torch.cuda.synchronize(self.x.device)
            hk.fresh = False
        return hk


def hook_capturable(hook, y):
    """Whether a WHOLE hook step can be captured.  The gate of the correction hook is host-known (t <= 500 and t % 50 == 0,
    eval_smpl_short.py:85) and a hook that reads its one per-call scalar on the device (HipCorrection.apply_dev: blend weight =
    table[state[0]][3]) launches the same kernels with the same arguments at every timestep.  Hooks without apply_dev, or with debug
    outputs switched on, keep the eager hook step."""
    return (hook is not None and getattr(hook, 'graph_capturable', False) and getattr(hook, 'debug', None) is None
            and getattr(hook, 'is_active', None) is not None and all(k in y for k in ('inpainted_motion',) + HOOK_KEYS)
            and os.environ.get('INTERDIFF_EAGER_HOOK') != '1')


def hook_gate(hook):
    """t -> whether t is a hook step (a hook without ``is_active`` is called in every step)."""
    if hook is None:
        return lambda t: False
    return getattr(hook, 'is_active', None) or (lambda t: True)


class Run:
    """One sample on ``entry``.  ``fused``: the plain step's update runs in the epilogue of the denoiser's last GEMM; ``split``: the
    plain steps run as the entry's chains; ``hook`` / ``hk``: the hook and, when whole hook steps are captured, its buffers."""

    def __init__(self, model, entry, table, rows, fused, split, hook, hk, tmap=None):
        self.model, self.entry, self.table, self.rows, self.tmap = model, entry, table, rows, tmap
        self.fused, self.split, self.hook, self.hk = fused, split, hook, hk

    def enqueue_forward(self):
        st = self.entry
        self.model(st.x, st.ts, out=st.x0, **st.kwargs, batch_rows=self.rows)

    def enqueue_plain(self, k):
        """k consecutive plain steps on the current (capturing) stream: every per-step scalar is read from HBM, so they fit any position.
        Inside such a run nothing touches x or the workspace between two steps, so step i's last launch also computes step i + 1's embedding
        (``entry.chain_steps``: MDM.forward_step embed_next / embed_ready, csrc/tail_h2.h -- same bits, one launch and its boundary less per step)."""
        st, model = self.entry, self.model
        links = [dict(embed_ready=i > 0, embed_next=i + 1 < k) if st.chain_steps else {} for i in range(k)]
        if self.split:                  # fork: each chain runs its k steps on its own branch; join at the end
            cur = torch.cuda.current_stream()
            for ch in st.chains:
                ch.stream.wait_stream(cur)
                with torch.cuda.stream(ch.stream):
                    for link in links:
                        model.forward_step(ch.x, ch.ts, self.table, ch.state, gt=ch.gt, mask=ch.mask, tmap=self.tmap, memctx=ch.memctx, ws=ch.ws, batch_rows=self.rows, **link, **ch.kwargs)
            for ch in st.chains:
                cur.wait_stream(ch.stream)
        elif self.fused:
            for link in links:
                model.forward_step(st.x, st.ts, self.table, st.state, gt=st.gt, mask=st.mask, tmap=self.tmap, **link, **st.kwargs, batch_rows=self.rows)
        else:
            for _ in links:
                self.enqueue_forward()
                posterior_update(st.x, st.x0, st.gt, st.mask, self.table, st.state, st.ts, self.tmap)

    def finish_hook_step(self, x0):
        """The whole-batch update from the hook's x0; it advanced chain 0's state, the others follow."""
        st = self.entry
        posterior_update(st.x, x0, None, None, self.table, st.state, st.ts, self.tmap)
        if self.split:
            for ch in st.chains[1:]:
                ch.state[:6].copy_(st.state[:6])

    def enqueue_hook_block(self, k):
        """k plain steps and ONE hook step [denoiser forward -> inpaint -> hook -> posterior update]: the same kernels in the same order
        as the eager hook step, same bits (tests)."""
        st = self.entry
        if k:
            self.enqueue_plain(k)
        self.enqueue_forward()
        if st.mask is not None:
            diffusion.inpaint(st.x0, st.gt, st.mask)
        self.hook.apply_dev(st.x0, self.table, st.state, self.hk.y, self.hk.ws)
        self.finish_hook_step(st.x0)

    def graph(self, key, enqueue, *args):
        graphs = self.entry.graphs
        if key not in graphs:
            graphs[key] = capture(enqueue, *args)
        return graphs[key]

    def plain_block(self, k):
        return self.graph((k, self.fused, self.split), self.enqueue_plain, k)

    def hook_block(self, k):
        return self.graph(('hook', self.hook._uid, k, self.fused, self.split), self.enqueue_hook_block, k)

    def eager_hook_step(self, t, model_kwargs):
        """Hook step, two-call form; its denoiser forward is replayed from a graph too (24 eager launches cost the host more than the
        GPU needs to run them)."""
        st = self.entry
        self.graph('fwd', self.enqueue_forward).replay()
        if st.mask is not None:
            diffusion.inpaint(st.x0, st.gt, st.mask)
        self.finish_hook_step(self.hook(st.x0, t, model_kwargs).contiguous())

    def first_step(self, t, ts_all, model_kwargs):
        raise NotImplementedError('only a PLMS plan has a first step')

    def play(self, plan, t_start, ts_all, model_kwargs):
        """One replay or eager hook step per op; the dumps.  ``ts_all``: the LOOP-side timesteps, what an eager hook is handed."""
        st, dump, i = self.entry, [], t_start
        for op in plan:
            if op[0] == 'plain':
                self.plain_block(op[1]).replay()
                i -= op[1]
            elif op[0] == 'hook':
                self.hook_block(op[1]).replay()
                i -= op[1] + 1
            elif op[0] == 'first':
                self.first_step(i, ts_all, model_kwargs)
                i -= 1
            elif op[0] == 'eager_hook':
                t = ts_all[i]
                t.host_value = i
                self.eager_hook_step(t, model_kwargs)
                i -= 1
            else:
                dump.append(st.x.clone())
        return dump


class PlmsRun(Run):
    """One PLMS sample on ``entry``: every step is the two-call form [forward -> inpaint -> hook -> PLMS update] on one chain (the update needs
    the eps ring, which the fused tail of the denoiser does not carry), so ``Run``'s blocks serve with the update swapped; the first step --
    two denoiser calls around the two halves of its update -- is an op of its own."""

    def __init__(self, model, entry, table, ptable, order, rows, hook, hk, tmap=None):
        super().__init__(model, entry, table, rows, False, False, hook, hk, tmap)
        self.ptable, self.order = ptable, order

    def enqueue_plain(self, k):
        st = self.entry
        for _ in range(k):
            self.enqueue_forward()
            plms_step(st.x, st.x0, st.gt, st.mask, st.ring, self.order, self.ptable, st.state, st.ts, self.tmap)

    def finish_hook_step(self, x0):
        st = self.entry
        plms_step(st.x, x0, None, None, st.ring, self.order, self.ptable, st.state, st.ts, self.tmap)

    def enqueue_forward_mid(self):
        st = self.entry
        self.model(st.x_mid, st.ts, out=st.x0, **st.kwargs, batch_rows=self.rows)

    def enqueue_first(self, hooked):
        """The first step with the captured hook in the calls ``hooked`` = (at t, at t - 1) says: the second call finds ``state[0]`` == t - 1,
        which is where ``apply_dev`` reads its blend weight."""
        st = self.entry
        for half, with_hook in enumerate(hooked):
            self.enqueue_forward() if half == 0 else self.enqueue_forward_mid()
            if st.mask is not None:
                diffusion.inpaint(st.x0, st.gt, st.mask)
            if with_hook:
                self.hook.apply_dev(st.x0, self.table, st.state, self.hk.y, self.hk.ws)
            if half == 0:
                plms_first_half(st.x, st.x0, None, None, st.ring, st.x_mid, self.ptable, st.state, st.ts, self.tmap)
            else:
                plms_second_half(st.x, st.x0, None, None, st.ring, st.x_mid, self.ptable, st.state)

    def first_step(self, t, ts_all, model_kwargs):
        """Captured when no call of it takes an eager hook; else the two forwards are replayed and the rest runs eagerly."""
        st, gate = self.entry, hook_gate(self.hook)
        hooked = (bool(gate(t)), bool(gate(t - 1)))
        if self.hk is not None or not any(hooked):
            self.graph(('first', self.hook._uid if any(hooked) else None) + hooked, self.enqueue_first, hooked).replay()        # (a first step without a hook call serves any hook)
            return
        for half, (ti, with_hook) in enumerate(zip((t, t - 1), hooked)):
            self.graph('fwd' if half == 0 else 'fwd_mid', self.enqueue_forward if half == 0 else self.enqueue_forward_mid).replay()
            if st.mask is not None:
                diffusion.inpaint(st.x0, st.gt, st.mask)
            x0 = st.x0
            if with_hook:
                th = ts_all[ti]
                th.host_value = ti
                x0 = self.hook(st.x0, th, model_kwargs).contiguous()
            if half == 0:
                plms_first_half(st.x, x0, None, None, st.ring, st.x_mid, self.ptable, st.state, st.ts, self.tmap)
            else:
                plms_second_half(st.x, x0, None, None, st.ring, st.x_mid, self.ptable, st.state)


def sample(diff, model, img, model_kwargs, hook, seed, todo, dump_steps, t_start, shard=None, sampler=('ddpm',)):
    """``todo`` reverse steps from x_{t_start} = ``img`` on captured graphs: the plain step [denoiser forward -> inpaint + posterior ->
    advance] with its per-step scalars (c1, c2, sigma, t, loop index, seed) in HBM, and whole hook steps when the hook allows it.
    ``sampler``: whose table rows (``GaussianDiffusion._rows``).  The captured launches bake the table's and the timestep map's addresses
    in, so the graphs are kept per (schedule, sampler).  ``t_start``, the plan and the hook gate count loop-side (spaced) steps; ``ts``
    holds the model's timesteps (``diff._tmap``)."""
    y = model_kwargs.get('y', {})
    B, T, dev = img.shape[0], img.shape[-1], img.device
    first, total = (0, B) if shard is None else shard
    per_clip = img.numel() // B
    elem0 = first * per_clip                    # position of this batch's x[0] inside the whole (possibly sharded) batch: the Philox counter base (p_sample_loop checked it)
    rows = total * T                            # the WHOLE batch's token rows: what every launch's feed-forward tile is picked by (MDM._pick_ffn_tile)
    plms = sampler[0] == 'plms'                 # ('plms', order): the hook still reads its blend weight from a {c1, c2, sigma, t/1000} table
    table, tmap = diff._table(dev, ('ddpm',) if plms else sampler), diff._tmap(dev)
    mask, gt = diffusion.mask_operands(y.get('inpainting_mask'), y.get('inpainted_motion'), img)
    cond, zpo = y['cond'], model_kwargs.get('zero_pose_obj')
    key = (diff._uid, tuple(img.shape), mask is not None, tuple(cond.shape), model.ffn_graph_key(rows)) + (() if sampler == ('ddpm',) and tmap is None else (sampler, tmap is not None))    # the captured launches bake the feed-forward kernel choice in
    if zpo is not None:
        key += (tuple(zpo.shape),)
    st, fresh = Entry.of(model, key, img, cond, mask is not None, zpo)
    st.load(cond, zpo, gt, mask)
    pools_before = model.shape_buffer_keys() if fresh else None      # (taken before the first fold of this shape allocates its memory context)
    model.prepare_memory(st.cond)                   # once per sample, on the current stream (inside the caller's clock)
    if plms and st.ring is None:
        st.ring, st.x_mid = torch.empty(3, img.numel(), dtype=torch.float32, device=dev), torch.empty_like(img)
    if fresh:
        st.warm_up_plms(model, diff._plms_table(dev), rows, tmap) if plms else st.warm_up(model, table, rows, tmap)
        st.pool_keys = model.shape_buffer_keys() - pools_before      # what this entry made the denoiser allocate: released with the entry

    fused = diff.fuse_plain_step and model.supports_forward_step and not plms
    # Chains: at <= 16 clips every kernel of a step is one partial wave of workgroups bounded by latency (operand round trips,
    # kernel boundaries), so the two halves of the batch, stepped as independent kernel chains on two branches of the SAME captured
    # graph, overlap each other's dead time.  Clips never interact in a plain step, the noise of a chain is drawn at the whole
    # batch's counters (state[6]), so the result is bit-identical to the single chain.  Hook steps stay whole-batch.  An odd batch
    # splits into parts that differ by one clip (more than two chains measured slower: 0.296 / 0.309 vs 0.281 ms per step with 3 / 4 at B = 16).
    # Smaller batches: launch-latency bound either way, and the feed-forward's 16-row grid already spans the chip (tools/small_batch_ab.py:
    # equal at B = 8, one chain 7 % faster at B = 4).
    nch = diffusion.N_CHAINS
    split = (fused and diff.split_chains and nch > 1 and 2 * nch <= B <= diffusion.SPLIT_MAX_BATCH
             and B * T > (model.one_chain_max_rows() if diff.split_min_rows is None else diff.split_min_rows))
    if split:
        if not st.chains:
            st.split_into_chains(model, nch)
        for ch in st.chains:                        # this sample's memory, folded per chain (its layout is per batch)
            ch.cond.copy_(st.cond[:, ch.sl])
            model.prepare_memory(ch.cond, into=ch.memctx)
    chain_steps = diff.chain_plain_steps and fused and model.step_chaining
    if st.chain_steps != chain_steps:               # captured launches bake it in
        st.graphs.clear()
        st.chain_steps = chain_steps
    fuse_hook = hook_capturable(hook, y)
    hk = st.hook_buffers(hook, y, table) if fuse_hook else None
    if plms:
        run = PlmsRun(model, st, table, diff._plms_table(dev), sampler[1], rows, hook, hk, tmap)
    else:
        run = Run(model, st, table, rows, fused, split, hook, hk, tmap)

    st.x.copy_(img)
    st.state.copy_(diffusion.seeded_state(t_start, seed, elem0))
    if split:                                       # the other chains' states: the same schedule position, their x starts where their clips do
        for ch in st.chains[1:]:                    # (an odd offset when T % 4 != 0: the per-row form of the fused update takes any)
            ch.state.copy_(diffusion.seeded_state(t_start, seed, elem0 + ch.sl.start * per_clip))
    st.ts.fill_(diff.timestep_map[t_start])
    if plms:                                        # the first step is loop step 0: the plan of the rest starts at loop index 1
        plan = [('first',)] + ([('dump', 0)] if dump_steps is not None and 0 in dump_steps else [])
        plan += plan_steps(t_start - 1, todo - 1, hook_gate(hook), dump_steps, fuse_hook, it0=1)
    else:
        plan = plan_steps(t_start, todo, hook_gate(hook), dump_steps, fuse_hook)
    dump = run.play(plan, t_start, diff._timesteps(B, dev, loop_side=True), model_kwargs)
    return dump if dump_steps is not None else st.x.clone()
