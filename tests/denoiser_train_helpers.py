"""What the denoiser trainers' test modules share (test_mdm_train, test_mdm_encoder_train, test_skeleton_mdm_train, test_pointnet2_finetune): conversions,
the relative-error measure, the gradient gates (recorded e_ref; ``flat_gate`` / ``shape_gate`` where nothing is recorded), the comparison of every gradient tensor,
the SMPL trainers' synthetic point, the injected gradients of the optimiser tests, the check of a module's C entries, and the far-parameter count of the trajectory
tests.  Each module keeps its own tests, fixtures, points and figures."""
import os
import re
import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
FLOOR = 1e-5


def tn(a):
    return torch.from_numpy(np.asarray(a))


def rel(a, b):
    a, b = (x.detach().cpu().double() if isinstance(x, torch.Tensor) else tn(x).double() for x in (a, b))
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-300))


def betas():
    from interdiff_amd.diffusion import get_named_beta_schedule
    return get_named_beta_schedule('cosine', 1000, 1.)


def gate(e_ref):
    """The project's gradient gate: 4 x the reference's own fp32 distance from fp64, floored."""
    return max(4.0 * float(e_ref), FLOOR)


def check_new_symbols(symbols):
    """Every entry of ``symbols`` {name: argument list} is declared with these types in include/interdiff_hip.h, typed in _lib._SIGS and exported, and the ABI
    version has not moved (additive entries).  Returns the loaded library."""
    from interdiff_amd import _lib
    src = re.sub(r'\s+', ' ', open(os.path.join(ROOT, 'include', 'interdiff_hip.h')).read())
    for name, args in symbols.items():
        assert '%s(%s);' % (name, args) in src, name
        assert name in _lib._SIGS and len(_lib._SIGS[name][1]) == args.count(',') + 1, name
    lib = _lib.load()
    for name in symbols:
        assert hasattr(lib, name)
    assert lib.interdiff_abi_version() == _lib.ABI_VERSION == 17
    return lib


def flat_gate(ref, r32, wk_names):
    """The absolute gate of the tests that have no recorded e_ref: 1e-4 max|g64| on every tensor.  For the ``wk`` tensors (``wk_names``) that figure is below what fp32 can
    compute (the oracle run in fp32 is itself up to 2.9e-2 of max|g64| away at past_len 2), so theirs is four times the fp32 rounding noise of the same point: the
    rounding error of d wk[n] is proportional to the sum of the magnitudes of the products it adds up, the constant c32 is the worst of the fp32 oracle's
    ``wk`` tensors on that scale (``r32``: the oracle on the same point in fp32), and 4 is the project's multiple of a reference's own error.  Never below
    1e-4 max|g64| and never above 1e-4 of the sum of magnitudes.  Returns (gate_abs(k), the widest ``wk`` gate as a fraction of max|g64|)."""
    WK = wk_names
    top = lambda k: float(ref['grads'][k].abs().max())
    c32 = max(float((r32['grads'][k].double() - ref['grads'][k]).abs().max()) / ref['wk_scale'][k] for k in WK)

    def gate_abs(k):
        if k not in WK:
            return 1e-4 * top(k)
        return max(1e-4 * top(k), min(1e-4, 4.0 * c32) * ref['wk_scale'][k])
    return gate_abs, max(gate_abs(k) / top(k) for k in WK)


def d32_of(ref, r32, k):
    """The fp32 oracle's distance from the fp64 oracle on tensor ``k`` of the same point: the reference arithmetic's own error, not the code under test's."""
    return float((r32['grads'][k].double() - ref['grads'][k]).abs().max())


def shape_gate(ref, r32, wk_names):
    """The gate of the SMPL trainer's synthetic shapes: ``flat_gate`` for the ``wk`` tensors; for every other tensor max(1e-4 max|g64|, 4 d32(k)), d32 the fp32
    oracle's distance from the fp64 oracle on the same point (``encoder.layers.6.queries`` at past_len 2 is 3e-4 .. 9e-4 of max|g64| away in fp32 itself, so the flat
    1e-4 is below what fp32 computes there; tests/test_mdm_encoder_train.py caps 4 d32 at 1e-2 max|g64| in an unmarked test).  Returns (gate_abs(k), the widest ``wk``
    gate and the widest other gate, both as fractions of max|g64|)."""
    flat, widest_wk = flat_gate(ref, r32, wk_names)
    top = lambda k: float(ref['grads'][k].abs().max())

    def gate_abs(k):
        return flat(k) if k in wk_names else max(flat(k), 4.0 * d32_of(ref, r32, k))
    return gate_abs, widest_wk, max(gate_abs(k) / top(k) for k in ref['grads'] if k not in wk_names and top(k) > 0)


def worst_d32(ref, r32, wk_names):
    """(the worst 4 d32(k) / max|g64| over the non-``wk`` tensors, its name; the worst fp32 ``wk`` distance on max|g64| and on ``wk_scale``): what the cap tests assert on."""
    worst, name, wk_top, wk_scale = 0.0, None, 0.0, 0.0
    for k, g in ref['grads'].items():
        top, d = float(g.abs().max()), d32_of(ref, r32, k)
        if k in wk_names:
            wk_top, wk_scale = max(wk_top, d / top), max(wk_scale, d / ref['wk_scale'][k])
        elif top > 0 and 4.0 * d / top > worst:
            worst, name = 4.0 * d / top, k
    return worst, name, wk_top, wk_scale


def compare_all(grads, ref, names, gate_abs, tag):
    """Every gradient tensor ``names`` of ``grads`` {name: device tensor} against the fp64 oracle; gate_abs(k) the absolute gate.  A tensor the oracle has exactly zero
    must be exactly zero.  Prints before it asserts; returns the worst fraction of a gate."""
    worst, worst_wk, worst_frac, bad = 0.0, 0.0, 0.0, []
    for k in names:
        top = float(ref['grads'][k].abs().max())
        dist, g = float((grads[k].cpu().double() - ref['grads'][k]).abs().max()), gate_abs(k)
        if top == 0.0:
            if dist != 0.0:
                bad.append('%s: %.3e where the oracle is exactly zero' % (k, dist))
            continue
        if k.endswith('.wk'):
            worst_wk = max(worst_wk, dist / top)
        else:
            worst = max(worst, dist / top)
        worst_frac = max(worst_frac, dist / g)
        if dist > g:
            bad.append('%s %.3e > %.3e (of max|g64|: %.3e)' % (k, dist, g, dist / top))
    print('%s: %d gradient tensors: worst rel err %.3e (the wk tensors, on max|g64|: %.3e), worst fraction of its gate %.3f' % (tag, len(names), worst, worst_wk, worst_frac))
    assert not bad, bad
    return worst_frac


def synthetic_point(seed, B, T, past, mem_len=None):
    """Inputs of a synthetic SMPL point (no golden, no oracle): x0 = the tokens of a synthetic clip batch, seeded t / eps, pc [B,256] and, when ``mem_len`` is given,
    cond [mem_len,B,256]; x_t = q_sample(x0, t, eps)."""
    from interdiff_amd import synthetic as syn
    from tests import fixtures as fx
    from tests import losses_oracle as lo
    x0 = tn(syn.make_clip_batch(seed, B, T, past_len=past, n_points=8)['gt'])
    rs = np.random.RandomState(seed + 1)
    t, eps, pc = tn(rs.randint(0, 1000, size=B).astype(np.int64)), fx._randn(rs, B, 1, 144, T), 0.5 * fx._randn(rs, B, 256)
    p = dict(x0=x0, t=t, eps=eps, pc=pc, x_t=lo.q_sample(betas(), x0, t, eps), past=past)
    if mem_len is not None:
        p['cond'] = fx._randn(rs, mem_len, B, 256)
    return p


def adam_vectors(n, steps=3, seed=7430):
    """``steps`` seeded gradient vectors of ``n`` entries, the special values at known places (as far as ``n`` reaches): exact zeros [0,64), +-1e-40 (denormal)
    [64,128), a band around eps = 1e-8 [128,192), a log-uniform bulk e^-9 .. 1 behind them (the recipe of tests/test_skeleton_finetune.py).  Below 193 entries the
    bands shrink to an eighth of ``n`` each, so that a bulk is left."""
    rs = np.random.RandomState(seed)
    w = 64 if n > 192 else n // 8
    gs = [(s * rs.standard_normal(n) * np.exp(rs.uniform(-9, 0, n))).astype(np.float32) for s in (1.0, -0.5, 2.0, -1.5, 0.7)[:steps]]
    for gv in gs:
        gv[0:w] = 0.0
        gv[w:w + w // 2] = np.float32(1e-40)
        gv[w + w // 2:2 * w] = np.float32(-1e-40)
        gv[2 * w:3 * w] = (1e-8 * np.exp(rs.uniform(-2, 2, w)) * rs.choice([-1, 1], w)).astype(np.float32)
    return gs


def far_parameters(got, theta, names, y):
    """(how many entries of the tensors ``names`` of ``got`` lie further than 8 y from the fp64 trajectory ``theta``, the largest distance)."""
    far, worst = 0, 0.0
    for k in names:
        dist = (got[k].cpu().double() - theta[k]).abs()
        far += int((dist > 8 * y).sum())
        worst = max(worst, float(dist.max()))
    return far, worst
