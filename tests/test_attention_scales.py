"""The denoiser's attention at the logit scales of a TRAINED model, against the oracle run in float64.

Every other numerical test of the denoiser runs on one weight draw (a PyTorch default initialisation: logits of standard deviation ~0.6, softmax rows
nearly uniform).  Here the Q and K rows of every standard self-attention and every cross-attention are multiplied by a gain g (tests/fixtures.py
``sharpen_attention``): g = 2 gives the spread of a trained checkpoint (logit std ~2.4, rows led by one or two keys), g = 4 saturates them (std ~9.5, max |logit| ~50).
That is where an absolute logit error of the split-f16 planes becomes a relative probability error, where the exp(m_old - m_new) rescale of the K/V-tiled kernel
does something, where the power-of-two scales of the folded cross-attention memory move, where __expf sees arguments of -50 and where a padded key column
that leaked would show.  Nothing is recorded from the reference: the float64 run of oracle/denoiser.py is the ground truth, and its float32 run on the same inputs
(``e_oracle32``) is the yardstick of what an honest fp32 implementation delivers.

Errors are max|d| / max|ref|.  Asserted on every case, every route:
  * north star: HIP vs fp64 <= 1e-4 (header of tests/test_hip_parity.py) and every output finite;
  * the fp32 routes (everything denied; ``ffn_math = 'exact'``): <= max(2e-6, 4 e_oracle32) -- 2e-6 is the gate of
    test_mdm_forward_with_either_self_attention_kernel_by_deny_list, 4 the headroom that gate has over the 5-7e-7 of the oracle's own fp32 run at g = 1;
  * the split routes: the project's rule, err_split <= max(2 err_fp32_route, 2e-6), against the fp32 route of the same contraction -- the fp32 self-attention
    for the self-attention kernels, the fp32 row block for the cross-attention.
The routes are selected by the debug deny list (tests/test_hip_parity.py DENY_CASES) and ``ffn_math``; the measured table is in DESIGN.md
("Attention accuracy at trained logit scales")."""
import functools
import numpy as np
import pytest
import torch
from tests import fixtures as fx
from tests.test_hip_parity import DENY_CASES, _philox_step, rel, dev
from oracle import denoiser as oden, diffusion as odf

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = 'cuda'
NORTH_STAR, FP32_GATE, FP32_HEADROOM, SPLIT_FACTOR = 1e-4, 2e-6, 4.0, 2.0
GAINS = (2, 4)
SPLIT_ATTENTION_MAX_T = 192          # csrc/attn_h2.h MAX_T

ROUTES = {            # name -> (debug deny list, ffn_math)
    'default': ('', 'split'),
    'amax_split_attention': ('self_attn_h2_kernel<planes in>', 'split'),      # fp32 rows out of the projection; the attention splits them by the measured amax per tile
    'fp32_attention': ('self_attn_h2_kernel', 'split'),
    'fp32_rowblock': ('rowblock', 'split'),                                    # fp32 cross-attention (and QaN taps, out of scope here)
    'all_fp32': (DENY_CASES[-1][0], 'split'),
    'exact': ('', 'exact'),
}
# (split route, the fp32 route of the contraction it is measured against)
SPLIT_RULE = [('default', 'fp32_attention'), ('amax_split_attention', 'fp32_attention'), ('default', 'fp32_rowblock')]
# T: below / straddling the 16- and 32-key paddings and the 32-query tile of csrc/attn_h2.h | the bench clip | first clip past NIT0's 128-key sweep and NC0 |
# last clip of the split kernel | fp32 one-shot kernel only | the K/V-tiled kernel (257 = four full 64-key tiles + one key: the running maximum moves between
# tiles and the last tile holds a single key)
CLIPS = [1, 13, 17, 33, 100, 129, 192, 193, 208, 209, 257]
MEMORIES = [1, 7, 10, 16]            # cross-attention memory lengths at (B, T) = (2, 35)

_models = {}


def model_for(weights_key, route, make=None):
    """One model per (weights, route), reused across shapes.  ``weights_key``: the arguments of fx.mdm_weights_sharp, or any key with ``make`` building the model."""
    from interdiff_amd.mdm import MDM
    m = _models.get((weights_key, route))
    if m is None:
        m = make() if make is not None else MDM(fx.mdm_weights_sharp(*weights_key), device=DEV)
        m.ffn_math = ROUTES[route][1]
        _models[(weights_key, route)] = m
    return m


def on_route(route, model, call, kind='denoiser', T=1):
    """``call(model)`` with the route's deny list in force; the list is cleared whatever happens.  Then ``arithmetic_report()`` must name the route that ran -- on the default
    route nothing silently ran elsewhere.  ``kind``: 'denoiser', 'skeleton' (its embedding and heads are fp32 on every route) or 'encoder' (the report describes the decoder's
    layers, which an encoder call does not launch: only the list of refused kernels is checked).  ``T``: a clip longer than 192 frames never launches the split-f16 attention
    (csrc/denoiser.hip takes the fp32 kernels at launch time, which the pack-time report does not know), so the two routes that deny only that kernel are the default route
    there and nothing is asked of the report."""
    from interdiff_amd import _lib
    deny = ROUTES[route][0]
    try:
        _lib.debug_deny_exclusive(deny)
        out = call(model)
        rep = model.arithmetic_report()
    finally:
        _lib.debug_deny_exclusive('')
    if T > SPLIT_ATTENTION_MAX_T and route in ('amax_split_attention', 'fp32_attention'):
        return out
    assert bool(rep['not_exclusive']) == bool(deny), rep
    if kind == 'encoder':
        return out
    std = [d for d in rep['layers'] if d['kind'] == 'std']
    layers_split = all(d['ffn'] == 'split' and d['rowblock'] == 'split' and d.get('qkv', 'split') == 'split' and d.get('self_attention', 'split') == 'split' for d in rep['layers'])
    if route == 'default':
        assert layers_split and (rep['all_split'] or kind == 'skeleton'), rep
        assert len(std) == 2 and all(d['qkv_hands_over_planes'] for d in std), rep
    elif route == 'amax_split_attention':
        assert all(d['self_attention'] == 'split' and not d['qkv_hands_over_planes'] for d in std), rep
    elif route == 'fp32_attention':
        assert all(d['self_attention'] == 'exact' for d in std), rep
    elif route == 'fp32_rowblock':
        assert all(d['rowblock'] == 'exact' for d in rep['layers']), rep
    else:                                                 # all_fp32, exact
        assert all(d['ffn'] == 'exact' and d['rowblock'] == 'exact' and d.get('qkv', 'exact') == 'exact' and d.get('self_attention', 'exact') == 'exact'
                   for d in rep['layers']) and rep['embedding_and_heads'] == 'exact', rep
    return out


def judge(name, err, e32, finite, routes=ROUTES, split_rule=SPLIT_RULE):
    """Record the measured errors, then the three assertion kinds of the module docstring (all of them evaluated, so that the record is complete when one fails)."""
    fx.record_parity(name, e_oracle32=e32, **err)
    print('%s: oracle fp32 %.2e | %s' % (name, e32, '  '.join('%s %.2e' % (r, err[r]) for r in routes)))
    bad = []
    for r in routes:
        if not finite[r]:
            bad.append('%s: non-finite output' % r)
        if not err[r] <= NORTH_STAR:
            bad.append('%s: %.3e > north star %.0e' % (r, err[r], NORTH_STAR))
    for r in ('all_fp32', 'exact'):
        if r in routes and not err[r] <= max(FP32_GATE, FP32_HEADROOM * e32):
            bad.append('%s (fp32 route): %.3e > max(%.0e, %g x oracle fp32 %.3e)' % (r, err[r], FP32_GATE, FP32_HEADROOM, e32))
    for s, f in split_rule:
        if not err[s] <= max(SPLIT_FACTOR * err[f], FP32_GATE):
            bad.append('%s (split): %.3e > max(%g x %s %.3e, %.0e)' % (s, err[s], SPLIT_FACTOR, f, err[f], FP32_GATE))
    assert not bad, '%s: %s' % (name, '; '.join(bad))


def measure(weights_key, x, ts, cond, routes=ROUTES):
    """(errors vs the oracle in float64 per route, the oracle's own fp32 error, finiteness per route) of one forward."""
    sd = fx.mdm_weights_sharp(*weights_key)
    ref64 = oden.mdm_forward(sd64_of(weights_key), x.double(), ts, cond.double())
    e32 = rel(oden.mdm_forward(sd, x, ts, cond), ref64)
    err, finite = {}, {}
    xd, td, cd = x.to(DEV), ts.to(DEV), cond.to(DEV)
    for r in routes:
        got = on_route(r, model_for(weights_key, r), lambda m: m(xd, td, y={'cond': cd}), T=x.shape[-1]).cpu()
        err[r], finite[r] = rel(got, ref64), bool(torch.isfinite(got).all())
    return err, e32, finite


@functools.lru_cache(None)
def sd64_of(weights_key):
    return {k: v.double() for k, v in fx.mdm_weights_sharp(*weights_key).items()}


# ------------------------------------------------------------------------------------------ every code path of the three self-attention kernels
@pytest.mark.parametrize('T', CLIPS)
@pytest.mark.parametrize('g', GAINS)
def test_forward_at_trained_logit_scales_every_clip_length(lib, g, T):
    B = 2 if T <= 129 else 1
    err, e32, finite = measure((g,), *fx.mdm_inputs(B, T))
    judge('attn_scale_g%g_B%d_T%d' % (g, B, T), err, e32, finite)


# ------------------------------------------------------------------------------------------ the folded cross-attention memory
@pytest.mark.parametrize('M', MEMORIES)
@pytest.mark.parametrize('g', GAINS)
def test_forward_at_trained_logit_scales_every_memory_length(lib, g, M):
    """Memory lengths 1..16 (10 = the compact layout, the others the generic one with absent slots masked): at g = 4 the folded G of interdiff_mdm_prepare_memory is sixteen
    times its initialisation size, so the per-(layer, sample) power-of-two scales of its f16 planes move by four."""
    B, T = 2, 35
    rs = np.random.RandomState(7000 + 100 * M + T)                 # (built as test_denoiser_any_memory_length_and_long_clips builds them)
    x = torch.from_numpy(rs.standard_normal((B, 1, 144, T)).astype(np.float32))
    ts = torch.from_numpy(rs.randint(0, 1000, size=B).astype(np.int64))
    cond = torch.from_numpy(rs.standard_normal((M, B, 256)).astype(np.float32))
    err, e32, finite = measure((g,), x, ts, cond)
    assert model_for((g,), 'default').mem_len == M
    judge('attn_scale_g%g_B%d_T%d_M%d' % (g, B, T, M), err, e32, finite)


# ------------------------------------------------------------------------------------------ one layer's attention at a time
LOCALISERS = {'self_layer0': (4, (0,), ()), 'self_layer7': (4, (7,), ()), 'cross_only': (4, (), None)}


@pytest.mark.parametrize('which', sorted(LOCALISERS))
def test_one_attention_at_gain_4_localises_a_failure(lib, which):
    """Gain 4 on layer 0's self-attention only, on layer 7's only, on the cross-attention only, at the bench clip: which contraction a failure above belongs to."""
    routes = ('default', 'fp32_attention', 'fp32_rowblock')
    err, e32, finite = measure(LOCALISERS[which], *fx.mdm_inputs(2, 100), routes=routes)
    judge('attn_scale_g4_%s_B2_T100' % which, err, e32, finite, routes=routes, split_rule=[('default', 'fp32_attention'), ('default', 'fp32_rowblock')])


# ------------------------------------------------------------------------------------------ per-step errors do not compound
def test_twenty_plain_steps_at_trained_scale_graph_equals_eager_and_oracle(lib):
    """20 plain steps of p_sample_loop at g = 2: the graph route equals the eager route fed the materialised Philox stream bit for bit, and both are within 1e-4 of the
    oracle's loop (the construction of test_one_layer_failing_its_f16_range_proof_runs_mixed)."""
    from interdiff_amd.diffusion import create_gaussian_diffusion
    sd = fx.mdm_weights_sharp(2)
    model = model_for((2,), 'default')
    diff = create_gaussian_diffusion('cosine', 1000)
    bt, y = fx.timed_inputs(2)
    yd, x_t = dev(y), bt['noise'].to(DEV)
    n, seed = 20, 4321
    kw = dict(noise=x_t, clip_denoised=False, model_kwargs={'y': yd}, n_steps=n, first_t=fx.TIMED_FIRST_T)
    g = diff.p_sample_loop(model, tuple(x_t.shape), seed=seed, **kw)
    draw = _philox_step(lib, seed)
    stream = [draw(it, x_t) for it in range(n)]
    ea = diff.p_sample_loop(model, tuple(x_t.shape), step_noise=torch.stack(stream), **kw)
    rep = model.arithmetic_report()
    assert rep['all_split'] and all(d['qkv_hands_over_planes'] for d in rep['layers'] if d['kind'] == 'std'), rep
    assert torch.isfinite(g).all()
    assert torch.equal(g, ea), float((g - ea).abs().max())
    ref = odf.p_sample_loop(lambda x, t, y: oden.mdm_forward(sd, x, t, y['cond']), tuple(x_t.shape), odf.make_schedule(1000),
                            bt['noise'].clone(), lambda i, xx: stream[i].cpu(), {'y': y}, n_steps=n, first_t=fx.TIMED_FIRST_T)
    e = rel(g, ref)
    fx.record_parity('attn_scale_g2_B2_T100_chain_20_steps', window_20_steps=e)
    print('20 plain steps at g = 2 vs the oracle loop: %.2e' % e)
    assert e <= NORTH_STAR, e


# ------------------------------------------------------------------------------------------ the other users of these kernels
@pytest.mark.parametrize('g', GAINS)
def test_encoder_at_trained_logit_scales(lib, g):
    """MDM._get_embeddings with the gain on the encoder's two standard layers: ``cond`` against oracle get_embeddings in float64."""
    key = (g, None, None, g)
    ei = fx.embedding_inputs()
    names = ('body_pose', 'body_trans', 'obj_angles', 'obj_trans', 'obj_points')
    ref64, _ = oden.get_embeddings(sd64_of(key), *(ei[k].double() for k in names), fx.PAST)
    e32 = rel(oden.get_embeddings(fx.mdm_weights_sharp(*key), *(ei[k] for k in names), fx.PAST)[0], ref64)
    d = dev(ei)
    routes = ('default', 'all_fp32', 'exact')
    err, finite = {}, {}
    for r in routes:
        got = on_route(r, model_for(key, r), lambda m: m._get_embeddings(*(d[k] for k in names), fx.PAST)[0], kind='encoder').cpu()
        err[r], finite[r] = rel(got, ref64), bool(torch.isfinite(got).all())
    judge('attn_scale_g%g_embeddings_B%d_T%d' % ((g,) + fx.EMB_SHAPE[1::-1]), err, e32, finite, routes=routes, split_rule=[('default', 'all_fp32')])


@pytest.mark.parametrize('g', GAINS)
def test_skeleton_denoiser_at_trained_logit_scales(lib, g):
    """The skeleton-mode denoiser (tests/test_skeleton_mdm.py's model against its restatement oracle) with the same row scaling at a ragged shape, both arithmetics.  The
    inputs keep the predicted quaternion away from zero, as that file's fixture does (2 / (q . q) is ill-conditioned there)."""
    from interdiff_amd import skeleton as sk
    from tests import skeleton_mdm_oracle as smo
    from tests.test_skeleton_mdm import weights, rand_case
    B, T = 3, 21
    sd = fx.sharpen_attention(weights(), g)
    sd64 = {k: v.double() for k, v in sd.items()}
    x, ts, zp, cond = rand_case(900 + B * 100 + T, B, T)
    ref64 = smo.forward(sd64, x.double(), ts, zp.double(), cond.double())
    assert float((ref64[:, 0, -4:] ** 2).sum(1).min()) >= 0.25
    e32 = rel(smo.forward(sd, x, ts, zp, cond), ref64)
    xd, td, zd, cd = x.to(DEV), ts.to(DEV), zp.to(DEV), cond.to(DEV)
    routes = ('default', 'fp32_attention', 'fp32_rowblock', 'all_fp32', 'exact')
    err, finite = {}, {}
    for r in routes:
        m = model_for(('skeleton', g), r, make=lambda: sk.SkeletonMDM(sd, device=DEV))
        got = on_route(r, m, lambda m: m(xd, td, zero_pose_obj=zd, y={'cond': cd}), kind='skeleton').cpu()
        err[r], finite[r] = rel(got, ref64), bool(torch.isfinite(got).all())
    judge('attn_scale_g%g_skeleton_B%d_T%d' % (g, B, T), err, e32, finite, routes=routes, split_rule=[('default', 'fp32_attention'), ('default', 'fp32_rowblock')])

