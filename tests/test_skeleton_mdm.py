"""The HO-GCN skeleton denoiser (model/diffusion_skeleton.py ``MDM``) on the HIP kernels: ``interdiff_amd.skeleton.SkeletonMDM``
(conditioning encoder with the shape embedding, feed-forward width 256 riding the 1024-wide streams zero-padded, keypoint head
``calc_obj_pred`` inside the heads GEMM: csrc/skel_head.h) against the reference's own outputs (tests/golden/skel_mdm.npz,
tests/golden/make_golden_skeleton_mdm.py) and the CPU restatement tests/skeleton_mdm_oracle.py.

Parity gate: max|d| / max|ref| <= 1e-4; bit-identity claims are ``torch.equal``.  The fixture's inputs keep the
predicted quaternion away from zero (``min_qq`` >= 0.25, asserted by the generator on the reference's own run): 2 / (q . q) is
ill-conditioned there, and no token is excluded from any comparison here."""
import numpy as np
import pytest
import torch
from tests import fixtures as fx
from tests import skeleton_mdm_oracle as smo
from interdiff_amd import skeleton as sk
from interdiff_amd import synthetic as syn
from interdiff_amd import mdm as hmdm
from interdiff_amd import _lib

DEV = 'cuda'
GATE = 1e-4
SHAPES = [(1, 20), (3, 21), (64, 20), (2, 35)]


def rel(a, b):
    a, b = (x.detach().cpu().double().numpy() if isinstance(x, torch.Tensor) else np.asarray(x, np.float64) for x in (a, b))
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def close(a, b, tol, what):
    e = rel(a, b)
    print('%s: rel err %.3e (gate %.1e)' % (what, e, tol))
    assert e <= tol, '%s: rel err %.3e > %.1e' % (what, e, tol)
    return e


def g():
    z = fx.golden('skel_mdm.npz')
    return {k: z[k] for k in z.files}


def weights(dtype=torch.float32, seed=None):
    return {k: torch.from_numpy(v).to(dtype) for k, v in syn.skeleton_mdm_state_dict(int(g()['seed']) if seed is None else seed).items()}


def tn(a, dtype=None):
    t = torch.from_numpy(np.asarray(a))
    return t.to(dtype) if dtype is not None and t.is_floating_point() else t


def mask_for(gt):
    m = torch.ones(gt.shape, dtype=torch.bool)
    m[..., fx.PAST:] = False
    return m


def rand_case(seed, B, T):
    rs = np.random.RandomState(seed)
    return (fx._randn(rs, B, 1, 106, T), torch.from_numpy(rs.randint(0, 1000, B)), torch.from_numpy((0.3 * rs.standard_normal((B, 12, 3))).astype(np.float32)),
            fx._randn(rs, fx.PAST, B, 256))


# ------------------------------------------------------------------------------------------------------------ CPU

def test_condition_on_the_inputs_is_recorded():
    z = g()
    assert float(z['min_qq']) >= 0.25 and float(z['c50_rel64']) <= 2.5e-5 and float(z['c1000_rel64']) <= 2.5e-5


def test_restatement_equals_golden_embeddings_and_forwards():
    z, sd = g(), weights(torch.float64)
    tb = lambda k: tn(z[k], torch.float64).transpose(0, 1).contiguous()
    cond, gt = smo.get_embeddings(sd, tb('emb_body'), tb('emb_obj'), tb('emb_pose'), tn(z['emb_zero'], torch.float64))
    close(cond, z['emb_cond'], 1e-5, 'restated _get_embeddings cond')
    assert rel(gt, z['emb_gt']) == 0.0
    for T in (20, 35):
        out = smo.forward(sd, *(tn(z['fwd%d_%s' % (T, k)], torch.float64) for k in ('x', 'ts', 'zero', 'cond')))
        close(out, z['fwd%d_out' % T], 1e-5, 'restated forward T=%d' % T)


def test_restatement_equals_golden_config1_chain():
    """The 50-step chain of BASELINE config #1 (identity hook) on oracle/diffusion.py with the restated model, fp32."""
    from oracle import diffusion as odf
    z, sd = g(), weights()
    gt, noise, zp, cond = (tn(z['c50_' + k]) for k in ('gt', 'noise', 'zero_pose_obj', 'cond'))
    stream = fx.NoiseStream(int(z['c50_noise_seed']))
    got = odf.p_sample_loop(lambda x, t, y: smo.forward(sd, x, t, zp, y['cond']), tuple(gt.shape), odf.make_schedule(50), noise.clone(),
                            lambda i, x: stream.next_like(x), {'y': dict(cond=cond, inpainted_motion=gt, inpainting_mask=mask_for(gt))},
                            denoised_fn=lambda x, t, kw: x)
    close(got, z['c50_final'], GATE, 'restated 50-step chain')


def test_calc_obj_pred_does_not_normalise():
    """two_s = 2 / (q . q): a quaternion of length 2 gives the same rotation as the unit one, and the keypoints are R z + t."""
    rs = np.random.RandomState(3)
    q = torch.from_numpy(rs.standard_normal((5, 2, 4)))
    pose = torch.cat([torch.from_numpy(rs.standard_normal((5, 2, 3))), q], dim=2)
    zero = torch.from_numpy(rs.standard_normal((2, 12, 3)))
    a = smo.calc_obj_pred(pose, zero)
    pose2 = pose.clone()
    pose2[..., 3:] *= 2.0
    assert rel(smo.calc_obj_pred(pose2, zero), a) < 1e-12
    qn = q / q.norm(dim=-1, keepdim=True)
    x, y, zz, w = qn.unbind(-1)
    R = torch.stack([1 - 2 * (y * y + zz * zz), 2 * (x * y - zz * w), 2 * (x * zz + y * w),
                     2 * (x * y + zz * w), 1 - 2 * (x * x + zz * zz), 2 * (y * zz - x * w),
                     2 * (x * zz - y * w), 2 * (y * zz + x * w), 1 - 2 * (x * x + y * y)], dim=-1).reshape(5, 2, 3, 3)
    ref = torch.einsum('tbij,bkj->tbki', R, zero) + pose[:, :, None, :3]
    assert rel(a, ref) < 1e-12


def test_ffn_width_256_rides_the_padded_streams():
    """The pack rules: a width-256 block is packed as ``pack_ffn`` / ``pack_ffn_h2`` / ``pad_ffn_bias`` of the zero-padded 1024-wide matrices --
    the slices that hold no real unit (208-unit slices 2..4) are all-zero weights and zero bias, so they contribute exactly nothing."""
    sd = syn.skeleton_mdm_state_dict(5)
    packed, ff = sk.skeleton_state_dict_for_pack(sd)
    assert ff == 256
    for p in ('decoder.layers.0.', 'decoder.layers.3.', 'encoder.layers.7.'):
        w1, b1, w2 = sd[p + 'linear1.weight'], sd[p + 'linear1.bias'], sd[p + 'linear2.weight']
        w1p, b1p, w2p = np.zeros((1024, 256), np.float32), np.zeros(1024, np.float32), np.zeros((256, 1024), np.float32)
        w1p[:256], b1p[:256], w2p[:, :256] = w1, b1, w2
        assert np.array_equal(packed[p + 'linear1.weight'], w1p) and np.array_equal(packed[p + 'linear1.bias'], b1p) and np.array_equal(packed[p + 'linear2.weight'], w2p)
        stream = hmdm.pack_ffn(packed[p + 'linear1.weight'], packed[p + 'linear2.weight'])
        assert np.array_equal(stream, hmdm.pack_ffn(w1p, w2p))
        per_slice = stream.size // _lib.FFN_SLICES
        assert np.abs(stream[:2 * per_slice]).max() > 0 and not stream[2 * per_slice:].any()          # 256 units = slice 0 and 48 units of slice 1
        h2 = hmdm.pack_ffn_h2(packed[p + 'linear1.weight'], packed[p + 'linear2.weight'])
        assert np.array_equal(h2, hmdm.pack_ffn_h2(w1p, w2p)) and not h2[2 * hmdm.H2_SLICE_FLOATS:].any()
        bias = hmdm.pad_ffn_bias(packed[p + 'linear1.bias'])
        assert np.array_equal(bias[:256], b1) and not bias[256:].any()
        # the range proof of the padded block is the proof of the real one: zero rows add nothing to any bound
        ln = sd[p + ('norm2' if p.startswith('dec') else 'norm1') + '.weight'], sd[p + ('norm2' if p.startswith('dec') else 'norm1') + '.bias']
        assert hmdm.ffn_h2_range_ok(w1p, b1p, w2p, *ln) == hmdm.ffn_h2_range_ok(w1, b1, w2, *ln)
    assert packed['objEmbedding.weight'].shape == (256, 43) and not packed['objEmbedding.weight'][:, 36:].any()


def test_head_pack_puts_the_pose_rows_first_in_every_tile():
    sd = syn.skeleton_mdm_state_dict(5)
    W, b, tiles = sk.pack_skeleton_head(sd['bodyFinalLinear.weight'], sd['bodyFinalLinear.bias'], sd['objFinalLinear.weight'], sd['objFinalLinear.bias'])
    assert tiles == 3 and W.shape == (96, 256) and b.shape == (96,)
    for t in range(3):
        assert np.array_equal(W[32 * t:32 * t + 7], sd['objFinalLinear.weight']) and np.array_equal(b[32 * t:32 * t + 7], sd['objFinalLinear.bias'])
        n = min(25, 63 - 25 * t)
        assert np.array_equal(W[32 * t + 7:32 * t + 7 + n], sd['bodyFinalLinear.weight'][25 * t:25 * t + n])
        assert np.array_equal(b[32 * t + 7:32 * t + 7 + n], sd['bodyFinalLinear.bias'][25 * t:25 * t + n])
        assert not W[32 * t + 7 + n:32 * t + 32].any() and not b[32 * t + 7 + n:32 * t + 32].any()
    assert tuple(sd['objFinalLinear.bias'][3:]) == (0.0, 0.0, 0.0, 1.0)


@pytest.mark.parametrize('ff', [1040, 2048, 250, 8])
def test_bad_feed_forward_widths_are_refused(ff):
    sd = syn.skeleton_mdm_state_dict(5, ff=ff)
    with pytest.raises(ValueError):
        sk.SkeletonMDM(sd, device=DEV)
    with pytest.raises(ValueError):
        sk.pad_ffn_width(sd['decoder.layers.0.linear1.weight'], sd['decoder.layers.0.linear1.bias'], sd['decoder.layers.0.linear2.weight'])


def test_mdm_draw_order_is_untouched():
    """``mdm_state_dict`` is pinned by goldens: the new generator draws from its own RandomState."""
    a = syn.mdm_state_dict(233)
    syn.skeleton_mdm_state_dict(233)
    b = syn.mdm_state_dict(233)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert a['decoder.layers.0.linear1.weight'].shape == (1024, 256)


# ------------------------------------------------------------------------------------------------------------ GPU

@pytest.fixture(scope='module')
def model(lib):
    return sk.SkeletonMDM(weights(), device=DEV)


@pytest.fixture(scope='module')
def model50(lib):
    return sk.SkeletonMDM(weights(), device=DEV, n_steps=50)


@pytest.mark.gpu
def test_abi_is_additive(lib):
    assert lib.interdiff_abi_version() == 17


@pytest.mark.gpu
@pytest.mark.parametrize('B,T', SHAPES)
def test_forward_vs_restatement(model, B, T):
    x, ts, zp, cond = rand_case(900 + B * 100 + T, B, T)
    got = model(x.to(DEV), ts.to(DEV), **{'y': {'cond': cond.to(DEV)}, 'zero_pose_obj': zp.to(DEV)})
    ref = smo.forward(weights(torch.float64), x.double(), ts, zp.double(), cond.double())
    assert float((ref[:, 0, -4:] ** 2).sum(1).min()) >= 0.25
    close(got, ref, GATE, 'skeleton forward B=%d T=%d vs fp64 restatement' % (B, T))
    close(got[:, :, 63:99], ref[:, :, 63:99], GATE, '... its 36 keypoint channels alone')


@pytest.mark.gpu
@pytest.mark.parametrize('B,T', SHAPES)
def test_encoder_vs_restatement(model, B, T):
    bt = {k: torch.from_numpy(v) for k, v in syn.make_skeleton_batch(800 + B * 100 + T, B=B, T=T).items()}
    tb = lambda a: a.transpose(0, 1).contiguous()
    cond, gt = model._get_embeddings(tb(bt['body']).to(DEV), tb(bt['obj']).to(DEV), tb(bt['pose']).to(DEV), bt['zero_pose_obj'].to(DEV))
    rc, rg = smo.get_embeddings(weights(torch.float64), tb(bt['body']).double(), tb(bt['obj']).double(), tb(bt['pose']).double(), bt['zero_pose_obj'].double())
    assert cond.shape == (10, B, 256) and gt.shape == (T, B, 106)
    close(cond, rc, GATE, 'skeleton encoder B=%d T=%d vs fp64 restatement' % (B, T))
    assert torch.equal(gt.cpu(), rg.float())


@pytest.mark.gpu
def test_forward_and_encoder_vs_golden(model):
    z = g()
    for T in (20, 35):
        x, ts, zp, cond = (tn(z['fwd%d_%s' % (T, k)]).to(DEV) for k in ('x', 'ts', 'zero', 'cond'))
        close(model(x, ts, zero_pose_obj=zp, y={'cond': cond}), z['fwd%d_out' % T], GATE, 'skeleton forward T=%d vs the reference' % T)
    tb = lambda k: tn(z[k]).transpose(0, 1).contiguous().to(DEV)
    cond, gt = model._get_embeddings(tb('emb_body'), tb('emb_obj'), tb('emb_pose'), tn(z['emb_zero']).to(DEV))
    close(cond, z['emb_cond'], GATE, 'skeleton _get_embeddings vs the reference')
    assert np.array_equal(gt.cpu().numpy(), z['emb_gt'])


@pytest.mark.gpu
@pytest.mark.parametrize('math', ['exact', 'split'])
def test_both_arithmetics_within_tolerance(lib, math):
    m = sk.SkeletonMDM(weights(), device=DEV)
    m.ffn_math = math
    z = g()
    x, ts, zp, cond = (tn(z['fwd20_%s' % k]).to(DEV) for k in ('x', 'ts', 'zero', 'cond'))
    close(m(x, ts, zero_pose_obj=zp, y={'cond': cond}), z['fwd20_out'], GATE, 'skeleton forward, %s feed-forward arithmetic' % math)
    rep = m.arithmetic_report()
    assert rep['ff_size'] == 256 and rep['embedding_and_heads'] == 'exact'
    assert all(d['ffn'] == math for d in rep['layers']) or (math == 'split' and rep['not_exclusive'])


def _kwargs(z, pre, device=DEV):
    gt, zp, cond = (tn(z[pre + k]).to(device) for k in ('gt', 'zero_pose_obj', 'cond'))
    return {'y': {'cond': cond, 'inpainted_motion': gt, 'inpainting_mask': mask_for(gt).to(device)}, 'zero_pose_obj': zp}


@pytest.mark.gpu
def test_config1_50_step_chain_vs_golden(model50):
    from interdiff_amd.diffusion import create_gaussian_diffusion
    z = g()
    stream = fx.NoiseStream(int(z['c50_noise_seed']))
    got = create_gaussian_diffusion('cosine', 50).p_sample_loop(
        model50, tuple(z['c50_gt'].shape), noise=tn(z['c50_noise']).to(DEV), clip_denoised=False, model_kwargs=_kwargs(z, 'c50_'),
        denoised_fn=lambda x, t, kw: x, step_noise=lambda i, x: stream.next_like(x).to(DEV))
    e = close(got, z['c50_final'], GATE, 'config #1: 50-step chain through the skeleton denoiser vs the reference')
    fx.record_parity('skeleton_mdm_config1_B1_T20_50steps_vs_reference', worst_rel_err=e, asserted=GATE)


@pytest.mark.gpu
def test_1000_step_chain_with_the_hook_vs_golden(model):
    from interdiff_amd.diffusion import create_gaussian_diffusion
    z = g()
    ck = {k: torch.from_numpy(v) for k, v in fx.golden('skel_ckpt.npz').items()}
    hook = sk.HipSkeletonCorrection(sk.SkeletonObjProjector(ck, device=DEV), device=DEV)
    stream = fx.NoiseStream(int(z['c1000_noise_seed']))
    steps = [int(s) for s in z['c1000_dump_steps']]
    dumps = create_gaussian_diffusion('cosine', 1000).p_sample_loop(
        model, tuple(z['c1000_gt'].shape), noise=tn(z['c1000_noise']).to(DEV), clip_denoised=False, model_kwargs=_kwargs(z, 'c1000_'),
        denoised_fn=hook, step_noise=lambda i, x: stream.next_like(x).to(DEV), dump_steps=steps)
    worst = max(close(d, z['c1000_dump_%d' % s], GATE, '1000-step chain + hook, loop step %d' % s) for s, d in zip(steps, dumps))
    fx.record_parity('skeleton_mdm_B2_T20_1000steps_hook_vs_reference', worst_rel_err=worst, asserted=GATE)


def _philox_step(lib_, seed):
    def draw(it, x):
        out = torch.empty_like(x)
        _lib.check(lib_.interdiff_randn(_lib.dptr(out), out.numel(), seed, it, _lib.stream()), 'randn')
        return out
    return draw


def _batch_kwargs(seed, B, T):
    bt = syn.make_skeleton_batch(seed, B=B, T=T)
    rs = np.random.RandomState(seed + 1)
    gt = torch.from_numpy(np.ascontiguousarray(np.concatenate([bt['body'].reshape(B, T, -1), bt['obj'].reshape(B, T, -1), bt['pose']], axis=2).transpose(0, 2, 1)[:, None]))
    kw = {'y': {'cond': fx._randn(rs, fx.PAST, B, 256).to(DEV), 'inpainted_motion': gt.to(DEV), 'inpainting_mask': mask_for(gt).to(DEV)},
          'zero_pose_obj': torch.from_numpy(bt['zero_pose_obj']).to(DEV)}
    return kw, fx._randn(rs, B, 1, 106, T).to(DEV)


@pytest.mark.gpu
@pytest.mark.parametrize('B,T,hooked', [(1, 20, False), (2, 35, False), (64, 20, False), (4, 20, True)])
def test_graph_route_equals_eager_route(lib, model50, B, T, hooked):
    """Captured fused steps (one chain, and two half-batch chains at B = 64: 1280 rows) with in-kernel Philox == the eager route fed the same stream."""
    from interdiff_amd.diffusion import create_gaussian_diffusion
    assert model50.graph_safe and model50.supports_forward_step and model50.accepts_batch_rows and not model50.step_chaining
    kw, noise = _batch_kwargs(5000 + B + T, B, T)
    hook = None
    if hooked:
        ck = {k: torch.from_numpy(v) for k, v in fx.golden('skel_ckpt.npz').items()}
        hook = sk.HipSkeletonCorrection(sk.SkeletonObjProjector(ck, device=DEV), device=DEV)
    diff = create_gaussian_diffusion('cosine', 50)
    n = 50 if B < 64 else 12
    timed = diff.p_sample_loop(model50, tuple(noise.shape), noise=noise, clip_denoised=False, model_kwargs=kw, denoised_fn=hook, seed=23, n_steps=n)
    eager = diff.p_sample_loop(model50, tuple(noise.shape), noise=noise, clip_denoised=False, model_kwargs=kw, denoised_fn=hook, use_graph=False,
                               step_noise=_philox_step(lib, 23), n_steps=n)
    assert torch.isfinite(timed).all()
    assert torch.equal(timed, eager), 'graph route differs from eager: %g' % (timed - eager).abs().max()
    assert any(isinstance(k, tuple) and len(k) == 3 for st in model50._graph_cache.values() for k in st.graphs), 'the captured route was not taken'


@pytest.mark.gpu
@pytest.mark.parametrize('B,T,masked', [(3, 20, True), (2, 35, True), (64, 20, False), (5, 21, True)])
def test_fused_step_equals_forward_plus_posterior(lib, model, B, T, masked):
    from interdiff_amd.diffusion import create_gaussian_diffusion
    kw, x = _batch_kwargs(6000 + B + T, B, T)
    table = create_gaussian_diffusion('cosine', 1000)._table(torch.device(DEV))
    gt = kw['y']['inpainted_motion'] if masked else None
    mk = kw['y']['inpainting_mask'].view(torch.uint8).contiguous() if masked else None
    t0 = 417
    mk_state = lambda: torch.tensor([t0, 3, 99, 0, 0, 0, 0, 0], dtype=torch.int64, device=DEV)
    xa, tsa, sta = x.clone(), torch.full((B,), t0, dtype=torch.int64, device=DEV), mk_state()
    model.forward_step(xa, tsa, table, sta, gt=gt, mask=mk, y=kw['y'], zero_pose_obj=kw['zero_pose_obj'])
    xb, tsb, stb = x.clone(), torch.full((B,), t0, dtype=torch.int64, device=DEV), mk_state()
    x0 = model(xb, tsb, zero_pose_obj=kw['zero_pose_obj'], y=kw['y'])
    _lib.check(lib.interdiff_posterior_step_dev(_lib.dptr(xb), _lib.dptr(x0), _lib.dptr(gt, allow_none=True), _lib.dptr(mk, allow_none=True), xb.numel(),
                                                _lib.dptr(table), _lib.dptr(stb), _lib.dptr(tsb), B, _lib.stream()), 'posterior_step_dev')
    assert torch.equal(xa, xb), 'fused step differs from forward + posterior: %g' % (xa - xb).abs().max()
    assert not torch.equal(xa, x)
    assert torch.equal(tsa, tsb) and torch.equal(sta[:3], stb[:3]) and int(sta[0]) == t0 - 1


@pytest.mark.gpu
def test_clip_sharded_run_equals_unsharded(lib, model50):
    from interdiff_amd.diffusion import create_gaussian_diffusion
    B, T = 6, 20
    kw, noise = _batch_kwargs(7000, B, T)
    diff = create_gaussian_diffusion('cosine', 50)
    whole = diff.p_sample_loop(model50, tuple(noise.shape), noise=noise, clip_denoised=False, model_kwargs=kw, seed=31)
    parts = []
    for first, n in ((0, 2), (2, 4)):
        sl = slice(first, first + n)
        kws = {'y': {'cond': kw['y']['cond'][:, sl].contiguous(), 'inpainted_motion': kw['y']['inpainted_motion'][sl].contiguous(),
                     'inpainting_mask': kw['y']['inpainting_mask'][sl].contiguous()}, 'zero_pose_obj': kw['zero_pose_obj'][sl].contiguous()}
        parts.append(diff.p_sample_loop(model50, (n,) + tuple(noise.shape[1:]), noise=noise[sl].contiguous(), clip_denoised=False, model_kwargs=kws, seed=31,
                                        shard=(first, B)))
    assert torch.equal(torch.cat(parts), whole)


@pytest.mark.gpu
def test_sample_once_proj_feeds_the_metrics(lib, model50):
    """eval_skeleton.py:114-142 end to end on the GPU: encoder, sampler on the captured route, hook, metrics; and eval_skeleton_no_correction.py's form."""
    from interdiff_amd.diffusion import create_gaussian_diffusion
    B, T = 4, 20
    bt = {k: torch.from_numpy(v) for k, v in syn.make_skeleton_batch(7100, B=B, T=T).items()}
    batch = (bt['body'], bt['obj'], bt['pose'], bt['zero_pose_obj'])
    ck = {k: torch.from_numpy(v) for k, v in fx.golden('skel_ckpt.npz').items()}
    diff = create_gaussian_diffusion('cosine', 50)
    for obj_model in (None, sk.SkeletonObjProjector(ck, device=DEV)):
        out = sk.sample_once_proj(batch, model50, diff, obj_model=obj_model, seed=5)
        obj_pred, body_pred, pose_pred, obj_gt, body_gt, pose_gt = out
        assert obj_pred.shape == (T, B, 36) and body_pred.shape == (T, B, 63) and pose_pred.shape == (T, B, 7)
        assert torch.equal(body_pred[:fx.PAST], body_gt[:fx.PAST])              # past frames are inpainted (the hook passes the body through)
        if obj_model is None:                                                   # (the hook rewrites pose and keypoints in EVERY frame, eval_skeleton.py:104-111)
            assert torch.equal(pose_pred[:fx.PAST], pose_gt[:fx.PAST]) and torch.equal(obj_pred[:fx.PAST], obj_gt[:fx.PAST])
        m = sk.skeleton_metrics(body_pred.view(T, B, -1, 3), body_gt.view(T, B, -1, 3), obj_pred.view(T, B, -1, 3), obj_gt.view(T, B, -1, 3), pose_pred, pose_gt)
        assert all(np.isfinite(v) for v in m.values())
        again = sk.sample_once_proj(batch, model50, diff, obj_model=obj_model, seed=5)
        assert all(torch.equal(a, b) for a, b in zip(out, again))


@pytest.mark.gpu
def test_plain_mdm_still_rejects_the_top_level_entry(lib):
    from interdiff_amd.mdm import MDM
    m = MDM(fx.mdm_weights(), device=DEV)
    with pytest.raises(TypeError):
        m(torch.zeros(1, 1, 144, 16, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV), y={'cond': torch.zeros(10, 1, 256, device=DEV)},
          zero_pose_obj=torch.zeros(1, 12, 3, device=DEV))
