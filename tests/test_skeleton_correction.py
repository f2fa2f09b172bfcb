"""HO-GCN skeleton mode (eval_skeleton.py): the correction predictor, the correction hook and the metrics on the HIP kernels of
csrc/skeleton.hip, against the reference's own outputs (tests/golden/skel_*.npz, tests/golden/make_golden_skeleton.py) and the CPU
restatement tests/skeleton_oracle.py."""
import os
import re
import numpy as np
import pytest
import torch
from tests import fixtures as fx
from tests import skeleton_oracle as so
from interdiff_amd import skeleton as sk

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
DEV = 'cuda'
METRIC_KEYS = ('mpjpe_h', 'mpjpe_o', 'translation_error', 'rotation_error')
METRIC_ARGS = ('body_pred', 'body_gt', 'obj_pred', 'obj_gt', 'pose_pred', 'pose_gt')


def rel(a, b):
    a, b = (x.detach().cpu().double().numpy() if isinstance(x, torch.Tensor) else np.asarray(x, np.float64) for x in (a, b))
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def g(name):
    z = fx.golden(name)
    return {k: z[k] for k in z.files}


def t64(a):
    return torch.from_numpy(np.asarray(a)).double()


def ckpt():
    return {k: torch.from_numpy(v) for k, v in g('skel_ckpt.npz').items()}


def standin_model(w, steps):
    """The deterministic denoiser stand-in of skel_loop.npz (make_golden_skeleton.py StandIn)."""
    def model(x, t, y=None, **kw):
        return (torch.tanh(torch.einsum('dc,bgct->bgdt', w, x)) * (1.0 + 0.01 * t.float().view(-1, 1, 1, 1) / steps)).contiguous()
    return model


# ------------------------------------------------------------------------------------------------------------ CPU

@pytest.mark.parametrize('B', [1, 64])
def test_oracle_objprojector_golden(B):
    z = g('skel_objproj.npz')
    q, tr = so.objprojector_sample(so.state_dict_layers(ckpt()), *[t64(z['%s_b%d' % (k, B)]) for k in ('angles', 'trans', 'human')])
    assert rel(q, z['quat_out_b%d' % B]) <= 1e-5 and rel(tr, z['trans_out_b%d' % B]) <= 1e-5


def test_oracle_hook_golden():
    z = g('skel_hook.npz')
    layers = so.state_dict_layers(ckpt())
    for t0 in (500, 250, 50, 0):
        out = so.denoised_fn(layers, t64(z['x']), t0, {'inpainted_motion': t64(z['gt'])}, t64(z['zero_pose_obj']))
        assert rel(out, z['out_t%d' % t0]) <= 1e-5, t0


def test_oracle_metrics_golden():
    z = g('skel_metrics.npz')
    got = so.calc_metric_single(*[t64(z[k]) for k in METRIC_ARGS])
    for k in METRIC_KEYS:
        assert abs(got[k] - float(z[k])) <= 1e-5 * abs(float(z[k])), k


def test_oracle_loop_golden():
    """The 1000-step loop of skel_loop.npz on the CPU oracle (oracle/diffusion.py) with the restated hook."""
    from oracle import diffusion as odf
    z = g('skel_loop.npz')
    gt, noise, zp = (torch.from_numpy(z[k]) for k in ('gt', 'noise', 'zero_pose_obj'))
    B, _, C, T = gt.shape
    mask = torch.ones(B, 1, C, T, dtype=torch.bool)
    mask[..., fx.PAST:] = False
    layers = so.state_dict_layers(ckpt(), dtype=torch.float32)
    stream = fx.NoiseStream(int(z['noise_seed']))
    dumps = odf.p_sample_loop(standin_model(torch.from_numpy(z['w']), 1000), (B, 1, C, T), odf.make_schedule(1000), noise.clone(),
                              lambda i, x: stream.next_like(x), {'y': dict(inpainted_motion=gt, inpainting_mask=mask)},
                              denoised_fn=lambda x, t, kw: so.denoised_fn(layers, x, int(t[0]), kw['y'], zp),
                              dump_steps=[int(s) for s in z['dump_steps']])
    for s, d in zip(z['dump_steps'], dumps):
        assert rel(d, z['dump_%d' % s]) <= 1e-5, s


def test_packer_folds_batchnorm_like_the_reference():
    """The CPU restatement fed the PACKED arena (BatchNorm folded in float64, fp32 arena, idx_pad and DCT as packed) equals the
    reference; the checkpoint's ``model.`` prefix is optional."""
    sd = ckpt()
    op, arena = sk.pack_skeleton_objprojector(sd)
    op2, arena2 = sk.pack_skeleton_objprojector({'model.' + k: v for k, v in sd.items()})
    assert np.array_equal(arena, arena2) and list(op.layer) == list(op2.layer)
    assert list(op.cin) == [9, 32, 16, 32] * 2 + [9, 64, 32, 64] and list(op.cout) == [32, 16, 32, 9] * 2 + [64, 32, 64, 9]
    layers = so.packed_layers(op, arena)
    z = g('skel_objproj.npz')
    for B in (1, 64):
        q, tr = so.objprojector_sample(layers, *[t64(z['%s_b%d' % (k, B)]) for k in ('angles', 'trans', 'human')])
        assert rel(q, z['quat_out_b%d' % B]) <= 1e-5 and rel(tr, z['trans_out_b%d' % B]) <= 1e-5, B
    h = g('skel_hook.npz')
    out = so.denoised_fn(layers, t64(h['x']), 250, {'inpainted_motion': t64(h['gt'])}, t64(h['zero_pose_obj']))
    assert rel(out, h['out_t250']) <= 1e-5
    with pytest.raises(ValueError):
        sk.pack_skeleton_objprojector(sd, past_len=10, future_len=15)


def test_skeleton_symbols_declared_and_typed():
    from interdiff_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'interdiff_hip.h')).read()
    names = ('interdiff_skeleton_objprojector_sample', 'interdiff_skeleton_correction', 'interdiff_skeleton_metrics')
    for n in names:
        assert re.search(r'\bint %s\(' % n, src), n
        assert n in _lib._SIGS, n
    assert 'idf_skel_objproj;' in src
    assert [f[0] for f in _lib.SkelObjProj._fields_] == ['T', 'past_len', 'J', 'n_pre', 'arena', 'dct_pad', 'dct', 'idct', 'layer', 'cin', 'cout']
    assert _lib.ABI_VERSION == 17
    lib = _lib.load()
    assert lib.interdiff_abi_version() == 17


# ------------------------------------------------------------------------------------------------------------ GPU

@pytest.fixture(scope='module')
def proj(lib):
    return sk.SkeletonObjProjector(ckpt(), device=DEV)


@pytest.fixture(scope='module')
def hook(proj):
    return sk.HipSkeletonCorrection(proj, device=DEV)


def hook_inputs():
    z = g('skel_hook.npz')
    return (torch.from_numpy(z['x']).to(DEV), {'inpainted_motion': torch.from_numpy(z['gt']).to(DEV)},
            torch.from_numpy(z['zero_pose_obj']).to(DEV), z)


def tsteps(t0, B):
    return torch.full((B,), t0, dtype=torch.int64, device=DEV)


@pytest.mark.gpu
@pytest.mark.parametrize('B', [1, 4, 64])
def test_objprojector_matches_golden_and_oracle(proj, B):
    z = g('skel_objproj.npz')
    src = 1 if B == 1 else 64
    ins = [z['%s_b%d' % (k, src)][:, :B] for k in ('angles', 'trans', 'human')]
    q, tr = proj.sample(*[torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in ins])
    assert rel(q, z['quat_out_b%d' % src][:, :B]) <= 1e-4 and rel(tr, z['trans_out_b%d' % src][:, :B]) <= 1e-4
    oq, otr = so.objprojector_sample(so.state_dict_layers(ckpt()), *[t64(a) for a in ins])
    assert rel(q, oq) <= 1e-4 and rel(tr, otr) <= 1e-4


@pytest.mark.gpu
def test_hook_matches_golden_at_each_t(hook):
    x, y, zp, z = hook_inputs()
    for t0 in (500, 250, 50, 0):
        out = hook(x, tsteps(t0, x.shape[0]), {'y': y, 'zero_pose_obj': zp})
        assert out is not x
        assert rel(out, z['out_t%d' % t0]) <= 1e-4, t0


@pytest.mark.gpu
def test_hook_gated_off_returns_x_and_launches_nothing(proj):
    x, y, zp, _ = hook_inputs()
    h = sk.HipSkeletonCorrection(proj, device=DEV)

    class NoLaunch:
        def __getattr__(self, name):
            raise AssertionError('the gated-off hook called %s' % name)
    h.lib = NoLaunch()
    before = x.clone()
    for t0 in (499, 510, 525):
        out = h(x, tsteps(t0, x.shape[0]), {'y': y, 'zero_pose_obj': zp})
        assert out is x and torch.equal(x, before), t0
        assert not h.is_active(t0)


@pytest.mark.gpu
def test_hook_leaves_inputs_untouched(hook):
    x, y, zp, _ = hook_inputs()
    xb, gb, zb = x.clone(), y['inpainted_motion'].clone(), zp.clone()
    hook(x, tsteps(250, x.shape[0]), {'y': y, 'zero_pose_obj': zp})
    torch.cuda.synchronize()
    assert torch.equal(x, xb) and torch.equal(y['inpainted_motion'], gb) and torch.equal(zp, zb)


@pytest.mark.gpu
def test_hook_ignores_future_frames_of_inpainted_motion(hook):
    """Only the past pose rows of inpainted_motion enter (idx_pad repeats frame 9): changing frames 10.. changes no bit."""
    x, y, zp, _ = hook_inputs()
    a = hook(x, tsteps(250, x.shape[0]), {'y': y, 'zero_pose_obj': zp})
    gt2 = y['inpainted_motion'].clone()
    gt2[..., fx.PAST:] = torch.randn_like(gt2[..., fx.PAST:]) * 3.0
    b = hook(x, tsteps(250, x.shape[0]), {'y': {'inpainted_motion': gt2}, 'zero_pose_obj': zp})
    assert torch.equal(a, b)


@pytest.mark.gpu
def test_hook_batch_equals_single_clips_and_repeats(hook):
    """Clip i of a B = 64 call == a B = 1 call on clip i, bit for bit; two calls give the same bits.  zero_pose_obj from y (fallback)."""
    gen = torch.Generator().manual_seed(64)
    B = 64
    x = (0.5 * torch.randn(B, 1, 106, 20, generator=gen)).to(DEV)
    gt = (0.5 * torch.randn(B, 1, 106, 20, generator=gen)).to(DEV)
    zp = (0.3 * torch.randn(B, 12, 3, generator=gen)).to(DEV)
    full = hook(x, tsteps(100, B), {'y': {'inpainted_motion': gt, 'zero_pose_obj': zp}})
    again = hook(x, tsteps(100, B), {'y': {'inpainted_motion': gt, 'zero_pose_obj': zp}})
    assert torch.equal(full, again)
    for i in (0, 17, 63):
        one = hook(x[i:i + 1].contiguous(), tsteps(100, 1), {'y': {'inpainted_motion': gt[i:i + 1].contiguous()}, 'zero_pose_obj': zp[i:i + 1].contiguous()})
        assert torch.equal(one[0], full[i]), i
    assert torch.isfinite(full).all()


@pytest.mark.gpu
def test_metrics_match_golden_and_repeat(lib):
    z = g('skel_metrics.npz')
    args = [torch.from_numpy(z[k]).to(DEV) for k in METRIC_ARGS]
    got = sk.skeleton_metrics(*args)
    for k in METRIC_KEYS:
        assert abs(got[k] - float(z[k])) <= 1e-5 * abs(float(z[k])), (k, got[k], float(z[k]))
    assert sk.skeleton_metrics(*args) == got


@pytest.mark.gpu
def test_end_to_end_loop_matches_reference(hook):
    """The project's 1000-step p_sample_loop (eager route: injected noise) with HipSkeletonCorrection and the stand-in denoiser of
    skel_loop.npz, vs the reference's p_sample_loop with its own denoised_fn and the real predictor."""
    from interdiff_amd.diffusion import create_gaussian_diffusion
    z = g('skel_loop.npz')
    gt, noise, zp = (torch.from_numpy(z[k]).to(DEV) for k in ('gt', 'noise', 'zero_pose_obj'))
    B, _, C, T = gt.shape
    mask = torch.ones(B, 1, C, T, dtype=torch.bool, device=DEV)
    mask[..., fx.PAST:] = False
    stream = fx.NoiseStream(int(z['noise_seed']))
    diff = create_gaussian_diffusion('cosine', 1000)
    steps = [int(s) for s in z['dump_steps']]
    dumps = diff.p_sample_loop(standin_model(torch.from_numpy(z['w']).to(DEV), 1000), (B, 1, C, T), noise=noise, clip_denoised=False,
                               model_kwargs={'y': dict(inpainted_motion=gt, inpainting_mask=mask), 'zero_pose_obj': zp}, denoised_fn=hook,
                               device=DEV, dump_steps=steps, step_noise=lambda i, x: stream.next_like(x).to(DEV))
    worst = 0.0
    for s, d in zip(steps, dumps):
        e = rel(d, z['dump_%d' % s])
        worst = max(worst, e)
        assert e <= 1e-4, (s, e)
    fx.record_parity('skeleton_loop_B4_T20_1000steps_vs_reference', worst_rel_err=worst, asserted=1e-4, dumps=steps)


def _philox_step(lib_, seed):
    from interdiff_amd import _lib

    def draw(it, x):
        out = torch.empty_like(x)
        _lib.check(lib_.interdiff_randn(_lib.dptr(out), out.numel(), seed, it, _lib.stream()), 'randn')
        return out
    return draw


@pytest.mark.gpu
def test_graph_route_equals_eager_route_with_the_hook(lib, hook):
    """BASELINE config #1's C = 106 denoiser kernels (test_config1_skeleton_tokens_through_the_denoiser_kernels' synthetic weights) with
    this hook over the corrected part of a 1000-step schedule (t = 520 .. 0: eleven hook steps): the graph route (captured plain steps,
    the hook called eagerly between them) and the eager route fed the same Philox stream give the same bits."""
    from interdiff_amd import synthetic as syn
    from interdiff_amd.mdm import MDM
    from interdiff_amd.diffusion import create_gaussian_diffusion
    sd = {k: torch.from_numpy(v) for k, v in syn.mdm_state_dict(233).items()}
    gen = torch.Generator().manual_seed(106)
    n_body, n_obj = 63, 43
    sd['bodyEmbedding.weight'] = torch.randn(256, n_body, generator=gen) / n_body ** 0.5
    sd['objEmbedding.weight'] = torch.cat([torch.randn(256, 36, generator=gen) / 6.0, torch.zeros(256, 7)], dim=1)
    sd['bodyFinalLinear.weight'], sd['bodyFinalLinear.bias'] = torch.randn(n_body, 256, generator=gen) / 16.0, 0.1 * torch.randn(n_body, generator=gen)
    sd['objFinalLinear.weight'], sd['objFinalLinear.bias'] = torch.randn(n_obj, 256, generator=gen) / 16.0, 0.1 * torch.randn(n_obj, generator=gen)
    model = MDM(sd, device=DEV, n_steps=1000)
    B, T = 2, 20
    gt, noise, cond = torch.randn(B, 1, 106, T, generator=gen), torch.randn(B, 1, 106, T, generator=gen), torch.randn(10, B, 256, generator=gen)
    mask = torch.ones(B, 1, 106, T, dtype=torch.bool)
    mask[..., fx.PAST:] = False
    zp = 0.3 * torch.randn(B, 12, 3, generator=gen)
    y = {k: v.to(DEV) for k, v in dict(cond=cond, inpainting_mask=mask, inpainted_motion=gt, zero_pose_obj=zp).items()}
    diff = create_gaussian_diffusion('cosine', 1000)
    calls = []

    class Counted:                      # the hook, recording the timesteps it is called at
        is_active = staticmethod(hook.is_active)

        def __call__(self, x, t, kw):
            calls.append(int(t.host_value))
            return hook(x, t, kw)
    counted = Counted()
    graph = diff.p_sample_loop(model, (B, 1, 106, T), noise=noise.to(DEV), clip_denoised=False, model_kwargs={'y': y}, seed=17,
                               first_t=520, denoised_fn=counted)
    n_graph = len(calls)
    eager = diff.p_sample_loop(model, (B, 1, 106, T), noise=noise.to(DEV), clip_denoised=False, model_kwargs={'y': y}, use_graph=False,
                               step_noise=_philox_step(lib, 17), first_t=520, denoised_fn=counted)
    assert torch.isfinite(graph).all()
    assert torch.equal(graph, eager), 'graph route differs from eager: %g' % (graph - eager).abs().max()
    assert calls[:n_graph] == list(range(500, -1, -50))


@pytest.mark.gpu
def test_t_other_than_twenty_frames_is_refused(hook, proj):
    gen = torch.Generator().manual_seed(21)
    x = torch.randn(2, 1, 106, 21, generator=gen).to(DEV)
    with pytest.raises(ValueError):
        hook(x, tsteps(250, 2), {'y': {'inpainted_motion': x.clone()}, 'zero_pose_obj': torch.zeros(2, 12, 3, device=DEV)})
    with pytest.raises(ValueError):
        proj.sample(torch.randn(21, 2, 4, device=DEV), torch.randn(21, 2, 3, device=DEV), torch.randn(21, 2, 21, 3, device=DEV))
