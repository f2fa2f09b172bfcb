"""Pin the oracle (CPU restatement) against golden vectors recorded from the
reference's OWN source (tests/golden/make_golden.py) and against the known
answers / closed-form identities of SURVEY.md §8(c).  CPU only."""
import numpy as np
import torch
import pytest
from tests import fixtures as fx
from oracle import diffusion as odf, denoiser as oden, smpl as osmpl, geometry as ogeo
from oracle import objprojector as oobj, correction as ocor, rotations as R

torch.set_grad_enabled(False)


def close(a, b, tol, what=''):
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    err = (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)
    assert err <= tol, '%s rel err %.3e > %.1e' % (what, err, tol)


def test_schedule_tables_and_known_answers():
    z = fx.golden('schedule.npz')
    for steps in (1000, 50):
        s = odf.make_schedule(steps)
        for k in ('betas', 'posterior_mean_coef1', 'posterior_mean_coef2', 'posterior_log_variance_clipped',
                  'posterior_variance', 'alphas_cumprod'):
            np.testing.assert_allclose(s[k], z['%s_%d' % (k, steps)], rtol=0, atol=1e-15)
    s = odf.make_schedule(1000)                                   # SURVEY.md §8(c) known answers
    assert abs(s['betas'][0] - 4.12842248e-05) < 1e-12 and s['betas'][-1] == 0.999
    np.testing.assert_allclose(s['posterior_mean_coef1'][[0, 1, 500, 999]],
                               [1, 0.52778141, 0.00436787, 0.00155689], atol=1e-8)
    np.testing.assert_allclose(s['posterior_log_variance_clipped'][[0, 1, 500, 999]],
                               [-10.7340825, -10.7340825, -5.76162185, -1.00292667e-3], atol=1e-7)
    assert s['posterior_mean_coef2'][0] == 0.0


def test_rotation_identities():
    g = torch.Generator().manual_seed(0)
    aa = torch.randn(500, 3, generator=g, dtype=torch.float64)
    M = R.axis_angle_to_matrix(aa)
    close(M @ M.transpose(-1, -2), torch.eye(3, dtype=torch.float64).expand_as(M), 1e-12, 'orthonormal')
    close(R.rotation_6d_to_matrix(R.matrix_to_rotation_6d(M)), M, 1e-12, '6d round trip')
    close(R.axis_angle_to_matrix(R.matrix_to_axis_angle(M)), M, 1e-9, 'aa round trip')
    close(R.rodrigues_smpl(aa), M, 1e-7, 'SMPL rodrigues == pytorch3d rotation (up to the 1e-8 quirk)')
    z = torch.zeros(1, 3)
    close(R.rodrigues_smpl(z), torch.eye(3)[None], 1e-7, 'zero rotation through the +1e-8 quirk')
    close(R.axis_angle_to_matrix(z), torch.eye(3)[None], 0, 'zero rotation series branch')
    # scipy as an independent witness
    from scipy.spatial.transform import Rotation
    close(M, torch.from_numpy(Rotation.from_rotvec(aa.numpy()).as_matrix()), 1e-12, 'vs scipy')


def test_dct_is_orthonormal():
    for N in (35, 100):
        d, i = oobj.dct_matrices(N)
        np.testing.assert_allclose(d @ i, np.eye(N), atol=1e-12)
        np.testing.assert_allclose(i, d.T, atol=1e-12)


def test_mdm_forward():
    z = fx.golden('mdm.npz')
    for tag, (B, T) in (('a', (2, 12)), ('b', (3, 35))):
        x, ts, cond = fx.mdm_inputs(B, T)
        close(oden.mdm_forward(fx.mdm_weights(), x, ts, cond), z['out_' + tag], 2e-5, 'mdm ' + tag)


def test_qan_closed_form_matches_local_attention():
    """The fused form the HIP kernel uses (constant pre-rotated queries, 3-tap
    stencil) equals the literal LocalAttention pipeline."""
    sd, p = fx.mdm_weights(), 'decoder.layers.3'
    x = torch.randn(9, 2, 256, generator=torch.Generator().manual_seed(1))
    lit = oden.qan_block(x, sd, p, rotary=True)
    from interdiff_amd.mdm import qan_constants
    Qc = torch.from_numpy(qan_constants(sd[p + '.queries'].numpy(), rotary=True))     # [Nq,3,D]
    T = x.shape[0]
    xp = torch.cat([torch.zeros(1, 2, 256), x, torch.zeros(1, 2, 256)])
    nb = torch.stack([xp[0:T], xp[1:T + 1], xp[2:T + 2]], dim=2)                       # [T,B,3,D]
    logit = torch.einsum('tbjd,njd->tbnj', nb, Qc)
    valid = torch.ones(T, 3, dtype=torch.bool)
    valid[0, 0] = valid[-1, 2] = False
    logit = logit.masked_fill(~valid[:, None, None, :], -torch.finfo(torch.float32).max)
    c = torch.einsum('tbnj,n->tbj', torch.softmax(logit, -1), sd[p + '.wk'][:, 0])
    close(torch.einsum('tbj,tbjd->tbd', c, nb), lit, 2e-5, 'qan closed form')


def test_smpl_and_normals():
    z = fx.golden('smpl.npz')
    model, sub = fx.smpl_model(), fx.vertex_subset()
    verts, jtr, v_posed = osmpl.smpl_forward(model, *fx.smpl_inputs(4))
    close(verts[:, sub], z['verts'], 2e-6, 'verts')
    close(jtr, z['jtr'], 2e-6, 'jtr')
    close(v_posed[:, sub], z['v_posed'], 2e-6, 'v_posed')
    close(ogeo.vertex_normals(verts, model['faces'])[:, sub], z['normals'], 1e-4, 'normals')
    # identity pose: LBS reduces to v_shaped + trans (SURVEY.md §4 closed form)
    pose, betas, trans = fx.smpl_inputs(4)
    v0, _, vp0 = osmpl.smpl_forward(model, torch.zeros_like(pose), betas, trans)
    close(v0, vp0 + trans[:, None], 1e-5, 'identity pose')


def test_point2point_signed():
    z = fx.golden('p2p.npz')
    x, y, xn = fx.p2p_inputs()
    r = ogeo.point2point_signed(x, y, x_normals=xn, return_vector=True)
    assert torch.equal(r[2], torch.from_numpy(z['yidx'])) and torch.equal(r[3], torch.from_numpy(z['xidx']))
    assert r[3][1, 40] == r[3][1, 3] and r[2][0, 5] == 17
    for got, k in zip((r[0], r[1], r[4], r[5]), ('y2x_signed', 'x2y_signed', 'y2x', 'x2y')):
        close(got, z[k], 1e-6, k)
    with pytest.raises(ValueError):
        ogeo.point2point_signed(x, y[:2])


def test_objprojector_real_checkpoint():
    z = fx.golden('objproj.npz')
    for tag, (T, B) in (('a', (35, 3)), ('b', (100, 2))):
        oa, ot, hv, contact = fx.objproj_inputs(T, B)
        close(oobj.objprojector_sample(fx.objproj_weights(), oa, ot, hv, contact, fx.PAST), z['out_' + tag], 1e-5, tag)


def _y(y):
    return dict(y, smpl=fx.smpl_model(), obj_model=fx.objproj_weights())


def test_denoised_fn():
    z = fx.golden('denoised_fn.npz')
    x, y = fx.denoised_fn_inputs()
    B = x.shape[0]
    for tval in fx.DFN_TS:
        got = ocor.denoised_fn(x.clone(), torch.full((B,), tval, dtype=torch.int64), {'y': _y(y)}, past_len=fx.PAST)
        close(got, z['out_t%d' % tval], 1e-5, 't=%d' % tval)
    assert np.array_equal(z['out_t499'], x.numpy()) and not np.array_equal(z['out_t500'], x.numpy())


def test_full_1000_step_loop():
    """Oracle sampler + oracle denoiser + oracle correction vs the reference's own
    p_sample_loop / MDM / denoised_fn over the full 1000 steps (11 corrections)."""
    z = fx.golden('loop.npz')
    noise, y, stream = fx.loop_inputs()
    sd = fx.mdm_weights()
    model = lambda x, t, y: oden.mdm_forward(sd, x, t, y['cond'])
    dumps = odf.p_sample_loop(model, tuple(noise.shape), odf.make_schedule(1000), noise.clone(),
                              lambda i, x: stream.next_like(x), {'y': _y(y)},
                              denoised_fn=lambda x, t, kw: ocor.denoised_fn(x, t, kw, past_len=fx.PAST),
                              dump_steps=fx.LOOP_DUMPS)
    for s, d in zip(fx.LOOP_DUMPS, dumps):
        close(d, z['dump_%d' % s], 2e-4, 'loop index %d' % s)


def test_eval_glue_and_metrics():
    """Oracle sample_once_proj / get_gt / metrics vs the reference's own functions (eval_smpl_short.py:24-81,133-250)
    on a tiny clip with a 50-step schedule (the hook fires once, at t = 0)."""
    z = fx.golden('eval.npz')
    batch, noise, stream = fx.eval_inputs()
    T, B, P = fx.EVAL_SHAPE
    past, sd, smpl = fx.PAST, fx.mdm_weights(), fx.smpl_model()
    y = _y(fx.model_kwargs_y(dict(batch, noise=noise), T))
    sample = odf.p_sample_loop(lambda x, t, y: oden.mdm_forward(sd, x, t, y['cond']), tuple(noise.shape),
                               odf.make_schedule(fx.EVAL_STEPS), noise.clone(), lambda i, x: stream.next_like(x), {'y': y},
                               denoised_fn=lambda x, t, kw: ocor.denoised_fn(x, t, kw, past_len=past))
    obj, body, verts, jtr = ocor.finalize(sample, batch['gt'], batch['hand_pose'], batch['beta'], smpl, past)
    sub = fx.vertex_subset()
    close(obj[..., 3:], z['obj'][..., 3:], 1e-4, 'obj translation')
    close(R.axis_angle_to_matrix(obj[..., :3]), R.axis_angle_to_matrix(torch.from_numpy(z['obj'][..., :3])), 1e-4, 'obj rotation')
    close(body[..., 66:], z['body'][..., 66:], 1e-4, 'hands + translation')
    close(verts[:, :, sub], z['verts'], 1e-4, 'verts')
    close(jtr, z['jtr'], 1e-4, 'jtr')
    obj_gt, jtr_gt, body_gt = ocor.ground_truth(batch['gt'], batch['hand_pose'], batch['beta'], smpl)
    close(jtr_gt, z['jtr_gt'], 1e-5, 'jtr_gt')
    close(body_gt[..., 66:], z['body_gt'][..., 66:], 1e-5, 'body_gt')
    # metrics on the REFERENCE's own sample (isolates the metric arithmetic from sampling noise)
    full = lambda k: torch.from_numpy(z[k])
    verts_ref = ocor.finalize(sample, batch['gt'], batch['hand_pose'], batch['beta'], smpl, past)[2]
    m = ocor.metrics(full('obj')[past:], full('jtr')[past:], full('body')[past:], full('obj_gt')[past:], full('jtr_gt')[past:],
                     full('body_gt')[past:], verts_ref[past:], smpl['faces'], batch['obj_points'])
    for k, v in m.items():
        close(v, z['m_' + k], 1e-4 if k != 'penetrate' else 2e-2, 'metric ' + k)


def test_get_embeddings_encoder_side():
    """"Next" row N1: oracle MDM._get_embeddings (PointNet++ restatement + embeddings + 8-layer encoder) vs the reference's
    own module run (tests/golden/embed.npz); plus the properties the restated PointNet++ ops must have."""
    from oracle import pointnet2 as opn
    z = fx.golden('embed.npz')
    ei = fx.embedding_inputs()
    cond, gt = oden.get_embeddings(fx.mdm_weights(), ei['body_pose'], ei['body_trans'], ei['obj_angles'], ei['obj_trans'],
                                   ei['obj_points'], fx.PAST)
    close(cond, z['cond'], 1e-5, 'cond')
    close(gt, z['gt'], 1e-6, 'gt')
    xyz = ei['obj_points'][:1]
    idx = opn.furthest_point_sample(xyz, 64)[0]
    assert idx[0] == 0 and len(set(idx.tolist())) == 64 and 7 not in idx.tolist()       # point 7 has |p|^2 <= 1e-3: skipped
    d = ((xyz[0, idx][:, None] - xyz[0, idx][None]) ** 2).sum(-1)
    assert d[1:, 0].min() > 0.01                                                         # spread out
    bq = opn.ball_query(0.1, 16, xyz, xyz[:, :5])
    for m in range(5):
        hits = torch.nonzero(((xyz[0] - xyz[0, m]) ** 2).sum(-1) < 0.01)[:, 0][:16]
        assert torch.equal(bq[0, m, :len(hits)], hits) and (bq[0, m, len(hits):] == hits[0]).all()


def test_optimization_golden():
    """oracle/optimization.py against the reference's own optimize() (optimization.py:19-173) run on the same clip:
    losses and gradients at the parameters the reference's Adam saw.  Iteration 1 starts AT the initial pose, where
    verts - verts_gt is rounding noise and its sign (the verts_reg gradient, 0.01/T per vertex) is implementation noise:
    gradients are compared from the second executed iteration on."""
    from oracle import optimization as oo
    g = fx.golden('optim.npz')
    model = fx.smpl_model()
    inp = fx.optim_inputs()
    for k, ii in enumerate(fx.OPT_ITERS[:3]):
        params = {n: torch.from_numpy(g['before_' + n][k]) for n in oo.PARAM_ORDER}
        parts, grads = oo.loss_and_grads(model, params, *inp, ii)
        np.testing.assert_allclose(parts.numpy(), g['losses'][k], atol=6e-5, rtol=2e-5)       # printed with 4 decimals
        if k == 0:
            continue
        for n in oo.PARAM_ORDER:
            ref = g['grad_' + n][k]
            assert np.abs(grads[n].numpy() - ref).max() <= 2e-4 * np.abs(ref).max() + 1e-6, n
            assert ((grads[n].numpy() == 0) == (ref == 0)).all(), n                             # exact-zero pattern (Adam leaves those untouched)


def test_long_horizon_window_algebra_vs_reference_get_batch():
    """tests/golden/long.npz = the reference's own ``get_batch`` (eval_smpl_long.py:26-84; imported through refshim, its one
    non-executable method chain removed -- see make_golden.py gen_long) on two windows of one clip.  Checked against it: the oracle's
    ``next_window_raw`` and the product's host function ``interdiff_amd.eval.next_window_raw`` (pure torch tensor algebra, the same code
    on the GPU) -- centroid, re-centred translations, rotations, copied pose, padding frames."""
    from oracle import long_horizon as olh
    from interdiff_amd import eval as ev
    z = fx.golden('long.npz')
    assert 'repeat' in str(z['shipped_get_batch_error'])          # the shipped function raises; the golden says how
    past, fut = fx.PAST, fx.LONG_FUTURE
    for w in range(fx.LONG_WINDOWS):
        body, obj, pel, verts = fx.long_inputs(w)
        raw = dict(beta=torch.zeros(past + fut, 1, 10), obj_points=torch.zeros(1, 8, 3))
        assert np.array_equal(z['w%d_rotation' % w], np.eye(3, dtype=np.float32))
        for name, (nxt, centroid) in (('oracle', olh.next_window_raw(body, obj, pel, raw, past, fut)), ('product', ev.next_window_raw(body, obj, pel, raw, fut))):
            close(centroid[0], z['w%d_centroid' % w], 0, name + ' centroid')
            close(nxt['body_trans'][:, 0], z['w%d_trans' % w], 1e-6, name + ' body translation')
            close(nxt['obj_trans'][:, 0], z['w%d_obj_trans' % w], 1e-6, name + ' object translation')
            pose = torch.cat([nxt['body_pose'], nxt['hand_pose']], dim=2)[:, 0]
            close(pose[:, 3:], z['w%d_pose' % w][:, 3:], 0, name + ' pose[3:] copied')
            close(R.axis_angle_to_matrix(pose[:, :3]), R.axis_angle_to_matrix(torch.from_numpy(z['w%d_pose' % w][:, :3])), 1e-5, name + ' root rotation')
            close(R.axis_angle_to_matrix(nxt['obj_angles'][:, 0]), R.axis_angle_to_matrix(torch.from_numpy(z['w%d_obj_angle' % w])), 1e-5, name + ' object rotation')
            if name == 'oracle':                              # the oracle also reproduces scipy's canonical representative
                close(pose[:, :3], z['w%d_pose' % w][:, :3], 1e-5, 'canonical root rotation vector')
                close(nxt['obj_angles'][:, 0], z['w%d_obj_angle' % w], 1e-5, 'canonical object rotation vector')
            for k in ('body_pose', 'hand_pose', 'body_trans', 'obj_angles', 'obj_trans'):
                assert nxt[k].shape[0] == past + fut and all(torch.equal(nxt[k][t], nxt[k][past - 1]) for t in range(past, past + fut))
        close(verts[0, 0, :3] - pel[0, 0], z['w%d_verts0' % w][0, :, :3], 1e-6, 'vertices re-centred on the same origin')
    assert float(torch.from_numpy(z['w1_pose'][0, :3]).norm()) <= np.pi + 1e-5 < float(fx.long_inputs(1)[0][0, 0, :3].norm())


def test_long_horizon_restatement_properties():
    """oracle/long_horizon.py ("next" row N3; upstream eval_smpl_long.py is broken, parity unpinned): what can be pinned without a
    reference run -- ``next_window_raw`` IS get_batch's arithmetic for clip 0 (origin = first pelvis, rotation = I, scipy-canonical
    rotation vectors, future = copies of the last past frame), window 0 of a rollout is the short-horizon sample, and the appended
    frames are translated back by exactly the window's centroid."""
    from scipy.spatial.transform import Rotation
    from oracle import long_horizon as olh
    from interdiff_amd import synthetic as syn
    T, B, P, past, steps, K = 12, 2, 64, fx.PAST, 4, 1
    ei = {k: torch.from_numpy(v) for k, v in syn.make_embedding_inputs(seed=5, B=B, T=T, n_points=P).items()}
    g = torch.Generator().manual_seed(2)
    raw = dict(ei, hand_pose=0.1 * torch.randn(T, B, 90, generator=g), beta=torch.randn(1, B, 10, generator=g).expand(T, B, 10).contiguous())
    body = torch.randn(past, B, 159, generator=g)
    body[0, 0, :3] = torch.tensor([4.0, 0.3, -0.2])                 # angle > pi: scipy re-expresses it, the rotation is unchanged
    obj, pelvis = torch.randn(past, B, 6, generator=g), torch.randn(past, B, 3, generator=g)
    nxt, centroid = olh.next_window_raw(body, obj, pelvis, raw, past, T - past)
    assert torch.equal(centroid, pelvis[0])
    # get_batch's own lines for clip 0, frame i (eval_smpl_long.py:40-63 with rotation = I)
    for i in (0, past - 1):
        c0 = pelvis[0, 0].numpy()
        trans = body[i, 0, -3:].numpy() - c0
        pel = pelvis[i, 0].numpy() - c0
        pel_orig = pel - trans
        np.testing.assert_allclose(nxt['body_trans'][i, 0].numpy(), np.dot(trans + pel_orig, np.eye(3)) - pel_orig, atol=1e-6)
        np.testing.assert_allclose(nxt['body_pose'][i, 0, :3].numpy(), Rotation.from_rotvec(body[i, 0, :3].numpy()).as_rotvec(), atol=1e-6)
        np.testing.assert_allclose(nxt['obj_trans'][i, 0].numpy(), obj[i, 0, 3:6].numpy() - c0, atol=1e-6)
        assert torch.equal(nxt['body_pose'][i, :, 3:], body[i, :, 3:66]) and torch.equal(nxt['hand_pose'][i], body[i, :, 66:156])
    close(R.axis_angle_to_matrix(nxt['body_pose'][0, 0, :3]), R.axis_angle_to_matrix(body[0, 0, :3]), 1e-5, 'same rotation')
    assert float(nxt['body_pose'][0, 0, :3].norm()) <= np.pi + 1e-6
    for k in ('body_pose', 'hand_pose', 'body_trans', 'obj_angles', 'obj_trans'):
        assert nxt[k].shape[0] == T and all(torch.equal(nxt[k][t], nxt[k][past - 1]) for t in range(past, T))
    # rollout: window 0 = the short-horizon sample; appended frames = the second window's future, moved back by its centroid
    sched = odf.make_schedule(steps)
    xT = lambda k: torch.from_numpy(np.random.RandomState(50 + k).standard_normal((B, 1, 144, T)).astype(np.float32))
    sn = lambda k: (lambda i, x: torch.from_numpy(np.random.RandomState(60 + 10 * k + i).standard_normal(tuple(x.shape)).astype(np.float32)))
    args = (fx.mdm_weights(), fx.smpl_model(), fx.objproj_weights())
    o, b, v, j, p = olh.rollout(*args, raw, K, past, sched, xT, sn)
    o0, b0, v0, j0, p0 = olh.sample_window(*args, raw, past, sched, xT(0), sn(0))
    F = T - past
    assert o.shape == (T + K * F, B, 6) and v.shape[0] == T + K * F
    assert torch.equal(o[:T], o0) and torch.equal(v[:T], v0) and torch.equal(p, j[:, :, 0])
    nxt, c = olh.next_window_raw(b0[-past:], o0[-past:], p0[-past:], raw, past, F)
    o1, b1, v1, j1, p1 = olh.sample_window(*args, nxt, past, sched, xT(1), sn(1))
    close(o[T:, :, 3:], o1[past:, :, 3:] + c, 1e-6, 'appended object translation')
    close(v[T:], v1[past:] + c[None, :, None, :], 1e-6, 'appended vertices')
    assert torch.equal(o[T:, :, :3], o1[past:, :, :3])


def test_well_conditioned_full_size_fixture_pair():
    """tests/golden/fullwc.npz (the REFERENCE's own full-size run with the well-conditioned synthetic denoiser, fixtures.mdm_weights_wc) against fullwc64.npz (the oracle's
    float64 twin on the same inputs): the pair that carries the flat 1e-4 end-to-end gate of the GPU suite.  Checked here, on CPU, without re-running the 1000 steps:
      * the oracle in float64 agrees with the reference's fp32 run at every dump (the sampler state to a few 1e-6; the final sample, behind eleven corrections, to 1e-4)
        and took the SAME 176 hook decisions (clips rewritten, reference marker picked) -- the oracle restates the reference on this fixture too;
      * the fixture is what it claims to be: on the reference's final sample no joint's two rot6d 3-vectors are anywhere near parallel (|cos| < 0.5; the random-init
        fixture full.npz: 0.99998), i.e. Gram-Schmidt cannot amplify fp32 rounding there;
      * the body rotations the reference returned equal the oracle's rot6d -> matrix of that sample as rotations (1e-5)."""
    z, z64 = fx.golden('fullwc.npz'), fx.golden('fullwc64.npz')
    assert list(z['corr_t']) == list(z64['corr_t']) == [500 - 50 * k for k in range(11)]
    assert np.array_equal(z['condition'], z64['condition']) and z['condition'].shape == (11, 16)
    def pick(c):                                                  # the node ObjProjector.sample reads its answer from (model/correction_smpl.py:125-136): no contact -> 0, else 1 + argmax(count + hand bonus)
        score = c.astype(np.float64).copy()
        score[..., oobj.HAND_MARKERS] += 0.5
        return np.where(c.sum(-1) > 0, 1 + score.argmax(-1), 0)
    assert np.array_equal(pick(z['contact']), pick(z64['contact']))
    for s_ in fx.FULLWC_DUMPS:
        d, d64 = z['dump_%d' % s_], z64['dump_%d' % s_]
        err = np.abs(d - d64).max() / np.abs(d64).max()
        assert err <= (1e-4 if s_ == 999 else 1e-5), (s_, err)
    body, _ = ocor.split_tokens(torch.from_numpy(z['dump_999']))
    T, B = body.shape[:2]
    r6 = body[..., :132].reshape(T, B, 22, 6)
    a1, a2 = r6[..., :3], r6[..., 3:]
    cos = ((a1 * a2).sum(-1) / (a1.norm(dim=-1) * a2.norm(dim=-1))).abs().max().item()
    assert cos < 0.5 and a1.norm(dim=-1).min().item() > 0.5, cos
    z0 = fx.golden('full.npz')
    b0, _ = ocor.split_tokens(torch.from_numpy(z0['dump_999']))
    r0 = b0[..., :132].reshape(T, B, 22, 6)
    cos0 = ((r0[..., :3] * r0[..., 3:]).sum(-1) / (r0[..., :3].norm(dim=-1) * r0[..., 3:].norm(dim=-1))).abs().max().item()
    assert cos0 > 0.999                                              # what the older fixture looks like
    close(R.rotation_6d_to_matrix(r6), R.axis_angle_to_matrix(torch.from_numpy(z['body'][..., :66]).reshape(T, B, 22, 3)), 1e-5, 'reference body rotations vs oracle rot6d -> matrix')


def test_sharpened_attention_fixture_reaches_trained_softmax_scales(monkeypatch):
    """tests/fixtures.py mdm_weights_sharp (the weights of tests/test_attention_scales.py): only the Q and K rows of the chosen attentions move, the default fixture is left
    alone, and the softmax rows the oracle then computes are what the fixture is for -- nearly uniform at gain 1 (largest probability of a self-attention row below 0.1 on
    average, ~0.2 of a cross-attention row), led by one or two keys at gain 2, saturated at gain 4 -- while the problem stays well conditioned: the oracle's own fp32 run
    is within 1e-5 of its float64 run (a tenth of the 1e-4 gate), so a whole-forward comparison against float64 stays a sharp test."""
    base = fx.mdm_weights()
    keep = {k: v.clone() for k, v in base.items()}
    one = fx.mdm_weights_sharp(4, (7,), ())
    for k, v in base.items():
        assert torch.equal(v, keep[k])
        if k in ('decoder.layers.7.self_attn.in_proj_weight', 'decoder.layers.7.self_attn.in_proj_bias'):
            assert torch.equal(one[k][:512], 4 * v[:512]) and torch.equal(one[k][512:], v[512:])
        else:
            assert torch.equal(one[k], v), k
    enc = fx.mdm_weights_sharp(2, None, None, 3)
    assert torch.equal(enc['encoder.layers.0.self_attn.in_proj_weight'][:512], 3 * base['encoder.layers.0.self_attn.in_proj_weight'][:512])
    assert torch.equal(enc['decoder.layers.3.multihead_attn.in_proj_bias'][:512], 2 * base['decoder.layers.3.multihead_attn.in_proj_bias'][:512])
    assert torch.equal(fx.mdm_weights_sharp(2)['encoder.layers.7.self_attn.in_proj_weight'], base['encoder.layers.7.self_attn.in_proj_weight'])
    B, T = 2, 35
    x, ts, cond = fx.mdm_inputs(B, T)
    rows = []
    real = torch.softmax

    def spy(s, dim=-1, **kw):
        p = real(s, dim=dim, **kw)
        if s.dim() == 4 and s.shape[-2] == T and s.shape[-1] in (T, fx.PAST):      # nn.MultiheadAttention's [B, heads, T, keys]: self- and cross-attention (not the QaN taps)
            rows.append((s.shape[-1], float(p.max(dim=-1)[0].mean())))
        return p
    monkeypatch.setattr(torch, 'softmax', spy)
    top = {}
    for g in (1, 2, 4):
        sd = base if g == 1 else fx.mdm_weights_sharp(g)
        del rows[:]
        out32 = oden.mdm_forward(sd, x, ts, cond)
        top[g] = {n: [p for keys, p in rows if keys == n] for n in (T, fx.PAST)}
        assert len(top[g][T]) == 2 and len(top[g][fx.PAST]) == 8
        out64 = oden.mdm_forward({k: v.double() for k, v in sd.items()}, x.double(), ts, cond.double())
        close(out32.double(), out64, 1e-5, 'oracle fp32 vs float64 at gain %d' % g)
    # mean largest probability of a row, per attention (measured: self 0.075 / 0.041, cross 0.18-0.21 | self 0.37 / 0.09, cross 0.47-0.59 | self 0.82 / 0.50, cross 0.83-0.90)
    assert max(top[1][T]) <= 0.1 and max(top[1][fx.PAST]) <= 0.25
    assert max(top[2][T]) >= 0.3 and min(top[2][fx.PAST]) >= 0.4
    assert max(top[4][T]) >= 0.7 and min(top[4][T]) >= 0.4 and min(top[4][fx.PAST]) >= 0.8
