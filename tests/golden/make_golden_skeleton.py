"""Generate the HO-GCN skeleton-mode golden fixtures under tests/golden/ by running the REFERENCE's own source (imported
read-only through refshim.py, like make_golden.py).  Run in the build container only:

    python tests/golden/make_golden_skeleton.py

What each fixture pins (reference file:line in brackets):
  skel_ckpt.npz     the trained predictor's state_dict (checkpoints/obj_skeleton.ckpt, ``model.`` prefix stripped) as float32
  skel_objproj.npz  ObjProjector.sample at B = 1 and B = 64, some quaternions non-unit and some with w < 0, inputs stored
                    [model/correction_skeleton.py:84-137]
  skel_hook.npz     eval_skeleton.denoised_fn at t = 500, 250, 50, 0 on one B = 4 batch, inputs stored [eval_skeleton.py:82-111]
  skel_metrics.npz  eval_skeleton.calc_metric_single, inputs stored [eval_skeleton.py:46-68]
  skel_loop.npz     GaussianDiffusion.p_sample_loop, 1000-step cosine schedule, B = 4, T = 20, with a deterministic stand-in
                    denoiser (its weight stored), the reference denoised_fn with the real predictor and per-step noise
                    tests.fixtures.NoiseStream(SKEL_LOOP_NOISE) injected through gd.th.randn_like; the sampler state at SKEL_LOOP_DUMPS
                    [gaussian_diffusion.py:598-736]
"""
import os
import sys
import types
import warnings
from argparse import Namespace
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, '..', '..'))
warnings.filterwarnings('ignore')
import refshim                                    # noqa: E402
from tests import fixtures as fx                  # noqa: E402

torch.set_grad_enabled(False)
np_ = lambda t: t.detach().cpu().numpy()
CKPT = os.path.join(refshim.REF, 'checkpoints', 'obj_skeleton.ckpt')
T, PAST = 20, 10
SKEL_LOOP_NOISE, SKEL_LOOP_DUMPS = 5106, [0, 499, 500, 749, 949, 999]
HOOK_TS = [500, 250, 50, 0]


def save(name, **arrs):
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **arrs)
    print('%-22s %8.1f KB' % (name, os.path.getsize(path) / 1024))


def install():
    refshim.install()
    mod = lambda name, **a: sys.modules.setdefault(name, types.ModuleType(name)).__dict__.update(a)
    mod('train_correction_skeleton', LitObjInteraction=None)     # eval_skeleton.py:10-12, never touched by what is recorded
    mod('train_diffusion_skeleton', LitInteraction=None)
    mod('data.dataset_skeleton', get_datasets=None)


def ref_objprojector():
    ck = torch.load(CKPT, map_location='cpu', weights_only=False)
    cm = refshim.load('model.correction_skeleton')
    op = cm.ObjProjector(Namespace(**ck['hyper_parameters'])).eval()
    sd = {k[6:]: v for k, v in ck['state_dict'].items() if k.startswith('model.')}
    missing, unexpected = op.load_state_dict(sd, strict=True)
    assert not missing and not unexpected
    return op, sd


def quats(rs, *shape):
    q = rs.standard_normal(shape + (4,)).astype(np.float32)
    q[..., 3] = -np.abs(q[..., 3])                        # w < 0 everywhere in the even clips ...
    q[:, 1::2, 3] = np.abs(q[:, 1::2, 3])                 # ... and > 0 in the odd ones; none of them unit length
    return torch.from_numpy(q)


def poses(rs, T_, B, scale=0.5):
    """[T,B,7] translation | quaternion xyzw (non-unit: the hook takes what the sampler produces)."""
    return torch.cat([torch.from_numpy((scale * rs.standard_normal((T_, B, 3))).astype(np.float32)), quats(rs, T_, B)], dim=2)


def tokens(rs, B):
    """[B,1,106,T]: body 21x3 | object keypoints 12x3 | pose 7."""
    body = 0.5 * rs.standard_normal((T, B, 63))
    obj = 0.5 * rs.standard_normal((T, B, 36))
    pose = np_(poses(rs, T, B))
    x = np.concatenate([body, obj, pose], axis=2).astype(np.float32)
    return torch.from_numpy(np.ascontiguousarray(x.transpose(1, 2, 0)[:, None]))


def main():
    install()
    op, sd = ref_objprojector()
    save('skel_ckpt.npz', **{k: np_(v).astype(np.float32) for k, v in sd.items() if not k.endswith('num_batches_tracked')})

    # ---- ObjProjector.sample
    out = {}
    for B in (1, 64):
        rs = np.random.RandomState(7000 + B)
        oa = quats(rs, T, B)
        ot = torch.from_numpy((0.5 * rs.standard_normal((T, B, 3))).astype(np.float32))
        hp = torch.from_numpy((0.5 * rs.standard_normal((T, B, 21, 3))).astype(np.float32))
        q, tr = op.sample(oa, ot, hp)
        out.update({'angles_b%d' % B: np_(oa), 'trans_b%d' % B: np_(ot), 'human_b%d' % B: np_(hp),
                    'quat_out_b%d' % B: np_(q), 'trans_out_b%d' % B: np_(tr)})
    save('skel_objproj.npz', **out)

    ev = refshim.load('eval_skeleton')
    holder = types.SimpleNamespace(model=op)

    # ---- denoised_fn
    B = 4
    rs = np.random.RandomState(7106)
    x, gt = tokens(rs, B), tokens(rs, B)
    z = torch.from_numpy((0.3 * rs.standard_normal((B, 12, 3))).astype(np.float32))
    out = dict(x=np_(x), gt=np_(gt), zero_pose_obj=np_(z))
    for tval in HOOK_TS:
        kw = {'y': {'inpainted_motion': gt.clone(), 'obj_model': holder}, 'zero_pose_obj': z}
        r = ev.denoised_fn(x.clone(), torch.full((B,), tval, dtype=torch.int64), kw)
        out['out_t%d' % tval] = np_(r)
    save('skel_hook.npz', **out)

    # ---- calc_metric_single
    rs = np.random.RandomState(7200)
    B = 8
    arr = lambda *s: torch.from_numpy((0.5 * rs.standard_normal(s)).astype(np.float32))
    m_in = dict(body_pred=arr(T, B, 21, 3), body_gt=arr(T, B, 21, 3), obj_pred=arr(T, B, 12, 3), obj_gt=arr(T, B, 12, 3),
                pose_pred=poses(rs, T, B), pose_gt=poses(rs, T, B))
    res = ev.calc_metric_single(*[m_in[k] for k in ('body_pred', 'body_gt', 'obj_pred', 'obj_gt', 'pose_pred', 'pose_gt')])
    save('skel_metrics.npz', **{k: np_(v) for k, v in m_in.items()}, **{k: np.float64(v) for k, v in res.items()})

    # ---- 1000-step p_sample_loop with the reference hook
    gd = refshim.load('diffusion.gaussian_diffusion')
    rsp = refshim.load('diffusion.respace')
    B, C, steps = 4, 106, 1000
    rs = np.random.RandomState(7300)
    w = (rs.standard_normal((C, C)) * (0.5 / np.sqrt(C))).astype(np.float32)
    gt, noise = tokens(rs, B), torch.from_numpy(rs.standard_normal((B, 1, C, T)).astype(np.float32))
    z = torch.from_numpy((0.3 * rs.standard_normal((B, 12, 3))).astype(np.float32))
    mask = torch.ones(B, 1, C, T, dtype=torch.bool)
    mask[..., PAST:] = False
    wt = torch.from_numpy(w)

    class StandIn(torch.nn.Module):                 # the same function as standin_model in tests/test_skeleton_correction.py
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(wt, requires_grad=False)

        def forward(self, x, t, y=None, **kw):
            return torch.tanh(torch.einsum('dc,bgct->bgdt', self.w, x)) * (1.0 + 0.01 * t.float().view(-1, 1, 1, 1) / steps)
    model = StandIn()
    d = rsp.SpacedDiffusion(use_timesteps=rsp.space_timesteps(steps, [steps]), betas=gd.get_named_beta_schedule('cosine', steps, 1.),
                            model_mean_type=gd.ModelMeanType.START_X, model_var_type=gd.ModelVarType.FIXED_SMALL,
                            loss_type=gd.LossType.MSE, rescale_timesteps=False, lambda_vel=1.)
    stream = fx.NoiseStream(SKEL_LOOP_NOISE)
    real = gd.th.randn_like
    gd.th.randn_like = lambda x: stream.next_like(x)
    try:
        kw = {'y': {'inpainted_motion': gt, 'inpainting_mask': mask, 'obj_model': holder}, 'zero_pose_obj': z}
        dumps = d.p_sample_loop(model, (B, 1, C, T), clip_denoised=False, noise=noise.clone(), model_kwargs=kw,
                                denoised_fn=ev.denoised_fn, dump_steps=SKEL_LOOP_DUMPS)
    finally:
        gd.th.randn_like = real
    save('skel_loop.npz', w=w, gt=np_(gt), noise=np_(noise), zero_pose_obj=np_(z), noise_seed=np.int64(SKEL_LOOP_NOISE),
         dump_steps=np.asarray(SKEL_LOOP_DUMPS), **{'dump_%d' % s: np_(v) for s, v in zip(SKEL_LOOP_DUMPS, dumps)})


if __name__ == '__main__':
    main()
