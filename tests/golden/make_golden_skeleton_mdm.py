"""Generate tests/golden/skel_mdm.npz by running the REFERENCE's own skeleton denoiser (model/diffusion_skeleton.py ``MDM``,
imported read-only through refshim.py like make_golden_skeleton.py) on the seeded synthetic weights
``interdiff_amd.synthetic.skeleton_mdm_state_dict(SEED)`` -- no skeleton diffusion checkpoint ships; the weights are NOT stored,
the tests regenerate them from the seed.  Run in the build container only:

    python tests/golden/make_golden_skeleton_mdm.py

Recorded (reference file:line in brackets), MDM built with ff_size=256, past_len=10, latent_usage='memory':
  emb_*      one _get_embeddings at B = 3, T = 20 [diffusion_skeleton.py:194-215]
  fwd20_*    one forward at B = 3, T = 20, fwd35_* one at B = 3, T = 35 [:250-257]
  c50_*      the 50-step chain of BASELINE config #1 (eval_skeleton_no_correction.py: B = 1, T = 20, identity hook), injected noise
  c1000_*    a 1000-step chain with the real obj_skeleton.ckpt hook (eval_skeleton.py:82-111) at B = 2, T = 20, injected noise
  min_qq     min over every recorded forward and every step of both chains of q . q of the predicted quaternion (asserted >= 0.25:
             calc_obj_pred's 2 / (q . q) is ill-conditioned near zero, and a trained head emits near-unit quaternions)
  c50_rel64, c1000_rel64   max|fp32 chain - fp64 chain| / max|fp64 chain| at the final sample, the same chain with the model in fp64
             (asserted <= 2.5e-5, a quarter of the tests' 1e-4 gate)
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
import make_golden_skeleton as mgs                # noqa: E402
from tests import fixtures as fx                  # noqa: E402
from interdiff_amd import synthetic as syn        # noqa: E402

torch.set_grad_enabled(False)
np_ = lambda t: t.detach().cpu().numpy()
SEED, T, PAST = 1106, 20, 10
C50_NOISE, C1000_NOISE = 5150, 5151
C1000_DUMPS = [0, 499, 500, 949, 999]
MIN_QQ, MAX_REL64 = 0.25, 2.5e-5


def ref_mdm(dtype=torch.float32):
    m = refshim.load('model.diffusion_skeleton')
    args = Namespace(embedding_dim=256, smpl_dim=63, num_joints=21, num_points=12, dropout=0.0, num_heads=4, ff_size=256,
                     activation='gelu', latent_usage='memory', past_len=PAST, cond_mask_prob=0)
    net = m.MDM(args).eval()
    sd = {k: torch.from_numpy(v) for k, v in syn.skeleton_mdm_state_dict(SEED).items()}
    missing, unexpected = net.load_state_dict(sd, strict=False)
    assert not unexpected, unexpected
    assert all(k.startswith(('PositionalEmbedding', 'embedTimeStep.sequence_pos_encoder')) for k in missing), missing
    return net.to(dtype)


def diffusion(steps):
    gd, rsp = refshim.load('diffusion.gaussian_diffusion'), refshim.load('diffusion.respace')
    d = rsp.SpacedDiffusion(use_timesteps=rsp.space_timesteps(steps, [steps]), betas=gd.get_named_beta_schedule('cosine', steps, 1.),
                            model_mean_type=gd.ModelMeanType.START_X, model_var_type=gd.ModelVarType.FIXED_SMALL,
                            loss_type=gd.LossType.MSE, rescale_timesteps=False, lambda_vel=1.)
    return gd, d


class Watch(torch.nn.Module):
    """The model with the smallest q . q of every forward noted."""

    def __init__(self, net, rec):
        super().__init__()
        self.net, self.rec = net, rec

    def forward(self, x, t, zero_pose_obj, y=None):
        out = self.net(x, t, zero_pose_obj, y=y)
        self.rec.append(float((out[:, 0, -4:] ** 2).sum(1).min()))
        return out


def chain(net, hook, holder, steps, seed, inputs, dumps, dtype, rec):
    gd, d = diffusion(steps)
    c = lambda v: v.to(dtype) if v.is_floating_point() else v
    gt, noise, z, cond = (c(inputs[k]) for k in ('gt', 'noise', 'zero_pose_obj', 'cond'))
    mask = torch.ones(gt.shape, dtype=torch.bool)
    mask[..., PAST:] = False
    stream = fx.NoiseStream(seed)
    real = gd.th.randn_like
    gd.th.randn_like = lambda x: stream.next_like(x).to(dtype)
    fn = hook
    if dtype == torch.float64 and holder is not None:
        # the fp64 twin is the MODEL in fp64; the reference's predictor casts its own constants to fp32 (correction_skeleton.py:92-93) and stays fp32
        kw32 = {'y': {'inpainted_motion': inputs['gt'], 'obj_model': holder}, 'zero_pose_obj': inputs['zero_pose_obj']}

        def fn(x, t, kw):
            xf = x.float()
            r = hook(xf, t, kw32)
            return x if r is xf else r.double()
    try:
        kw = {'y': {'cond': cond, 'inpainted_motion': gt, 'inpainting_mask': mask, 'obj_model': holder}, 'zero_pose_obj': z}
        return d.p_sample_loop(Watch(net, rec), tuple(gt.shape), clip_denoised=False, noise=noise.clone(), model_kwargs=kw,
                               denoised_fn=fn, dump_steps=dumps)
    finally:
        gd.th.randn_like = real


def chain_inputs(seed, B):
    rs = np.random.RandomState(seed)
    bt = syn.make_skeleton_batch(seed + 1, B=B, T=T)
    gt = np.concatenate([bt['body'].reshape(B, T, -1), bt['obj'].reshape(B, T, -1), bt['pose']], axis=2).transpose(0, 2, 1)[:, None]
    return dict(gt=torch.from_numpy(np.ascontiguousarray(gt)), noise=fx._randn(rs, B, 1, 106, T), zero_pose_obj=torch.from_numpy(bt['zero_pose_obj']),
                cond=fx._randn(rs, PAST, B, 256))


def main():
    mgs.install()
    net, net64 = ref_mdm(), ref_mdm(torch.float64)
    out, qq = {}, []
    # ---- _get_embeddings and forwards
    B = 3
    bt = {k: torch.from_numpy(v) for k, v in syn.make_skeleton_batch(7400, B=B, T=T).items()}
    tb = lambda a: a.transpose(0, 1).contiguous()
    cond, gt = net._get_embeddings(tb(bt['body']), tb(bt['obj']), tb(bt['pose']), bt['zero_pose_obj'])
    out.update(emb_body=np_(bt['body']), emb_obj=np_(bt['obj']), emb_pose=np_(bt['pose']), emb_zero=np_(bt['zero_pose_obj']),
               emb_cond=np_(cond), emb_gt=np_(gt))
    rs = np.random.RandomState(7401)
    for T_ in (20, 35):
        x, ts = fx._randn(rs, B, 1, 106, T_), torch.from_numpy(rs.randint(0, 1000, B))
        z, cd = torch.from_numpy((0.3 * rs.standard_normal((B, 12, 3))).astype(np.float32)), (cond if T_ == 20 else fx._randn(rs, PAST, B, 256))
        r = Watch(net, qq)(x, ts, z, y={'cond': cd})
        out.update({'fwd%d_x' % T_: np_(x), 'fwd%d_ts' % T_: np_(ts), 'fwd%d_zero' % T_: np_(z), 'fwd%d_cond' % T_: np_(cd), 'fwd%d_out' % T_: np_(r)})
    # ---- config #1: 50 steps, identity hook (eval_skeleton_no_correction.py:82-83)
    ident = lambda x, t, kw: x
    i50 = chain_inputs(7410, 1)
    a = chain(net, ident, None, 50, C50_NOISE, i50, None, torch.float32, qq)
    b = chain(net64, ident, None, 50, C50_NOISE, i50, None, torch.float64, [])
    rel50 = float((a.double() - b).abs().max() / b.abs().max())
    out.update({'c50_' + k: np_(v) for k, v in i50.items()}, c50_final=np_(a), c50_noise_seed=np.int64(C50_NOISE), c50_rel64=np.float64(rel50))
    # ---- 1000 steps with the real hook
    ev = refshim.load('eval_skeleton')
    op, _ = mgs.ref_objprojector()
    i1k = chain_inputs(7420, 2)
    a = chain(net, ev.denoised_fn, types.SimpleNamespace(model=op), 1000, C1000_NOISE, i1k, C1000_DUMPS, torch.float32, qq)
    b = chain(net64, ev.denoised_fn, types.SimpleNamespace(model=op), 1000, C1000_NOISE, i1k, C1000_DUMPS, torch.float64, [])
    rel1k = float((a[-1].double() - b[-1]).abs().max() / b[-1].abs().max())
    out.update({'c1000_' + k: np_(v) for k, v in i1k.items()}, c1000_noise_seed=np.int64(C1000_NOISE), c1000_dump_steps=np.asarray(C1000_DUMPS),
               c1000_rel64=np.float64(rel1k), **{'c1000_dump_%d' % s: np_(v) for s, v in zip(C1000_DUMPS, a)})
    out.update(seed=np.int64(SEED), min_qq=np.float64(min(qq)))
    print('min q.q = %.4f over %d forwards; fp32 vs fp64 at the final sample: 50 steps %.3e, 1000 steps + hook %.3e' % (min(qq), len(qq), rel50, rel1k))
    assert min(qq) >= MIN_QQ, 'a predicted quaternion came too close to zero: change the seed or the head scale, not the gate'
    assert rel50 <= MAX_REL64 and rel1k <= MAX_REL64, 'the chain amplifies rounding beyond a quarter of the gate: change the seed or the head scale'
    mgs.save('skel_mdm.npz', **out)


if __name__ == '__main__':
    main()
