"""Generate tests/golden/skel_losses.npz by running the REFERENCE's own trainer functions (train_diffusion_skeleton.py ``LitInteraction``:
``_common_step`` in modes 'train' / 'valid', ``forward_backward``, ``calc_val_loss``, ``log_loss_dict``) and its own
``GaussianDiffusion.training_losses`` / ``q_sample`` and skeleton ``MDM``, imported read-only through refshim.py.  The functions are called
as plain functions on an object that carries what they read (``args``, the reference model with the seeded synthetic weights
``interdiff_amd.synthetic.skeleton_mdm_state_dict(SEED)`` -- no skeleton diffusion checkpoint ships; the weights are NOT stored --, the
reference diffusion, a schedule sampler that returns the recorded ``t``); Lightning never runs.  Run in the build container only:

    python tests/golden/make_golden_skeleton_losses.py

Recorded (B = 3, T = 20, past_len = 10; weights = the trainer's own argparse defaults, read from its source text):
  batch_*  the dataset-layout batch (body, obj, pose, zero_pose_obj)
  fb_*     _common_step(mode='train') -> forward_backward: cond and gt from the reference's _get_embeddings, per-clip t, eps; outputs x_t, the
           model output, the 13 unweighted terms (recomputed from the reference's own pred / gt split by the expressions of :108-127, since
           forward_backward keeps its loss_dict to itself -- asserted equal, weighted, to what it hands log_loss_dict), the 13 weighted terms as
           handed to log_loss_dict, the scalar loss, every (key, value) it logs, and the per-clip means [13,B] of the same expressions
  val_*    _common_step(mode='valid') with the sampler returning the recorded sample (gt + seeded noise): 13 terms, 13 weighted, loss
  c50_* / c1000_*   calc_val_loss on the FINAL samples of the two reference chains recorded in skel_mdm.npz (c50_final: 50 steps, identity
           hook, B = 1; c1000_dump_999: 1000 steps with the real obj_skeleton.ckpt hook, B = 2) against their ground truth
With B = 3 the injected timesteps cover three of the four quartiles of the schedule (0, 1 and 3); the skeleton trainer's log_loss_dict makes no
quartile split, so nothing recorded depends on it.
Asserted here: q . q >= 0.25 on every predicted quaternion; no recorded fb_ / val_ term is below 1e-6, so a relative gate never divides by
nothing.  The chains' samples carry the inpainted past frames, so their *_past terms are EXACTLY zero in the reference (body_past in both;
all four in the chain without the hook): for the chains the assertion is "exactly 0.0 or >= 1e-6", and the tests ask for exact zeros there.
One more chain term cannot pass it: the hook of the 1000-step chain ends on a matrix -> quaternion conversion, so the final sample's quaternions
are unit to rounding and quaternion_reg_loss is the reference's own fp32 rounding noise (2.5e-15).  It is recorded as it is, asserted here to be
the ONLY such term and <= (5e-7)^2 = 2.5e-13 (q . q of a unit quaternion is 1 to four fp32 roundings), and the tests hold the kernel to that
same absolute bound instead of a relative one.
"""
import os
import re
import sys
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
import make_golden_skeleton_mdm as mgsm           # noqa: E402
import make_golden_corr_losses as mgc             # noqa: E402
from tests import fixtures as fx                  # noqa: E402
from interdiff_amd import synthetic as syn        # noqa: E402

torch.set_grad_enabled(False)
np_ = lambda t: t.detach().cpu().numpy()
B, T, PAST, SEED = 3, 20, 10, 8900
TS = [37, 412, 875]
SAMPLE_NOISE = 0.03
MIN_QQ, MIN_TERM = 0.25, 1e-6
UNIT_QUAT_REG_MAX = 2.5e-13                       # (5e-7)^2: q . q of a unit quaternion is 1 to four fp32 roundings, 4 x 1.2e-7
WEIGHT_NAMES = ('weight_past', 'weight_body', 'weight_obj', 'weight_obj_rot', 'weight_obj_nonrot', 'weight_quat_reg', 'weight_v')
KEYS = ('body_past', 'body_future', 'obj_past', 'obj_future', 'loss_obj_nonrot_past', 'loss_obj_nonrot_future', 'loss_obj_rot_past',
        'loss_obj_rot_future', 'quaternion_reg_loss', 'loss_obj_rot_v', 'loss_obj_nonrot_v', 'loss_body_v', 'loss_obj_v')


def cli_defaults():
    """The trainer's own argparse defaults (train_diffusion_skeleton.py:372-379), read from its source text."""
    txt = open(os.path.join(refshim.REF, 'train_diffusion_skeleton.py')).read()
    return {n: float(re.search(r'add_argument\("--%s", type=float, default=([0-9.e-]+)' % n, txt).group(1)) for n in WEIGHT_NAMES}


def unweighted(pred, gt, per_clip):
    """The expressions of forward_backward :108-127 on its own split (:101-104), fp32 torch; ``per_clip``: the same means clip by clip."""
    sp = lambda x: torch.split(x.squeeze(1).permute(2, 0, 1).contiguous(), [63, 36, 7], dim=2)
    (bp, op, pp), (bg, og, pg) = sp(pred), sp(gt)
    P = PAST
    if per_clip:
        mse = lambda a, b: ((a - b) ** 2).mean(dim=[0, 2])
        red = lambda v: v.mean(dim=0)
    else:
        mse = lambda a, b: torch.nn.MSELoss(reduction='mean')(a, b)
        red = lambda v: v.mean()
    vel = lambda a: a[1:] - a[:-1]
    d = dict(body_past=mse(bp[:P], bg[:P]), body_future=mse(bp[P:], bg[P:]), obj_past=mse(op[:P], og[:P]), obj_future=mse(op[P:], og[P:]),
             loss_obj_nonrot_past=mse(pp[:P, :, :3], pg[:P, :, :3]), loss_obj_nonrot_future=mse(pp[P:, :, :3], pg[P:, :, :3]),
             loss_obj_rot_past=mse(pp[:P, :, -4:], pg[:P, :, -4:]), loss_obj_rot_future=mse(pp[P:, :, -4:], pg[P:, :, -4:]),
             quaternion_reg_loss=red((pp[:, :, -4:].norm(p=2, dim=-1).square() - 1).square()),
             loss_obj_rot_v=mse(vel(pp[:, :, -4:]), vel(pg[:, :, -4:])), loss_obj_nonrot_v=mse(vel(pp[:, :, :3]), vel(pg[:, :, :3])),
             loss_body_v=mse(vel(bp), vel(bg)), loss_obj_v=mse(vel(op), vel(og)))
    return torch.stack([d[k] for k in KEYS])


def min_qq(x):
    return float((x[:, 0, -4:] ** 2).sum(1).min())


def main():
    tds = mgc.trainer('train_diffusion_skeleton')
    gd, diff = mgsm.diffusion(1000)
    net = mgsm.ref_mdm()
    w = cli_defaults()
    args = Namespace(num_joints=21, num_points=12, past_len=PAST, render=False, render_epoch=10 ** 9, debug=False, **w)
    bt = {k: torch.from_numpy(v) for k, v in syn.make_skeleton_batch(SEED, B=B, T=T).items()}
    batch = (bt['body'], bt['obj'], bt['pose'], bt['zero_pose_obj'])
    rs = np.random.RandomState(SEED + 1)
    eps = fx._randn(rs, B, 1, 106, T)
    t = torch.tensor(TS, dtype=torch.int64)
    wv = np.asarray([w['weight_body'] * w['weight_past'], w['weight_body'], w['weight_obj'] * w['weight_past'], w['weight_obj'],
                     w['weight_obj_nonrot'] * w['weight_past'], w['weight_obj_nonrot'], w['weight_obj_rot'] * w['weight_past'], w['weight_obj_rot'],
                     w['weight_quat_reg'], w['weight_obj_rot'] * w['weight_v'], w['weight_obj_nonrot'] * w['weight_v'],
                     w['weight_body'] * w['weight_v'], w['weight_obj'] * w['weight_v']])
    out = dict({'batch_' + k: np_(v) for k, v in bt.items()}, t=np_(t), eps=np_(eps), past_len=np.int64(PAST), seed=np.int64(mgsm.SEED),
               keys=np.asarray(KEYS), weights=np.asarray([w[k] for k in WEIGHT_NAMES]), weight_names=np.asarray(WEIGHT_NAMES))
    qq = []

    # ---- _common_step(mode='train'): _get_embeddings + forward_backward (teacher-forced objective) -------------------------------
    seen, logged = {}, []

    class Watch(torch.nn.Module):
        def forward(self, x, ts, zero_pose_obj, y=None):
            seen.update(x_t=x.clone(), ts=ts.clone(), cond=y['cond'].clone(), zero=zero_pose_obj.clone())
            seen['out'] = net(x, ts, zero_pose_obj, y=y)
            return seen['out']
    lit = mgc.Lit(tds.LitInteraction, net, args, 0)
    lit.diffusion, lit.ddp_model = diff, Watch()
    lit.schedule_sampler = Namespace(sample=lambda n, device: (t, torch.ones(n)))
    lit.log = lambda key, value, prog_bar=False: logged.append((key, float(value)))

    def log_loss_dict(diffusion, ts, losses, loss):
        seen['weighted'] = {k: v.clone() for k, v in losses.items()}
        return tds.LitInteraction.log_loss_dict(lit, diffusion, ts, losses, loss)
    lit.log_loss_dict = log_loss_dict
    real = gd.th.randn_like
    gd.th.randn_like = lambda x: eps.clone()
    try:
        loss = tds.LitInteraction._common_step(lit, batch, 1, 'train')
    finally:
        gd.th.randn_like = real
    assert list(seen['weighted']) == list(KEYS) and torch.equal(seen['ts'], t)
    assert [k for k, _ in logged] == ['train_loss'] and logged[0][1] == float(loss)          # ALL this trainer logs (:177-180)
    tb = lambda a: a.transpose(0, 1).contiguous()
    cond, gt_tbc = net._get_embeddings(tb(bt['body']), tb(bt['obj']), tb(bt['pose']), bt['zero_pose_obj'])
    gt = gt_tbc.permute(1, 2, 0).unsqueeze(1).contiguous()
    assert torch.equal(cond, seen['cond']) and torch.equal(diff.q_sample(gt, t, noise=eps.clone()), seen['x_t'])
    fb_weighted = torch.stack([seen['weighted'][k] for k in KEYS])
    fb_terms = unweighted(seen['out'], gt, False)
    fb_per_clip = unweighted(seen['out'], gt, True)
    assert np.abs(np_(fb_terms) * wv - np_(fb_weighted)).max() <= 1e-6 * np.abs(np_(fb_weighted)).max()
    assert np.abs(np_(fb_per_clip.mean(dim=1)) - np_(fb_terms)).max() <= 1e-6 * np.abs(np_(fb_terms)).max()
    qq.append(min_qq(seen['out']))
    out.update(gt=np_(gt), cond=np_(cond), fb_x_t=np_(seen['x_t']), fb_out=np_(seen['out']), fb_terms=np_(fb_terms), fb_weighted=np_(fb_weighted),
               fb_loss=np_(loss), fb_per_clip=np_(fb_per_clip), fb_logged_keys=np.asarray([k for k, _ in logged]),
               fb_logged_values=np.asarray([v for _, v in logged]))

    # ---- _common_step(mode='valid') with the sampler returning the recorded sample ------------------------------------------------
    sample = gt + SAMPLE_NOISE * fx._randn(rs, B, 1, 106, T)
    lit.diffusion = Namespace(p_sample_loop=lambda model, shape, clip_denoised, model_kwargs: sample.clone())
    vloss, vd, vw = tds.LitInteraction._common_step(lit, batch, 1, 'valid')
    assert list(vd) == list(KEYS) and list(vw) == list(KEYS)
    qq.append(min_qq(sample))
    stack = lambda d: np_(torch.stack([d[k] for k in KEYS]))
    out.update(val_sample=np_(sample), val_terms=stack(vd), val_weighted=stack(vw), val_loss=np_(vloss))
    for name in ('fb_terms', 'fb_weighted', 'fb_per_clip', 'val_terms', 'val_weighted'):
        assert float(out[name].min()) >= MIN_TERM, '%s has a term below %g: change the seed, not the gate' % (name, MIN_TERM)

    # ---- calc_val_loss on the final samples of the two chains recorded in skel_mdm.npz ---------------------------------------------
    z = np.load(os.path.join(HERE, 'skel_mdm.npz'))
    for pre, key in (('c50_', 'c50_final'), ('c1000_', 'c1000_dump_999')):
        s, g = torch.from_numpy(z[key]), torch.from_numpy(z[pre + 'gt'])
        sp = lambda x: torch.split(x.squeeze(1).permute(2, 0, 1).contiguous(), [63, 36, 7], dim=2)             # _common_step :280-283
        (bp, op, pp), (bg, og, pg) = sp(s), sp(g)
        closs, cd, cw = tds.LitInteraction.calc_val_loss(lit, bp, bg, op, og, pp, pg, batch=None)
        assert list(cd) == list(KEYS)
        qq.append(min_qq(s))
        out.update({pre + 'terms': stack(cd), pre + 'weighted': stack(cw), pre + 'loss': np_(closs)})
        vals = out[pre + 'terms']
        print('%-7s terms: %s' % (pre, ' '.join('%.3e' % v for v in vals)))
        tiny = [KEYS[i] for i, v in enumerate(vals.tolist()) if 0.0 < v < MIN_TERM]
        assert tiny == (['quaternion_reg_loss'] if pre == 'c1000_' else []) and all(v <= UNIT_QUAT_REG_MAX for v in vals[[KEYS.index(k) for k in tiny]]), (pre, tiny)
        assert vals[0] == 0.0 and vals[1] > 0.0                                                                # body_past: inpainted, exact
    out.update(min_qq=np.float64(min(qq)))
    print('min q.q = %.4f; forward_backward loss %.6f, val_loss %.6f, chains %.6f / %.6f' % (min(qq), float(loss), float(vloss), float(out['c50_loss']), float(out['c1000_loss'])))
    assert min(qq) >= MIN_QQ, 'a predicted quaternion came too close to zero: change the seed, not the gate'
    mgs.save('skel_losses.npz', **out)


if __name__ == '__main__':
    main()
