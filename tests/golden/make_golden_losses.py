"""Generate tests/golden/losses.npz by running the REFERENCE's own trainer functions (train_diffusion_smpl.py ``LitInteraction``:
``forward_backward``, ``_common_step`` in modes 'valid' / 'test', ``calc_val_loss``, ``calc_loss``, ``log_loss_dict``) and its own
``GaussianDiffusion.training_losses`` / ``q_sample``, imported read-only through refshim.py.  The functions are called as plain functions
on a namespace that carries what they read (``args``, ``l2``, ``log``, a schedule sampler that returns the recorded ``t``, the reference
MDM with the seeded synthetic weights, the reference diffusion); Lightning never runs.  Run in the build container only:

    python tests/golden/make_golden_losses.py

Third-party arithmetic the reference calls but does not ship is stubbed with restatements (refshim.py); new here: human_body_prior's
``tgm_conversion.angle_axis_to_rotation_matrix`` behind tools.py's ``aa2matrot`` = tests/losses_oracle.py ``aa2matrot`` (parity unpinned
-- restatement defines the contract), so the recorded numbers pin the reference's code AROUND it.

Recorded (B = 4, T = 35, K = 3, past_len = 10):
  fb_*     forward_backward: inputs x0 (= the clip batch's gt), per-clip t (one per timestep quartile), eps, cond; outputs x_t, the
           model output, the 16 weighted per-clip vectors [16,B] as handed to log_loss_dict, the scalar loss, every logged quartile value
  qs_x_t   q_sample + the inpainting of x_t through training_losses with the mask keys present (motion = x0 + 1, mask = past frames)
  val_*    _common_step(mode='valid') on sample 0: the 16 terms, their weighted forms, the loss
  test_*   _common_step(mode='test') on the K samples: the 32 terms, the 16 weighted, the loss, and the reference's per-(sample, clip)
           means [K,16,B] recomputed from its own intermediate tensors for the tie check below
The K samples are the ground truth plus seeded perturbations whose size differs per (sample, clip, channel group), laid out so that
the best sample of clip 0 differs between the body and the object terms; asserted here: for every term and clip the reference's own
per-clip values of any two samples differ by more than 1e-3 relative, so no ``_min`` pick can flip within rounding.
"""
import importlib
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
import make_golden as mg                          # noqa: E402
import make_golden_skeleton as mgs                # noqa: E402
from tests import fixtures as fx                  # noqa: E402
from tests import losses_oracle as lo             # noqa: E402
from interdiff_amd import synthetic as syn        # noqa: E402

torch.set_grad_enabled(False)
np_ = lambda t: t.detach().cpu().numpy()
B, T, K, PAST, SEED = 4, 35, 3, 10, 8800
TS = [37, 412, 655, 999]                          # one per quartile of the 1000-step schedule
SCALES = (0.02, 0.032, 0.05)                      # rot6d / metre perturbation sizes of the three samples
MIN_GAP = 1e-3


def trainer():
    refshim.install()

    def to_4x4(aa):
        m = torch.zeros(aa.shape[0], 4, 4, dtype=aa.dtype)
        m[:, :3, :3] = lo.aa2matrot(aa)
        m[:, 3, 3] = 1
        return m
    shim = types.SimpleNamespace(angle_axis_to_rotation_matrix=to_4x4)
    sys.modules['human_body_prior.tools'].tgm_conversion = shim
    if 'tools' in sys.modules:
        sys.modules['tools'].tgm = shim
    pl = sys.modules['pytorch_lightning']
    pl.profiler = types.ModuleType('pytorch_lightning.profiler')
    pl.profiler.SimpleProfiler = pl.profiler.AdvancedProfiler = None
    sys.modules['pytorch_lightning.profiler'] = pl.profiler
    sys.modules.pop('train_diffusion_smpl', None)          # refshim parks a placeholder there for eval_smpl_short.py
    tds = importlib.import_module('train_diffusion_smpl')
    tds.device = torch.device('cpu')
    return tds


def inputs():
    bt = {k: (torch.from_numpy(v) if isinstance(v, np.ndarray) else v) for k, v in syn.make_clip_batch(seed=SEED, B=B, T=T, past_len=PAST, n_points=8).items()}
    rs = np.random.RandomState(SEED + 1)
    eps = fx._randn(rs, B, 1, 144, T)
    # sample k of clip b: gt + SCALES[perm] x N(0,1); the permutation differs between the body channels (0..134) and the object channels
    samples = torch.empty(K, B, 1, 144, T)
    for b in range(B):
        pb, po = np.roll(np.arange(K), b), np.roll(np.arange(K), b + 2)
        for k in range(K):
            z = fx._randn(rs, 144, T)
            z[:135] *= SCALES[pb[k]]
            z[135:] *= SCALES[po[k]]
            samples[k, b, 0] = bt['gt'][b, 0] + z
    return bt, eps, samples


def main():
    tds = trainer()
    gd, diff = mgs_diffusion()
    net = mg.ref_mdm()
    bt, eps, samples = inputs()
    gt, cond, hands = bt['gt'], bt['cond'], bt['hand_pose']
    t = torch.tensor(TS, dtype=torch.int64)
    w = lo.WEIGHTS
    args = Namespace(smpl_dim=132, past_len=PAST, future_len=T - PAST, diverse_samples=K, render_epoch=10 ** 9, debug=False, **w)
    out = dict(x0=np_(gt), cond=np_(cond), hand_pose=np_(hands), t=np_(t), eps=np_(eps), samples=np_(samples), past_len=np.int64(PAST),
               weights=np.asarray([w[k] for k in sorted(w)]), weight_names=np.asarray(sorted(w)))

    # ---- forward_backward (teacher-forced objective) --------------------------------------------------------------------
    seen, logged = {}, []

    class Watch(torch.nn.Module):
        def forward(self, x, ts, y=None):
            seen['x_t'], seen['ts'] = x.clone(), ts.clone()
            seen['out'] = net(x, ts, y=y)
            return seen['out']
    lit = Namespace(args=args, diffusion=diff, ddp_model=Watch(), model=None, current_epoch=0,
                    schedule_sampler=Namespace(sample=lambda n, device: (t, torch.ones(n))))
    lit.l2 = lambda a, b: tds.LitInteraction.l2(lit, a, b)
    lit.log = lambda key, value, prog_bar=False: logged.append((key, float(value)))

    def log_loss_dict(diffusion, ts, losses, loss):
        seen['weighted'] = {k: v.clone() for k, v in losses.items()}
        return tds.LitInteraction.log_loss_dict(lit, diffusion, ts, losses, loss)
    lit.log_loss_dict = log_loss_dict
    real = gd.th.randn_like
    gd.th.randn_like = lambda x: eps.clone()
    try:
        loss = tds.LitInteraction.forward_backward(lit, gt, {'y': {'cond': cond}})[0]
    finally:
        gd.th.randn_like = real
    assert list(seen['weighted']) == list(lo.LOSS_KEYS) and torch.equal(seen['ts'], t)
    quart = {}
    for key, v in logged:
        if '_q' in key:
            quart.setdefault(key, []).append(v)
    out.update(fb_x_t=np_(seen['x_t']), fb_out=np_(seen['out']), fb_weighted=np_(torch.stack([seen['weighted'][k] for k in lo.LOSS_KEYS])),
               fb_loss=np_(loss), fb_keys=np.asarray(list(seen['weighted'])), fb_quartile_keys=np.asarray(sorted(quart)),
               fb_quartile_values=np.asarray([np.mean(quart[k]) for k in sorted(quart)]))
    assert sorted({int(k[-1]) for k in quart}) == [0, 1, 2, 3]

    # ---- q_sample + inpainting of x_t (training_losses with the mask keys) -----------------------------------------------
    mask = torch.ones_like(gt, dtype=torch.bool)
    mask[..., PAST:] = False
    motion = gt + 1.0
    diff.training_losses(Watch(), gt, t, model_kwargs={'y': {'cond': cond, 'inpainting_mask': mask, 'inpainted_motion': motion}}, noise=eps.clone())
    assert torch.equal(diff.q_sample(gt, t, noise=eps.clone()), torch.from_numpy(out['fb_x_t']))
    out.update(qs_x_t=np_(seen['x_t']))                     # (inpainted_motion = x0 + 1, mask = the past frames: rebuilt by the tests)

    # ---- validation_step / test_step scoring: the reference's own _common_step with the sampler returning the recorded samples ------
    gt_tbn = gt.squeeze(1).permute(2, 0, 1).contiguous()
    pose = torch.cat([torch.zeros(T, B, 66), hands], dim=2)
    batch = dict(frames=[dict(smplfit_params=dict(pose=pose[i])) for i in range(T)])
    queue = []
    lit.model = Namespace(_get_embeddings=lambda b: (cond, gt_tbn))
    lit.diffusion = Namespace(p_sample_loop=lambda model, shape, clip_denoised, model_kwargs: queue.pop(0).clone())
    inter = {}

    def spy(name):
        fn = getattr(tds.LitInteraction, name)

        def run(body_pred, body_gt, obj_pred, obj_gt, batch):
            inter[name] = (body_pred, body_gt, obj_pred, obj_gt)
            return fn(lit, body_pred, body_gt, obj_pred, obj_gt, batch=batch)
        return run
    lit.calc_val_loss, lit.calc_loss = spy('calc_val_loss'), spy('calc_loss')
    queue[:] = [samples[0]]
    vloss, vd, vw = tds.LitInteraction._common_step(lit, batch, 1, 'valid')
    queue[:] = list(samples)
    tloss, td, tw = tds.LitInteraction._common_step(lit, batch, 1, 'test')
    assert list(vd) == list(lo.LOSS_KEYS) and list(td) == list(lo.LOSS_KEYS) + [k + '_min' for k in lo.LOSS_KEYS]
    stack = lambda d, keys: np_(torch.stack([d[k] for k in keys]))
    out.update(val_terms=stack(vd, vd), val_weighted=stack(vw, vw), val_loss=np_(vloss), val_keys=np.asarray(list(vd)),
               test_terms=stack(td, td), test_weighted=stack(tw, tw), test_loss=np_(tloss), test_keys=np.asarray(list(td)))

    # ---- the reference's own per-(sample, clip) means, from the tensors it handed calc_loss: tie check + the on-purpose case ----------
    bp, bg, op, og = inter['calc_loss']
    mat = lambda v, n: tds.rotvec_to_rotmat(v).view(*v.shape[:-1], n)
    X = [mat(bp[..., :-3], 52 * 9), bp[..., -3:], mat(op[..., :-3], 9), op[..., -3:]]
    G = [mat(bg[..., :-3], 52 * 9)[None], bg[None, ..., -3:], mat(og[..., :-3], 9)[None], og[None, ..., -3:]]
    per = torch.zeros(K, 16, B)
    P = PAST
    for gi, (x, g) in enumerate(zip(X, G)):
        mse = lambda a, b_: ((a - b_) ** 2).mean(dim=[1, 3])
        per[:, gi] = mse(x[:, :P], g[:, :P])
        per[:, 4 + gi] = mse(x[:, 1:P + 1] - x[:, :P], g[:, 1:P + 1] - g[:, :P])
        per[:, 8 + gi] = mse(x[:, P:], g[:, P:])
        per[:, 12 + gi] = mse(x[:, P + 1:] - x[:, P:-1], g[:, P + 1:] - g[:, P:-1])
    for i, key in enumerate(lo.LOSS_KEYS):
        assert abs(float(per[:, i].min(dim=0)[0].mean()) - float(td[key + '_min'])) <= 1e-6 * abs(float(td[key + '_min'])), key
    srt = per.sort(dim=0)[0]
    gaps = ((srt[1:] - srt[:-1]) / srt[1:]).min()
    # body_rot_* of the past frames carries the hand joints, which are the same in every sample: its gaps are the smallest
    print('smallest relative gap between two samples of one clip and term: %.3e' % float(gaps))
    assert float(gaps) > MIN_GAP, 'two samples tie within %g: change the seed or SCALES, not the gate' % MIN_GAP
    best = per.argmin(dim=0)
    assert int(best[10, 0]) != int(best[8, 0]), 'clip 0: the best sample of obj_rot_future and body_rot_future must differ'
    out.update(test_per_clip=np_(per), min_gap=np.float64(gaps))
    print('forward_backward loss %.6f, val_loss %.6f, test loss %.6f' % (float(loss), float(vloss), float(tloss)))
    mgs.save('losses.npz', **out)


def mgs_diffusion():
    import make_golden_skeleton_mdm as mgsm
    return mgsm.diffusion(1000)


if __name__ == '__main__':
    main()
