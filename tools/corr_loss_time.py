"""hip-event timing of the correction-checkpoint scoring (interdiff_amd/correction_losses.py, csrc/corr_losses.hip); not on the
product path.

    python tools/corr_loss_time.py [--reps 20] [--json PATH]

At B = 16 and B = 32 (the reference's default batch), T = 35, V = 6890, P = 2048, warmed medians in microseconds of
  (a) ``calc_loss_contact`` on ``interdiff_correction_losses``, and
  (b) the same scoring composed from the entries the library had before: the rotation entry, elementwise posing,
      ``interdiff_point2point_signed`` with ``return_vector=True``, torch masks and means for the two geometry terms
      (tests/corr_fixtures.py ``composed``), eight ``mse_loss`` calls, the ten weights and the sum,
plus the forward (``initialize`` False / True) and the whole ``validation_step``.  The device launches of one call of (a) and of (b)
are counted with the torch profiler, and the kernels' registers / LDS / scratch are read from a device-only compile of
csrc/corr_losses.hip (``--no-resources`` skips that)."""
import argparse
import re
import subprocess
import json
import os
import sys
import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)
from interdiff_amd import correction_losses as cl, transforms           # noqa: E402
from interdiff_amd.objprojector import ObjProjector                     # noqa: E402
from tests import corr_fixtures as cf, fixtures as fx                   # noqa: E402

DEV = 'cuda'


def median_us(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return float(np.median(out))


def composed_loss(pred, gt, pts, hv, vec, past=cf.PAST):
    """(b): calc_loss_contact line by line on the library's earlier entries + torch."""
    mse = torch.nn.functional.mse_loss
    pen, con, _ = cf.composed(pred, gt, pts, hv)
    terms = [pen, con]
    for v in (0, 1):
        for lo, hi in ((0, past), (past, pred.shape[0])):
            for c in (slice(0, 6), slice(6, 9)):
                x, g = pred[..., c], gt[..., c]
                if not v:
                    terms.append(mse(x[lo:hi], g[lo:hi]))
                elif lo == 0:
                    terms.append(mse(x[1:past + 1] - x[:past], g[1:past + 1] - g[:past]))
                else:
                    terms.append(mse(x[past:] - x[past - 1:-1], g[past:] - g[past - 1:-1]))
    return (torch.stack(terms) * vec).sum()


def launches(fn):
    """Device activity of one call from the torch profiler: {kernels, copies, names}; None where the profiler is not available."""
    try:
        from torch.profiler import profile, ProfilerActivity
        from torch.autograd import DeviceType
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        dev = [e.name for e in prof.events() if e.device_type == DeviceType.CUDA]
        copies = [n for n in dev if 'memcpy' in n.lower() or 'copybuffer' in n.lower()]
        return dict(kernels=len(dev) - len(copies), copies=len(copies), names=sorted(set(dev)))
    except Exception as e:                                            # pragma: no cover
        print('launch count unavailable: %r' % e)
        return None


def kernel_resources():
    """{kernel: vgprs, sgprs, lds_bytes, scratch_bytes} of csrc/corr_losses.hip from the compiler's metadata (gfx950, the product's flags)."""
    from interdiff_amd.csrc import build
    src = os.path.join(ROOT, 'interdiff_amd', 'csrc', 'corr_losses.hip')
    try:
        asm = subprocess.run([build.HIPCC] + build.FLAGS + ['--cuda-device-only', '-S', '-o', '-', src], capture_output=True, text=True, check=True).stdout
    except Exception as e:                                            # pragma: no cover
        print('kernel resources unavailable: %r' % e)
        return None
    out = {}
    for blk in asm.split('- .agpr_count')[1:]:
        get = lambda k: int(re.search(r'\.%s:\s+(\d+)' % k, blk).group(1))
        name = re.search(r'\.name:\s+(\S+)', blk).group(1)
        short = 'corr_geometry_kernel' if 'corr_geometry' in name else 'corr_finish_kernel' if 'corr_finish' in name else name
        out[short] = dict(vgprs=get('vgpr_count'), sgprs=get('sgpr_count'), lds_bytes=get('group_segment_fixed_size'),
                          scratch_bytes=get('private_segment_fixed_size'), vgpr_spills=get('vgpr_spill_count'))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--json', default=None)
    ap.add_argument('--no-resources', action='store_true')
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    T, V, P = 35, 6890, 2048
    op = ObjProjector(fx.objproj_weights(), T=T, past_len=cf.PAST, device=DEV)
    res = {}
    for B in (16, 32):
        sc = {k: torch.from_numpy(v).to(DEV) for k, v in cf.scene(9900 + B, T, B, V, P).items()}
        batch = dict(obj_angle=sc['obj_angle'], obj_trans=sc['obj_trans'], markers=sc['markers'], human_verts=sc['human_verts'], obj_points=sc['obj_points'])
        gt = torch.cat([transforms.matrix_to_rotation_6d(transforms.axis_angle_to_matrix(sc['obj_angle'])), sc['obj_trans']], dim=2)
        pred = gt + 0.01 * torch.randn(gt.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
        tag = 'B%d_T%d' % (B, T)
        vec = torch.tensor(cl.CorrectionLossWeights().vector(20), device=DEV)
        fused = lambda: cl.calc_loss_contact(pred, gt, batch, cf.PAST, current_epoch=20)
        comp = lambda: composed_loss(pred, gt, sc['obj_points'], sc['human_verts'], vec)
        la, lb = float(fused()[0]), float(comp())
        print('%s: loss fused %.7f composed %.7f' % (tag, la, lb))
        res['loss_fused_%s' % tag], res['loss_composed_%s' % tag] = la, lb
        res['fused_%s_us' % tag] = median_us(fused, a.reps)
        res['composed_%s_us' % tag] = median_us(comp, max(3, a.reps // 4), warm=2)
        res['fused_terms_only_%s_us' % tag] = median_us(lambda: cl.correction_terms(pred, gt, sc['obj_points'], sc['human_verts'], cf.PAST), a.reps)
        if B == 16:
            res['launches_fused'], res['launches_composed'] = launches(fused), launches(comp)
        res['mse_only_%s_us' % tag] = median_us(lambda: cl.correction_terms(pred, gt, past_len=cf.PAST), a.reps)
        res['forward_%s_us' % tag] = median_us(lambda: op.forward(batch, False), a.reps)
        res['forward_initialize_%s_us' % tag] = median_us(lambda: op.forward(batch, True), a.reps)
        res['validation_step_%s_us' % tag] = median_us(lambda: cl.validation_step(op, batch, current_epoch=20), a.reps)
    for k, v in res.items():
        print('%-44s %s' % (k, '%10.1f' % v if isinstance(v, float) else v))
    if not a.no_resources:
        res['kernel_resources'] = kernel_resources()
        print(res['kernel_resources'])
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(res, open(a.json, 'w'), indent=1, sort_keys=True)


if __name__ == '__main__':
    main()
