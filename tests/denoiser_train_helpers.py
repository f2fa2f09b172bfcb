"""What the denoiser trainers' test modules share (test_mdm_train, test_mdm_encoder_train, test_skeleton_mdm_train, test_pointnet2_finetune): conversions,
the relative-error measure, the gradient gate, the check of a module's C entries, and the far-parameter count of the trajectory tests.  Each module keeps its own
tests, fixtures, points and figures."""
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


def far_parameters(got, theta, names, y):
    """(how many entries of the tensors ``names`` of ``got`` lie further than 8 y from the fp64 trajectory ``theta``, the largest distance)."""
    far, worst = 0, 0.0
    for k in names:
        dist = (got[k].cpu().double() - theta[k]).abs()
        far += int((dist > 8 * y).sum())
        worst = max(worst, float(dist.max()))
    return far, worst
