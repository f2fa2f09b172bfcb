"""Seeded input builders shared by tests/golden/make_golden.py (which feeds them to
the reference) and by the tests (which feed the SAME inputs to the oracle and to
the HIP path).  numpy RandomState streams only, so every machine sees the same
numbers.  Torch CPU tensors out."""
import os
import functools
import numpy as np
import torch
from interdiff_amd import synthetic as syn

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
PAST = 10


def golden(name):
    return np.load(os.path.join(GOLDEN, name))


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _randn(rs, *shape):
    return _t(rs.standard_normal(shape).astype(np.float32))


@functools.lru_cache(None)
def mdm_weights():
    return {k: _t(v) for k, v in syn.mdm_state_dict(seed=233).items()}


WC_GAIN = 0.05                        # gain of the two output heads of the well-conditioned denoiser (tests/golden/fullwc.npz)


@functools.lru_cache(None)
def mdm_weights_wc():
    """The synthetic denoiser of mdm_weights() with WELL-CONDITIONED output heads (round 5, tests/golden/fullwc.npz): bodyFinalLinear /
    objFinalLinear keep their random directions at WC_GAIN of their size, and their biases are a VALID pose -- per joint the rot6d of a
    seeded rotation of ~0.3 rad (1 rad for the object), a body translation, the object 0.3 m beside it.  x0 predictions are then a
    valid rot6d + O(0.03), so the Gram-Schmidt step of rot6d -> matrix is far from its singular set (two nearly parallel 3-vectors),
    which a random-init head is not: there the reference's OWN fp32 run is 1e-3 from the fp64 answer on the body rotations and no
    fp32 implementation can be held to 1e-4.  Everything in front of the heads (embedding, the 8 layers) is unchanged."""
    sd = {k: v.clone() for k, v in mdm_weights().items()}
    rs = np.random.RandomState(2330)
    body_aa, obj_aa = 0.3 * rs.standard_normal((22, 3)), 1.0 * rs.standard_normal((1, 3))
    body_tr = 0.1 * rs.standard_normal(3)
    off = rs.standard_normal(3)
    obj_tr = body_tr + 0.3 * off / np.linalg.norm(off)
    sd['bodyFinalLinear.weight'] *= WC_GAIN
    sd['objFinalLinear.weight'] *= WC_GAIN
    sd['bodyFinalLinear.bias'] = _t(np.concatenate([syn.matrix_to_6d(syn.aa_to_matrix(body_aa)).reshape(132), body_tr]).astype(np.float32))
    sd['objFinalLinear.bias'] = _t(np.concatenate([syn.matrix_to_6d(syn.aa_to_matrix(obj_aa)).reshape(6), obj_tr]).astype(np.float32))
    return sd


def sharpen_attention(sd, gain, self_layers=None, cross_layers=None, encoder_gain=None):
    """A copy of a denoiser state_dict (the SMPL one or the skeleton one) whose attention LOGITS are ``gain`` ** 2 times as large: the Q and K rows ([:512]) of
    ``in_proj_weight`` / ``in_proj_bias`` of the decoder's standard self-attention (``self_layers``) and of its cross-attention (``cross_layers``) are multiplied
    by ``gain``; None = every layer that has one, () = none.  ``encoder_gain`` does the same to the encoder's standard layers.  A default initialisation gives logits
    of standard deviation ~0.6 and nearly uniform softmax rows; 2 is the scale of a trained checkpoint (rows led by one or two keys), 4 saturates them.
    The QaN layers have no such rows (their queries are normalised per head)."""
    out = {k: torch.as_tensor(v).clone() for k, v in sd.items()}

    def scale(prefix, g):
        out[prefix + 'in_proj_weight'][:512] *= g
        out[prefix + 'in_proj_bias'][:512] *= g
    for k in list(out):
        side, _, rest = k.partition('.layers.')
        if not rest.endswith('attn.in_proj_weight'):
            continue
        layer, kind = int(rest.split('.')[0]), rest.split('.')[1]
        prefix = k[:-len('in_proj_weight')]
        if side == 'encoder':
            if encoder_gain is not None and kind == 'self_attn':
                scale(prefix, encoder_gain)
        elif kind == 'self_attn':
            if self_layers is None or layer in self_layers:
                scale(prefix, gain)
        elif cross_layers is None or layer in cross_layers:
            scale(prefix, gain)
    return out


@functools.lru_cache(None)
def mdm_weights_sharp(gain, self_layers=None, cross_layers=None, encoder_gain=None):
    """``mdm_weights()`` at the attention logit scale of a trained checkpoint (``sharpen_attention``; layer lists as tuples).  Nothing is recorded from the
    reference for these weights: the oracle run in float64 is the ground truth (tests/test_attention_scales.py)."""
    return sharpen_attention(mdm_weights(), gain, self_layers, cross_layers, encoder_gain)


@functools.lru_cache(None)
def smpl_model():
    return {k: _t(v) for k, v in syn.smplh_model(seed=7).items()}


@functools.lru_cache(None)
def objproj_weights():
    z = golden('correction_ckpt.npz')
    return {k: _t(z[k]) for k in z.files}


def vertex_subset():
    from oracle.correction import MARKERS67
    return sorted(set(range(0, 6890, 13)) | set(MARKERS67))


def mdm_inputs(B, T):
    rs = np.random.RandomState(1000 + 37 * B + T)
    ts = _t(rs.randint(0, 1000, size=B).astype(np.int64))
    ts[0] = 999
    return _randn(rs, B, 1, 144, T), ts, _randn(rs, PAST, B, 256)


def smpl_inputs(N):
    rs = np.random.RandomState(2000 + N)
    pose = 0.4 * _randn(rs, N, 156)
    pose[0] = 0.0                       # exercises the +1e-8 Rodrigues quirk at zero rotation
    if N > 1:
        pose[1, :3] = _t(np.array([3.0, 0.6, -0.4], dtype=np.float32))   # root angle near pi (BEHAVE-like)
    return pose, _randn(rs, N, 10), _randn(rs, N, 3)


def p2p_inputs(N=3, P1=700, P2=300):
    rs = np.random.RandomState(3000)
    x, y = 0.5 * _randn(rs, N, P1, 3), 0.5 * _randn(rs, N, P2, 3)
    y[0, 5] = x[0, 17]                  # zero distance
    x[1, 40] = x[1, 3]                  # exact tie -> lowest index must win
    xn = _randn(rs, N, P1, 3)
    return x, y, xn / xn.norm(dim=-1, keepdim=True)


def objproj_inputs(T, B):
    rs = np.random.RandomState(4000 + T)
    contact = torch.zeros(B, 67, dtype=torch.int64)
    contact[1, 20], contact[1, 10], contact[1, 30] = 3, 3, 3     # hand marker 10 wins via +0.5
    if B > 2:
        contact[2, 5] = 2
    return _randn(rs, T, B, 6), _randn(rs, T, B, 3), _randn(rs, T, B, 67, 3), contact


def _clip(seed, B, T, P):
    bt = syn.make_clip_batch(seed=seed, B=B, T=T, past_len=PAST, n_points=P)
    return {k: (_t(v) if isinstance(v, np.ndarray) else v) for k, v in bt.items()}


def model_kwargs_y(bt, T):
    """The tensor entries of model_kwargs['y'] (eval_smpl_short.py:138-150); the caller adds
    'smpl' and 'obj_model' in its own representation."""
    pad = list(range(PAST)) + [PAST - 1] * (T - PAST)
    mask = torch.ones_like(bt['gt'], dtype=torch.bool)
    mask[..., PAST:] = False
    return dict(cond=bt['cond'], inpainted_motion=bt['gt'], inpainting_mask=mask,
                hand_pose=bt['hand_pose'][pad], beta=bt['beta'], obj_points=bt['obj_points'])


DFN_SHAPE = (14, 3, 256)               # T, B, P
DFN_TS = (500, 250, 0, 499, 550)


def denoised_fn_inputs():
    T, B, P = DFN_SHAPE
    bt = _clip(5, B, T, P)
    rs = np.random.RandomState(5000)
    x = bt['gt'] + 0.05 * _randn(rs, *bt['gt'].shape)
    x[0, 0, 141:144, :] += 3.0          # clip 0: object far away -> no contact
    return x, model_kwargs_y(bt, T)


LOOP_SHAPE = (12, 2, 64)               # T, B, P : tiny clip, full 1000 steps
LOOP_DUMPS = [0, 498, 499, 549, 899, 999]


class NoiseStream:
    """Sequential N(0,1) draws; draw k is what the reference's k-th randn_like returned."""

    def __init__(self, seed):
        self.rs = np.random.RandomState(seed)

    def next_like(self, x):
        return _randn(self.rs, *x.shape)


def loop_inputs():
    T, B, P = LOOP_SHAPE
    bt = _clip(11, B, T, P)
    return bt['noise'], model_kwargs_y(bt, T), NoiseStream(6000)


EVAL_SHAPE = (14, 2, 128)              # T, B, P : eval glue (sample_once_proj / get_gt / metrics), 50-step schedule
EVAL_STEPS = 50


def eval_inputs():
    """Clip batch in the tensor schema of interdiff_amd/eval.py + the injected noise."""
    T, B, P = EVAL_SHAPE
    bt = _clip(21, B, T, P)
    batch = dict(gt=bt['gt'], cond=bt['cond'], hand_pose=bt['hand_pose'], beta=bt['beta'], obj_points=bt['obj_points'])
    return batch, bt['noise'], NoiseStream(7000)


FULL_SHAPE = (100, 16, 2048)          # T, B, P : BASELINE config #2 itself (eval_smpl_short.py, correction mode), full 1000 steps
FULL_STEPS = 1000
FULL_DUMPS = [0, 499, 500, 549, 749, 949, 999]      # loop indices (it): 499 = the first corrected step (t = 500), 999 = the sample


FULLWC_DUMPS = [0, 499, 500, 949, 999]              # dumps of the well-conditioned twin fixture (tests/golden/fullwc.npz, fullwc64.npz)


def full_inputs():
    """Clip batch + x_T + per-step noise stream of the full-size end-to-end golden (tests/golden/full.npz)."""
    T, B, P = FULL_SHAPE
    bt = _clip(31, B, T, P)
    batch = dict(gt=bt['gt'], cond=bt['cond'], hand_pose=bt['hand_pose'], beta=bt['beta'], obj_points=bt['obj_points'])
    return batch, bt['noise'], NoiseStream(8000)


CORR32_SHAPE = (100, 32, 2048)        # T, B, P : one corrected step at BASELINE config #3's size (tests/golden/corr32.npz)
CORR32_T = 250


def corr32_inputs():
    T, B, P = CORR32_SHAPE
    bt = _clip(132, B, T, P)
    rs = np.random.RandomState(5032)
    x = bt['gt'] + 0.05 * _randn(rs, *bt['gt'].shape)
    x[0, 0, 141:144, :] += 3.0          # clip 0: object far away -> no contact, condition still true
    return x, model_kwargs_y(bt, T)


PARITY_LOG = os.path.join(os.path.dirname(GOLDEN), '..', 'gpurun_out', 'parity_r06.json')


def record_parity(name, **values):
    """Measured errors of the chain / end-to-end parity tests -> gpurun_out/parity_r06.json (merged back from the GPU box; the
    copy that is judged lives in profiles/).  Never fails a test."""
    import json
    try:
        path = os.path.abspath(PARITY_LOG)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        data = json.load(open(path)) if os.path.exists(path) else {}
        data[name] = {k: (float(v) if isinstance(v, (int, float, np.floating, np.integer)) else v) for k, v in values.items()}      # (nested dicts of floats pass through)
        json.dump(data, open(path, 'w'), indent=1, sort_keys=True)
    except Exception as e:                                        # pragma: no cover
        print('record_parity(%s): %r' % (name, e))


EMB_SHAPE = (35, 3, 2048)              # T, B, P : MDM._get_embeddings (encoder side, "next" row N1)


def embedding_inputs():
    T, B, P = EMB_SHAPE
    return {k: _t(v) for k, v in syn.make_embedding_inputs(seed=77, B=B, T=T, n_points=P).items()}


OPT_SHAPE = (12, 96)                   # T, P : physics post-optimisation ("next" row N4), one clip
OPT_ITERS = (151, 152, 153, 154)       # iteration numbers ii the golden run executes (ratio = ii/350, saving starts after 150)


def optim_inputs(seed=9000, T=None, P=None):
    """One clip in optimization.py's schema: pose [T,156] axis-angle, trans, obj_angles, obj_trans [T,3], betas [T,10],
    obj_points [P,3].  Slow motion (some foot frames are 'static'), a few hand joints exactly at the identity, the object
    overlapping the body so that the collision term and both contact-radius cases are exercised."""
    T = T or OPT_SHAPE[0]
    P = P or OPT_SHAPE[1]
    rs = np.random.RandomState(seed)
    pose = 0.3 * rs.standard_normal((1, 156)) + np.cumsum(0.004 * rs.standard_normal((T, 156)), axis=0)
    pose[:, 66 + 9:66 + 18] = 0.0                                   # three hand joints at exactly zero rotation
    pose[:, :3] = np.array([2.9, 0.5, -0.3]) + np.cumsum(0.004 * rs.standard_normal((T, 3)), axis=0)   # root angle near pi (BEHAVE-like)
    trans = 0.1 * rs.standard_normal((1, 3)) + np.cumsum(0.002 * rs.standard_normal((T, 3)), axis=0)
    obj_angles = rs.standard_normal((1, 3)) + np.cumsum(0.02 * rs.standard_normal((T, 3)), axis=0)
    obj_trans = trans + np.array([0.25, 0.1, -0.2]) + np.cumsum(0.004 * rs.standard_normal((T, 3)), axis=0)
    betas = np.repeat(rs.standard_normal((1, 10)), T, axis=0)
    obj_points = rs.uniform(-0.25, 0.25, (P, 3))
    return tuple(_t(np.float32(a)) for a in (pose, trans, obj_angles, obj_trans, betas, obj_points))


TIMED_T, TIMED_P = 100, 2048          # the shape bench.py times (BASELINE configs #2 / #3): B = 16 / 32 clips of T = 100, P = 2048
TIMED_FIRST_T, TIMED_STEPS = 560, 120  # a window that crosses the corrected steps t = 500 and t = 450


def timed_inputs(B, T=None):
    """Clip batch + x_{first_t} of the timed-route parity tests (no golden: the routes are compared with each other and the oracle)."""
    T = TIMED_T if T is None else T
    bt = _clip(300 + B + (0 if T == TIMED_T else 1000 * T), B, T, TIMED_P)
    return bt, model_kwargs_y(bt, T)


LONG4_SHAPE = (100, 8, 2048, 2, 50)    # T, B, P, K windows, schedule steps: BASELINE config #4's per-GPU share (8 of 64 clips), tests/golden/long4.npz


def long4_inputs():
    """Raw (dataset-side) clips of the config #4 golden + the injected noise: x_T(k) [B,1,144,T] and the per-step stream of window k."""
    T, B, P, K, steps = LONG4_SHAPE
    ei = {k: _t(v) for k, v in syn.make_embedding_inputs(seed=404, B=B, T=T, n_points=P).items()}
    g = torch.Generator().manual_seed(405)
    raw = dict(ei, hand_pose=0.1 * torch.randn(T, B, 90, generator=g), beta=torch.randn(1, B, 10, generator=g).expand(T, B, 10).contiguous())
    x_T = lambda k: torch.from_numpy(np.random.RandomState(9400 + k).standard_normal((B, 1, 144, T)).astype(np.float32))

    def step_noise(k):
        rs = np.random.RandomState(9500 + k)
        return lambda i, x: torch.from_numpy(rs.standard_normal(tuple(x.shape)).astype(np.float32))
    return raw, x_T, step_noise


LONG_FUTURE, LONG_WINDOWS = 4, 2       # tests/golden/long.npz: eval_smpl_long.get_batch on two windows of one clip


def long_inputs(w):
    """The last PAST predicted frames of a window as eval_smpl_long.py:276 hands them to get_batch, one clip: body [PAST,1,159]
    (66 axis-angle | 90 hands | 3 trans), obj [PAST,1,6], pelvis [PAST,1,3], verts [PAST,1,6890,3].  Window 1 has a root angle > pi."""
    rs = np.random.RandomState(9100 + w)
    body, obj = _randn(rs, PAST, 1, 159), _randn(rs, PAST, 1, 6)
    pel, verts = _randn(rs, PAST, 1, 3), _randn(rs, PAST, 1, 6890, 3)
    if w == 1:
        body[0, 0, :3] = _t(np.array([4.0, 0.3, -0.2], dtype=np.float32))
        obj[3, 0, :3] = _t(np.array([-3.5, 1.0, 0.4], dtype=np.float32))
    return body, obj, pel, verts
