"""Record tests/golden/skel_dataset.npz: the REFERENCE's own skeleton-dataset functions on six small synthetic videos.  Run in the build container only:

    python tests/golden/make_golden_skeleton_dataset.py

data/dataset_skeleton.py cannot be imported (``os`` is used before it is imported, a YAML of local paths is opened at import), so -- the precedent is
make_golden.py gen_long -- the source text between ``def recover_init_obj`` and ``def get_datasets`` (recover_init_obj, get_consistent_poses, pose_init_to_seq,
check_sequences, get_sequences) is ``exec``ed as it stands, with ONE replacement: the two lines that open and unpickle ``pathName`` become ``dataList = pathName``,
so that the in-memory list goes where the file's content went.  Nothing is re-typed and nothing of it is stored.

Stored per video v (data only): ``v_pose`` [F,7] and ``v_contact`` [F,1] at full rate, ``v_skeleton`` / ``v_obj`` at the frames 0, 12, 24, ... ONLY (the reference
reads no other frame of them; the recorder and the tests expand them with NaN everywhere else, so that a reader of another frame shows in its own output),
``v_name``; the reference's answers: ``v_sign`` int8 [F] (get_consistent_poses' output against its input), ``v_pose_rows`` (its output at the sampled frames),
``v_zero_pose_obj``, ``v_discrepancy`` (:98-99), ``v_valid_discard`` (check_sequences(discard_discrep=True) kept the video), ``v_starts`` / ``v_starts_unseen`` (the
first frame of every window it returned without / with ``unseen``).  Every returned window is asserted to be rows of the stored arrays, so the tests rebuild the
windows from them.  ``split_<n>_{train,valid,test}``: the index lists of :202-203's ``random_split`` for n = 10 and 57.

The videos (F = 240, 241, 252, 253, 805, 300): no window / one / one / two / 48 / five.  CHUNK = 256 is the scan chunk of csrc/skeleton_clip_batch.hip: the 805-frame
video spans three chunks and a remainder.  Raw quaternions = a smooth unit track times a sign pattern with flips at 0->1, on both sides of every chunk
boundary, in runs, as exact antipodal repeats and exact repeats, and at random (30 %) elsewhere; |q_i . q_{i+1}| >= 1e-3 everywhere (asserted), so the reference's
norm comparison and the sign of the dot product cannot disagree.
"""
import os
import sys
import warnings
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, '..', '..'))
warnings.filterwarnings('ignore')
import refshim                                    # noqa: E402

CHUNK, STRIDE, WINDOW = 256, 12, 240
VIDEOS = (('sub1_chair1_000', 240, 'ones', False), ('sub1_chair3_001', 241, 'ones', False), ('sub2_table_002', 252, 'zeros', False),
          ('sub2_chair4_003', 253, 'ones', True), ('sub3_chair3_004', 805, 'late', False), ('sub3_box_005', 300, 'ones', False))
SPLIT_N = (10, 57)


def reference_functions():
    import pickle
    from scipy.spatial.transform import Rotation as Rot
    src = open(os.path.join(refshim.REF, 'data', 'dataset_skeleton.py')).read()
    src = src[src.index('def recover_init_obj'):src.index('def get_datasets')]
    read = "    with open(pathName, 'rb') as f:\n        dataList = pickle.load(f)[0]\n"
    assert src.count(read) == 1
    ns = dict(np=np, Rot=Rot, pickle=pickle, counter=0)
    exec(src.replace(read, '    dataList = pathName\n', 1), ns)
    return ns


def make_video(seed, F, contact_kind, perturbed):
    """-> dict(skeleton [F,21,3], contact [F,1], pose [F,7], obj [F,12,3]) float64, and the sign pattern its raw quaternions carry."""
    from scipy.spatial.transform import Rotation as Rot
    rs = np.random.RandomState(seed)
    q = np.zeros((F, 4))
    q[0] = rs.standard_normal(4)
    q[0] /= np.linalg.norm(q[0])
    repeat = np.zeros(F, bool)                                  # frames whose smooth quaternion repeats the one before exactly
    for i in (5, 6, 40, 41, 100, 130, 131):
        if i < F:
            repeat[i] = True
    for i in range(1, F):
        if repeat[i]:
            q[i] = q[i - 1]
        else:
            q[i] = q[i - 1] + 0.02 * rs.standard_normal(4)
            q[i] /= np.linalg.norm(q[i])
    flip = rs.uniform(size=F - 1) < 0.3                        # flip[i]: the raw sign changes between frame i and i + 1
    flip[0] = True
    for b in range(CHUNK, F, CHUNK):                            # transitions b - 2 .. b + 1: both sides of the boundary between chunk b / CHUNK - 1 and the next
        flip[b - 2:min(b + 2, F - 1)] = True
    flip[20:27] = True                                          # a run
    flip[60:63] = False                                         # and a run of none
    flip[4], flip[5] = True, False                              # frame 5 = -frame 4 exactly (antipodal repeat), frame 6 = frame 5 exactly (repeat)
    flip[39], flip[40] = True, True                             # antipodal repeats twice in a row
    sign = np.concatenate([[1.0], np.where(np.cumsum(flip) % 2 == 1, -1.0, 1.0)])
    raw = q * sign[:, None]
    trans = 0.3 * rs.standard_normal((1, 3)) + np.cumsum(0.004 * rs.standard_normal((F, 3)), axis=0)
    zero = 0.3 * rs.standard_normal((12, 3))
    obj = np.einsum('fij,kj->fki', Rot.from_quat(raw).as_matrix(), zero) + trans[:, None]
    if perturbed:
        obj[1:] += 0.1 * rs.standard_normal((F - 1, 12, 3))
    skeleton = 0.4 * rs.standard_normal((1, 21, 3)) + np.cumsum(0.004 * rs.standard_normal((F, 21, 3)), axis=0)
    contact = np.ones((F, 1))
    if contact_kind == 'zeros':
        contact[:] = 0.0
    elif contact_kind == 'late':
        contact[:400] = 0.0                                     # windows that end before frame 400 have no contact
    return dict(skeleton=skeleton, contact=contact, pose=np.concatenate([trans, raw], axis=1), obj=obj)


def with_nan(a, F):
    """Rows at the frames 0, 12, ... -> the full-rate array, NaN in every other frame."""
    out = np.full((F,) + a.shape[1:], np.nan)
    out[::STRIDE] = a
    return out


def main():
    ref = reference_functions()
    out = {}
    for v, (name, F, contact_kind, perturbed) in enumerate(VIDEOS):
        vid = make_video(9100 + v, F, contact_kind, perturbed)
        pose, contact = vid['pose'], vid['contact']
        skel, obj = with_nan(vid['skeleton'][::STRIDE], F), with_nan(vid['obj'][::STRIDE], F)
        data = [skel, contact, pose, obj]                                          # pickle.load(f)[0]
        d = np.einsum('ij,ij->i', pose[:-1, 3:], pose[1:, 3:])
        assert np.abs(d).min() >= 1e-3, np.abs(d).min()
        cons = ref['get_consistent_poses'](pose)
        sign = np.where((cons[:, 3:] == pose[:, 3:]).all(1), 1, -1).astype(np.int8)
        assert np.array_equal(cons[:, 3:], sign[:, None] * pose[:, 3:]) and np.array_equal(cons[:, :3], pose[:, :3])
        parity = np.concatenate([[0], np.cumsum(d < 0) % 2])
        assert np.array_equal(sign, np.where(parity == 1, -1, 1)), 'the reference sign is the prefix parity of the raw dots'
        assert (sign == -1).any() and (sign == 1).any()
        ok, zero = ref['check_sequences'](pose, obj, False)
        assert ok
        pred = ref['pose_init_to_seq'](zero, pose[::STRIDE])
        disc = float(np.linalg.norm(pred - obj[::STRIDE], axis=-1, ord=2).mean())   # the expression of :99
        assert disc >= 5e-2 if perturbed else disc < 1e-3 * 1e-2, disc
        starts = {}
        for unseen in (False, True):
            wins = ref['get_sequences'](data, False, unseen, name, name.split('_')[1])
            st = []
            for w in wins:
                s = int(np.nonzero((pose[:, :3] == w[2][0, :3]).all(1))[0][0])     # translations are distinct: the window's first frame
                st.append(s)
                rows = slice(s, s + WINDOW, STRIDE)
                assert s % STRIDE == 0 and np.array_equal(w[0], skel[rows]) and np.array_equal(w[1], obj[rows]) and np.array_equal(w[2], cons[rows])
                assert np.array_equal(w[3], zero) and w[4] == name and w[5] == name.split('_')[1] and w[0].shape == (20, 21, 3) and not np.isnan(w[0]).any()
            starts[unseen] = np.asarray(st, np.int64)
        valid = bool(ref['check_sequences'](pose, obj, True)[0])                  # what get_sequences(discard_discrep=True) goes by
        assert (len(ref['get_sequences'](data, True, False, name, name.split('_')[1])) > 0) == (valid and len(starts[False]) > 0)
        k = 'v%d_' % v
        out.update({k + 'name': np.array(name), k + 'pose': pose, k + 'contact': contact, k + 'skeleton': skel[::STRIDE], k + 'obj': obj[::STRIDE],
                    k + 'sign': sign, k + 'pose_rows': cons[::STRIDE], k + 'zero_pose_obj': zero, k + 'discrepancy': np.float64(disc),
                    k + 'valid_discard': np.bool_(valid), k + 'starts': starts[False], k + 'starts_unseen': starts[True]})
        print('%-18s F %4d  windows %2d  unseen %2d  discrepancy %.3e  kept under discard_discrep %s  flips %d'
              % (name, F, len(starts[False]), len(starts[True]), disc, valid, int((d < 0).sum())))
    from torch.utils.data import random_split
    for n in SPLIT_N:
        parts = random_split(list(range(n)), [int(0.7 * n), int(0.2 * n), n - int(0.2 * n) - int(0.7 * n)], generator=torch.Generator().manual_seed(42))
        for tag, p in zip(('train', 'valid', 'test'), parts):
            out['split_%d_%s' % (n, tag)] = np.asarray(p.indices, np.int64)
    out['n_videos'] = np.int64(len(VIDEOS))
    path = os.path.join(HERE, 'skel_dataset.npz')
    np.savez_compressed(path, **out)
    print('skel_dataset.npz %.1f KB' % (os.path.getsize(path) / 1024))


if __name__ == '__main__':
    main()
