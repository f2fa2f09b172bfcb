"""interdiff_amd/skeleton_dataset.py and the skeleton loops of interdiff_amd/fit.py against the reference's OWN data/dataset_skeleton.py functions, recorded by
tests/golden/make_golden_skeleton_dataset.py into tests/golden/skel_dataset.npz (six synthetic videos; what each is for is said there).

Host: the window rule worked by hand; the ``unseen`` / ``discard_discrep`` / ``min_windows`` filters against the recorded window starts; ``split_seen`` against the
recorded ``random_split``; the pickle loader; the C entries; the per-video code on its host instance (``interdiff_debug_skeleton_video_prepare``): signs equal on
every frame, table rows bit-equal to float32(sign * reference), zero_pose_obj within the ETL gate of tests/test_dataset.py (1e-6 max(1, |ref|max)), the discrepancy
within 1e-12 max(1, ref) (two float64 evaluations of the same ~250-term mean in different orders: ~250 * 2.2e-16 = 6e-14 of the value); ``fit`` and
``skeleton_evaluate`` on fake pieces.  GPU: the device prepare against the host instance bit for bit; ``assemble`` at B = 1, 3, 4 (one window twice) and 70 against the reference's windows bit
for bit; the call contract; the three skeleton trainers; ``fit``; ``skeleton_evaluate``.

The kernels at their edges, on seeded synthetic videos (``synth_video``; references: a sequential numpy loop of get_consistent_poses' rule, scipy ``Rotation``, numpy):
flips on the wave seam (63 | 64) and the chunk seam (255 | 256) of the sign scan, in runs, F = 1 and 2, stride 1 and 7, P = 1 and 64; degenerate transitions (a zero
quaternion, a NaN quaternion, an exactly orthogonal pair), after which the reference leaves the next frame as stored -- host instance on the CPU, device on the GPU,
all videos of a geometry in one launch; the window kernel at W odd (no padding column), T = 1 and 128, a 65,224 B tile, B = 1 and 65.

The skeleton / object arrays are NaN in every frame that is no multiple of 12 -- the reference reads none of them -- so a kernel that does shows in its own output.
Without the feature every test below fails: the module, the loops and the entries do not exist.
"""
import functools
import os
import pickle
import numpy as np
import pytest
import torch
from scipy.spatial.transform import Rotation
from tests import fixtures as fx
from tests.test_dataset import gate

DEV = 'cuda'
STRIDE, WINDOW, T = 12, 240, 20
NEW_SYMBOLS = {
    'interdiff_skeleton_video_prepare': 'const double *skel, const double *obj, const double *pose, const double *contact, const int64_t *seq_off, '
                                        'const int64_t *row_off, int32_t n_video, int32_t J, int32_t P, int32_t stride, float *table, float *zero_pose_obj, '
                                        'double *report, double *row_contact, int8_t *signs, void *stream',
    'interdiff_debug_skeleton_video_prepare': 'const double *skel, const double *obj, const double *pose, const double *contact, int64_t F, int32_t J, int32_t P, '
                                              'int32_t stride, float *table, float *zero_pose_obj, double *report, double *row_contact, int8_t *signs',
    'interdiff_skeleton_window_batch': 'const idf_skel_clip_set *cs, const int32_t *clips, int32_t B, int32_t T, const idf_skel_window_batch *out, void *stream',
}


def sd_mod():
    from interdiff_amd import skeleton_dataset
    return skeleton_dataset


@functools.lru_cache(maxsize=None)
def recorded():
    """(the fixture as a dict, the videos as ``load_skeleton_video`` gives them -- skeleton / obj NaN off the sampled frames).  Computed once, never modified."""
    z = fx.golden('skel_dataset.npz')
    z = {k: z[k] for k in z.files}
    videos = []
    for v in range(int(z['n_videos'])):
        k = 'v%d_' % v
        F = z[k + 'pose'].shape[0]
        full = {}
        for name in ('skeleton', 'obj'):
            a = np.full((F,) + z[k + name].shape[1:], np.nan)
            a[::STRIDE] = z[k + name]
            full[name] = a
        name = str(z[k + 'name'])
        videos.append(dict(skeleton=full['skeleton'], obj=full['obj'], pose=z[k + 'pose'], contact=z[k + 'contact'], filename=name, obj_name=name.split('_')[1]))
    return z, videos


@functools.lru_cache(maxsize=None)
def host_prepared():
    return [sd_mod().prepare_host(v) for v in recorded()[1]]


def reference_table(z, v):
    """float32 of the reference's down-sampled frames of video v: body | object | get_consistent_poses' pose -> [rows,106]."""
    k = 'v%d_' % v
    rows = z[k + 'skeleton'].shape[0]
    return np.concatenate([z[k + 'skeleton'].reshape(rows, -1), z[k + 'obj'].reshape(rows, -1), z[k + 'pose_rows']], axis=1).astype(np.float32)


def reference_windows(z, clips):
    """The reference's windows [(video, first frame)] as its DataLoader collates them, cast as every consumer casts them (``.float()``) ->
    (body [B,T,21,3], obj [B,T,12,3], pose [B,T,7], zero_pose_obj [B,12,3]) torch fp32."""
    rows = [reference_table(z, v)[s // STRIDE:s // STRIDE + T] for v, s in clips]
    tab = torch.from_numpy(np.stack(rows))
    zpo = torch.from_numpy(np.stack([z['v%d_zero_pose_obj' % v] for v, _ in clips])).float()
    B = len(clips)
    return tab[..., :63].reshape(B, T, 21, 3).contiguous(), tab[..., 63:99].reshape(B, T, 12, 3).contiguous(), tab[..., 99:].contiguous(), zpo


def fake_reports(frame_counts, contact=1.0):
    VR = sd_mod().VideoReport
    return [VR(0.0, 0.0, contact * F, np.full(-(-F // STRIDE), contact)) for F in frame_counts]


# ------------------------------------------------------------------------------------------------------------------------ host
def test_window_rule_worked_by_hand():
    """start + 240 < F, strictly: F = 240 none, 241 and 252 one, 253 two, 700 -> starts 0 .. 456 = 39."""
    m = sd_mod()
    counts = [240, 241, 252, 253, 700]
    idx = m.SkeletonWindowIndex(counts, fake_reports(counts), min_windows=1)
    per = {k: [r for kk, r, _ in idx.entries if kk == k] for k in range(5)}
    assert per[0] == [] and per[1] == [0] and per[2] == [0] and per[3] == [0, 1] and per[4] == list(range(39))
    assert all(b == 1 for _, _, b in idx.entries) and idx.T == T and len(idx) == 43 and idx[1] == (2, 0, 1) and idx.videos == [1, 2, 3, 4]
    for k, row, _ in idx.entries:
        assert row * STRIDE + WINDOW < counts[k] and (row + T - 1) * STRIDE < counts[k]
    assert m.SkeletonWindowIndex([100], fake_reports([100]), min_windows=1).entries == []
    two = m.SkeletonWindowIndex(counts, fake_reports(counts))                      # get_datasets: len(sample_sequences) > 1
    assert two.videos == [3, 4] and len(two) == 41
    wide = m.SkeletonWindowIndex([300], fake_reports([300]), hop=24, min_windows=1)  # rows of a hop of 24 frames: 0, 2, 4
    assert wide.entries == [(0, 0, 1), (0, 2, 1), (0, 4, 1)]
    from interdiff_amd.dataset import draw_starts
    assert draw_starts(two.entries, np.random.RandomState(0)) == [(k, r) for k, r, _ in two.entries]
    sub = two.subset([40, 0])
    assert sub.entries == [two.entries[40], two.entries[0]] and len(sub) == 2 and sub.T == T
    for bad in (dict(hop=18), dict(window=250), dict(stride=0), dict(hop=0)):
        with pytest.raises(ValueError):
            m.SkeletonWindowIndex(counts, fake_reports(counts), **bad)
    with pytest.raises(ValueError):
        m.SkeletonWindowIndex(counts, fake_reports(counts[:2]))


@pytest.mark.parametrize('unseen', [False, True])
@pytest.mark.parametrize('discard', [False, True])
@pytest.mark.parametrize('min_windows', [1, 2])
def test_filters_match_the_recorded_window_starts(unseen, discard, min_windows):
    m = sd_mod()
    z, videos = recorded()
    reports = [p['report'] for p in host_prepared()]
    idx = m.SkeletonWindowIndex([len(v['pose']) for v in videos], reports, unseen=unseen, discard_discrep=discard, min_windows=min_windows)
    want, kept = [], []
    for v in range(len(videos)):
        starts = z['v%d_starts%s' % (v, '_unseen' if unseen else '')]
        if discard and not bool(z['v%d_valid_discard' % v]):
            starts = starts[:0]
        if len(starts) >= min_windows:
            want += [(v, int(s) // STRIDE, 1) for s in starts]
            kept.append(v)
    assert idx.entries == want and idx.videos == kept
    if not unseen and not discard and min_windows == 1:
        assert [len(z['v%d_starts' % v]) for v in range(6)] == [0, 1, 1, 2, 48, 5] and len(z['v4_starts_unseen']) == 33 and len(z['v2_starts_unseen']) == 0


def test_split_seen_equals_the_recorded_random_split():
    m = sd_mod()
    z, _ = recorded()
    for n in (10, 57):
        tr, va, te = m.split_seen(n)
        assert tr == z['split_%d_train' % n].tolist() and va == z['split_%d_valid' % n].tolist() and te == z['split_%d_test' % n].tolist()
        assert sorted(tr + va + te) == list(range(n)) and len(tr) == int(0.7 * n) and len(va) == int(0.2 * n)
    assert m.split_seen(10, seed=1) != m.split_seen(10)
    assert m.is_unseen('chair3') and m.is_unseen('chair4') and not m.is_unseen('chair1') and not m.is_unseen('table')


def test_loader_round_trip(tmp_path):
    m = sd_mod()
    _, videos = recorded()
    for v in (videos[1], videos[3]):
        d = tmp_path / ('dir_' + v['filename'])
        d.mkdir()
        frames = [[a.reshape(len(a), -1).tolist() for a in (v['skeleton'], v['contact'], v['pose'], v['obj'])], 'something else']
        with open(str(d / (v['filename'] + '.pkl')), 'wb') as f:
            pickle.dump(frames, f)
    (tmp_path / 'empty_dir').mkdir()
    (tmp_path / 'ds_seen.pkl').write_bytes(b'')
    files = m.parse_motion_dir(str(tmp_path))
    assert [(n, o) for _, n, o in files] == [('sub1_chair3_001', 'chair3'), ('sub2_chair4_003', 'chair4')]
    for (path, name, obj_name), v in zip(files, (videos[1], videos[3])):
        got = m.load_skeleton_video(path)
        assert got['filename'] == name and got['obj_name'] == obj_name
        for k in ('skeleton', 'contact', 'pose', 'obj'):
            assert got[k].dtype == np.float64 and got[k].shape == v[k].shape and np.array_equal(got[k], v[k], equal_nan=True), k
    bad = tmp_path / 'bad_dir'
    bad.mkdir()
    with open(str(bad / 'sub9_box_009.pkl'), 'wb') as f:
        pickle.dump([[np.zeros((5, 60)).tolist(), np.zeros((5, 1)).tolist(), np.zeros((5, 7)).tolist(), np.zeros((5, 36)).tolist()]], f)
    with pytest.raises(ValueError):
        m.load_skeleton_video(str(bad / 'sub9_box_009.pkl'))
    (bad / 'second.pkl').write_bytes(b'')
    with pytest.raises(ValueError):
        m.parse_motion_dir(str(tmp_path))


def test_skeleton_set_entries_are_declared_typed_and_exported():
    from tests.denoiser_train_helpers import check_new_symbols
    check_new_symbols(NEW_SYMBOLS)


def test_host_prepare_instance_matches_the_reference():
    """Printed before asserted: per video the number of negated frames, the zero-pose error, the discrepancy and its distance from the reference's."""
    z, videos = recorded()
    for v, (video, p) in enumerate(zip(videos, host_prepared())):
        k = 'v%d_' % v
        F = len(video['pose'])
        ref_disc, disc = float(z[k + 'discrepancy']), p['report'].discrepancy
        e_z = float(np.abs(p['zero_pose_obj'].astype(np.float64) - z[k + 'zero_pose_obj']).max())
        print('video %d (F %d): %d negated frames, zero_pose_obj err %.2e, discrepancy %.6e (reference %.6e, diff %.2e), check sum %.2e'
              % (v, F, int((p['signs'] < 0).sum()), e_z, disc, ref_disc, abs(disc - ref_disc), p['report'].quat_check))
        assert p['signs'].shape == (F,) and np.array_equal(p['signs'], z[k + 'sign'])
        ref = reference_table(z, v)
        assert p['table'].dtype == np.float32 and p['table'].shape == ref.shape == (-(-F // STRIDE), 106)
        assert np.array_equal(p['table'].view(np.uint32), ref.view(np.uint32))                   # bit for bit, -0.0 included; no NaN: nothing off the sampled frames was read
        assert np.array_equal(p['table'][:, 102:], np.float32(z[k + 'sign'][::STRIDE, None] * z[k + 'pose'][::STRIDE, 3:]))
        gate(p['zero_pose_obj'], z[k + 'zero_pose_obj'])
        assert abs(disc - ref_disc) <= 1e-12 * max(1.0, ref_disc)
        assert p['report'].contact_sum == float(z[k + 'contact'].sum()) and np.array_equal(p['report'].row_contact, z[k + 'contact'][::STRIDE, 0])
        assert abs(p['report'].quat_check) < 1e-4
        assert abs(p['report'].quat_check - float((np.linalg.norm(z[k + 'pose'][::STRIDE, 3:], axis=-1) - 1).sum())) < 1e-13
    assert host_prepared()[3]['report'].discrepancy >= 5e-2 and all(host_prepared()[v]['report'].discrepancy < 1e-3 for v in (0, 1, 2, 4, 5))


# ------------------------------------------------------------------------------------------------------------------------ synthetic adversarial videos
# (F, J, P, stride, flips): transition i = frames i | i + 1.  Flips sit on the wave seam (63 | 64), the chunk seam (255 | 256), in runs, at the ends; F = 1 and 2;
# stride 1 and a stride that does not divide 256; P = 1 and P = 64 (the LDS limit of the kernel's double zero pose).
GEOMETRIES = ((21, 12, 12), (1, 1, 1), (3, 64, 7))
A1_CASES = (
    (1, 21, 12, 12, ()), (2, 21, 12, 12, (0,)), (13, 21, 12, 12, (11,)), (64, 21, 12, 12, (62,)), (65, 21, 12, 12, (62, 63)), (66, 21, 12, 12, (63, 64)),
    (256, 21, 12, 12, (254,)), (257, 21, 12, 12, (254, 255)), (258, 21, 12, 12, (255, 256)), (513, 21, 12, 12, (0, 63, 64, 127, 128, 255, 256, 257, 511)),
    (700, 21, 12, 12, tuple(range(699))), (700, 21, 12, 12, tuple(range(0, 699, 2))), (300, 1, 1, 1, (5, 6, 7, 255)), (300, 3, 64, 7, (100, 255, 256)),
    (523, 21, 12, 12, (191, 192, 319, 383, 447, 448, 511, 512, 521)))
# On top of the fifteen: ONE flip early on, so that an odd parity is carried across every chunk seam (and wave seam) after it.  In the fifteen the flips before
# a chunk seam are mostly even in number, and a scan that dropped the carry between chunks would pass all of them but F = 258 and F = 523.
CARRY_CASES = ((700, 21, 12, 12, (3,)), (300, 1, 1, 1, (10,)), (300, 3, 64, 7, (10,)))
# A2: (F, J, P, stride, flips, degenerate frames {frame: kind}).  'zero' / 'nan' replace ONE frame's quaternion (both its transitions are degenerate) and sit off
# the sampled frames; 'ortho' replaces frames f and f + 1 by two different basis quaternions (d_f == 0 exactly; valid unit quaternions, so also on sampled frames).
# Every degenerate frame follows an odd number of flips since the last reset, which is where the reference's rule and a pure parity part.
A2_CASES = (
    (400, 21, 12, 12, (5, 100), {64: 'zero', 256: 'nan'}),
    (300, 21, 12, 12, (3, 70, 200), {63: 'ortho', 131: 'ortho', 255: 'ortho'}),           # frame 132 = row 11 is the second of an orthogonal pair
    (300, 1, 1, 1, (3, 70, 200), {63: 'ortho', 131: 'ortho', 255: 'ortho'}),
    (300, 3, 64, 7, (9, 80, 150), {64: 'zero', 100: 'ortho', 256: 'nan'}))
SIX_FRAMES = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, -1, 0, 0], [0, 0, 0, 1], [np.nan] * 4, [0, 0, 0, -1]], np.float64)


def synth_video(F, J, P, stride, flips, seed, degenerate=None, quats=None):
    """A slowly drifting unit-quaternion track, continuous (every consecutive dot product > 0), then negated from frame i + 1 on for every i of ``flips`` -- the
    stored data needs exactly those flips undone -- then the degenerate frames.  obj = t + R(q) z for a seeded z; skeleton and the 0/1 contact column random.
    Skeleton and obj are NaN off the sampled frames, as in ``recorded``.  ``quats``: the stored quaternions given outright.  -> (video dict, sign the flips imply)"""
    rs = np.random.RandomState(seed)
    q, cur = np.empty((F, 4)), rs.standard_normal(4)
    for i in range(F):
        cur = cur + 0.02 * rs.standard_normal(4)
        cur = cur / np.linalg.norm(cur)
        q[i] = cur if i == 0 or cur @ q[i - 1] > 0 else -cur
    for f, kind in sorted((degenerate or {}).items()):
        if kind == 'ortho':                                                        # the two largest components of the track there, signs kept: the neighbours' dots stay large
            a, b = np.argsort(-np.abs(q[f]))[:2]
            q[f], q[f + 1] = np.eye(4)[a] * np.sign(q[f, a]), np.eye(4)[b] * np.sign(q[f, b])
    implied = np.ones(F)
    for i in flips:
        implied[i + 1:] *= -1
    q = q * implied[:, None]
    for f, kind in (degenerate or {}).items():
        if kind != 'ortho':
            assert f % stride, 'a zero or NaN quaternion on a sampled frame has no rotation'
            q[f] = 0.0 if kind == 'zero' else np.nan
    if quats is not None:
        q = np.array(quats, np.float64)
    t = np.cumsum(0.01 * rs.standard_normal((F, 3)), axis=0) + rs.uniform(-1, 1, 3)
    z = rs.standard_normal((P, 3))
    obj, skel = np.full((F, P, 3), np.nan), np.full((F, J, 3), np.nan)
    obj[::stride] = t[::stride, None] + np.einsum('fij,pj->fpi', Rotation.from_quat(q[::stride]).as_matrix(), z)
    skel[::stride] = rs.standard_normal((len(skel[::stride]), J, 3))
    video = dict(skeleton=skel, obj=obj, pose=np.concatenate([t, q], axis=1), contact=rs.randint(0, 2, (F, 1)).astype(np.float64), filename='sub%d_box_%03d' % (seed, F),
                 obj_name='box')
    return video, implied


def reference_signs(quat):
    """get_consistent_poses' rule, one frame after the other on float64 norms: frame i + 1 is negated iff the corrected frame i is farther from it than from its
    negative; in every other case (a tie, a NaN) it is left as stored."""
    sign = np.ones(len(quat), np.int8)
    for i in range(len(quat) - 1):
        prev = sign[i] * quat[i]
        if np.linalg.norm(prev - quat[i + 1]) > np.linalg.norm(prev + quat[i + 1]):
            sign[i + 1] = -1
    return sign


def synth_reference(video, stride):
    """Signs by the loop above, the table as float32 of the strided sign-corrected rows, zero_pose_obj and the discrepancy through scipy ``Rotation`` on float64,
    check sum and contact sums by numpy."""
    pose, obj = video['pose'], video['obj']
    sign = reference_signs(pose[:, 3:])
    rows = pose[::stride].copy()
    rows[:, 3:] *= sign[::stride, None]
    n = len(rows)
    table = np.concatenate([video['skeleton'][::stride].reshape(n, -1), obj[::stride].reshape(n, -1), rows], axis=1).astype(np.float32)
    zpo = Rotation.from_quat(pose[0, 3:]).inv().apply(obj[0] - pose[0, :3])
    pred = pose[::stride, None, :3] + np.stack([Rotation.from_quat(qq).apply(zpo) for qq in pose[::stride, 3:]])
    return dict(signs=sign, table=table, zero_pose_obj=zpo, discrepancy=float(np.linalg.norm(pred - obj[::stride], axis=-1).mean()),
                quat_check=float((np.linalg.norm(pose[::stride, 3:], axis=-1) - 1).sum()), contact_sum=float(video['contact'].sum()), row_contact=video['contact'][::stride, 0])


@functools.lru_cache(maxsize=None)
def synthetic_videos():
    """Every A1 and A2 video with its geometry, its references and what the host instance makes of it: [dict(name, geom, video, implied, degenerate, ref, host)].
    Computed once, never modified."""
    cases = [('A1.%d' % k, c[:4], c[4], None, None) for k, c in enumerate(A1_CASES)] + [('A2.%d' % k, c[:4], c[4], c[5], None) for k, c in enumerate(A2_CASES)]
    cases += [('carry.%d' % k, c[:4], c[4], None, None) for k, c in enumerate(CARRY_CASES)]
    cases.append(('A2.six', (6, 21, 12, 12), (), None, SIX_FRAMES))
    out = []
    for k, (name, (F, J, P, stride), flips, degenerate, quats) in enumerate(cases):
        video, implied = synth_video(F, J, P, stride, flips, 500 + k, degenerate, quats)
        host = sd_mod().prepare_host(video, stride=stride, n_joints=J, n_points=P)
        out.append(dict(name=name, geom=(J, P, stride), video=video, implied=implied, degenerate=bool(degenerate) or quats is not None, ref=synth_reference(video, stride),
                        host=host))
    return out


def check_transitions(item):
    """What the tests assert about their own inputs: a transition is either far from a tie (|d| >= 1e-3, where the dot-sign form and the norm comparison must
    agree) or EXACTLY degenerate (d == 0 or NaN).  -> the number of degenerate transitions"""
    q = item['video']['pose'][:, 3:]
    d = (q[:-1] * q[1:]).sum(1)
    exact = np.isnan(d) | (d == 0.0)
    assert (np.abs(d[~exact]) >= 1e-3).all(), (item['name'], np.abs(d[~exact]).min())
    assert bool(exact.any()) == item['degenerate'], item['name']
    if not item['degenerate']:
        assert np.array_equal(item['ref']['signs'], item['implied']), item['name']      # the generator's flips are what the reference's rule undoes
    return int(exact.sum())


def check_prepared(item, got, what):
    """The A1 assertions on one video: ``got`` = dict(table, zero_pose_obj, report, signs) of the host instance or of the device.  Printed before asserted."""
    ref, (J, P, stride) = item['ref'], item['geom']
    F = len(item['video']['pose'])
    rep = got['report']
    e_z = float(np.abs(got['zero_pose_obj'].astype(np.float64) - ref['zero_pose_obj']).max())
    e_d, e_c = abs(rep.discrepancy - ref['discrepancy']), abs(rep.quat_check - ref['quat_check'])
    print('%s %s (F %d, J %d, P %d, stride %d): %d negated frames, %d signs differ, zero_pose_obj err %.2e (gate %.1e), discrepancy diff %.2e (gate %.1e), check sum diff %.2e'
          % (what, item['name'], F, J, P, stride, int((got['signs'] < 0).sum()), int((got['signs'] != ref['signs']).sum()), e_z,
             1e-6 * max(1.0, float(np.abs(ref['zero_pose_obj']).max())), e_d, 1e-12 * max(1.0, ref['discrepancy']), e_c))
    assert got['signs'].shape == (F,) and np.array_equal(got['signs'], ref['signs']), item['name']
    assert got['table'].dtype == np.float32 and got['table'].shape == ref['table'].shape == (-(-F // stride), 3 * (J + P) + 7)
    assert np.array_equal(got['table'].view(np.uint32), ref['table'].view(np.uint32)), item['name']
    gate(got['zero_pose_obj'], ref['zero_pose_obj'])
    assert e_d <= 1e-12 * max(1.0, ref['discrepancy']) and e_c < 1e-13, item['name']
    assert rep.contact_sum == ref['contact_sum'] and np.array_equal(rep.row_contact, ref['row_contact']), item['name']


def test_host_prepare_on_adversarial_videos_matches_the_references():
    """A1: the fifteen (F, J, P, stride, flips) cases -- flips on the wave seam, on the chunk seam, in runs, F = 1 and 2, stride 1 and 7, P = 1 and 64 -- on the host
    instance against the sequential sign loop, scipy and numpy.  None has a degenerate transition."""
    items = [it for it in synthetic_videos() if it['name'].startswith('A1')]
    assert len(items) == 15 and [len(it['video']['pose']) for it in items] == [c[0] for c in A1_CASES]
    for it in items:
        assert check_transitions(it) == 0
        check_prepared(it, it['host'], 'host')
    assert int((items[10]['ref']['signs'] < 0).sum()) == 350 and int((items[11]['ref']['signs'] < 0).sum()) == 350      # every / every second transition
    for it in [it for it in synthetic_videos() if it['name'].startswith('carry')]:
        assert check_transitions(it) == 0 and it['ref']['signs'][256] == -1 and it['ref']['signs'][-1] == -1
        check_prepared(it, it['host'], 'host')


def test_host_prepare_follows_the_reference_on_degenerate_transitions():
    """A2: after a tie or a NaN the reference leaves the next frame as stored (+1), whatever the sign before; a pure prefix parity carries a -1 over.  The six
    quoted frames, and longer videos with a zero quaternion, a NaN quaternion and exactly orthogonal basis pairs after an odd number of flips -- one degenerate
    transition at 63 | 64 and one at 255 | 256 in each, an orthogonal pair on a sampled row, stride 1 included.  Fails with the pure-parity recurrence."""
    items = [it for it in synthetic_videos() if it['name'].startswith('A2')]
    assert len(items) == 5
    six = items[-1]
    assert six['ref']['signs'].tolist() == [1, 1, -1, 1, 1, 1]
    for it in items:
        n = check_transitions(it)
        q = it['video']['pose'][:, 3:]
        d = (q[:-1] * q[1:]).sum(1)
        exact = np.nonzero(np.isnan(d) | (d == 0.0))[0]
        parity = np.concatenate([[1], np.where(np.cumsum(np.nan_to_num(d) < 0) % 2, -1, 1)])          # what carrying the sign over a tie would give
        print('%s: %d degenerate transitions at %s; the reference and a pure parity differ on %d frames' % (it['name'], n, exact.tolist(), int((parity != it['ref']['signs']).sum())))
        assert (parity != it['ref']['signs']).any()                                                   # the case does tell the two rules apart
        entered = [int(it['ref']['signs'][i]) for i in exact[np.r_[True, np.diff(exact) > 1]]]        # the reference's sign on entering each degenerate stretch
        assert -1 in entered and (it is six or set(entered) == {-1}), (it['name'], entered)
        if it is not six:
            assert 63 in exact and 255 in exact
        check_prepared(it, it['host'], 'host')


class FakeSet:
    """``assemble`` records what it was asked for."""

    def __init__(self):
        self.calls = []

    def assemble(self, ids, starts, body=None):
        self.calls.append((list(ids), list(starts)))
        return (torch.zeros(len(ids), T, 21, 3),)


class FakeTrainer:
    def training_step(self, batch):
        return 0.0

    def state_dict(self):
        return {}


def test_fit_drives_a_window_index():
    """7 entries at batch size 3: two training batches per epoch (the last partial one dropped), no entry twice in an epoch; validation in index order, 3 + 3 + 1."""
    from interdiff_amd import fit as F
    m = sd_mod()
    idx = m.SkeletonWindowIndex([253, 300], fake_reports([253, 300]))
    assert len(idx) == 7
    train, val = FakeSet(), FakeSet()
    seen = []

    def validate(trainer, batches):
        seen.append([b[0].shape[0] for b in batches])
        return 1.0
    out = F.fit(FakeTrainer(), train, idx, batch_size=3, max_epochs=2, seed=4, validate=validate, val_index=idx, val_set=val, check_val_every_n_epoch=1)
    assert out['steps'] == 4 and out['epochs'] == 2 and len(train.calls) == 4 and seen == [[3, 3, 1], [3, 3, 1]]
    for e in range(2):
        drawn = [c for ids, starts in train.calls[2 * e:2 * e + 2] for c in zip(ids, starts)]
        assert len(drawn) == 6 and len(set(drawn)) == 6 and set(drawn) <= {(k, r) for k, r, _ in idx.entries}
    assert train.calls[:2] != train.calls[2:]                                        # a new permutation every epoch
    flat = [c for ids, starts in val.calls[:3] for c in zip(ids, starts)]
    assert flat == [(k, r) for k, r, _ in idx.entries] and val.calls[:3] == val.calls[3:]


def test_skeleton_evaluate_divides_by_the_index_length(monkeypatch):
    """5 windows at batch size 2 -> batches of 2, 2, 1 in index order; a metric that is the batch's B gives (4 + 4 + 1) / 5, not / 4 and not the mean of the batches."""
    from interdiff_amd import fit as F, skeleton as sk
    m = sd_mod()
    idx = m.SkeletonWindowIndex([300], fake_reports([300]), min_windows=1)
    assert len(idx) == 5
    fake = FakeSet()
    monkeypatch.setattr(sk, 'sample_once_proj', lambda batch, model, diffusion, obj_model=None, **kw: (batch[0].shape[0],) * 6)
    monkeypatch.setattr(sk, 'skeleton_metrics', lambda bp, bg, op, og, pp, pg: dict(mpjpe_h=float(bp), mpjpe_o=1.0, translation_error=2.0 * bp, rotation_error=0.0))
    out = F.skeleton_evaluate(None, None, None, fake, idx, 2, seed=1)
    assert fake.calls == [([0, 0], [0, 1]), ([0, 0], [2, 3]), ([0], [4])]
    assert out == dict(mpjpe_h=9.0 / 5, mpjpe_o=1.0, translation_error=18.0 / 5, rotation_error=0.0)
    with pytest.raises(ValueError):
        F.skeleton_evaluate(None, None, None, fake, idx.subset([]), 2)


# ------------------------------------------------------------------------------------------------------------------------ GPU
@functools.lru_cache(maxsize=None)
def device_set():
    return sd_mod().SkeletonClipSet(recorded()[1], device=DEV)


@pytest.mark.gpu
def test_device_prepare_gives_the_host_instance_bits():
    cs = device_set()
    z, videos = recorded()
    table, zpo = cs.t['table'].cpu().numpy(), cs.t['zero_pose_obj'].cpu().numpy()
    assert cs.frame_counts == [240, 241, 252, 253, 805, 300] and cs.T == T and len(cs) == 6
    assert cs.filename == [v['filename'] for v in videos] and cs.obj_name == ['chair1', 'chair3', 'table', 'chair4', 'chair3', 'box']
    assert not np.isnan(table).any() and table.shape == (int(cs.row_off[-1]), 106)
    for v, p in enumerate(host_prepared()):
        rep = cs.reports[v]
        print('video %d: device report (%.17g, %.17g, %.17g); host (%.17g, %.17g, %.17g)' % (v, rep.discrepancy, rep.quat_check, rep.contact_sum, p['report'].discrepancy,
                                                                                              p['report'].quat_check, p['report'].contact_sum))
        assert np.array_equal(table[cs.row_off[v]:cs.row_off[v + 1]].view(np.uint32), p['table'].view(np.uint32)), v
        assert np.array_equal(zpo[v].view(np.uint32), p['zero_pose_obj'].view(np.uint32)), v
        assert (rep.discrepancy, rep.quat_check, rep.contact_sum) == (p['report'].discrepancy, p['report'].quat_check, p['report'].contact_sum), v
        assert np.array_equal(rep.row_contact, p['report'].row_contact)
    idx = cs.index(unseen=True, min_windows=1)
    assert len(idx) == sum(len(z['v%d_starts_unseen' % v]) for v in range(6))
    bad = dict(videos[5], pose=videos[5]['pose'] * np.array([1, 1, 1, 1.01, 1.01, 1.01, 1.01]))          # |q| = 1.01 on 25 rows: check sum 0.25
    with pytest.raises(ValueError, match='not unit'):
        sd_mod().SkeletonClipSet([videos[1], bad], device=DEV)


def batch_clips(B):
    """[(video, first frame)]: B = 1 the last window of the long video; B = 3 windows of three videos, one repeated... B = 70 every window the fixture has, and more."""
    z, _ = recorded()
    every = [(v, int(s)) for v in range(6) for s in z['v%d_starts' % v]]
    if B == 1:
        return [every[-6]]
    if B == 3:
        return [(3, 12), (4, 300), (1, 0)]
    return (every + every[::-1])[:B]


@pytest.mark.gpu
@pytest.mark.parametrize('B', [1, 3, 4, 70])
def test_assemble_matches_the_reference_windows_bit_for_bit(B):
    from interdiff_amd.skeleton_mdm_train import tokens_of
    cs = device_set()
    z, _ = recorded()
    clips = batch_clips(B) if B != 4 else [(3, 12), (4, 300), (1, 0), (4, 300)]               # three different videos, one window twice
    bt = cs.assemble([v for v, _ in clips], [s // STRIDE for _, s in clips])
    ref = reference_windows(z, clips)
    assert isinstance(bt, tuple) and len(bt) == 6 and bt[4] == [cs.filename[v] for v, _ in clips] and bt[5] == [cs.obj_name[v] for v, _ in clips]
    for name, got, want in zip(('body', 'obj', 'pose'), bt[:3], ref[:3]):
        assert got.dtype == torch.float32 and got.is_contiguous() and tuple(got.shape) == tuple(want.shape), name
        assert torch.equal(got.cpu().view(torch.int32), want.view(torch.int32)), name
    gate(bt[3].cpu().numpy(), ref[3].numpy())
    gt, zz = tokens_of(tuple(t.cpu() for t in bt[:4]), 'cpu')
    assert tuple(bt.gt.shape) == (len(clips), 1, 106, T) and bt.gt.is_contiguous() and torch.equal(bt.gt.cpu().view(torch.int32), gt.view(torch.int32))
    assert torch.equal(bt.gt.cpu(), tokens_of(ref, 'cpu')[0])
    d = bt.as_dict()
    assert sorted(d) == ['gt', 'zero_pose_obj'] and d['gt'] is bt.gt and d['zero_pose_obj'] is bt[3] and torch.equal(zz, bt[3].cpu())
    again = cs.assemble([v for v, _ in clips], [s // STRIDE for _, s in clips], body=True)
    assert all(torch.equal(a, b) for a, b in zip(bt[:4], again[:4])) and torch.equal(bt.gt, again.gt)
    assert not any(bool(torch.isnan(t).any()) for t in (*bt[:4], bt.gt))


@pytest.mark.gpu
def test_assemble_contract():
    m = sd_mod()
    cs = device_set()
    _, videos = recorded()
    rows = cs.rows
    assert rows == [20, 21, 21, 22, 68, 25]
    cs.assemble([0], [0])                                                          # 20 rows hold one window of rows (the index, not the set, applies start + 240 < F)
    for ids, starts in (([0], [1]), ([4], [49]), ([4], [-1]), ([6], [0]), ([-1], [0]), ([1, 2], [0]), ([], []), ([0.0], [0]), ([1], [0.5]),
                        (torch.tensor([1]), torch.tensor([0])), ([1], torch.tensor([0]))):
        with pytest.raises(ValueError):
            cs.assemble(ids, starts)
    with pytest.raises(ValueError):
        m.SkeletonClipSet(videos[:2], window=129 * 12, device=DEV)                 # T = 129
    with pytest.raises(ValueError):
        m.SkeletonClipSet(videos[:2], hop=18, device=DEV)
    with pytest.raises(ValueError):
        m.SkeletonClipSet([], device=DEV)
    with pytest.raises(ValueError):
        m.SkeletonClipSet([dict(videos[1], obj=videos[1]['obj'][:, :11])], device=DEV)
    short = m.SkeletonClipSet(videos[3:5], window=48, hop=24, device=DEV)          # T = 4, a hop of two rows
    z, _ = recorded()
    bt = short.assemble([1, 0], [66 - 4 + 2, 3])                                   # the long video's last admissible row
    tab = reference_table(z, 4)
    assert torch.equal(bt[2].cpu()[0], torch.from_numpy(tab[64:68, 99:])) and tuple(bt.gt.shape) == (2, 1, 106, 4)
    assert torch.equal(bt.gt.cpu()[1, 0], torch.from_numpy(reference_table(z, 3)[3:7].T.copy()))


SEED_MDM = 1106


@pytest.mark.gpu
def test_trainers_take_the_batch_as_it_comes():
    """One ``training_step`` each on the B = 4 device batch and on the hand-built tuple of the same windows (host tensors): the same loss bits."""
    from interdiff_amd import synthetic as syn, skeleton_train as st
    from interdiff_amd.skeleton_mdm_train import SkeletonDenoiserTrainer
    from interdiff_amd.skeleton_finetune import SkeletonFineTuner
    cs = device_set()
    z, _ = recorded()
    clips = [(4, 0), (5, 24), (3, 12), (4, 552)]
    bt = cs.assemble([v for v, _ in clips], [s // STRIDE for _, s in clips])
    hand = reference_windows(z, clips)
    hand = hand[:3] + (bt[3].cpu(),)                                               # (zero_pose_obj: the set's own fp32, within the gate of the reference's)
    msd = {k: torch.from_numpy(v) for k, v in syn.skeleton_mdm_state_dict(SEED_MDM).items()}
    ck = dict(fx.golden('skel_ckpt.npz'))
    t = torch.tensor([37, 412, 875, 3])
    losses = []
    for batch in (bt, hand, bt.as_dict()):
        losses.append(SkeletonDenoiserTrainer(msd, device=DEV).training_step(batch, t=t, seed=3)[0])
    assert tuple(losses[0].shape) == (4,) and bool(torch.isfinite(losses[0]).all()) and torch.equal(losses[0], losses[1]) and torch.equal(losses[0], losses[2])
    a, b = SkeletonFineTuner(ck, device=DEV).training_step(bt), SkeletonFineTuner(ck, device=DEV).training_step(hand)
    assert bool(torch.isfinite(a)) and torch.equal(a, b)
    sd = st.init_state_dict(11)
    a, b = st.SkeletonTrainer(sd, dropout=0.1, seed=5, device=DEV).training_step(bt), st.SkeletonTrainer(sd, dropout=0.1, seed=5, device=DEV).training_step(hand)
    assert bool(torch.isfinite(a)) and torch.equal(a, b)


@pytest.mark.gpu
def test_fit_trains_validates_and_checkpoints(tmp_path):
    """2 epochs of 2 batches of 2, a validation after each: ``best.pt`` and ``last.pt``, and ``last.pt`` is the trainer's final state."""
    from interdiff_amd import synthetic as syn, fit as F
    from interdiff_amd.diffusion import create_gaussian_diffusion
    from interdiff_amd.skeleton_mdm_train import SkeletonDenoiserTrainer
    from interdiff_amd.skeleton_finetune import SkeletonFineTuner
    cs = device_set()
    full = cs.index()
    idx, vidx = full.subset([0, 1, 10, 30, 49]), full.subset([5, 48, 51])          # 5 entries: the fifth is dropped with the partial batch
    msd = {k: torch.from_numpy(v) for k, v in syn.skeleton_mdm_state_dict(SEED_MDM).items()}
    short = create_gaussian_diffusion('cosine', 1000, '4')
    runs = ((SkeletonFineTuner(dict(fx.golden('skel_ckpt.npz')), device=DEV), F.skeleton_correction_validate()),
            (SkeletonDenoiserTrainer(msd, device=DEV), F.skeleton_denoiser_validate(short, seed=1)))
    for k, (tr, validate) in enumerate(runs):
        d = str(tmp_path / ('run%d' % k))
        out = F.fit(tr, cs, idx, batch_size=2, max_epochs=2, seed=9, validate=validate, val_index=vidx, check_val_every_n_epoch=1, ckpt_dir=d)
        assert out['steps'] == 4 and len(out['val']) == 2 and all(np.isfinite(v) for _, v in out['val']) and sorted(os.listdir(d)) == ['best.pt', 'last.pt']
        last, now = torch.load(os.path.join(d, 'last.pt')), tr.state_dict()
        assert sorted(last) == sorted(now) and all(torch.equal(torch.as_tensor(now[n]).cpu(), torch.as_tensor(last[n]).cpu()) for n in last)
        assert sorted(torch.load(os.path.join(d, 'best.pt'))) == sorted(now)


@pytest.mark.gpu
def test_skeleton_evaluate_equals_the_hand_written_loop():
    """5 windows at batch size 2 under a 4-step respaced schedule, with and without the correction hook: the loop of eval_skeleton.py:145-165 written out."""
    from interdiff_amd import synthetic as syn, fit as F, skeleton as sk
    from interdiff_amd.diffusion import create_gaussian_diffusion
    cs = device_set()
    idx = cs.index().subset([0, 3, 20, 47, 52])
    model = sk.SkeletonMDM({k: torch.from_numpy(v) for k, v in syn.skeleton_mdm_state_dict(SEED_MDM).items()}, device=DEV)
    diff = create_gaussian_diffusion('cosine', 1000, '4')
    proj = sk.SkeletonObjProjector({k: torch.from_numpy(v) for k, v in fx.golden('skel_ckpt.npz').items()}, device=DEV)
    for obj_model in (None, proj):
        got = F.skeleton_evaluate(model, diff, obj_model, cs, idx, 2, seed=5)
        sums = dict(mpjpe_h=[], mpjpe_o=[], translation_error=[], rotation_error=[])
        for part in (idx.entries[0:2], idx.entries[2:4], idx.entries[4:5]):
            batch = cs.assemble([k for k, _, _ in part], [r for _, r, _ in part])
            obj_pred, body_pred, pose_pred, obj_gt, body_gt, pose_gt = sk.sample_once_proj(batch, model, diff, obj_model, seed=5)
            B = pose_gt.shape[1]
            md = sk.skeleton_metrics(body_pred.view(T, B, -1, 3), body_gt.view(T, B, -1, 3), obj_pred.view(T, B, -1, 3), obj_gt.view(T, B, -1, 3), pose_pred, pose_gt)
            for k, v in md.items():
                sums[k].append(v * B)
        want = {k: float(np.sum(v) / 5) for k, v in sums.items()}
        print('skeleton_evaluate (hook %s): %s' % (obj_model is not None, got))
        assert sorted(got) == sorted(want) and all(np.isfinite(v) for v in got.values())
        for k in want:
            assert abs(got[k] - want[k]) <= 1e-12 * max(1.0, abs(want[k])), k      # the same products, summed by Python instead of numpy


# ------------------------------------------------------------------------------------------------------------------------ GPU: the kernels at their edges
def device_prepare(videos, J, P, stride):
    """``SkeletonClipSet.__init__``'s call of ``interdiff_skeleton_video_prepare`` with a ``signs`` buffer (the class passes None): every video of one geometry in
    ONE launch, side by side behind seq_off / row_off.  -> per video dict(table, zero_pose_obj, report, signs) on the host"""
    from interdiff_amd import _lib
    m = sd_mod()
    parts = [m._video_arrays(v, k, J, P) for k, v in enumerate(videos)]
    counts = [F for F, _ in parts]
    rows = [-(-F // stride) for F in counts]
    seq_off, row_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
    n, R, W = len(videos), int(row_off[-1]), 3 * (J + P) + 7
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    raw = [up(np.concatenate([a[i].reshape(F, -1) for F, a in parts])) for i in range(4)]
    d_seq, d_row = up(seq_off), up(row_off)
    table, zpo = torch.full((R, W), np.nan, dtype=torch.float32, device=DEV), torch.full((n, P, 3), np.nan, dtype=torch.float32, device=DEV)
    report, rc = torch.full((n, 3), np.nan, dtype=torch.float64, device=DEV), torch.full((R,), np.nan, dtype=torch.float64, device=DEV)
    signs = torch.zeros(int(seq_off[-1]), dtype=torch.int8, device=DEV)
    _lib.check(_lib.load().interdiff_skeleton_video_prepare(*[_lib.dptr(a, torch.float64) for a in raw], _lib.dptr(d_seq, torch.int64), _lib.dptr(d_row, torch.int64), n, J, P,
                                                            stride, _lib.dptr(table), _lib.dptr(zpo), _lib.dptr(report), _lib.dptr(rc), signs.data_ptr(), _lib.stream()),
               'skeleton_video_prepare')
    table, zpo, report, rc, signs = (t.cpu().numpy() for t in (table, zpo, report, rc, signs))
    return [dict(table=table[row_off[k]:row_off[k + 1]], zero_pose_obj=zpo[k], signs=signs[seq_off[k]:seq_off[k + 1]],
                 report=m.VideoReport(float(report[k, 0]), float(report[k, 1]), float(report[k, 2]), rc[row_off[k]:row_off[k + 1]])) for k in range(n)]


def same_bits(got, host):
    return (np.array_equal(got['table'].view(np.uint32), host['table'].view(np.uint32)) and np.array_equal(got['zero_pose_obj'].view(np.uint32), host['zero_pose_obj'].view(np.uint32))
            and tuple(got['report'][:3]) == tuple(host['report'][:3]) and np.array_equal(got['report'].row_contact, host['report'].row_contact)
            and np.array_equal(got['signs'], host['signs']))


@pytest.mark.gpu
@pytest.mark.parametrize('geom', GEOMETRIES)
def test_device_prepare_on_adversarial_videos_gives_the_host_bits_and_the_references(geom):
    """A4: every A1 and A2 video of one geometry in one launch (F from 1 to 700 side by side): table, zero_pose_obj, the three report doubles, the row contacts and
    the signs ``==`` the host instance's, and the A1 assertions against the sequential sign loop / scipy / numpy hold for the device's own output."""
    items = [it for it in synthetic_videos() if it['geom'] == geom]
    assert len(items) == {(21, 12, 12): 17, (1, 1, 1): 3, (3, 64, 7): 3}[geom] and any(it['degenerate'] for it in items) and not all(it['degenerate'] for it in items)
    got = device_prepare([it['video'] for it in items], *geom)
    for it, g in zip(items, got):
        print('%s: device report (%.17g, %.17g, %.17g); host (%.17g, %.17g, %.17g); %d signs differ from the host instance'
              % ((it['name'],) + tuple(g['report'][:3]) + tuple(it['host']['report'][:3]) + (int((g['signs'] != it['host']['signs']).sum()),)))
    for it, g in zip(items, got):
        assert same_bits(g, it['host']), it['name']
        check_prepared(it, g, 'device')


@functools.lru_cache(maxsize=None)
def synthetic_set(geom, window, hop=None):
    J, P, stride = geom
    items = [it for it in synthetic_videos() if it['geom'] == geom]
    cs = sd_mod().SkeletonClipSet([it['video'] for it in items], window=window, stride=stride, hop=hop or stride, n_joints=J, n_points=P, device=DEV)
    return cs, items


def check_windows(cs, hosts, ids, starts):
    """``assemble`` against plain slicing of the host instance's tables: everything bit-equal, ``gt`` the transpose."""
    bt = cs.assemble(ids, starts)
    T, J, P = cs.T, cs.J, cs.P
    want = np.stack([hosts[k]['table'][r:r + T] for k, r in zip(ids, starts)])
    assert want.shape == (len(ids), T, cs.W)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
    for name, got, ref in (('body', bt[0], want[..., :3 * J].reshape(-1, T, J, 3)), ('obj', bt[1], want[..., 3 * J:3 * (J + P)].reshape(-1, T, P, 3)),
                           ('pose', bt[2], want[..., 3 * (J + P):]), ('zero_pose_obj', bt[3], np.stack([hosts[k]['zero_pose_obj'] for k in ids])),
                           ('gt', bt.gt, want.transpose(0, 2, 1)[:, None])):
        assert got.dtype == torch.float32 and got.is_contiguous() and tuple(got.shape) == ref.shape, name
        assert np.array_equal(bits(got.cpu().numpy()), bits(ref)), name
    return bt


@pytest.mark.gpu
def test_public_route_and_batch_shapes_on_the_64_point_set():
    """A4: ``SkeletonClipSet`` on the (3, 64, 7) videos reports the host instance's ``VideoReport``s.  B: windows of T = 5 (W = 208, LD = 209) at B = 1 and at
    B = 65 with repeated windows, first and last admissible rows included."""
    cs, items = synthetic_set((3, 64, 7), 35)
    assert cs.T == 5 and cs.W == 208 and cs.rows == [43, 43, 43] and len(cs.reports) == 3
    for rep, it in zip(cs.reports, items):
        print('%s: class report (%.17g, %.17g, %.17g)' % ((it['name'],) + tuple(rep[:3])))
        assert tuple(rep[:3]) == tuple(it['host']['report'][:3]) and np.array_equal(rep.row_contact, it['host']['report'].row_contact)
    hosts = [it['host'] for it in items]
    check_windows(cs, hosts, [1], [38])
    ids = [k % 3 for k in range(65)]
    starts = [(7 * k) % 39 for k in range(62)] + [0, 38, 38]
    assert len(set(zip(ids, starts))) < 65 and 0 in starts and max(starts) == 43 - 5
    check_windows(cs, hosts, ids, starts)


@pytest.mark.gpu
@pytest.mark.parametrize('T', [1, 128])
def test_windows_of_odd_width_have_no_padding_column(T):
    """B: J = 1, P = 1 gives W = 13 = LD (W | 1 = W: the tile has no padding column), at T = 1 (window = stride) and T = 128 (the kernel's limit)."""
    cs, items = synthetic_set((1, 1, 1), T)
    assert cs.W == 13 and (cs.W | 1) == cs.W and cs.T == T and cs.rows == [300, 300, 300]
    ids, starts = [0, 1, 0, 2, 1], [0, 300 - T, 300 - T, 0, 131 if T == 1 else 100]                 # the first and the last admissible start row of both videos
    bt = check_windows(cs, [it['host'] for it in items], ids, starts)
    assert tuple(bt.gt.shape) == (5, 1, 13, T) and not bool(torch.isnan(bt.gt).any())
    with pytest.raises(ValueError):
        cs.assemble([0], [300 - T + 1])


@pytest.mark.gpu
def test_a_nearly_full_tile_assembles_and_a_larger_one_is_refused_before_any_launch():
    """B: J = 21, P = 64: W = 262, LD = 263.  T = 62 is 65,224 B of dynamic LDS (the launcher allows 65,536) and assembles bit for bit; T = 63 (66,276 B) is a
    ValueError of the class and IDF_E_INVAL of the C entry called directly -- its outputs keep their sentinel."""
    import ctypes as C
    from interdiff_amd import _lib
    m = sd_mod()
    video, _ = synth_video(200, 21, 64, 1, (63, 64, 130), 900)
    host = m.prepare_host(video, stride=1, n_joints=21, n_points=64)
    cs = m.SkeletonClipSet([video], window=62, stride=1, hop=1, n_joints=21, n_points=64, device=DEV)
    lds = cs.T * (cs.W | 1) * 4
    print('tile: T %d x LD %d x 4 = %d B of %d' % (cs.T, cs.W | 1, lds, _lib.SKEL_WINDOW_LDS))
    assert cs.W == 262 and lds == 65224 and lds <= _lib.SKEL_WINDOW_LDS < 63 * 263 * 4 == 66276
    check_windows(cs, [host], [0, 0, 0], [0, 200 - 62, 77])
    with pytest.raises(ValueError):
        m.SkeletonClipSet([video], window=63, stride=1, hop=1, n_joints=21, n_points=64, device=DEV)
    B, T = 1, 63
    clips = torch.zeros(2, B, dtype=torch.int32, device=DEV)
    new = lambda *shape: torch.full(shape, -7.0, dtype=torch.float32, device=DEV)
    o = dict(body=new(B, T, 21, 3), obj=new(B, T, 64, 3), pose=new(B, T, 7), zero_pose_obj=new(B, 64, 3), gt=new(B, 1, 262, T))
    wb = _lib.SkelWindowBatch()
    for k in _lib.SKEL_WINDOW_FIELDS:
        setattr(wb, k, o[k].data_ptr())
    rc = cs.lib.interdiff_skeleton_window_batch(C.byref(cs.cset), _lib.dptr(clips, torch.int32), B, T, C.byref(wb), _lib.stream())
    torch.cuda.synchronize()
    assert rc == -22 and all(bool((t == -7.0).all()) for t in o.values())
