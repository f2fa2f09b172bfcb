"""interdiff_amd/skeleton_dataset.py and the skeleton loops of interdiff_amd/fit.py against the reference's OWN data/dataset_skeleton.py functions, recorded by
tests/golden/make_golden_skeleton_dataset.py into tests/golden/skel_dataset.npz (six synthetic videos; what each is for is said there).

Host: the window rule worked by hand; the ``unseen`` / ``discard_discrep`` / ``min_windows`` filters against the recorded window starts; ``split_seen`` against the
recorded ``random_split``; the pickle loader; the C entries; the per-video code on its host instance (``interdiff_debug_skeleton_video_prepare``): signs equal on
every frame, table rows bit-equal to float32(sign * reference), zero_pose_obj within the ETL gate of tests/test_dataset.py (1e-6 max(1, |ref|max)), the discrepancy
within 1e-12 max(1, ref) (two float64 evaluations of the same ~250-term mean in different orders: ~250 * 2.2e-16 = 6e-14 of the value); ``fit`` and
``skeleton_evaluate`` on fake pieces.  GPU: the device prepare against the host instance bit for bit; ``assemble`` at B = 1, 3, 4 (one window twice) and 70 against the reference's windows bit
for bit; the call contract; the three skeleton trainers; ``fit``; ``skeleton_evaluate``.

The skeleton / object arrays are NaN in every frame that is no multiple of 12 -- the reference reads none of them -- so a kernel that does shows in its own output.
Without the feature every test below fails: the module, the loops and the entries do not exist.
"""
import functools
import os
import pickle
import numpy as np
import pytest
import torch
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
