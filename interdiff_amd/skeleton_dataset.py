"""The skeleton-mode (HO-GCN) dataset: the raw pickles, which windows a split holds, and -- on the GPU -- the whole set resident and a batch of windows in one launch.

    load_skeleton_video / parse_motion_dir   data/dataset_skeleton.py:20-38, 109-121 -- one pickle per directory -> float64 arrays (host)
    SkeletonWindowIndex                      :122-124, 144-160, 188 -- the 240-frame windows every 12 frames, the ``unseen`` contact filters, the discrepancy filter,
                                             ``len(sample_sequences) > 1`` (host); ``entries`` are what ``fit.epoch_batches`` / ``dataset.draw_starts`` take
    split_seen / is_unseen                   :185, 202-203 -- the 0.7 / 0.2 / rest ``random_split`` under seed 42; chairs 3 and 4 are the unseen instances (host)
    SkeletonClipSet                          :40-65, 85-104, 148-158 -- every video uploaded once, ``interdiff_skeleton_video_prepare`` (quaternion signs, the fp32
                                             table of the down-sampled frames, zero_pose_obj, the per-video report: one launch for all videos);
                                             ``assemble(seq_ids, starts)`` = ``__getitem__`` + the DataLoader's collation + the denoiser's token for B windows
                                             (``interdiff_skeleton_window_batch``, one launch)
    prepare_host                             the same per-video code on the CPU (``interdiff_debug_skeleton_video_prepare``): the reports an index needs, without a GPU

``assemble`` returns a ``SkeletonBatch``: the reference's collated tuple (body [B,T,21,3], obj [B,T,12,3], pose [B,T,7], zero_pose_obj [B,12,3], filenames,
obj_names) that ``SkeletonDenoiserTrainer``, ``SkeletonTrainer`` / ``SkeletonFineTuner``, ``skeleton_losses.validation_step`` / ``test_step``,
``skeleton.skeleton_validation_step`` and ``skeleton.sample_once_proj`` read as it is, with the token ``.gt`` [B,1,106,T] on the side.

The reference module is a restatement's source, not a program that runs: it uses ``os`` on line 2 before importing it and opens a YAML of local paths at import, so it
cannot be imported; ``get_datasets`` calls ``get_sequences(f, align_data, discard_discrep, unseen, filename=...)``, which passes ``filename`` twice, so only its
cached-pickle branch can ever have run; and its ingestion walks every full-rate frame of ~500 videos in a Python loop (``get_consistent_poses``), then stores every
20-frame window separately -- each down-sampled frame up to 20 times, in float64 -- a cost it hides behind ``ds_seen.pkl``.  Here the ingestion is one kernel launch and
the resident set holds each down-sampled frame once (424 B), so that cache has no purpose and is not built.

NOT built: ``align_data``.  ``get_datasets(align_data=...)`` hands it to ``get_sequences`` in the position of ``discard_discrep``; no function of the module has a
parameter of that name or reads one, so there is no behaviour to restate.  Learning-rate schedules (as in ``fit``).
"""
import collections
import ctypes as C
import os
import pickle
import numpy as np
import torch
from . import _lib

N_JOINTS, N_POINTS = 21, 12
UNSEEN_OBJECTS = ('chair3', 'chair4')
DISCREPANCY_LIMIT, QUAT_CHECK_LIMIT = 1e-2, 1e-4                     # :100, :93

VideoReport = collections.namedtuple('VideoReport', 'discrepancy quat_check contact_sum row_contact')
VideoReport.__doc__ = """What ``check_sequences`` and the contact filters look at: the discrepancy of :98-99, the signed sum of |q| - 1 over the down-sampled frames
(:93), the contact sum over all frames (:122), and the contact value of every down-sampled frame (float64 [rows])."""


def is_unseen(obj_name):
    """``object_name in ["chair3", "chair4"]`` (:185, :213)."""
    return obj_name in UNSEEN_OBJECTS


def load_skeleton_video(path, n_joints=N_JOINTS, n_points=N_POINTS):
    """One pickle of the HO-GCN release (:109-121): ``pickle.load(f)[0]`` = [skeleton, contact, pose, object] per frame ->
    dict(skeleton [F,21,3], contact [F,1], pose [F,7] (xyz | quaternion xyzw), obj [F,12,3], all float64; filename = the file's stem, obj_name = its second
    ``_`` field).  A pickle is code: load only files you trust.  ValueError for arrays that do not have these shapes."""
    with open(path, 'rb') as f:
        data = pickle.load(f)[0]
    stem = os.path.splitext(os.path.basename(path))[0]
    parts = stem.split('_')
    if len(parts) < 2:
        raise ValueError('%s: the object name is the second "_" field of the file name' % path)
    try:
        F = len(data[0])
        video = dict(skeleton=np.array(data[0], dtype='float64').reshape((F, n_joints, 3)), contact=np.array(data[1], dtype='float64').reshape((F, 1)),
                     pose=np.array(data[2], dtype='float64').reshape((F, 7)), obj=np.array(data[3], dtype='float64').reshape((F, n_points, 3)))
    except (TypeError, IndexError, ValueError) as e:
        raise ValueError('%s: expected [skeleton [F,%d,3], contact [F,1], pose [F,7], object [F,%d,3]] (%s)' % (path, n_joints, n_points, e))
    if F == 0:
        raise ValueError('%s: no frames' % path)
    video.update(filename=stem, obj_name=parts[1])
    return video


def parse_motion_dir(root):
    """``parse_paths`` (:20-38): every sub-directory of ``root`` holds one file (an empty one is skipped, more than one is a ValueError) ->
    [(path, filename, obj_name)], sorted by directory name (the reference takes the file system's order)."""
    files = []
    for d in sorted(os.listdir(root)):
        p = os.path.join(root, d)
        if not os.path.isdir(p):
            continue                                                   # (ds_seen.pkl and its kind live next to the directories)
        inside = sorted(os.listdir(p))
        if not inside:
            continue
        if len(inside) != 1:
            raise ValueError('%s: one file per directory expected, found %d' % (p, len(inside)))
        stem = os.path.splitext(inside[0])[0]
        if len(stem.split('_')) < 2:
            raise ValueError('%s: the object name is the second "_" field of the file name' % inside[0])
        files.append((os.path.join(p, inside[0]), stem, stem.split('_')[1]))
    return files


def split_seen(n, seed=42):
    """The index lists of ``random_split(ds, [int(.7 n), int(.2 n), rest], generator=torch.Generator().manual_seed(42))`` (:202-203): consecutive slices of
    one ``torch.randperm(n, generator=...)``.  -> (train, valid, test)"""
    perm = torch.randperm(int(n), generator=torch.Generator().manual_seed(seed)).tolist()
    a, b = int(0.7 * n), int(0.2 * n)
    return perm[:a], perm[a:a + b], perm[a + b:]


class SkeletonWindowIndex:
    """``entries``: [(k, first_row, 1)] -- every window the reference's ``get_sequences`` keeps, in its order; ``k`` the video's position in the constructor's
    lists, ``first_row`` the window's first row of the down-sampled table (frame ``first_row * stride``); the bias of 1 makes ``dataset.draw_starts`` return the row.

    Window starts are 0, hop, 2 hop, ... while ``start + window < F`` (strict, :146); a window is the ``T = window // stride`` frames ``start + t * stride``.
    ``reports``: one ``VideoReport`` per video (``SkeletonClipSet.reports`` or ``prepare_host``).  ``unseen=True`` (:122-124, :154): a video whose contact sum
    is < 0.5 is dropped, and so is a window whose T sampled contact values sum to < 0.5.  ``discard_discrep=True`` (:97-104): a video whose discrepancy is
    > 1e-2 is dropped.  ``min_windows``: a video with fewer kept windows is dropped -- 2 restates ``get_datasets``' ``len(sample_sequences) > 1``,
    1 ``get_unseen_dataset``.  ``videos``: the kept videos' positions; ``subset(positions)``: an index over some of the entries (a split)."""

    def __init__(self, frame_counts, reports, *, window=240, stride=12, hop=12, unseen=False, discard_discrep=False, min_windows=2):
        window, stride, hop = int(window), int(stride), int(hop)
        if window <= 0 or stride <= 0 or hop <= 0 or window % stride or hop % stride:
            raise ValueError('window and hop must be positive multiples of stride: a window is rows of the down-sampled table')
        if len(frame_counts) != len(reports):
            raise ValueError('one report per video')
        self.window, self.stride, self.hop, self.T = window, stride, hop, window // stride
        self.frame_counts = [int(F) for F in frame_counts]
        self.entries, self.videos = [], []
        for k, (F, rep) in enumerate(zip(self.frame_counts, reports)):
            if unseen and float(rep.contact_sum) < 0.5:
                continue
            if discard_discrep and float(rep.discrepancy) > DISCREPANCY_LIMIT:
                continue
            rc = np.asarray(rep.row_contact, np.float64).reshape(-1)
            if rc.size != -(-F // stride):
                raise ValueError('video %d: %d contact rows for %d frames at stride %d' % (k, rc.size, F, stride))
            kept = []
            for start in range(0, max(F - window, 0), hop):                          # start + window < F
                row = start // stride
                if unseen and rc[row:row + self.T].sum() < 0.5:
                    continue
                kept.append((k, row, 1))
            if len(kept) >= min_windows:
                self.entries += kept
                self.videos.append(k)

    def subset(self, positions):
        out = object.__new__(SkeletonWindowIndex)
        out.__dict__.update(self.__dict__)
        out.entries = [self.entries[int(i)] for i in positions]
        out.videos = sorted({k for k, _, _ in out.entries})
        return out

    def __len__(self):
        return len(self.entries)

    def __getitem__(self, i):
        return self.entries[i]


class SkeletonBatch(tuple):
    """(body [B,T,21,3], obj [B,T,12,3], pose [B,T,7], zero_pose_obj [B,12,3], filenames, obj_names): the reference's collated batch; ``.gt`` [B,1,106,T] is the
    denoiser's token of the same windows, ``.as_dict()`` the dict form ``skeleton_mdm_train.tokens_of`` takes."""

    def __new__(cls, body, obj, pose, zero_pose_obj, filenames, obj_names, gt):
        self = super().__new__(cls, (body, obj, pose, zero_pose_obj, filenames, obj_names))
        self.gt = gt
        return self

    def as_dict(self):
        return {'gt': self.gt, 'zero_pose_obj': self[3]}


def _video_arrays(video, k, J, P):
    try:
        arrs = [np.ascontiguousarray(video[n], dtype=np.float64) for n in ('skeleton', 'obj', 'pose', 'contact')]
    except (KeyError, TypeError, ValueError) as e:
        raise ValueError('video %d: skeleton, obj, pose and contact arrays expected (%s)' % (k, e))
    F = arrs[2].shape[0] if arrs[2].ndim else 0
    if F == 0 or arrs[0].shape != (F, J, 3) or arrs[1].shape != (F, P, 3) or arrs[2].shape != (F, 7) or arrs[3].size != F:
        raise ValueError('video %d: skeleton [F,%d,3], obj [F,%d,3], pose [F,7], contact [F,1] with F >= 1 expected' % (k, J, P))
    return F, arrs


def _check_reports(reports):
    for k, rep in enumerate(reports):
        if not rep.quat_check < QUAT_CHECK_LIMIT:                                    # the reference asserts it (:93); a NaN fails as well
            raise ValueError('video %d: the quaternions of its down-sampled frames are not unit (sum of |q| - 1 = %r)' % (k, rep.quat_check))


def prepare_host(video, stride=12, n_joints=N_JOINTS, n_points=N_POINTS):
    """ONE video through the CPU instance of the device's per-video code -> dict(table fp32 [rows,106], zero_pose_obj fp32 [12,3], report ``VideoReport``,
    signs int8 [F]); bit for bit what ``SkeletonClipSet`` holds for it.  No quaternion check is made here."""
    F, (skel, obj, pose, contact) = _video_arrays(video, 0, n_joints, n_points)
    if stride <= 0 or n_points > _lib.SKEL_SET_MAX_P:
        raise ValueError('stride >= 1 and at most %d object points' % _lib.SKEL_SET_MAX_P)
    rows, W = -(-F // stride), 3 * (n_joints + n_points) + 7
    table, zpo = np.zeros((rows, W), np.float32), np.zeros((n_points, 3), np.float32)
    report, rc, signs = np.zeros(3, np.float64), np.zeros(rows, np.float64), np.zeros(F, np.int8)
    _lib.check(_lib.load().interdiff_debug_skeleton_video_prepare(skel.ctypes.data, obj.ctypes.data, pose.ctypes.data, contact.ctypes.data, F, n_joints, n_points,
                                                                  stride, table.ctypes.data, zpo.ctypes.data, report.ctypes.data, rc.ctypes.data, signs.ctypes.data),
               'debug_skeleton_video_prepare')
    return dict(table=table, zero_pose_obj=zpo, report=VideoReport(float(report[0]), float(report[1]), float(report[2]), rc), signs=signs)


class SkeletonClipSet:
    """Every video of a split on the device: uploaded once, ingested by one launch, addressed through a per-video row table.

    ``videos``: ``load_skeleton_video`` dicts.  ``window`` / ``stride`` / ``hop`` as in ``SkeletonWindowIndex`` (T = window // stride <= 128).  Kept: ``reports``
    (a ``VideoReport`` per video; ValueError when a video's quaternion check sum is >= 1e-4, which the reference asserts), ``frame_counts``, ``filename``,
    ``obj_name``; ``index(**filters)`` is the ``SkeletonWindowIndex`` of the set.  Resident per down-sampled frame: one fp32 row of 106 values = 424 B
    (plus 144 B per video); during the upload also the raw float64 arrays, of which the kernel reads the quaternions and contact values at full rate and the
    rest at the down-sampled frames only.  Nobody has measured the resident size on the real data."""

    def __init__(self, videos, *, window=240, stride=12, hop=12, device='cuda', n_joints=N_JOINTS, n_points=N_POINTS):
        if not videos:
            raise ValueError('no videos')
        self.window, self.stride, self.hop = int(window), int(stride), int(hop)
        if self.window <= 0 or self.stride <= 0 or self.hop <= 0 or self.window % self.stride or self.hop % self.stride:
            raise ValueError('window and hop must be positive multiples of stride')
        self.T, self.J, self.P = self.window // self.stride, int(n_joints), int(n_points)
        self.W = 3 * (self.J + self.P) + 7
        if self.T > _lib.CLIP_MAX_T or self.P > _lib.SKEL_SET_MAX_P or self.T * (self.W | 1) * 4 > _lib.SKEL_WINDOW_LDS:
            raise ValueError('at most %d frames per window, %d object points and %d bytes per window tile' % (_lib.CLIP_MAX_T, _lib.SKEL_SET_MAX_P, _lib.SKEL_WINDOW_LDS))
        self.lib = _lib.load()
        self.device = torch.device(device)
        parts = [_video_arrays(v, k, self.J, self.P) for k, v in enumerate(videos)]
        self.frame_counts = [F for F, _ in parts]
        self.filename, self.obj_name = [v.get('filename') for v in videos], [v.get('obj_name') for v in videos]
        self.rows = [-(-F // self.stride) for F in self.frame_counts]
        self.seq_off = np.concatenate([[0], np.cumsum(self.frame_counts)]).astype(np.int64)
        self.row_off = np.concatenate([[0], np.cumsum(self.rows)]).astype(np.int64)
        n, R = len(videos), int(self.row_off[-1])
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
        raw = [up(np.concatenate([a[i].reshape(F, -1) for F, a in parts])) for i in range(4)]          # skeleton, obj, pose, contact: float64, released below
        seq_off = up(self.seq_off)
        new = lambda *shape, dtype=torch.float32: torch.empty(*shape, dtype=dtype, device=self.device)
        self.t = dict(row_off=up(self.row_off), table=new(R, self.W), zero_pose_obj=new(n, self.P, 3))
        report, row_contact = new(n, 3, dtype=torch.float64), new(R, dtype=torch.float64)
        _lib.check(self.lib.interdiff_skeleton_video_prepare(*[_lib.dptr(a, torch.float64) for a in raw], _lib.dptr(seq_off, torch.int64),
                                                             _lib.dptr(self.t['row_off'], torch.int64), n, self.J, self.P, self.stride, _lib.dptr(self.t['table']),
                                                             _lib.dptr(self.t['zero_pose_obj']), _lib.dptr(report), _lib.dptr(row_contact), None, _lib.stream()),
                   'skeleton_video_prepare')
        rep, rc = report.cpu().numpy(), row_contact.cpu().numpy()                  # (synchronises: the raw arrays may go)
        del raw
        self.reports = [VideoReport(float(rep[k, 0]), float(rep[k, 1]), float(rep[k, 2]), rc[self.row_off[k]:self.row_off[k + 1]].copy()) for k in range(n)]
        _check_reports(self.reports)
        self.cset = _lib.SkelClipSet()
        self.cset.n_video, self.cset.J, self.cset.P = n, self.J, self.P
        for k in ('row_off', 'table', 'zero_pose_obj'):
            setattr(self.cset, k, self.t[k].data_ptr())

    def __len__(self):
        return len(self.frame_counts)

    def index(self, **filters):
        return SkeletonWindowIndex(self.frame_counts, self.reports, window=self.window, stride=self.stride, hop=self.hop, **filters)

    def _checked(self, seq_ids, starts):
        if isinstance(seq_ids, torch.Tensor) or isinstance(starts, torch.Tensor):
            raise ValueError('seq_ids and starts are host integer sequences (they are range-checked before anything is launched)')
        ids, st = np.asarray(seq_ids), np.asarray(starts)
        if ids.ndim != 1 or st.shape != ids.shape or ids.size == 0 or ids.dtype.kind not in 'iu' or st.dtype.kind not in 'iu':
            raise ValueError('seq_ids and starts must be integer sequences of one (non-zero) length')
        ids, st = ids.astype(np.int64), st.astype(np.int64)
        if ids.min() < 0 or ids.max() >= len(self):
            raise ValueError('video id outside [0, %d)' % len(self))
        rows = np.asarray(self.rows, np.int64)[ids]
        bad = (st < 0) | (st + self.T > rows)
        if bad.any():
            b = int(np.nonzero(bad)[0][0])
            raise ValueError('window %d: rows %d .. %d do not lie inside video %d (%d rows)' % (b, st[b], st[b] + self.T - 1, ids[b], rows[b]))
        return ids, st

    def assemble(self, seq_ids, starts, body=None):
        """B windows: window b = the rows ``starts[b] .. starts[b] + T - 1`` of video ``seq_ids[b]`` (frames ``(starts[b] + t) * stride``) -> ``SkeletonBatch``.
        ``body`` is accepted and ignored (``fit`` passes it to every set).  ValueError -- before anything is launched -- for anything but two host integer sequences
        of equal, non-zero length that name rows inside their videos."""
        ids, st = self._checked(seq_ids, starts)
        B, T, dev = int(ids.size), self.T, self.device
        clips = torch.from_numpy(np.stack([ids, st]).astype(np.int32)).to(dev)
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
        o = dict(body=new(B, T, self.J, 3), obj=new(B, T, self.P, 3), pose=new(B, T, 7), zero_pose_obj=new(B, self.P, 3), gt=new(B, 1, self.W, T))
        wb = _lib.SkelWindowBatch()
        for k in _lib.SKEL_WINDOW_FIELDS:
            setattr(wb, k, o[k].data_ptr())
        _lib.check(self.lib.interdiff_skeleton_window_batch(C.byref(self.cset), _lib.dptr(clips, torch.int32), B, T, C.byref(wb), _lib.stream()), 'skeleton_window_batch')
        return SkeletonBatch(o['body'], o['obj'], o['pose'], o['zero_pose_obj'], [self.filename[i] for i in ids], [self.obj_name[i] for i in ids], o['gt'])
