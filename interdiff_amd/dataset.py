"""The SMPL-mode training set on the GPU: which clips a split holds, where each one starts this epoch, and a batch of them in a fixed number of launches.

    ClipIndex        data/dataset_smpl.py:27-33, 90-97 -- the split by sequence name and the (sequence, offset, bias) entry of every fragment (host)
    draw_starts      :108 -- ``np.random.choice(bias) + offset`` per entry, from a ``numpy.random.RandomState`` (host)
    DeviceClipSet    :44-89 -- every sequence of a split uploaded once; ``assemble(seq_ids, starts)`` is ``__getitem__`` (:105-204) plus the DataLoader's collation
                     for B clips: ``interdiff_clip_batch`` (canonicalisation, gt token, foot labels, object cloud: one launch; contact labels: one more) and, with
                     ``body=True``, the SMPL forward and the vertex normals per gender plus ``interdiff_clip_body_records`` (human_verts, markers, contact labels)

The batch is one dict of contiguous device tensors that ``DenoiserTrainer``, ``CorrectionFineTuner`` / ``CorrectionTrainer``, ``eval.batch_from_raw`` and
``ObjProjector.batch_tensors`` read as it is.  ``data.canonicalize_clip`` / ``clip_labels`` / ``collate_raw`` and ``correction_losses.body_records`` stay: they are the
host route this one is tested against.

NOT built, on purpose: the per-frame posed object cloud ``frames[t]['obj_points']`` [T,B,P,7] (:155-165).  No model, loss or trainer reads it -- they read the
top-level [B,P,6] cloud; ``data.clip_labels`` still produces it on the host.  The object contact lists are uploaded (CSR) for whoever builds it.  The skeleton
dataset (data/dataset_skeleton.py) is interdiff_amd/skeleton_dataset.py.
"""
import ctypes as C
import numpy as np
import torch
from . import _lib


class ClipIndex:
    """``entries``: [(k, offset, bias)] of one split -- ``k`` the sequence's position in the FILTERED list (``names`` / ``frame_counts`` hold that list,
    ``source`` its positions in the constructor's), one entry per whole fragment of ``(past_len + future_len) * sample_rate`` frames.  ``bias`` bounds the random
    start inside the fragment: 1 in test mode; in train mode the fragment length, and for a sequence's last fragment what is left of the sequence + 1, so that
    ``offset + draw + T * rate <= F`` always.  ``frame_counts``: what ``load_behave_sequence`` returns (already cut to the shorter of the two fit files)."""

    def __init__(self, names, frame_counts, mode, past_len=10, future_len=25, sample_rate=1):
        if mode not in ('train', 'test'):
            raise ValueError('mode must be train or test.')
        if len(names) != len(frame_counts):
            raise ValueError('one frame count per sequence name')
        keep = [i for i, n in enumerate(names) if (n[:6] != 'Date03') == (mode == 'train')]
        self.mode, self.past_len, self.future_len, self.sample_rate = mode, int(past_len), int(future_len), int(sample_rate)
        self.source = keep
        self.names, self.frame_counts = [names[i] for i in keep], [int(frame_counts[i]) for i in keep]
        self.fragment = fragment = (self.past_len + self.future_len) * self.sample_rate
        self.entries = []
        for k, F in enumerate(self.frame_counts):
            n = F // fragment
            for i in range(n):
                bias = 1 if mode == 'test' else (F + 1 - n * fragment if i == n - 1 else fragment)
                self.entries.append((k, i * fragment, bias))

    def __len__(self):
        return len(self.entries)

    def __getitem__(self, i):
        return self.entries[i]


def draw_starts(entries, rng):
    """[(k, start)] with ``start = rng.choice(bias) + offset``: one call of ``rng`` (a ``numpy.random.RandomState``) per entry, in order -- the stream
    ``np.random.choice(bias)`` of :108 consumes under the same seed."""
    return [(int(k), int(rng.choice(bias)) + int(off)) for k, off, bias in entries]


def _csr(lists, bound, what):
    """Per-frame index lists -> (int32 pointer [F + 1], int32 indices); every index must lie in [0, bound)."""
    arrs = [np.asarray(a, dtype=np.int64).reshape(-1) for a in lists]
    idx = np.concatenate(arrs) if arrs else np.zeros(0, np.int64)
    if idx.size and (idx.min() < 0 or idx.max() >= bound):
        raise ValueError('%s holds an index outside [0, %d)' % (what, bound))
    ptr = np.zeros(len(arrs) + 1, np.int64)
    np.cumsum([a.size for a in arrs], out=ptr[1:])
    if ptr[-1] >= 2 ** 31:
        raise ValueError('%s: more than 2^31 entries' % what)
    return ptr.astype(np.int32), idx.astype(np.int32)


def sequence_joints(seq, smpl, device='cuda', chunk=512, joints=(0, 10, 11)):
    """Pelvis, left foot, right foot (data/dataset_smpl.py:57,68-70) over every frame from ONE chunked SMPL pass -> fp32 [F,3,3] (``data.sequence_pelvis`` for three joints)."""
    out = []
    for s in range(0, len(seq['poses']), chunk):
        up = lambda k: torch.from_numpy(np.asarray(seq[k][s:s + chunk], dtype=np.float32)).to(device)
        out.append(smpl(up('poses'), th_betas=up('betas'), th_trans=up('trans'), want_v_posed=False)[1][:, list(joints)].cpu().numpy())
    return np.float32(np.concatenate(out))


class DeviceClipSet:
    """Every sequence of a split on the device, uploaded once and addressed through a per-sequence offset table.

    ``sequences``: ``data.load_behave_sequence`` dicts WITH the contact-side records (``obj_points`` [P,6], the two per-frame contact lists, ``ground_joint_label``,
    ``gender``, ``obj_name``); all must share P (ValueError).  ``smpl_layers``: one ``SMPL_Layer`` or ``{'male': ..., 'female': ...}`` keyed by ``seq['gender']``.
    ``joints``: per sequence (pelvis, left_foot, right_foot), each [F,3], in place of the SMPL pass (then ``smpl_layers`` may be None and ``assemble(body=True)``
    raises; ``n_verts`` bounds the body contact lists).  Held per frame: pose 624 B, betas 40 B, the fp64 fit fields 96 B, three joints 36 B, plus 4 B per contact
    index -- by that count a whole BEHAVE split is a few hundred MB; nobody has measured the figure on the real data."""

    def __init__(self, sequences, smpl_layers, past_len, future_len, sample_rate=1, device='cuda', joints=None, n_verts=6890, markers=None):
        from .correction import MARKERS67
        if not sequences:
            raise ValueError('no sequences')
        self.lib = _lib.load()
        self.device = torch.device(device)
        self.past_len, self.future_len, self.sample_rate = int(past_len), int(future_len), int(sample_rate)
        self.T = self.past_len + self.future_len
        if not 0 < self.T <= _lib.CLIP_MAX_T or self.sample_rate <= 0:
            raise ValueError('1 <= past_len + future_len <= %d and sample_rate >= 1' % _lib.CLIP_MAX_T)
        self.layers = smpl_layers if isinstance(smpl_layers, dict) or smpl_layers is None else {None: smpl_layers}
        layer_of = lambda seq: None if self.layers is None else self.layers[seq.get('gender') if None not in self.layers else None]
        self.V = int(n_verts) if self.layers is None else int(next(iter(self.layers.values())).cmodel.V)
        if self.layers is not None and any(int(l.cmodel.V) != self.V or int(l.cmodel.J) != 52 for l in self.layers.values()):
            raise ValueError('the body models must share their vertex count and have 52 joints (a [F,156] pose)')
        if joints is None and self.layers is None:
            raise ValueError('pass the body model(s) or the joints')
        pts = [np.asarray(s['obj_points'], np.float32) for s in sequences]
        if any(p.ndim != 2 or p.shape[1] != 6 for p in pts) or len({p.shape[0] for p in pts}) != 1:
            raise ValueError('every sequence needs obj_points [P,6] with the same P (got %s)' % sorted({p.shape for p in pts}))
        self.P = int(pts[0].shape[0])
        self.frame_counts = [len(s['poses']) for s in sequences]
        self.seq_name = [s.get('seq_name') for s in sequences]
        self.gender = [s.get('gender') for s in sequences]
        self.obj_name = [s.get('obj_name') for s in sequences]
        fit, jts, first, body_lists, obj_lists = [], [], [], [], []
        for i, s in enumerate(sequences):
            F = self.frame_counts[i]
            fields = [np.asarray(s[k], np.float64).reshape(F, -1) for k in ('poses', 'trans', 'obj_angles', 'obj_trans')]
            if fields[0].shape[1] != 156 or any(f.shape[1] != 3 for f in fields[1:]) or np.asarray(s['betas']).shape != (F, 10):
                raise ValueError('sequence %d: poses [F,156], betas [F,10], trans / obj_angles / obj_trans [F,3] expected' % i)
            fit.append(np.concatenate([fields[0][:, :3]] + fields[1:], axis=1))
            j = np.stack([np.asarray(a, np.float32) for a in joints[i]], axis=1) if joints is not None else sequence_joints(s, layer_of(s), self.device)
            if j.shape != (F, 3, 3):
                raise ValueError('sequence %d: pelvis, left foot and right foot must each be [F,3]' % i)
            jts.append(j.reshape(F, 9))
            if len(s['contact_label']) != F or len(s['obj_contact_label']) != F:
                raise ValueError('sequence %d: one contact list per frame expected' % i)
            lab = int(np.asarray(s['ground_joint_label']).reshape(-1)[0])
            if lab not in (10, 11):
                raise ValueError('sequence %d: the stored foot label must be 10 or 11' % i)
            first.append(lab)
            body_lists += list(s['contact_label'])
            obj_lists += list(s['obj_contact_label'])
        body_ptr, body_idx = _csr(body_lists, self.V, 'contact_label')                  # range-checked here: the kernels trust them
        obj_ptr, obj_idx = _csr(obj_lists, self.P, 'obj_contact_label')
        cat32 = lambda k: np.concatenate([np.asarray(s[k], np.float32) for s in sequences])
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
        mk = np.asarray(list(MARKERS67 if markers is None else markers), np.int32)
        if mk.size and (mk.min() < 0 or mk.max() >= self.V):
            raise ValueError('marker index outside the mesh')
        self.seq_off = np.concatenate([[0], np.cumsum(self.frame_counts)]).astype(np.int64)
        self.t = dict(seq_off=up(self.seq_off), pose=up(cat32('poses')), betas=up(cat32('betas')), fit64=up(np.concatenate(fit)), joints=up(np.concatenate(jts)),
                      obj_points6=up(np.stack(pts)), first_label=up(np.asarray(first, np.int32)), body_ptr=up(body_ptr),
                      body_idx=up(body_idx if body_idx.size else np.zeros(1, np.int32)), markers_idx=up(mk),
                      obj_ptr=up(obj_ptr), obj_idx=up(obj_idx if obj_idx.size else np.zeros(1, np.int32)))            # (the object CSR: uploaded, read by no kernel yet)
        self.cset = _lib.ClipSet()
        self.cset.n_seq, self.cset.P, self.cset.V, self.cset.n_markers = len(sequences), self.P, self.V, int(mk.size)
        for k in ('seq_off', 'pose', 'betas', 'fit64', 'joints', 'obj_points6', 'first_label', 'body_ptr', 'body_idx', 'markers_idx'):
            setattr(self.cset, k, self.t[k].data_ptr())
        self.n_markers = int(mk.size)
        self._topo = {}

    def __len__(self):
        return len(self.frame_counts)

    def _checked(self, seq_ids, starts):
        if isinstance(seq_ids, torch.Tensor) or isinstance(starts, torch.Tensor):
            raise ValueError('seq_ids and starts are host integer sequences (they are range-checked before anything is launched)')
        ids, st = np.asarray(seq_ids), np.asarray(starts)
        if ids.ndim != 1 or st.shape != ids.shape or ids.size == 0 or ids.dtype.kind not in 'iu' or st.dtype.kind not in 'iu':
            raise ValueError('seq_ids and starts must be integer sequences of one (non-zero) length')
        ids, st = ids.astype(np.int64), st.astype(np.int64)
        if ids.min() < 0 or ids.max() >= len(self):
            raise ValueError('sequence id outside [0, %d)' % len(self))
        F = np.asarray(self.frame_counts, np.int64)[ids]
        bad = (st < 0) | (st + (self.T - 1) * self.sample_rate >= F)
        if bad.any():
            b = int(np.nonzero(bad)[0][0])
            raise ValueError('clip %d: frames %d .. %d do not lie inside sequence %d (%d frames)' % (b, st[b], st[b] + (self.T - 1) * self.sample_rate, ids[b], F[b]))
        return ids, st

    def _topology(self, key):
        if key not in self._topo:
            from .geometry import MeshTopology
            self._topo[key] = MeshTopology(self.layers[key].th_faces, self.V, device=self.device)
        return self._topo[key]

    def assemble(self, seq_ids, starts, body=True):
        """B clips: clip b = the frames ``starts[b] + t * sample_rate`` of sequence ``seq_ids[b]``.  -> dict: body_pose [T,B,66], hand_pose [T,B,90], body_trans /
        obj_angles / obj_trans / pelvis [T,B,3], beta [T,B,10], gt [B,1,144,T], obj_points [B,P,3], obj_points6 [B,P,6], obj_angle (= obj_angles, the name
        ``ObjProjector.batch_tensors`` reads), ground_joint_label [T,B,2], contact_label uint8 [T,B,V], centroid [B,3], rotation [B,3,3]; host lists start_frame,
        seq_name, gender, obj_name; with ``body`` also human_verts [T,B,V,7] and markers [T,B,67,7].  A first frame whose heading is undefined (global orientation
        entries [0,0] = [2,0] = 0) gives non-finite output, as in the reference.  ValueError -- before anything is launched -- for anything but two host integer
        sequences of equal length that name frames inside their sequences."""
        ids, st = self._checked(seq_ids, starts)
        if body and self.layers is None:
            raise ValueError('body=True needs the body model(s): this set was built from injected joints alone')
        B, T, P, V, dev = int(ids.size), self.T, self.P, self.V, self.device
        clips = torch.from_numpy(np.stack([ids, st]).astype(np.int32)).to(dev)
        new = lambda *shape, dtype=torch.float32: torch.empty(*shape, dtype=dtype, device=dev)
        o = dict(body_pose=new(T, B, 66), hand_pose=new(T, B, 90), body_trans=new(T, B, 3), obj_angles=new(T, B, 3), obj_trans=new(T, B, 3), pelvis=new(T, B, 3),
                 beta=new(T, B, 10), gt=new(B, 1, 144, T), ground=new(T, B, 2), centroid=new(B, 3), rotation=new(B, 3, 3), obj_points=new(B, P, 3),
                 obj_points6=new(B, P, 6), contact_label=new(T, B, V, dtype=torch.uint8))
        cb = _lib.ClipBatch()
        for k in _lib.CLIP_BATCH_FIELDS:
            setattr(cb, k, o[k].data_ptr() if not (body and k == 'contact_label') else None)        # with body the record kernel writes the labels
        _lib.check(self.lib.interdiff_clip_batch(C.byref(self.cset), _lib.dptr(clips, torch.int32), B, T, self.sample_rate, C.byref(cb), _lib.stream()), 'clip_batch')
        o['ground_joint_label'] = o.pop('ground')
        o['obj_angle'] = o['obj_angles']
        o.update(start_frame=[int(s) for s in st], seq_name=[self.seq_name[i] for i in ids], gender=[self.gender[i] for i in ids], obj_name=[self.obj_name[i] for i in ids])
        if body:
            from .geometry import vertex_normals
            o['human_verts'], o['markers'] = new(T, B, V, 7), new(T, B, self.n_markers, 7)
            keys = [None] * B if None in self.layers else o['gender']
            pose = torch.cat([o['body_pose'], o['hand_pose']], dim=2)
            for key in sorted(set(keys), key=str):                      # one body model at a time; its clips' frames land in their slots through frame_map
                cols = [b for b in range(B) if keys[b] == key]
                if len(cols) == B:
                    sub, fmap = (lambda a: a.reshape(T * B, -1)), None
                else:
                    ci = torch.tensor(cols, dtype=torch.long, device=dev)
                    sub = lambda a: a[:, ci].reshape(T * len(cols), -1)
                    fmap = (torch.arange(T, device=dev)[:, None] * B + ci[None, :]).to(torch.int32).reshape(-1).contiguous()
                verts = self.layers[key](sub(pose), th_betas=sub(o['beta']), th_trans=sub(o['body_trans']), want_v_posed=False)[0]
                normals = vertex_normals(verts, self._topology(key))
                _lib.check(self.lib.interdiff_clip_body_records(C.byref(self.cset), _lib.dptr(clips, torch.int32), B, T, self.sample_rate, _lib.dptr(verts, torch.float32),
                                                                _lib.dptr(normals, torch.float32), _lib.dptr(fmap, torch.int32, allow_none=True), verts.shape[0],
                                                                _lib.dptr(o['human_verts']), _lib.dptr(o['markers']), _lib.dptr(o['contact_label']), _lib.stream()),
                           'clip_body_records')
        return o
