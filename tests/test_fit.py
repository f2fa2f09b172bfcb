"""interdiff_amd/fit.py on a fake trainer and a fake clip set (no GPU): the epoch loop's batching, shuffling, validation schedule, checkpoints and early stop."""
import os
import numpy as np
import pytest
import torch
from interdiff_amd.dataset import ClipIndex
from interdiff_amd import fit as F


class FakeSet:
    def __init__(self):
        self.calls = []

    def assemble(self, seq_ids, starts, body=True):
        self.calls.append((list(seq_ids), list(starts)))
        return dict(seq_ids=list(seq_ids), starts=list(starts), gt=torch.zeros(len(seq_ids), 1, 144, 4))


class FakeTrainer:
    def __init__(self):
        self.w, self.seen = 0, []

    def training_step(self, batch, current_epoch=None):
        self.w += 1
        self.seen.append((tuple(zip(batch['seq_ids'], batch['starts'])), current_epoch))

    def state_dict(self):
        return {'w': torch.tensor(self.w)}


def index(n_seq=7, F_=80):
    return ClipIndex(['Date01_s%d' % i for i in range(n_seq)], [F_ + 3 * i for i in range(n_seq)], 'train', 10, 25)


def test_epoch_batches_drop_last_and_every_entry_at_most_once():
    idx = index()                                            # 7 sequences x 2 fragments = 14 entries
    assert len(idx) == 14
    tr, cs = FakeTrainer(), FakeSet()
    out = F.fit(tr, cs, idx, batch_size=4, max_epochs=3, seed=11)
    assert out['epochs'] == 3 and out['steps'] == 3 * (14 // 4) == len(cs.calls) and not out['stopped_early'] and out['val'] == []
    assert all(len(ids) == 4 for ids, _ in cs.calls)
    got = [pos for _, _, pos in F.epoch_batches(idx, 4, np.random.RandomState(0))]
    flat = [p for b in got for p in b]
    assert len(got) == 3 and len(flat) == len(set(flat)) == 12 and set(flat) <= set(range(14))
    # a start lies inside its entry's fragment (bias <= fragment), so (sequence, start // fragment) names the entry: none twice in an epoch, all admissible
    for e in range(3):
        clips = [(k, s) for ids, sts in cs.calls[3 * e:3 * e + 3] for k, s in zip(ids, sts)]
        frags = [(k, s // 35) for k, s in clips]
        assert len(frags) == len(set(frags)) == 12 and set(frags) <= {(k, o // 35) for k, o, _ in idx.entries}
        assert all(s + 35 <= idx.frame_counts[k] for k, s in clips)
    assert all(ep is None for _, ep in tr.seen)              # the default step passes no epoch


def test_same_seed_same_order_and_another_seed_another():
    runs = []
    for seed in (5, 5, 6):
        cs = FakeSet()
        F.fit(FakeTrainer(), cs, index(), batch_size=4, max_epochs=2, seed=seed)
        runs.append(cs.calls)
    assert runs[0] == runs[1] and runs[0] != runs[2]
    assert runs[0][:3] != runs[0][3:]                        # the second epoch is shuffled anew


def test_validation_epochs_checkpoints_and_early_stop(tmp_path):
    idx, vidx = index(), ClipIndex(['Date03_a', 'Date03_b'], [80, 40], 'test', 10, 25)
    values = iter([5.0, 3.0, 4.0, 3.0, 3.5, 9.0, 9.0])
    seen = []

    def validate(trainer, batches):
        bs = list(batches)
        seen.append((trainer.w, [b['starts'] for b in bs]))
        return next(values)
    tr, cs = FakeTrainer(), FakeSet()
    d = str(tmp_path / 'ck')
    out = F.fit(tr, cs, idx, batch_size=4, max_epochs=100, seed=3, validate=validate, val_index=vidx, check_val_every_n_epoch=2, patience=3, ckpt_dir=d,
                step=F.correction_step)
    # validation after epochs 1, 3, 5, ... (0-based); values 5 3 4 3 3.5: the best is the FIRST 3.0 (min_delta = 0: an equal value is no improvement), then three
    # validations without improvement stop the run
    assert [e for e, _ in out['val']] == [1, 3, 5, 7, 9] and [v for _, v in out['val']] == [5.0, 3.0, 4.0, 3.0, 3.5]
    assert out['best'] == (3, 3.0) and out['stopped_early'] and out['epochs'] == 10 and out['steps'] == 30
    assert [w for w, _ in seen] == [6, 12, 18, 24, 30]
    assert all(s == [[0, 35, 0]] for _, s in seen)           # 3 test fragments (bias 1: no jitter), one partial batch kept
    assert int(torch.load(os.path.join(d, 'best.pt'))['w']) == 12 and int(torch.load(os.path.join(d, 'last.pt'))['w']) == 30
    assert [ep for _, ep in tr.seen] == [e for e in range(10) for _ in range(3)]      # the correction step receives the epoch
    # no validation: last.pt alone
    d2 = str(tmp_path / 'ck2')
    F.fit(FakeTrainer(), FakeSet(), idx, batch_size=4, max_epochs=1, seed=3, ckpt_dir=d2)
    assert sorted(os.listdir(d2)) == ['last.pt']
    with pytest.raises(ValueError):
        F.fit(FakeTrainer(), FakeSet(), idx, batch_size=4, max_epochs=1, seed=3, validate=validate)
    with pytest.raises(ValueError):
        F.fit(FakeTrainer(), FakeSet(), idx, batch_size=0, max_epochs=1, seed=3)
