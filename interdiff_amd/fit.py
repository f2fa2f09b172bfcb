"""The epoch loop that drives a trainer from a ``DeviceClipSet`` or a ``skeleton_dataset.SkeletonClipSet``: what ``DataLoader(shuffle=True, drop_last=True)`` + ``Trainer.fit`` with
``ModelCheckpoint(monitor='val_loss', save_last=True, save_weights_only=True)`` and ``EarlyStopping(monitor='val_loss', min_delta=0)`` do in
train_diffusion_smpl.py:612-651 and train_correction_smpl.py.  Host only.  Lightning is not a dependency and nothing here is pinned against it: the loop
RESTATES those semantics (validation every ``check_val_every_n_epoch`` epochs, lowest value kept as ``best.pt``, the final weights as ``last.pt``, stop after
``patience`` validations without improvement).  The shuffle is a seeded numpy permutation per epoch, not torch's sampler stream.  Learning-rate schedules are
not built (the reference constructs ``ReduceLROnPlateau`` and never returns it from ``configure_optimizers``).  The skeleton half: ``fit`` takes a
``SkeletonWindowIndex`` as it takes a ``ClipIndex`` (train_diffusion_skeleton.py / train_correction_skeleton.py); ``skeleton_denoiser_validate`` /
``skeleton_correction_validate`` are its ``validate``, ``skeleton_evaluate`` is eval_skeleton.py's loop over a test split.
"""
import os
import numpy as np
import torch
from .dataset import draw_starts


def epoch_batches(index, batch_size, rng, drop_last=True):
    """One epoch: a permutation of ``index`` drawn from ``rng``, cut into batches (the last partial one dropped), each with its starts drawn in order ->
    yields (seq_ids, starts, entry positions)."""
    order = rng.permutation(len(index))
    stop = len(order) - (len(order) % batch_size if drop_last else 0)
    for s in range(0, stop, batch_size):
        pos = order[s:s + batch_size]
        drawn = draw_starts([index[int(i)] for i in pos], rng)
        yield [k for k, _ in drawn], [st for _, st in drawn], [int(i) for i in pos]


def fit(trainer, clip_set, index, *, batch_size=32, max_epochs, seed, step=None, validate=None, val_index=None, check_val_every_n_epoch=50, patience=1000,
        ckpt_dir=None, body=True, val_set=None):
    """``max_epochs`` epochs of ``step(trainer, batch, epoch)`` (default ``trainer.training_step(batch)``; ``correction_step`` passes the epoch) over
    ``clip_set.assemble`` batches of ``index`` (a ``ClipIndex`` of the set's sequences).  After every ``check_val_every_n_epoch``-th epoch
    ``validate(trainer, batches) -> float`` runs on the batches of ``val_index`` over ``val_set`` (default: ``clip_set``; an index's ``k`` addresses ITS split's
    sequence list, so a test-split index usually comes with a set of its own) (in order, starts drawn from their own seeded stream, a last partial batch
    kept); ``ckpt_dir`` then holds ``best.pt`` (``trainer.state_dict()`` at the lowest value so far) and ``last.pt`` (at the latest epoch), weights only.
    Returns dict(epochs, steps, val=[(epoch, value)], best=(epoch, value) or None, stopped_early)."""
    if batch_size <= 0 or max_epochs < 0 or check_val_every_n_epoch <= 0:
        raise ValueError('batch_size, check_val_every_n_epoch > 0 and max_epochs >= 0')
    if validate is not None and val_index is None:
        raise ValueError('validate needs val_index')
    step = step or (lambda tr, batch, epoch: tr.training_step(batch))
    rng = np.random.RandomState(seed)
    save = lambda name: torch.save(trainer.state_dict(), os.path.join(ckpt_dir, name)) if ckpt_dir is not None else None
    if ckpt_dir is not None:
        os.makedirs(ckpt_dir, exist_ok=True)
    out = dict(epochs=0, steps=0, val=[], best=None, stopped_early=False)
    wait = 0
    for epoch in range(max_epochs):
        trainer.current_epoch = epoch                                   # (what a LightningModule exposes: the ready validate helpers read it)
        for ids, starts, _ in epoch_batches(index, batch_size, rng):
            step(trainer, clip_set.assemble(ids, starts, body=body), epoch)
            out['steps'] += 1
        out['epochs'] = epoch + 1
        if validate is not None and (epoch + 1) % check_val_every_n_epoch == 0:
            vrng = np.random.RandomState(seed)                          # the same validation clips every time
            drawn = draw_starts(val_index.entries, vrng)
            batches = ((val_set or clip_set).assemble([k for k, _ in drawn[s:s + batch_size]], [st for _, st in drawn[s:s + batch_size]], body=body)
                       for s in range(0, len(drawn), batch_size))
            value = float(validate(trainer, batches))
            out['val'].append((epoch, value))
            if out['best'] is None or value < out['best'][1]:
                out['best'], wait = (epoch, value), 0
                save('best.pt')
            else:
                wait += 1
            save('last.pt')
            if wait >= patience:
                out['stopped_early'] = True
                break
    save('last.pt')
    return out


def correction_step(trainer, batch, epoch):
    """The ``step`` of the correction trainers: ``training_step(batch, current_epoch=epoch)`` (initialisation below epoch 10, annealed geometry terms)."""
    return trainer.training_step(batch, current_epoch=epoch)


def denoiser_validate(diffusion, past_len=10, seed=0, **loop_kw):
    """``validate`` for a ``DenoiserTrainer``: ``export_mdm`` -> ``eval.batch_from_raw`` -> ``losses.validation_step`` (one full sample per batch, scored by the
    16-term val_loss), the clip-weighted mean over the batches.  ``diffusion`` / ``loop_kw``: what ``validation_step`` hands the sample loop (a respaced
    ``diffusion`` keeps it short)."""
    from . import eval as ev, losses

    def validate(trainer, batches):
        model = trainer.export_mdm()
        total, clips = 0.0, 0
        for batch in batches:
            B = batch['gt'].shape[0]
            total += B * float(losses.validation_step(model, diffusion, ev.batch_from_raw(model, batch, past_len), past_len, seed=seed, **loop_kw)[0])
            clips += B
        return total / max(clips, 1)
    return validate


def correction_validate():
    """``validate`` for the correction trainers: ``correction_losses.validation_step(trainer.predictor, batch, epoch)``, the clip-weighted mean; the epoch (it
    decides ``initialize`` and the annealing of the geometry terms) is the ``trainer.current_epoch`` that ``fit`` maintains."""
    from . import correction_losses

    def validate(trainer, batches):
        total, clips = 0.0, 0
        epoch = getattr(trainer, 'current_epoch', 0)
        for batch in batches:
            B = batch['gt'].shape[0]
            total += B * float(correction_losses.validation_step(trainer.predictor, batch, epoch)[0])
            clips += B
        return total / max(clips, 1)
    return validate


def skeleton_denoiser_validate(diffusion, past_len=10, seed=0, **loop_kw):
    """``validate`` for a ``SkeletonDenoiserTrainer`` over a ``skeleton_dataset.SkeletonClipSet``: ``export_mdm`` -> ``skeleton_losses.validation_step`` (one full
    sample per batch, scored by the 13-term val_loss), the clip-weighted mean over the batches.  ``diffusion`` / ``loop_kw`` as in ``denoiser_validate``."""
    from . import skeleton_losses

    def validate(trainer, batches):
        model = trainer.export_mdm()
        total, clips = 0.0, 0
        for batch in batches:
            B = batch[0].shape[0]
            total += B * float(skeleton_losses.validation_step(model, diffusion, batch, past_len, seed=seed, **loop_kw)[0])
            clips += B
        return total / max(clips, 1)
    return validate


def skeleton_correction_validate():
    """``validate`` for ``SkeletonTrainer`` / ``SkeletonFineTuner``: ``skeleton.skeleton_validation_step(trainer.predictor, batch)``, the clip-weighted mean."""
    from . import skeleton

    def validate(trainer, batches):
        total, clips = 0.0, 0
        for batch in batches:
            B = batch[0].shape[0]
            total += B * float(skeleton.skeleton_validation_step(trainer.predictor, batch)[0])
            clips += B
        return total / max(clips, 1)
    return validate


def skeleton_evaluate(model, diffusion, obj_model, clip_set, index, batch_size, seed=None, past_len=10, **loop_kw):
    """The loop of eval_skeleton.py:145-165 (``sample(t, dataloader, data_size)``) over the windows of ``index`` (a ``SkeletonWindowIndex`` or a ``subset`` of one)
    in ``clip_set``: batches in index order, the last partial one KEPT (the script's loaders do not drop it); per batch ``skeleton.sample_once_proj`` ->
    ``skeleton.skeleton_metrics``, every metric times the batch's B, summed, divided by ``len(index)``.  ``obj_model=None``: eval_skeleton_no_correction.py.
    ``seed``: the sampler's, the same for every batch.  -> dict(mpjpe_h, mpjpe_o, translation_error, rotation_error)."""
    from . import skeleton
    if batch_size <= 0 or len(index) == 0:
        raise ValueError('batch_size > 0 and a non-empty index')
    entries = [index[i] for i in range(len(index))]
    total = {}
    for s in range(0, len(entries), batch_size):
        part = entries[s:s + batch_size]
        batch = clip_set.assemble([int(k) for k, _, _ in part], [int(r) for _, r, _ in part])
        obj_pred, body_pred, pose_pred, obj_gt, body_gt, pose_gt = skeleton.sample_once_proj(batch, model, diffusion, obj_model, seed=seed, past_len=past_len, **loop_kw)
        metric = skeleton.skeleton_metrics(body_pred, body_gt, obj_pred, obj_gt, pose_pred, pose_gt)
        for k, v in metric.items():
            total[k] = total.get(k, 0.0) + len(part) * v
    return {k: v / len(entries) for k, v in total.items()}
