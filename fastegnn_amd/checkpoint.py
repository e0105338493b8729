"""Resumable training: one-file checkpoints of everything a run carries from epoch to epoch, and ``fit()``, the counterpart of the
reference's ``train()`` (``utils/train.py:181-226``: the loop every reference entry point calls) over ``train_epoch`` / ``evaluate``.

A checkpoint holds tensors and plain Python values only (``torch.load(weights_only=True)`` reads it) and is replaced atomically, so
a run that is killed while it writes leaves the previous checkpoint behind.  Nothing here launches a kernel of its own: the device
work is ``train_epoch``'s and ``evaluate``'s, the read-backs are theirs plus the ones a checkpoint needs (the optimizer's step counts,
the sampler's and a ``PackedStream``'s words: one small copy each, at an epoch boundary).
"""
from __future__ import annotations

import json
import os
import tempfile
import time
from typing import Optional, Sequence

import torch

from .train import FusedAdam, MMDSampler, evaluate, train_epoch

FORMAT = "fastegnn_amd.checkpoint"
FORMAT_VERSION = 1


def _atomic_write(path, write) -> None:
    """``write(file_name)`` into a temporary file next to ``path`` (same directory: same file system), then ``os.replace``: a reader
    sees the old file or the new one, never a part of either; a writer that fails leaves ``path`` as it was and no temporary file"""
    path = os.fspath(path)
    directory = os.path.dirname(os.path.abspath(path))
    os.makedirs(directory, exist_ok=True)
    fd, tmp = tempfile.mkstemp(dir=directory, prefix=os.path.basename(path) + ".", suffix=".tmp")
    os.close(fd)
    try:
        write(tmp)
        os.replace(tmp, path)
    except BaseException:
        try:
            os.unlink(tmp)
        except OSError:
            pass
        raise


def _loader_state(loader):
    return loader.state_dict() if hasattr(loader, "state_dict") else None


def save_checkpoint(path, model, optimizer, *, sampler: Optional[MMDSampler] = None, loaders: Sequence = (), extra=None) -> None:
    """One file with everything needed to continue a run bit for bit:

    * ``model``: its ``state_dict()``; ``guard``: its RangeGuard's state (the arithmetic build in use), ``None`` for a module without one;
    * ``optimizer``: ``optimizer.state_dict()`` (``FusedAdam``: torch.optim.Adam's layout; capturable: one read-back of the step counts);
    * ``sampler``: ``MMDSampler.state_dict()`` (seed and draw counter) or ``None``;
    * ``loaders``: for every loader given, its ``state_dict()`` -- ``PackedStream``'s ``{seed, epoch, cursor}``, the own generator of a
      ``DataLoader`` / ``PackedLoader`` -- or ``None`` where it has none;
    * ``rng``: torch's CPU generator state (what a loader without a generator of its own shuffles with);
    * ``extra``: the caller's values (``fit``: the epoch index and the logs); tensors and plain Python values only;
    * ``format`` / ``version``.

    Written to a temporary file in the same directory and moved over ``path`` with ``os.replace``.  Not inside a stream capture."""
    guard = getattr(model, "_range", None)
    blob = {
        "format": FORMAT, "version": FORMAT_VERSION,
        "model": model.state_dict(),
        "guard": guard.state_dict() if guard is not None else None,
        "optimizer": optimizer.state_dict(),
        "sampler": sampler.state_dict() if sampler is not None else None,
        "loaders": [_loader_state(ld) for ld in loaders],
        "rng": {"cpu": torch.get_rng_state()},
        "extra": extra,
    }
    _atomic_write(path, lambda tmp: torch.save(blob, tmp))


def load_checkpoint(path, model, optimizer, *, sampler: Optional[MMDSampler] = None, loaders: Sequence = (), map_location=None):
    """The inverse of ``save_checkpoint``: loads INTO the objects given (the same kinds, in the same order, as were saved; nothing is
    rebuilt, the optimizer is written in place) and returns ``extra``.  Read with ``weights_only=True``.  A checkpoint saved with a
    sampler / a loader state needs one to load into, and the reverse: a mismatch is a ``ValueError`` before anything is written."""
    blob = torch.load(path, map_location=map_location, weights_only=True)
    if not isinstance(blob, dict) or blob.get("format") != FORMAT:
        raise ValueError(f"fastegnn_amd.load_checkpoint: {path} is not a checkpoint of save_checkpoint")
    if blob.get("version") != FORMAT_VERSION:
        raise ValueError(f"fastegnn_amd.load_checkpoint: {path} has format version {blob.get('version')}, this code reads {FORMAT_VERSION}")
    if (blob["sampler"] is None) != (sampler is None):
        raise ValueError(f"fastegnn_amd.load_checkpoint: the checkpoint was saved {'without' if blob['sampler'] is None else 'with'} an "
                         f"MMD sampler, the call has {'none' if sampler is None else 'one'}")
    loaders = list(loaders)
    if len(blob["loaders"]) != len(loaders):
        raise ValueError(f"fastegnn_amd.load_checkpoint: the checkpoint holds {len(blob['loaders'])} loader states, the call has "
                         f"{len(loaders)} loaders")
    for i, (state, ld) in enumerate(zip(blob["loaders"], loaders)):
        if (state is None) != (not hasattr(ld, "load_state_dict")):
            raise ValueError(f"fastegnn_amd.load_checkpoint: loader {i} was saved {'without' if state is None else 'with'} a state, the "
                             f"loader given {'takes one' if state is None else 'takes none'}")
    model.load_state_dict(blob["model"])
    guard = getattr(model, "_range", None)
    if guard is not None and blob["guard"] is not None:
        guard.load_state_dict(blob["guard"])
    optimizer.load_state_dict(blob["optimizer"])
    if sampler is not None:
        sampler.load_state_dict(blob["sampler"])
    for state, ld in zip(blob["loaders"], loaders):
        if state is not None:
            ld.load_state_dict(state)
    torch.set_rng_state(blob["rng"]["cpu"].cpu())
    return blob["extra"]


def _write_log(log_path, best_log_dict, log_dict) -> None:
    def write(tmp):
        with open(tmp, "w") as out:
            out.write(json.dumps([best_log_dict, log_dict], indent=4))
    _atomic_write(log_path, write)


def fit(model, optimizer: FusedAdam, loader_train, loader_valid, loader_test, sigma, weight, *, max_epochs: int,
        sampler: Optional[MMDSampler] = None, num_sample: Optional[int] = None, early_stop=float("inf"), test_interval: int = 5,
        log_path=None, best_path=None, checkpoint_path=None, checkpoint_interval: int = 1, resume: bool = False):
    """The reference's ``train()`` (utils/train.py:181-226) -> ``(best_log_dict, log_dict)``, for epochs ``1 .. max_epochs`` (the reference
    counts to 10^6 and relies on ``early_stop``):

    * every epoch: ``train_epoch`` (with ``sampler`` / ``num_sample``); its ``mse`` -- the reference logs the MSE before it adds the MMD term
      (train.py:107) -- is appended to ``log_dict['loss_train']``;
    * every ``test_interval`` epochs: ``evaluate`` on ``loader_valid`` and ``loader_test`` (forward-only, no MMD term: the reference
      computes it in these epochs and throws it away); the epoch goes to ``log_dict['epochs']``, the test MSE to ``log_dict['loss']``;
      a validation MSE STRICTLY below the best so far makes ``best_log_dict = {epoch_index, loss_valid, loss_test, loss_train}`` and,
      with ``best_path``, saves ``model.state_dict()`` there; then ``epoch_index - best_log_dict['epoch_index'] >= early_stop`` ends
      the run with ``best_log_dict['early_stop'] = epoch_index``;
    * after every epoch ``best_log_dict['time_cost']`` is the run's seconds so far and, with ``log_path``, ``[best_log_dict, log_dict]`` is
      rewritten as JSON (indent 4, the reference's keys).  The reference leaves its loop before these two lines on the epoch that stops
      early; here that epoch writes them too, so that the file names the stop.

    ``checkpoint_path``: ``save_checkpoint`` (model, guard, optimizer, sampler, the three loaders, torch's RNG, the epoch and both logs)
    after every ``checkpoint_interval``-th epoch and after the last one.  ``resume=True`` with an existing file loads it into the objects
    given and continues with the next epoch -- the same bits as the uninterrupted run where the model runs in its ordered mode
    (``deterministic = True``); ``time_cost`` continues from the saved seconds.  Without a file the run starts at epoch 1.

    Host synchronisations per epoch: the one read-back of ``train_epoch``, one per ``evaluate``, and at a checkpoint the optimizer's step
    counts (capturable mode), the sampler's and a ``PackedStream``'s words and the copy of the tensors into the file."""
    if int(max_epochs) < 0 or int(test_interval) < 1 or int(checkpoint_interval) < 1:
        raise ValueError("fastegnn_amd.fit: max_epochs >= 0, test_interval >= 1 and checkpoint_interval >= 1")
    if sampler is not None and num_sample is None:
        raise ValueError("fastegnn_amd.fit: a sampler needs num_sample (the reference's sample * C)")
    max_epochs, test_interval, checkpoint_interval = int(max_epochs), int(test_interval), int(checkpoint_interval)
    log_dict = {"epochs": [], "loss": [], "loss_train": []}
    best_log_dict = {"epoch_index": 0, "loss_valid": 1e8, "loss_test": 1e8, "loss_train": 1e8}
    loaders = (loader_train, loader_valid, loader_test)
    first, seconds_before = 1, 0.0
    if resume and checkpoint_path is not None and os.path.exists(checkpoint_path):
        extra = load_checkpoint(checkpoint_path, model, optimizer, sampler=sampler, loaders=loaders)
        first, seconds_before = int(extra["epoch_index"]) + 1, float(extra["time_cost"])
        best_log_dict, log_dict = dict(extra["best_log_dict"]), {k: list(v) for k, v in extra["log_dict"].items()}
        if extra["stopped"]:
            return best_log_dict, log_dict

    def checkpoint(epoch_index, stopped):
        extra = {"epoch_index": epoch_index, "best_log_dict": dict(best_log_dict), "log_dict": {k: list(v) for k, v in log_dict.items()},
                 "time_cost": best_log_dict.get("time_cost", seconds_before), "stopped": bool(stopped)}
        save_checkpoint(checkpoint_path, model, optimizer, sampler=sampler, loaders=loaders, extra=extra)

    start = time.perf_counter()
    for epoch_index in range(first, max_epochs + 1):
        loss_train = train_epoch(model, optimizer, loader_train, sigma, weight, sampler=sampler, num_sample=num_sample)["mse"]
        log_dict["loss_train"].append(loss_train)
        stopped = False
        if epoch_index % test_interval == 0:
            loss_valid = evaluate(model, loader_valid, sigma, weight)["mse"]
            loss_test = evaluate(model, loader_test, sigma, weight)["mse"]
            log_dict["epochs"].append(epoch_index)
            log_dict["loss"].append(loss_test)
            if loss_valid < best_log_dict["loss_valid"]:
                best_log_dict = {"epoch_index": epoch_index, "loss_valid": loss_valid, "loss_test": loss_test, "loss_train": loss_train}
                if best_path is not None:
                    state = model.state_dict()
                    _atomic_write(best_path, lambda tmp: torch.save(state, tmp))
            if epoch_index - best_log_dict["epoch_index"] >= early_stop:
                best_log_dict["early_stop"] = epoch_index
                stopped = True
        best_log_dict["time_cost"] = seconds_before + (time.perf_counter() - start)
        if log_path is not None:
            _write_log(log_path, best_log_dict, log_dict)
        if checkpoint_path is not None and (stopped or epoch_index == max_epochs or epoch_index % checkpoint_interval == 0):
            checkpoint(epoch_index, stopped)
        if stopped:
            break
    return best_log_dict, log_dict
