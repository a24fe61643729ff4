"""Checkpoints in Lightning 2.x's file layout, and the two callbacks the reference hands `pl.Trainer` next to them.

    save_checkpoint(path, model, optimizer=None, scheduler=None, extra=None)     load_checkpoint(path, map_location="cpu")
    ModelCheckpoint(dirpath, filename=None, monitor=None, mode="min", save_top_k=1, save_last=False, every_n_epochs=1)
    EarlyStopping(monitor, mode="min", patience=3, min_delta=0.0, check_finite=True)
    WeightAveraging(avg="ema", decay=0.999, update_on="step", ...)              an EMA / SWA of the weights (optim.AveragedWeights)
    trainer.Trainer(callbacks=[...]).fit(model, train, val, ckpt_path=...)      Trainer.save_checkpoint(path)

The file is a `torch.save` of ONE plain dict with the top-level keys `epoch`, `global_step`, `pytorch-lightning_version`,
`state_dict`, `optimizer_states`, `lr_schedulers`, `callbacks` -- so the reference's `load_model`
(`torch.load(path)["state_dict"]`) reads ours and we read the reference's -- plus `msn` for what is ours alone: the
Trainer's `history` lists, the RNG states of every rank and the world size.  It holds tensors (on the CPU) and Python
primitives / containers only and loads with `torch.load(path, weights_only=True)`.  Keys we do not know in a file we load
(Lightning's `loops`, `hparams_name`, `hyper_parameters`, ...) are ignored.

The write is atomic: a temporary file in the target's directory, then `os.replace`.  A write that fails or is killed
leaves the previous file as it was, and a write that fails leaves no temporary file.

What resumes exactly (`Trainer.fit(ckpt_path=...)`, tests/test_checkpoint_gpu.py):

  * eager steps resume BITWISE, dropout included: parameters, buffers, RAdam moments and step counts, scheduler, history
    and the RNG streams (torch's CPU generator -- dropout seeds through `ops.new_seed`, a DataLoader's shuffle and base
    seeds --, the training device's generator -- `augment.py` --, Python's `random` -- the masks of the pretraining
    model -- and numpy's) are those of the uninterrupted run;
  * graph-replayed steps (`graphed_steps=True`) with dropout 0 resume to the closeness the project demands between
    graphed and eager steps (tests/test_grad_clip_gpu.py: rtol 1e-5, atol 1e-7): the warm-up steps of the resumed fit
    are real eager steps and `RAdam.graph_prepare` seeds the device step counter from the loaded (int) step counts;
  * graph-replayed steps with dropout > 0 draw a new seed base at the new capture: the masks after a resume are not those
    of the uninterrupted run -- the same distribution, not the same bits.

Gradient accumulation (`Trainer(accumulate_grad_batches=k)`): checkpoints are written at epoch ends, where the last batch has
always closed its window and the optimizer has stepped, so NO accumulator state goes into the file; `global_step` counts
optimizer steps, and a resumed run with the same k is bitwise the uninterrupted one (tests/test_grad_accum_gpu.py).
Mid-epoch checkpoints -- which would have to carry an open window's partial sums -- are not built.

Weight averaging (`WeightAveraging`): `state_dict` stays the LIVE model's -- `Trainer.save_checkpoint` swaps the live weights back in
around the write if the model holds its average just then -- and the average travels in `callbacks["WeightAveraging"]`
(tensors by parameter name, the number of updates); a resumed eager run continues the average bitwise.

Several ranks: `save_checkpoint` is a collective (every rank calls it; the RNG states are gathered with
`all_gather_object`), rank 0 alone writes, and a barrier follows.  On resume rank r takes entry r of the saved RNG
states; if the world size differs from the saved one the RNG is left as it is, with a warning, and all else loads.
"""
import copy
import math
import os
import random
import re
import tempfile
import warnings

import numpy as np
import torch
import torch.distributed as dist

LIGHTNING_VERSION = "2.0.0"       # the layout written here; a string, as Lightning's own


# ------------------------------------------------------------------------------------------------- the file
def _plain(obj, where="checkpoint"):
    """A copy of `obj` made of CPU tensors and Python primitives / dicts / lists / tuples only (what
    torch.load(weights_only=True) accepts); anything else is an error here rather than a file that cannot be read."""
    if torch.is_tensor(obj):
        return obj.detach().to("cpu", copy=True).contiguous()
    if obj is None or isinstance(obj, (bool, int, float, str)):
        return obj
    if isinstance(obj, (np.integer, np.floating, np.bool_)):
        return obj.item()
    if isinstance(obj, dict):
        return {_plain(k, where): _plain(v, f"{where}[{k!r}]") for k, v in obj.items()}
    if isinstance(obj, tuple):
        return tuple(_plain(v, where) for v in obj)
    if isinstance(obj, list):
        return [_plain(v, where) for v in obj]
    raise TypeError(f"{where}: a {type(obj).__name__} cannot be stored in a checkpoint (tensors and Python primitives, dicts, "
                    "lists and tuples only)")


def _int_steps(opt_state):
    """Every per-parameter `step` of an optimizer state dict as a Python int, in place (int, CPU tensor or CUDA tensor)."""
    for st in opt_state.get("state", {}).values():
        if isinstance(st, dict) and "step" in st:
            st["step"] = int(st["step"])
    return opt_state


def atomic_save(obj, path):
    """torch.save(obj) to a temporary file beside `path`, then os.replace: `path` is either the old file or the new one."""
    path = os.fspath(path)
    folder = os.path.dirname(os.path.abspath(path))
    os.makedirs(folder, exist_ok=True)
    fd, tmp = tempfile.mkstemp(dir=folder, prefix="." + os.path.basename(path) + ".", suffix=".tmp")
    try:
        with os.fdopen(fd, "wb") as f:
            torch.save(obj, f)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
    except BaseException:
        try:
            os.remove(tmp)
        except OSError:
            pass
        raise


def _world(group):
    return dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1


def _rank(group):
    return dist.get_rank(group) if dist.is_available() and dist.is_initialized() else 0


def _model_device(model):
    for t in model.parameters():
        return t.device
    return torch.device("cpu")


def rng_state(device=None):
    """The RNG streams of this process as tensors and primitives: torch's CPU generator, the generator of `device` (a
    CUDA device; None on the CPU), Python's `random` and numpy's global state."""
    name, keys, pos, has_gauss, cached = np.random.get_state()
    dev = None
    if device is not None and torch.device(device).type == "cuda":
        dev = torch.cuda.get_rng_state(torch.device(device))
    return {"torch_cpu": torch.get_rng_state(), "torch_device": dev, "python": random.getstate(),
            "numpy": {"name": str(name), "keys": torch.from_numpy(keys.astype(np.int64)), "pos": int(pos),
                      "has_gauss": int(has_gauss), "cached_gaussian": float(cached)}}


def set_rng_state(state, device=None):
    torch.set_rng_state(state["torch_cpu"].cpu())
    if state.get("torch_device") is not None and device is not None and torch.device(device).type == "cuda":
        torch.cuda.set_rng_state(state["torch_device"].cpu(), torch.device(device))
    version, words, gauss = state["python"]
    random.setstate((version, tuple(words), gauss))
    n = state["numpy"]
    np.random.set_state((n["name"], n["keys"].cpu().numpy().astype(np.uint32), n["pos"], n["has_gauss"], n["cached_gaussian"]))


def save_checkpoint(path, model, optimizer=None, scheduler=None, extra=None, *, group=None, device=None):
    """Write `path` in the layout of the module docstring.  `extra`: {"epoch": int, "global_step": int, "callbacks":
    {state key: state dict}} fill the top-level keys of those names (0, 0, {} without them); every other entry of
    `extra` (the Trainer passes "history") goes under "msn" beside the RNG states and the world size.  `device`: whose
    generator to save (default: where the model's parameters live).  With several ranks every rank must call it."""
    extra = dict(extra or {})
    device = _model_device(model) if device is None else torch.device(device)
    world, rank = _world(group), _rank(group)
    rng = _plain(rng_state(device), "rng")
    if world > 1:
        states = [None] * world
        dist.all_gather_object(states, rng, group=group)
    else:
        states = [rng]
    try:
        if rank == 0:
            ckpt = {
                "epoch": int(extra.pop("epoch", 0)),
                "global_step": int(extra.pop("global_step", 0)),
                "pytorch-lightning_version": LIGHTNING_VERSION,
                "state_dict": _plain(dict(model.state_dict()), "state_dict"),
                "optimizer_states": [] if optimizer is None else [_int_steps(_plain(optimizer.state_dict(), "optimizer_states"))],
                "lr_schedulers": [] if scheduler is None else [_plain(scheduler.state_dict(), "lr_schedulers")],
                "callbacks": _plain(extra.pop("callbacks", {}), "callbacks"),
            }
            ckpt["msn"] = dict(_plain(extra, "extra"), rng=states, world_size=world)
            atomic_save(ckpt, path)
    finally:
        if world > 1:
            dist.barrier(group)      # no rank goes on (to read, or to delete an older file) before the file stands
    return path


def load_checkpoint(path, map_location="cpu"):
    """The dict of a checkpoint file -- ours or Lightning's -- read with weights_only=True: the keys of the layout (absent
    ones at their empty values; `msn` None in a file that is not ours), unknown keys dropped, every optimizer `step` a
    Python int."""
    raw = torch.load(path, map_location=map_location, weights_only=True)
    if not isinstance(raw, dict) or "state_dict" not in raw:
        raise ValueError(f"{path}: not a checkpoint (a dict with a 'state_dict' is expected)")
    ckpt = {"epoch": int(raw.get("epoch", -1)), "global_step": int(raw.get("global_step", 0)),
            "pytorch-lightning_version": str(raw.get("pytorch-lightning_version", "")), "state_dict": raw["state_dict"],
            "optimizer_states": [_int_steps(s) for s in raw.get("optimizer_states", [])],
            "lr_schedulers": list(raw.get("lr_schedulers", [])), "callbacks": dict(raw.get("callbacks", {}) or {}),
            "msn": raw.get("msn")}
    return ckpt


def restore_rng(ckpt, device=None, group=None):
    """Entry `rank` of the saved RNG states; untouched (with a warning) if the file was written by another world size."""
    msn = ckpt.get("msn")
    if not msn or not msn.get("rng"):
        return False
    world, rank = _world(group), _rank(group)
    if int(msn.get("world_size", len(msn["rng"]))) != world:
        warnings.warn(f"checkpoint written by {msn.get('world_size')} rank(s), resumed by {world}: the RNG states are not "
                      "restored (everything else is)")
        return False
    set_rng_state(msn["rng"][rank], device)
    return True


# ------------------------------------------------------------------------------------------------ callbacks
def _ranked(value, mode):
    """The value as it is ranked: a non-finite one (NaN, +-inf) is the worst there is."""
    value = float(value)
    if not math.isfinite(value):
        return math.inf if mode == "min" else -math.inf
    return value


def _check_mode(mode):
    if mode not in ("min", "max"):
        raise ValueError(f"mode must be 'min' or 'max' (got {mode!r})")
    return mode


class Callback:
    """What trainer.Trainer calls: on_epoch_end(trainer) once per epoch after validation (after the training epoch without
    a validation loader) and the scheduler step; on_resume(trainer) after load_state_dict in fit(ckpt_path=...).  A
    callback reads `trainer.current_epoch`, `trainer.global_step`, `trainer.monitored(name)` (rank 0's value on every
    rank), `trainer.is_global_zero`, and calls `trainer.save_checkpoint(path)` (a collective) / `trainer.barrier()`."""

    @property
    def state_key(self):
        return type(self).__name__

    def on_epoch_end(self, trainer):
        pass

    def on_resume(self, trainer):
        pass

    # The hooks below are no-ops unless a callback overrides them (WeightAveraging does).  Per fit: on_fit_start (the model is on
    # its device; before a checkpoint is loaded into it) ... on_fit_end (also after early stopping); per optimizer step:
    # on_optimizer_step, after optimizer.step() and the increment of trainer.global_step, eager or replayed; per epoch:
    # on_train_epoch_end (before the scheduler step and validation), on_validation_start / on_validation_end around the validation
    # epoch -- inside fit and in Trainer.validate.
    def on_fit_start(self, trainer):
        pass

    def on_optimizer_step(self, trainer):
        pass

    def on_train_epoch_end(self, trainer):
        pass

    def on_validation_start(self, trainer):
        pass

    def on_validation_end(self, trainer):
        pass

    def on_fit_end(self, trainer):
        pass

    def state_dict(self):
        return {}

    def load_state_dict(self, state):
        pass


class ModelCheckpoint(Callback):
    """pl.callbacks.ModelCheckpoint for epoch-end saves.  `monitor=None`: the latest file only (save_top_k 1), every file
    (-1) or none (0).  With a monitor: the `save_top_k` best files by `mode`, a file that falls out of them is deleted; a
    value equal to the k-th best does not replace it (Lightning's strict comparison) and a non-finite value ranks worst.
    `filename` is a template over {epoch}, {step} and monitored names, each with an optional format spec and written
    `name=value` as Lightning does ("{epoch}-{val_loss:.3f}" -> "epoch=2-val_loss=0.123.ckpt").  `save_last=True` also
    writes `last.ckpt` at every save -- a regular file, never a link."""

    def __init__(self, dirpath, filename=None, monitor=None, mode="min", save_top_k=1, save_last=False, every_n_epochs=1):
        self.dirpath = os.fspath(dirpath)
        self.filename = filename if filename is not None else "{epoch}-{step}"
        self.monitor, self.mode = monitor, _check_mode(mode)
        self.save_top_k, self.save_last, self.every_n_epochs = int(save_top_k), bool(save_last), int(every_n_epochs)
        if self.save_top_k < -1:
            raise ValueError(f"save_top_k must be -1, 0 or a positive count (got {save_top_k})")
        if monitor is None and self.save_top_k not in (-1, 0, 1):
            raise ValueError(f"ModelCheckpoint(save_top_k={save_top_k}, monitor=None): without a monitor save_top_k is -1, 0 or 1")
        if self.every_n_epochs < 0:
            raise ValueError(f"every_n_epochs must not be negative (got {every_n_epochs})")
        self.best_k_models = {}            # path -> score as ranked
        self.kth_best_model_path = ""
        self.best_model_path, self.best_model_score = "", None
        self.last_model_path = ""

    @property
    def state_key(self):
        return f"ModelCheckpoint{{'monitor': {self.monitor!r}, 'mode': {self.mode!r}, 'every_n_epochs': {self.every_n_epochs}}}"

    def format_checkpoint_name(self, epoch, step, metrics=None):
        values = dict(metrics or {}, epoch=int(epoch), step=int(step))

        def field(m):
            name, spec = m.group(1), (m.group(2) or ":")[1:]
            return f"{name}={format(values.get(name, 0), spec)}"

        return os.path.join(self.dirpath, re.sub(r"\{([^{}:]+)(:[^{}]*)?\}", field, self.filename) + ".ckpt")

    def _template_names(self):
        return [n for n in re.findall(r"\{([^{}:]+)(?::[^{}]*)?\}", self.filename) if n not in ("epoch", "step")]

    def _remove(self, trainer, path):
        if trainer.is_global_zero and path and os.path.exists(path):
            os.remove(path)

    def on_epoch_end(self, trainer):
        epoch = trainer.current_epoch
        if self.every_n_epochs < 1 or (epoch + 1) % self.every_n_epochs != 0:
            return
        metrics = {n: trainer.monitored(n) for n in dict.fromkeys(self._template_names() + ([self.monitor] if self.monitor else []))}
        path = self.format_checkpoint_name(epoch, trainer.global_step, metrics)
        drop, save = None, False
        if self.monitor is None:
            if self.save_top_k != 0:
                save = True
                if self.save_top_k == 1 and self.best_model_path and self.best_model_path != path:
                    drop = self.best_model_path
                self.best_model_path = path
        elif self.save_top_k != 0:
            score = _ranked(metrics[self.monitor], self.mode)
            worse = (lambda a, b: a > b) if self.mode == "min" else (lambda a, b: a < b)
            self.best_k_models.pop(path, None)          # a file of this name is overwritten (one below k: never "full")
            full = self.save_top_k != -1 and len(self.best_k_models) >= self.save_top_k
            if not full or worse(self.best_k_models[self.kth_best_model_path], score):
                save = True
                if full:
                    drop = self.kth_best_model_path
                    del self.best_k_models[drop]
                self.best_k_models[path] = score
            if self.best_k_models:
                # as Lightning: the earliest of equal scores is both the best and the next to go
                lowest = min(self.best_k_models, key=self.best_k_models.get)
                highest = max(self.best_k_models, key=self.best_k_models.get)
                self.best_model_path, self.kth_best_model_path = (lowest, highest) if self.mode == "min" else (highest, lowest)
                self.best_model_score = self.best_k_models[self.best_model_path]
        last = os.path.join(self.dirpath, "last.ckpt") if self.save_last else None
        if last:
            self.last_model_path = last
        if save:
            trainer.save_checkpoint(path)
        if last:
            trainer.save_checkpoint(last)
        if drop and drop != path:
            self._remove(trainer, drop)
        trainer.barrier()

    def state_dict(self):
        return {"monitor": self.monitor, "best_model_score": self.best_model_score, "best_model_path": self.best_model_path,
                "best_k_models": dict(self.best_k_models), "kth_best_model_path": self.kth_best_model_path,
                "last_model_path": self.last_model_path, "dirpath": self.dirpath}

    def load_state_dict(self, state):
        if os.path.abspath(state.get("dirpath", self.dirpath)) != os.path.abspath(self.dirpath):
            warnings.warn(f"ModelCheckpoint: the checkpoint was written under {state.get('dirpath')!r}, this run writes under "
                          f"{self.dirpath!r}: best_k_models of the earlier run are not tracked here")
            return
        self.best_model_score, self.best_model_path = state["best_model_score"], state["best_model_path"]
        self.best_k_models = dict(state["best_k_models"])
        self.kth_best_model_path, self.last_model_path = state["kth_best_model_path"], state["last_model_path"]


class EarlyStopping(Callback):
    """pl.callbacks.EarlyStopping at epoch end: the monitored value improves if it beats the best so far by more than
    `min_delta`; `patience` epochs in a row without improvement set `trainer.should_stop`; a non-finite value stops at
    once under `check_finite`.  The state dict holds the wait count, so a resumed run goes on counting -- and a run
    resumed from the checkpoint of its stopping epoch stops again before it trains."""

    def __init__(self, monitor, mode="min", patience=3, min_delta=0.0, check_finite=True):
        self.monitor, self.mode = monitor, _check_mode(mode)
        self.patience, self.check_finite = int(patience), bool(check_finite)
        self.min_delta = abs(float(min_delta))
        self.wait_count, self.stopped_epoch = 0, 0
        self.best_score = math.inf if mode == "min" else -math.inf
        self.stopped = False

    @property
    def state_key(self):
        return f"EarlyStopping{{'monitor': {self.monitor!r}, 'mode': {self.mode!r}}}"

    def on_epoch_end(self, trainer):
        current = float(trainer.monitored(self.monitor))
        if self.check_finite and not math.isfinite(current):
            self.stopped = True
        else:
            improved = current + self.min_delta < self.best_score if self.mode == "min" else current - self.min_delta > self.best_score
            if improved:
                self.best_score, self.wait_count = current, 0
            else:
                self.wait_count += 1
                self.stopped = self.wait_count >= self.patience
        if self.stopped:
            self.stopped_epoch = trainer.current_epoch
            trainer.should_stop = True

    def on_resume(self, trainer):
        if self.stopped:
            trainer.should_stop = True

    def state_dict(self):
        return {"wait_count": self.wait_count, "stopped_epoch": self.stopped_epoch, "best_score": self.best_score,
                "patience": self.patience, "stopped": self.stopped}

    def load_state_dict(self, state):
        self.wait_count, self.stopped_epoch = int(state["wait_count"]), int(state["stopped_epoch"])
        self.best_score = float(state["best_score"])
        self.stopped = bool(state.get("stopped", self.wait_count >= self.patience))


def averaging_due(global_step, start_step=0, every_n_steps=1):
    """WeightAveraging(update_on="step")'s rule: the average is updated after optimizer step number `global_step` (1-based: the
    Trainer's global_step after its increment) when it lies behind `start_step` and on the every_n_steps grid counted from it."""
    return global_step > start_step and (global_step - start_step) % every_n_steps == 0


def _one_weight_averaging(callbacks):
    found = [cb for cb in callbacks if isinstance(cb, WeightAveraging)]
    if len(found) > 1:
        raise ValueError(f"callbacks hold {len(found)} WeightAveraging callbacks: one model has one average (they would swap the "
                         "same weights twice for validation and share one key in the checkpoint)")
    return found[0] if found else None


class WeightAveraging(Callback):
    """An average of the weights over training, modelled on Lightning's WeightAveraging / StochasticWeightAveraging callbacks
    and torch's AveragedModel; the arithmetic and the memory are optim.AveragedWeights' (one HIP launch per update).

      avg="ema" | "swa", decay    what is averaged (AveragedWeights)
      update_on="step"            after optimizer step s (= trainer.global_step after its increment) when averaging_due(s,
                                  start_step, every_n_steps); with accumulate_grad_batches=k that is at window boundaries only.
                                  Under graphed_steps the update is the last launch of the recorded optimizer part and the rule
                                  acts through the average's device word `active`
      update_on="epoch"           one (eager) update at the end of every training epoch >= start_epoch, before the scheduler
                                  step and validation: classic SWA with avg="swa" (no SWALR annealing: the user's own scheduler)
      use_buffers                 also average BatchNorm's running statistics (AveragedWeights)
      validate_with_average       with an average in hand (n_averaged > 0) the weights are swapped in for every validation
                                  epoch and swapped back after it, bit for bit: ModelCheckpoint / EarlyStopping monitor the
                                  averaged weights' val_loss / AUC_val
      apply_at_end                at the end of fit (early stopping included) one swap: the model holds the averaged weights,
                                  `averager.swapped` is True, restore_live(trainer) undoes it; a later fit swaps back first

    Checkpoints: `state_dict` stays the LIVE model's, so a resume stays what it is; the average travels in
    callbacks[state_key] and on_resume puts it back.  load_average(model, ckpt) loads a file's averaged weights for inference.
    Data parallel: no collective -- after the gradient all-reduce every rank steps to identical parameters, hence to identical
    averages; rank 0 writes them.  Not built: SWALR, a timm-style decay warm-up, mid-epoch checkpoints."""

    def __init__(self, avg="ema", decay=0.999, update_on="step", start_step=0, every_n_steps=1, start_epoch=0, use_buffers=False,
                 validate_with_average=True, apply_at_end=True):
        from . import optim
        self.avg, self.decay = optim._avg_config(avg, decay)
        if update_on not in ("step", "epoch"):
            raise ValueError(f"update_on must be 'step' or 'epoch' (got {update_on!r})")
        for name, v, low in (("start_step", start_step, 0), ("every_n_steps", every_n_steps, 1), ("start_epoch", start_epoch, 0)):
            if isinstance(v, bool) or not isinstance(v, int) or v < low:
                raise ValueError(f"{name} must be an int >= {low} (got {v!r})")
        self.update_on, self.start_step, self.every_n_steps, self.start_epoch = update_on, start_step, every_n_steps, start_epoch
        self.use_buffers, self.validate_with_average, self.apply_at_end = bool(use_buffers), bool(validate_with_average), bool(apply_at_end)
        self.averager = None              # optim.AveragedWeights of the model being fitted (built in on_fit_start)
        self._model = None
        self._pending = None              # a state loaded before the averager exists
        self._swapped_for_validation = False

    def due(self, global_step):
        return averaging_due(global_step, self.start_step, self.every_n_steps)

    @property
    def in_graph(self):
        """Whether a graph-replayed step records the update itself (then on_optimizer_step launches nothing)."""
        return self.update_on == "step"

    def on_fit_start(self, trainer):
        from . import optim
        if self.averager is None or self._model is not trainer.model:
            self.averager = optim.AveragedWeights(trainer.model, avg=self.avg, decay=self.decay, use_buffers=self.use_buffers)
            self._model = trainer.model
            if self._pending is not None:
                self.averager.load_state_dict(self._pending)
                self._pending = None
        else:
            self.averager.graph_prepare()     # the same model again: look once more where its weights live
        if self.averager.swapped:         # an earlier fit applied the average at its end: training goes on from the live weights
            self.averager.swap()

    def on_optimizer_step(self, trainer):
        if self.update_on != "step" or trainer.graphed_step is not None:
            return                        # a graphed step averages inside its recording (and in its own eager calls)
        if self.due(trainer.global_step):
            self.averager.set_active(True)        # a graphed fit before this one may have left the device word off
            self.averager.update()

    def on_train_epoch_end(self, trainer):
        if self.update_on == "epoch" and trainer.current_epoch >= self.start_epoch:
            self.averager.set_active(True)
            self.averager.update()

    def _holds(self, trainer):
        return self.averager is not None and self._model is trainer.model

    def on_validation_start(self, trainer):
        if self.validate_with_average and self._holds(trainer) and self.averager.n_averaged > 0 and not self.averager.swapped:
            self.averager.swap()
            self._swapped_for_validation = True

    def on_validation_end(self, trainer):
        if self._swapped_for_validation:
            self.averager.swap()
            self._swapped_for_validation = False

    def on_fit_end(self, trainer):
        if self.apply_at_end and self.averager.n_averaged > 0 and not self.averager.swapped:
            self.averager.swap()

    def restore_live(self, trainer=None):
        """Undo apply_at_end: the model holds the live weights of the last step again, bit for bit."""
        if self.averager is not None and self.averager.swapped:
            self.averager.swap()

    def on_resume(self, trainer):
        if self.averager is not None and self.averager.swapped:
            self.averager.swap()          # the file's state_dict held the averages and the buffer the live values

    def state_dict(self):
        inner = self.averager.state_dict() if self.averager is not None else self._pending
        return {"avg": self.avg, "decay": self.decay, "update_on": self.update_on, "start_step": self.start_step,
                "every_n_steps": self.every_n_steps, "start_epoch": self.start_epoch, "use_buffers": self.use_buffers,
                "average": inner}

    def load_state_dict(self, state):
        if state.get("avg", self.avg) != self.avg:
            raise ValueError(f"WeightAveraging: the checkpoint's average was made with avg={state['avg']!r}, this callback "
                             f"averages with avg={self.avg!r}")
        inner = state.get("average")
        if inner is None:
            return
        if self.averager is not None:
            self.averager.load_state_dict(inner)
        else:
            self._pending = inner

    @staticmethod
    def load_average(model, ckpt, map_location="cpu"):
        """The averaged weights of a checkpoint (a path, or the dict load_checkpoint returned) into `model`: its state_dict, then
        every averaged tensor over it.  Returns the number of updates the average holds."""
        ckpt = ckpt if isinstance(ckpt, dict) else load_checkpoint(ckpt, map_location=map_location)
        keys = [k for k in ckpt["callbacks"] if k.startswith("WeightAveraging")]
        if not keys or ckpt["callbacks"][keys[0]].get("average") is None:
            raise ValueError("the checkpoint holds no weight average (no WeightAveraging callback wrote into it)")
        inner = ckpt["callbacks"][keys[0]]["average"]
        model.load_state_dict(ckpt["state_dict"], strict=True)
        if not inner["swapped"] and int(inner["n_averaged"]) > 0:      # swapped: the file's state_dict IS the average
            own = dict(model.named_parameters())
            own.update(dict(model.named_buffers()))
            with torch.no_grad():
                for k, a in inner["averages"].items():
                    own[k].copy_(a)
        return int(inner["n_averaged"])


def load_optimizer_state(optimizer, state):
    """`state` (one entry of `optimizer_states`) into `optimizer`, never aliasing its tensors; steps end up as ints for
    optim.RAdam (its load_state_dict) -- a torch optimizer keeps torch's own convention."""
    optimizer.load_state_dict(copy.deepcopy(state))
