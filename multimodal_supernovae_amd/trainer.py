"""A minimal stand-in for the `pl.Trainer.fit(model, train_loader, val_loader)` call the reference
makes (script_wandb.py:229-245, pretraining_clip_wandb.py:140-156): same hook order and per-batch
sequence as Lightning's automatic optimisation --

  on_train_epoch_start -> [zero_grad -> training_step -> backward -> optimizer.step]* ->
  on_train_epoch_end -> on_validation_start -> validation_step* -> on_validation_epoch_end

-- with the 9-tuple batch moved to the GPU (None / empty placeholders pass through), epoch means
of train_loss / val_loss, (multi-process) SUM all-reduce of the gradients before the step, and
pl.Trainer's gradient clipping (gradient_clip_val / gradient_clip_algorithm) between the all-reduce and the step.
Callbacks (checkpoint.ModelCheckpoint, checkpoint.EarlyStopping) run once per epoch where Lightning saves: after
validation -- after the training epoch without a validation loader -- and after the scheduler step; checkpoint.Callback's
other hooks (fit start / end, optimizer step, training-epoch end, validation start / end) serve checkpoint.WeightAveraging;
`fit(..., ckpt_path=...)` resumes a run from a checkpoint file (checkpoint.py says what resumes exactly).
A scheduler returned under "lr_scheduler" is stepped as Lightning's dict says: {"interval": "epoch"} (the default) after the
training epoch, {"interval": "step"} after every optimizer step, either one every `frequency`-th time; a scheduler that
needs a monitored value (ReduceLROnPlateau) is refused.
W&B logging of the reference harness is out of scope.
"""
import torch
import torch.distributed as dist

from . import checkpoint as C
from . import distributed as D
from . import markers
from . import optim


def _to_device(batch, device):
    out = []
    for t in batch:
        if t is None or not torch.is_tensor(t):
            out.append(t)
        elif t.numel() == 0:
            out.append(None)   # SimulationDataset hands over torch.empty(0) for absent modalities
        else:
            out.append(t.to(device, non_blocking=True))
    return tuple(out)


def _batch_rows(batch):
    """Rows of a 9-tuple batch = leading dimension of its first tensor (Lightning's batch-size inference)."""
    for t in batch:
        if torch.is_tensor(t) and t.dim() > 0:
            return int(t.shape[0])
    return 1


def _weighted_mean(values, rows):
    """Epoch mean the way Lightning's on_epoch=True reduction forms it: every step weighted by its batch size."""
    w = torch.tensor(rows, dtype=torch.float64, device=values[0].device)
    return float((torch.stack([v.double() for v in values]) * w).sum() / w.sum())


def _check_sharded_loader(loader, group, what):
    """Data parallel: every rank must see the same number of equally sized batches per epoch -- the embedding
    all-gather assumes equal local row counts, and a rank with one batch more would wait in a collective the others
    never enter.  Checked up front (an error instead of a hang) for anything that has a length."""
    import torch.distributed as dist
    n = len(loader) if hasattr(loader, "__len__") else -1
    bs, drop_last = getattr(loader, "batch_size", None), getattr(loader, "drop_last", None)
    # rows THIS rank iterates over: its sampler's length (a DistributedSampler holds the shard), else the whole dataset
    shard = getattr(loader, "sampler", None)
    if shard is None or not hasattr(shard, "__len__"):
        shard = getattr(loader, "dataset", None)
    rows = len(shard) if shard is not None and hasattr(shard, "__len__") else -1
    last = (rows % bs or bs) if (bs and rows > 0 and not drop_last) else (bs or -1)      # rows of this rank's last batch
    world = dist.get_world_size(group)
    seen = [None] * world
    dist.all_gather_object(seen, (n, last), group=group)
    if len({c for c, _ in seen}) != 1:
        raise ValueError(f"{what}: ranks disagree on the number of batches per epoch {[c for c, _ in seen]}; shard the "
                         "dataset into equal parts (e.g. DistributedSampler(drop_last=True))")
    if len({l for _, l in seen}) != 1:
        raise ValueError(f"{what}: data-parallel training with global negatives needs equal batches on every rank -- the "
                         f"last batches of the ranks have {[l for _, l in seen]} rows; build the DataLoader with drop_last=True")


def _hook(model, name):
    """A Lightning hook is optional on the module (LightningModule supplies no-op defaults)."""
    fn = getattr(model, name, None)
    if callable(fn):
        fn()


def _clip_config(gradient_clip_val, gradient_clip_algorithm):
    """pl.Trainer's clipping arguments -> None (no clipping: value None or 0) or (algorithm, value); algorithm None = "norm"."""
    algo = "norm" if gradient_clip_algorithm is None else str(gradient_clip_algorithm).lower()
    if algo not in ("norm", "value"):
        raise ValueError(f"gradient_clip_algorithm must be 'norm' or 'value' (got {gradient_clip_algorithm!r})")
    if gradient_clip_val is None:
        return None
    val = float(gradient_clip_val)
    if not val >= 0.0:
        raise ValueError(f"gradient_clip_val must be non-negative (got {gradient_clip_val!r})")
    return (algo, val) if val > 0.0 else None


def _clip_params(optimizer):
    """Every parameter of the optimizer's param_groups (Lightning clips what the optimizer steps)."""
    return [p for group in optimizer.param_groups for p in group["params"]]


def _clip_gradients(optimizer, clip):
    """Lightning's clip_gradients: torch.nn.utils.clip_grad_norm_ / clip_grad_value_ on the GPU (optim.py)."""
    if clip is None:
        return
    algo, val = clip
    if algo == "norm":
        optim.clip_grad_norm_(_clip_params(optimizer), val)
    else:
        optim.clip_grad_value_(_clip_params(optimizer), val)


def _accumulate_config(accumulate_grad_batches):
    """pl.Trainer's accumulate_grad_batches -> k: an int >= 1 (1 = every batch is an optimizer step)."""
    k = accumulate_grad_batches
    if isinstance(k, dict):
        raise ValueError("accumulate_grad_batches: Lightning's dict form (and GradientAccumulationScheduler) is out of scope "
                         "here; pass one int >= 1")
    if isinstance(k, bool) or not isinstance(k, int) or k < 1:
        raise ValueError(f"accumulate_grad_batches must be an int >= 1 (got {accumulate_grad_batches!r})")
    return k


def _closes_window(position, k, last):
    """Lightning's rule: the optimizer steps after micro-batch `position` (0-based, counted from the start of the epoch)
    when (position + 1) % k == 0, and after the last batch of the epoch."""
    return (position + 1) % k == 0 or bool(last)


def _with_last(loader):
    """(batch_idx, batch, is the last of the epoch) by looking one batch ahead: the loader may have no len()."""
    it = iter(loader)
    try:
        cur = next(it)
    except StopIteration:
        return
    idx = 0
    for nxt in it:
        yield idx, cur, False
        cur, idx = nxt, idx + 1
    yield idx, cur, True


_SEEDS = {}


def _backward_seed(loss):
    """d loss / d loss = 1 as a cached device tensor (autograd would launch a fill for it every step)."""
    key = (loss.device, loss.dtype, tuple(loss.shape))
    if key not in _SEEDS:
        _SEEDS[key] = torch.ones(loss.shape, dtype=loss.dtype, device=loss.device)
    return _SEEDS[key]


def _accumulate_seed(loss, k):
    """d (loss / k) / d loss = 1 / k as a cached device tensor beside _backward_seed: the fp32 quotient 1 / k that the
    backward of `loss / k` forms, made once on the device."""
    key = (loss.device, loss.dtype, tuple(loss.shape), k)
    if key not in _SEEDS:
        _SEEDS[key] = torch.ones(loss.shape, dtype=loss.dtype, device=loss.device) / k
    return _SEEDS[key]


class Trainer:
    """pl.Trainer's arguments as far as the reference's scripts and their users rely on them.

    accumulate_grad_batches=k (an int >= 1, Lightning 2.x's meaning): backward runs on loss / k, the gradients of k
    consecutive batches are added in batch order, and the optimizer steps when (batch_idx + 1) % k == 0 and on the last
    batch of the epoch (a shorter last window still divides by k; windows restart every epoch).  At a boundary: last add ->
    gradient all-reduce -> clipping -> optimizer.step(); on the other micro-batches nothing is exchanged but the loss's own
    embeddings.  global_step counts optimizer steps; step_losses, history and model.logged keep the undivided loss of
    every micro-batch.  The adds are one multi-tensor launch per micro-batch (optim.GradAccumulator), never autograd's.
    With the contrastive losses the negatives of a pair are those of ITS micro-batch: k micro-batches of B pairs are not a
    batch of k B pairs (Lightning behaves the same way); for losses that are a mean over rows (ClipMLP, masked
    pretraining) they are, up to the order of the sums.  k = 1 is the plain path: no buffer, no launch."""

    def __init__(self, max_epochs=1, device=None, group=None, log_fn=None, sync_batchnorm=False, graphed_steps=False,
                 gradient_clip_val=None, gradient_clip_algorithm=None, callbacks=None, accumulate_grad_batches=1):
        self.accumulate_grad_batches = _accumulate_config(accumulate_grad_batches)
        # pl.Trainer(gradient_clip_val=..., gradient_clip_algorithm=...): clip the all-reduced gradients before the step
        self.clip = _clip_config(gradient_clip_val, gradient_clip_algorithm)
        self.gradient_clip_val, self.gradient_clip_algorithm = gradient_clip_val, gradient_clip_algorithm
        self.max_epochs = max_epochs
        self.device = device if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.group = group
        self.log_fn = log_fn
        self.sync_batchnorm = sync_batchnorm   # pl.Trainer(sync_batchnorm=...): batch statistics over all ranks
        self.graphed_steps = graphed_steps     # replay the training step as HIP graphs (GraphedTrainStep; any world size)
        self.history = {"train_loss": [], "val_loss": []}
        self.step_losses = []
        self.global_step = 0
        # as Lightning: checkpoint callbacks run last, so the file holds the state the other callbacks reached this epoch
        callbacks = list(callbacks or [])
        self.weight_averaging = C._one_weight_averaging(callbacks)      # checkpoint.WeightAveraging, at most one
        self.callbacks = ([c for c in callbacks if not isinstance(c, C.ModelCheckpoint)]
                          + [c for c in callbacks if isinstance(c, C.ModelCheckpoint)])
        self.current_epoch = 0
        self.should_stop = False
        self.model = self.optimizer = self.scheduler = self.graphed_step = self.reducer = self.accumulator = None
        self.scheduler_interval, self.scheduler_frequency = "epoch", 1      # Lightning's lr_scheduler dict: "epoch" | "step", every n-th

    # ---- what callbacks see ----------------------------------------------------------------------------------------
    @property
    def is_global_zero(self):
        return not (dist.is_available() and dist.is_initialized()) or dist.get_rank(self.group) == 0

    def barrier(self):
        if D.world_size(self.group) > 1:
            dist.barrier(self.group)

    def monitored(self, name):
        """The value a callback monitors, as a float: the batch-weighted epoch mean of Trainer.history for train_loss /
        val_loss (model.logged holds the last batch's), model.logged[name] for any other name (AUC_val, f1_val, ...).
        With several ranks every rank gets rank 0's value: a rank that stopped or saved on a value of its own would
        leave the others in a collective."""
        if name in self.history:
            value = self.history[name][-1] if self.history[name] else None
        else:
            value = getattr(self.model, "logged", {}).get(name)
        value = None if value is None else float(value)
        if D.world_size(self.group) > 1:
            box = [value]
            src = dist.get_global_rank(self.group, 0) if self.group is not None else 0
            dist.broadcast_object_list(box, src=src, group=self.group)
            value = box[0]
        if value is None:
            raise RuntimeError(f"monitored value {name!r} has not been logged this run (history: {sorted(self.history)}; "
                               f"model.logged: {sorted(getattr(self.model, 'logged', {}))})")
        return value

    def save_checkpoint(self, path):
        """The state of the run (model, optimizer, scheduler, callbacks, history, RNG) as a Lightning-layout file
        (checkpoint.save_checkpoint); with several ranks every rank calls it and rank 0 writes."""
        if self.model is None:
            raise RuntimeError("Trainer.save_checkpoint: nothing to save before fit() has started")
        wa = self.weight_averaging
        held = wa is not None and wa.averager is not None and wa.averager.swapped and wa._model is self.model
        if held:                          # the file's state_dict is the LIVE model's, whatever the model holds just now
            wa.averager.swap()
        try:
            extra = {"epoch": self.current_epoch, "global_step": self.global_step,
                     "callbacks": {cb.state_key: cb.state_dict() for cb in self.callbacks},
                     "history": {k: list(v) for k, v in self.history.items()}}
            return C.save_checkpoint(path, self.model, self.optimizer, self.scheduler, extra, group=self.group, device=self.device)
        finally:
            if held:
                wa.averager.swap()

    def _resume(self, ckpt, model, optimizer, scheduler):
        """optimizer -> scheduler -> callbacks -> history -> global_step -> RNG (the model is loaded before); returns the epoch
        to go on with."""
        if ckpt["optimizer_states"]:
            C.load_optimizer_state(optimizer, ckpt["optimizer_states"][0])
        if scheduler is not None and ckpt["lr_schedulers"]:
            scheduler.load_state_dict(ckpt["lr_schedulers"][0])
        for cb in self.callbacks:
            if cb.state_key in ckpt["callbacks"]:
                cb.load_state_dict(ckpt["callbacks"][cb.state_key])
            cb.on_resume(self)
        msn = ckpt.get("msn") or {}
        if "history" in msn:
            self.history = {k: list(v) for k, v in msn["history"].items()}
            for k in ("train_loss", "val_loss"):
                self.history.setdefault(k, [])
        self.global_step = ckpt["global_step"]
        self.current_epoch = max(ckpt["epoch"], 0)
        C.restore_rng(ckpt, device=self.device, group=self.group)
        return ckpt["epoch"] + 1

    def fit(self, model, train_dataloaders, val_dataloaders=None, ckpt_path=None):
        """`ckpt_path`: a checkpoint file of this package or of Lightning (or the dict checkpoint.load_checkpoint returned
        for one) to resume from: training continues at the saved epoch + 1 up to `max_epochs` epochs in total."""
        model.to(self.device)
        self.should_stop = False
        self.model = model
        for cb in self.callbacks:
            cb.on_fit_start(self)         # before a checkpoint is loaded: a model that holds its average gets its live weights back
        ckpt = None
        if ckpt_path is not None:
            ckpt = ckpt_path if isinstance(ckpt_path, dict) else C.load_checkpoint(ckpt_path, map_location="cpu")
            model.load_state_dict(ckpt["state_dict"], strict=True)
        D.broadcast_module(model, group=self.group)
        D.enable_sync_batchnorm(self.group, enabled=self.sync_batchnorm and D.world_size(self.group) > 1)
        optim_config = model.configure_optimizers()
        optimizer = optim_config["optimizer"]
        self.optimizer = optimizer
        # bucket all-reduces run under backward; a graph-replayed step reduces every bucket after backward (deferred form)
        reducer = D.GradientReducer(model.parameters(), group=self.group, overlap=not self.graphed_steps)
        self.reducer = reducer
        world = D.world_size(self.group)
        if world > 1:
            _check_sharded_loader(train_dataloaders, self.group, "train_dataloaders")
        scheduler, self.scheduler_interval, self.scheduler_frequency = self._scheduler_of(optim_config)
        self.model, self.scheduler = model, scheduler
        first_epoch = self._resume(ckpt, model, optimizer, scheduler) if ckpt is not None else 0
        wa = self.weight_averaging
        in_graph = wa is not None and wa.in_graph
        graphed = GraphedTrainStep(model.train(), optimizer, reducer=reducer, group=self.group,
                                   gradient_clip_val=self.gradient_clip_val,
                                   gradient_clip_algorithm=self.gradient_clip_algorithm,
                                   accumulate_grad_batches=self.accumulate_grad_batches,
                                   weight_averaging=wa.averager if in_graph else None,
                                   weight_averaging_due=(lambda: wa.due(self.global_step + 1)) if in_graph else None,
                                   ) if self.graphed_steps else None
        self.graphed_step = graphed
        k = self.accumulate_grad_batches
        accum = None
        if k > 1 and graphed is None:
            accum = optim.GradAccumulator(_clip_params(optimizer))
            reducer.accumulator = accum
        self.accumulator = accum
        for epoch in range(first_epoch, self.max_epochs):
            if self.should_stop:
                break
            self.current_epoch = epoch
            model.train()
            _hook(model, "on_train_epoch_start")
            losses, rows = [], []
            if k > 1:
                self._accumulating_epoch(model, optimizer, reducer, accum, graphed, train_dataloaders, losses, rows)
            else:
                for batch_idx, batch in enumerate(train_dataloaders):
                    batch = _to_device(batch, self.device)
                    rows.append(_batch_rows(batch))
                    if graphed is not None:
                        losses.append(graphed(batch, batch_idx).detach().clone())   # the graph's loss tensor is overwritten by the next replay
                        self.global_step += 1
                        self._stepped()
                        continue
                    optimizer.zero_grad(set_to_none=True)
                    with markers.range("forward + loss"):
                        loss = model.training_step(batch, batch_idx)
                    with markers.range("backward"):
                        loss.backward(_backward_seed(loss))
                    reducer.finish()
                    _clip_gradients(optimizer, self.clip)
                    with markers.range("optimiser (RAdam)"):
                        optimizer.step()
                    losses.append(loss.detach())
                    self.global_step += 1
                    self._stepped()
            _hook(model, "on_train_epoch_end")
            for cb in self.callbacks:
                cb.on_train_epoch_end(self)
            self.step_losses += losses
            if losses:
                self.history["train_loss"].append(_weighted_mean(losses, rows))
            if scheduler is not None and self.scheduler_interval == "epoch" and (epoch + 1) % self.scheduler_frequency == 0:
                scheduler.step()                  # Lightning steps an epoch-interval scheduler after the training epoch
            if val_dataloaders is not None:
                self._validate_with_callbacks(model, val_dataloaders, world)
            if self.log_fn:
                self.log_fn(epoch, {k: v[-1] for k, v in self.history.items() if v})
            for cb in self.callbacks:
                cb.on_epoch_end(self)
        reducer.remove()
        for cb in self.callbacks:
            cb.on_fit_end(self)
        return self

    def _stepped(self):
        """The optimizer has stepped and global_step counts it: a step-interval scheduler follows every `frequency`-th such
        step (with accumulate_grad_batches that is once per window, never per micro-batch).  The new lr reaches an eager step
        through param_groups and a recorded one through the optimizer's graph_pre_replay in front of the next replay."""
        if self.scheduler is not None and self.scheduler_interval == "step" and self.global_step % self.scheduler_frequency == 0:
            self.scheduler.step()
        for cb in self.callbacks:
            cb.on_optimizer_step(self)

    def _validate_with_callbacks(self, model, val_dataloaders, world):
        """_validate between the callbacks' on_validation_start / on_validation_end (WeightAveraging swaps the average in and
        out); the end hooks run whatever the validation did."""
        for cb in self.callbacks:
            cb.on_validation_start(self)
        try:
            self._validate(model, val_dataloaders, world)
        finally:
            for cb in self.callbacks:
                cb.on_validation_end(self)

    def _accumulating_epoch(self, model, optimizer, reducer, accum, graphed, loader, losses, rows):
        """The batches of one epoch with accumulate_grad_batches > 1: the window's rule lives in _closes_window, and
        global_step advances when a micro-batch stepped the optimizer (the graphed step says whether its call did)."""
        k = self.accumulate_grad_batches
        for batch_idx, batch, last in _with_last(loader):
            batch = _to_device(batch, self.device)
            rows.append(_batch_rows(batch))
            if graphed is not None:
                losses.append(graphed(batch, batch_idx, last_batch=last).detach().clone())
                stepped = graphed.stepped
            else:
                stepped = _closes_window(batch_idx, k, last)
                losses.append(self._micro_batch(model, optimizer, reducer, accum, batch, batch_idx, stepped))
            self.global_step += int(stepped)
            if stepped:
                self._stepped()

    def _micro_batch(self, model, optimizer, reducer, accum, batch, batch_idx, boundary):
        """One micro-batch of an accumulation window (accumulate_grad_batches > 1), eager: backward on loss / k into fresh
        gradients, then ONE launch adds them to the window's sum; at a boundary the all-reduce, the clipping and the step."""
        k = self.accumulate_grad_batches
        optimizer.zero_grad(set_to_none=True)             # autograd never adds: every backward writes fresh gradients
        overlapped = bool(reducer.buckets) and reducer.overlap
        with markers.range("forward + loss"):
            loss = model.training_step(batch, batch_idx)
        if not boundary:
            with reducer.no_sync(), markers.range("backward"):
                loss.backward(_accumulate_seed(loss, k))
            with markers.range("gradient accumulation"):
                accum.accumulate(False)
            return loss.detach()
        with markers.range("backward"):
            loss.backward(_accumulate_seed(loss, k))
        if overlapped:
            reducer.finish()           # every bucket's gather was the window's last add, issued under backward (or here)
            accum.have.clear()
        else:
            with markers.range("gradient accumulation"):
                accum.accumulate(True)
            reducer.finish()
        _clip_gradients(optimizer, self.clip)
        with markers.range("optimiser (RAdam)"):
            optimizer.step()
        return loss.detach()

    def validate(self, model, val_dataloaders, ckpt_path=None):
        """pl.Trainer.validate: one validation epoch of `model` (with the weights of `ckpt_path`, if given) outside a fit.
        Returns {"val_loss": the batch-weighted epoch mean}; what the model's hooks log (AUC_val, f1_val, ...) is in
        model.logged.  Trainer.history is left as it is.  Without `ckpt_path` a WeightAveraging callback that holds an average of
        this model swaps it in for the epoch; with `ckpt_path` the file's state_dict is validated as it is."""
        model.to(self.device)
        if ckpt_path is not None:
            ckpt = ckpt_path if isinstance(ckpt_path, dict) else C.load_checkpoint(ckpt_path, map_location="cpu")
            model.load_state_dict(ckpt["state_dict"], strict=True)
        self.model = model
        kept = list(self.history["val_loss"])
        if ckpt_path is not None:         # the weights asked for are the file's: no average of an earlier fit is swapped in
            self._validate(model, val_dataloaders, D.world_size(self.group))
        else:
            self._validate_with_callbacks(model, val_dataloaders, D.world_size(self.group))
        new, self.history["val_loss"] = self.history["val_loss"][len(kept):], kept
        return {"val_loss": new[0] if new else None}

    @staticmethod
    def _scheduler_of(cfg):
        """`configure_optimizers` may return {"optimizer": ..., "lr_scheduler": scheduler | {"scheduler": ...}} as the
        reference's MaskedLightCurveEncoder does (src/models_pretraining.py:167-189: RAdam + StepLR per epoch).  Returns
        (scheduler | None, interval, frequency) with Lightning's defaults "epoch" and 1: interval "step" steps the scheduler
        after every `frequency`-th optimizer step, "epoch" after every `frequency`-th training epoch.  A `monitor` entry is
        accepted and unused: a scheduler that needs the monitored value (ReduceLROnPlateau) is not built."""
        sch = cfg.get("lr_scheduler")
        interval, frequency = "epoch", 1
        if isinstance(sch, dict):
            interval, frequency = sch.get("interval", "epoch"), sch.get("frequency", 1)
            sch = sch.get("scheduler")
        if interval not in ("epoch", "step"):
            raise ValueError(f"lr_scheduler: interval must be 'epoch' or 'step' (got {interval!r})")
        if isinstance(frequency, bool) or not isinstance(frequency, int) or frequency < 1:
            raise ValueError(f"lr_scheduler: frequency must be an int >= 1 (got {frequency!r})")
        if isinstance(sch, torch.optim.lr_scheduler.ReduceLROnPlateau):
            raise ValueError("lr_scheduler: ReduceLROnPlateau steps on a monitored value, which this Trainer does not hand to "
                             "a scheduler; use a scheduler that steps on its own count")
        return sch, interval, frequency

    def _validate(self, model, val_dataloaders, world):
        """on_validation_start -> validation_step* -> on_validation_epoch_end (ref src/models_multimodal.py:415-556).
        With several ranks each one validates ITS shard against local negatives (no collective inside the loop: a
        short last batch or an uneven shard cannot hang or mix row counts), then the batch-weighted loss sums are
        all-reduced once; the retrieval AUC a rank logs is that of its own shard."""
        model.eval()
        _hook(model, "on_validation_start")
        vlosses, vrows = [], []
        had = getattr(model, "global_negatives", None)
        if world > 1 and had is not None:
            model.global_negatives = False
        try:
            with torch.no_grad():
                for batch_idx, batch in enumerate(val_dataloaders):
                    batch = _to_device(batch, self.device)
                    vrows.append(_batch_rows(batch))
                    vlosses.append(model.validation_step(batch, batch_idx).detach())
        finally:
            if world > 1 and had is not None:
                model.global_negatives = had
        _hook(model, "on_validation_epoch_end")
        if not vlosses and world == 1:
            return
        w = torch.tensor(vrows, dtype=torch.float64, device=self.device)
        acc = torch.zeros(2, dtype=torch.float64, device=self.device)
        if vlosses:
            acc[0], acc[1] = (torch.stack([v.double() for v in vlosses]) * w).sum(), w.sum()
        if world > 1:
            D.all_reduce_sum(acc, self.group, kind="val_loss_all_reduce")
        if float(acc[1]) > 0:
            self.history["val_loss"].append(float(acc[0] / acc[1]))


class _RecordedStep:
    """A training step recorded as HIP-graph SEGMENTS separated by host-driven exchanges.  While it records it is installed
    as distributed.SEGMENTED_CAPTURE: every collective issued through distributed.py closes the segment under capture,
    is remembered (not run: see exchange) and opens the next segment.  All segments allocate from ONE private pool, so a tensor produced in one segment and consumed in a
    later one keeps its address.  replay() = segment, exchange, segment, ... in the recorded order.
    With gradient accumulation the items behind mark_boundary() (gradient all-reduce, clipping, RAdam) run only in a replay
    that closes a window: replay(boundary=False) stops in front of them."""

    def __init__(self, device):
        self.device = device
        self.items = []                 # ("graph", CUDAGraph) | ("call", fn)
        self.boundary_from = None       # index of the first item that runs at a window's boundary only (None: all run always)
        self.pool = torch.cuda.graph_pool_handle()
        self.cur = None

    def begin(self):
        self.cur = torch.cuda.CUDAGraph()
        # thread-local capture mode: the process group's watchdog THREAD polls the events of the exchanges that ran between the
        # segments (hipEventQuery); under the default global mode such a call from any thread while a segment is being captured
        # is an error, the watchdog throws and the process aborts -- about one recording in three with a one-rank RCCL group
        self.cur.capture_begin(pool=self.pool, capture_error_mode="thread_local")

    def exchange(self, fn):
        # The exchange is only REMEMBERED while recording -- nothing of a segment under capture executes, so there is no data to
        # exchange yet, and every rank skips the same collectives in the same order (the step is carried out by the first
        # replay).  Running it for real here put RCCL work between two captures: the process group's watchdog thread polls
        # such work with hipEventQuery while the next segment is being captured, which HIP refuses ("event last recorded in a
        # capturing stream" / "not permitted when stream is capturing") -- the watchdog throws and the process aborts, about
        # one recording in five.
        self.cur.capture_end()
        self.items.append(("graph", self.cur))
        self.items.append(("call", fn))
        self.begin()

    def mark_boundary(self):
        """Everything recorded from here on belongs to the optimizer step: close the segment of the micro-batch."""
        self.cur.capture_end()
        self.items.append(("graph", self.cur))
        self.boundary_from = len(self.items)
        self.begin()

    def end(self):
        self.cur.capture_end()
        self.items.append(("graph", self.cur))
        self.cur = None

    def abort(self):
        """A recording that failed half-way: close the segment under capture (the stream must not stay in capture mode) and
        drop every segment recorded so far."""
        if self.cur is not None:
            try:
                self.cur.capture_end()
            except Exception:          # noqa: BLE001 -- the capture is already invalid; the original error is the one to report
                pass
        self.cur = None
        self.items = []

    def replay(self, boundary=True):
        items = self.items if boundary or self.boundary_from is None else self.items[:self.boundary_from]
        for kind, x in items:
            if kind == "graph":
                x.replay()
            else:
                x()

    @property
    def segments(self):
        return sum(1 for k, _ in self.items if k == "graph")

    @property
    def exchanges(self):
        return sum(1 for k, _ in self.items if k == "call")


class GraphedTrainStep:
    """One training step (zero_grad -> training_step -> backward -> gradient all-reduce -> [gradient clipping] -> RAdam)
    recorded as HIP graphs and replayed.

    accumulate_grad_batches=k > 1 (Trainer's meaning): the towers are still recorded ONCE, as [forward, backward, one
    accumulate launch | gradient all-reduce, clipping, RAdam]; a call replays the first part, and the second part too when it
    closes a window -- every k-th call, and a call with last_batch=True, after which the count restarts.  The accumulate launch
    reads store / add from a device word written on the replaying stream in front of each replay.
    The reducer must be the deferred form (overlap=False, refused otherwise at construction): a hook-driven one would gather
    the last micro-batch's gradients alone and start their all-reduce before the window's sum is formed.

    The reference's own batch sizes (32 ... 256) -- and the 128 ... 256 rows a rank keeps when the global batch of 1024 is
    spread over 4 or 8 GPUs -- leave the GPU waiting for the host: a Maven step issues ~1300 launches and takes ~10 ms of
    host time whatever the batch, 1.5 ms of GPU time at batch 32.  The first `warmup` calls run eagerly (they are real
    steps: moment buffers, allocator, code objects); the next call records the step on the caller's batch shapes and every
    later call copies its batch into the recorded input tensors and replays.

    Data parallel (world size > 1): the step is recorded in SEGMENTS around its exchanges (_RecordedStep): embedding
    all-gather | InfoNCE forward | LSE all-gather | loss all-reduce | backward of the loss and the towers + gather of the
    gradient buckets | SUM all-reduce of the buckets | clipping + RAdam.  The collectives stay host-driven between two graph replays
    (gloo cannot be captured at all; RCCL needs no capture support this way), so the gradient reduction is the deferred
    form of GradientReducer (overlap=False: every bucket after backward) -- pass such a reducer or none.
    Restrictions: fixed batch shapes (others run eagerly, with the same reducer); synchronised BatchNorm issues
    collectives from inside autograd's backward threads and is refused.
    Dropout seeds are device-resident inside the graph (a base that one launch per replay advances + the ordinal of
    the call), so every replay draws new masks; the pretraining masks of MaskedLightCurveEncoder(mask_generator="device") take
    their seeds the same way (mask_generator="reference" draws on the host and is refused with an error that says so).  The
    base is drawn from torch's CPU generator when the step is recorded: a replayed run repeats under torch.manual_seed, but
    not the eager run's stream.  The towers' side streams fork from and join the capturing stream, so the
    graph keeps their concurrency.

        step = GraphedTrainStep(model, model.configure_optimizers()["optimizer"])
        for batch in loader: loss = step(batch)          # `loss` is a device tensor overwritten by the next call
    """

    def __init__(self, model, optimizer, warmup=3, concurrent_towers=None, reducer=None, group=None, gradient_clip_val=None,
                 gradient_clip_algorithm=None, accumulate_grad_batches=1, weight_averaging=None, weight_averaging_due=None):
        self.k = _accumulate_config(accumulate_grad_batches)
        self.clip = _clip_config(gradient_clip_val, gradient_clip_algorithm)    # as Trainer's: None = no clipping
        # optim.AveragedWeights updated after every optimizer step: the last launch of the recorded optimizer part, and the same
        # object in the eager calls.  weight_averaging_due(): asked once in front of each optimizer step whether that step is
        # averaged (None: every one); in a replay the answer travels as the average's device word `active`.
        self.averager, self._averaging_due = weight_averaging, weight_averaging_due
        self.concurrent_towers = concurrent_towers      # None: as the model is set (towers fork / join inside the graph)
        self.group = group
        self.world = D.world_size(group)
        if self.world > 1 and reducer is None:
            reducer = D.GradientReducer(model.parameters(), group=group, overlap=False)
        if reducer is not None and reducer.buckets and reducer.overlap:
            raise RuntimeError("GraphedTrainStep needs the deferred GradientReducer (overlap=False): hook-driven all-reduces "
                               "would be issued from autograd's threads in the middle of a graph segment")
        self.reducer = reducer
        self.model, self.optimizer, self.warmup = model, optimizer, int(warmup)
        self._check_capturable()              # e.g. a pretraining model that draws its masks on the host: refused here already
        self.calls, self.graph, self.static, self.loss = 0, None, None, None
        self._static_attrs = {}               # model attributes the recorded step writes (graph_static_attrs), kept after the capture
        # accumulate_grad_batches > 1: the window's buffers (shared by eager calls and replays), the position in the window
        self.accum = optim.GradAccumulator(_clip_params(optimizer)) if self.k > 1 and optimizer is not None else None
        self._micro, self._recorded, self._eager_steps = 0, [], 0
        self.stepped = True               # whether the last call stepped the optimizer (always, without accumulation)

    def _eager_micro(self, batch, batch_idx, boundary):
        """One micro-batch of an accumulation window, eager (warm-up calls, batches of another shape): into the same buffers
        as the replays."""
        self.optimizer.zero_grad(set_to_none=True)
        loss = self.model.training_step(batch, batch_idx)
        if boundary or self.reducer is None:
            loss.backward(_accumulate_seed(loss, self.k))
        else:
            with self.reducer.no_sync():
                loss.backward(_accumulate_seed(loss, self.k))
        self.accum.accumulate(boundary)
        if boundary:
            if self.reducer is not None:
                self.reducer.finish()
            _clip_gradients(self.optimizer, self.clip)
            self.optimizer.step()
            self._average_eager()
            self._eager_steps += 1
        return loss

    def _due(self):
        return True if self._averaging_due is None else bool(self._averaging_due())

    def _average_eager(self):
        """The averaging step of an eager call (warm-up, a batch of another shape): the same object the replays update."""
        if self.averager is not None and self._due():
            self.averager.set_active(True)
            self.averager.update()

    def _eager(self, batch, batch_idx=0):
        self.optimizer.zero_grad(set_to_none=True)
        loss = self.model.training_step(batch, batch_idx)
        loss.backward()
        if self.reducer is not None:
            self.reducer.finish()
        _clip_gradients(self.optimizer, self.clip)
        self.optimizer.step()
        self._average_eager()
        return loss

    def _check_capturable(self):
        """A model may name what keeps its step from being recorded (check_graph_capturable raises): asked at construction
        and again in front of the recording, before capture begins."""
        check = getattr(self.model, "check_graph_capturable", None)
        if check is not None:
            check()

    def _capture(self, batch):
        model = self.model
        from . import ops
        self._check_capturable()
        if self.world > 1 and ops.BN_SYNC_GROUP is not None:
            raise RuntimeError("GraphedTrainStep: synchronised BatchNorm exchanges statistics from inside backward and "
                               "cannot be recorded; use per-replica statistics or the eager step")
        self.static = tuple(t.clone() if torch.is_tensor(t) else t for t in batch)
        concurrent = getattr(model, "concurrent_towers", False)
        if self.concurrent_towers is not None:
            model.concurrent_towers = bool(self.concurrent_towers)
        self.optimizer.zero_grad(set_to_none=True)
        self.optimizer.graph_prepare()        # device copies of the hyper-parameters and the step count (eager)
        if self.clip is not None:
            optim.clip_graph_prepare(_clip_params(self.optimizer))    # the clip's pinned descriptor table (eager)
        if self.accum is not None:
            self.accum.graph_prepare()        # the selector word and the accumulate launch's pinned table (eager)
        if self.averager is not None:
            self.averager.graph_prepare()     # the descriptor table for the addresses the weights have now (eager)
        import gc
        gc.collect()                          # no autograd graph of an earlier step (bound to other streams) may survive
        device = self.static_device()
        seed0 = torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).to(device, non_blocking=False)
        ops.GRAPH_SEED = [seed0, 0]
        self._seed_base = seed0
        torch.cuda.synchronize()
        if dist.is_available() and dist.is_initialized() and dist.get_backend(self.group) == "nccl":
            import time
            # the warm-up steps' finished RCCL work must be retired by the process group's watchdog before a segment is under
            # capture (it polls with hipEventQuery): a barrier + synchronize makes the work complete, then > 3 watchdog sweeps
            # (TORCH_NCCL_HEARTBEAT... is not what paces it: the sweep period is 100 ms; MSN_WATCHDOG_QUIESCE_S overrides)
            dist.barrier(self.group)
            torch.cuda.synchronize()
            time.sleep(float(__import__("os").environ.get("MSN_WATCHDOG_QUIESCE_S", "0.35")))
        torch.cuda.empty_cache()              # (it must not be polled while a segment is under capture, see _RecordedStep.exchange)
        rec = _RecordedStep(device)
        stream = torch.cuda.Stream(device=device)
        stream.wait_stream(torch.cuda.current_stream(device))
        D.SEGMENTED_CAPTURE = rec
        failure = None
        try:
            with torch.cuda.stream(stream):
                rec.begin()
                ops.graph_seed_advance()
                self.loss = model.training_step(self.static, 0)
                if self.accum is None:
                    self.loss.backward()
                else:
                    self.loss.backward(_accumulate_seed(self.loss, self.k))
                    self._recorded = self.accum.record()      # store / add by the device word; .grad = the window's sums
                    rec.mark_boundary()                       # behind it: what runs only when a window closes
                if self.reducer is not None:
                    self.reducer.finish()         # several ranks: the clip below runs in the last segment, after the exchange
                _clip_gradients(self.optimizer, self.clip)
                self.optimizer.step()
                if self.averager is not None:
                    self.averager.update()        # the static table and the device words {n_averaged, active}
                rec.end()
        except Exception as exc:   # noqa: BLE001 -- out of memory in the private pool, an op that is illegal under capture, ...
            failure = exc
            rec.abort()            # leave capture mode, drop the segments: the next call must not record on a poisoned stream
        finally:
            D.SEGMENTED_CAPTURE = None
            ops.GRAPH_SEED = None
            model.concurrent_towers = concurrent
        torch.cuda.current_stream(device).wait_stream(stream)
        if self.world > 1:
            # every rank must have a recording before any rank replays: the first replay carries out the step's collectives,
            # and a rank that failed to record would leave the others waiting in them
            ok = torch.tensor([0.0 if failure is not None else 1.0], device=device)
            dist.all_reduce(ok, op=dist.ReduceOp.SUM, group=self.group)       # (not a step collective: kept out of COMM_LOG)
            if failure is None and float(ok) < self.world:
                rec.abort()
                failure = RuntimeError("GraphedTrainStep: another rank failed to record the step")
        if failure is not None:
            self.static, self.loss = None, None
            raise failure
        self.graph = rec
        # tensors the recorded step writes for the caller to read (a model names them in `graph_static_attrs`, e.g. the pretraining
        # masks): an eager call in between -- a batch of another shape, a validation step -- rebinds the attributes, a replay puts
        # the recorded tensors back, as it does for the loss and the gradients
        self._static_attrs = {name: getattr(model, name) for name in getattr(model, "graph_static_attrs", ())}
        self._final_grads = [(p, p.grad) for p in self._recorded]     # the accumulators, or the reducer's bucket slices
        self._recorded_set = set(self._recorded)

    def _rebind_static(self):
        for name, tensor in self._static_attrs.items():
            setattr(self.model, name, tensor)

    def static_device(self):
        return next(t.device for t in self.static if torch.is_tensor(t))

    def _call_accumulating(self, batch, batch_idx, last_batch):
        """__call__ with accumulate_grad_batches > 1: `boundary` = this micro-batch closes its window."""
        boundary = self.stepped = _closes_window(self._micro, self.k, last_batch)
        self._micro = 0 if last_batch else self._micro + 1
        if self.graph is None:
            # the recording needs RAdam's moment buffers: at least one eager OPTIMIZER step, not only `warmup` calls
            if self.calls <= self.warmup or self._eager_steps == 0:
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    loss = self._eager_micro(batch, batch_idx, boundary)
                torch.cuda.current_stream().wait_stream(side)
                return loss
            self._capture(batch)
        same = len(batch) == len(self.static) and all(
            (torch.is_tensor(d) and torch.is_tensor(s_) and d.shape == s_.shape) or (d is None and s_ is None)
            for d, s_ in zip(self.static, batch))
        # the recorded launch applies ONE store / add word to every recorded parameter: an open window whose partial sums are
        # not exactly theirs (an eager micro-batch of another shape gave other parameters a gradient) goes on eagerly
        if not same or (self.accum.have and self.accum.have != self._recorded_set):
            loss = self._eager_micro(batch, batch_idx, boundary)
            if boundary:
                self.optimizer.graph_note_eager_step()
            return loss
        for dst, src in zip(self.static, batch):
            if torch.is_tensor(dst):
                dst.copy_(src, non_blocking=True)
        self.accum.graph_pre_replay()
        if boundary:
            self.optimizer.graph_pre_replay()     # RAdam's device step count advances once per optimizer step
            if self.averager is not None:
                self.averager.graph_pre_replay(self._due())
        self.graph.replay(boundary)
        self._rebind_static()
        self.accum.graph_post_replay(self._recorded, boundary)
        if boundary:
            for p, g in self._final_grads:        # after the step p.grad holds the accumulated (clipped) gradient
                p.grad = g
        return self.loss

    def __call__(self, batch, batch_idx=0, last_batch=False):
        """`last_batch`: this is the last batch of the epoch -- with accumulate_grad_batches > 1 it closes its window."""
        self.calls += 1
        if self.accum is not None:
            return self._call_accumulating(batch, batch_idx, last_batch)
        if self.graph is None:
            if self.calls <= self.warmup:
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):             # torch's rule: warm up off the stream that will capture
                    loss = self._eager(batch, batch_idx)
                torch.cuda.current_stream().wait_stream(side)
                return loss
            self._capture(batch)
        same = len(batch) == len(self.static) and all(
            (torch.is_tensor(d) and torch.is_tensor(s_) and d.shape == s_.shape) or (d is None and s_ is None)
            for d, s_ in zip(self.static, batch))
        if not same:                 # e.g. the short last batch of an epoch: one eager step, the graph stays valid
            loss = self._eager(batch, batch_idx)
            self.optimizer.graph_note_eager_step()
            return loss
        for dst, src in zip(self.static, batch):
            if torch.is_tensor(dst):
                dst.copy_(src, non_blocking=True)
        self.optimizer.graph_pre_replay()
        if self.averager is not None:
            self.averager.graph_pre_replay(self._due())
        self.graph.replay()
        self._rebind_static()
        return self.loss
