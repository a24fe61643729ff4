"""The optimizers and what runs around their step, each as multi-tensor HIP launches through device tables of per-tensor records.

RAdam / Adam / AdamW / SGD are torch.optim's classes of the same names (constructors, `param_groups`, `state` keys, `zero_grad`,
`step`, state_dict interchange) stepped by one fused HIP launch per param group (csrc/optim_steps.hip).  RAdam is the one the
reference builds, `torch.optim.RAdam(self.parameters(), lr=..., **optimizer_kwargs)` in configure_optimizers
(src/models_multimodal.py:306-310) with torch defaults, so optimiser states of reference checkpoints map one to one; the others
are for fine-tuning a head or a ViT.  build_optimizer(name, params, lr, **kwargs) is what the models' `optimizer=` keyword goes
through.

LAMB / LARS are the layer-wise adaptive optimizers of large-batch training (timm's Lamb without its gradient pre-clipping,
lightning-bolts' LARS): per tensor a trust ratio from fp64 2-norms, formed and applied on the device by three multi-tensor HIP
launches per param group (csrc/optim_layerwise.hip); layerwise_param_groups splits a model into the group that adapts (weights)
and the one that does not (biases, norm weights).

All six share one piece of plumbing, _FusedStep: the checks, the bucketing of a group into launches, the descriptor tables on
their way to the device and the interface a step recorded in a HIP graph needs (graph_prepare, step() under capture,
graph_pre_replay, graph_note_eager_step).  Their state comes from one of two families: _MomentState (`step`, `exp_avg`,
`exp_avg_sq`: RAdam, Adam, AdamW, LAMB) or _MomentumState (`momentum_buffer`: SGD, LARS).

clip_grad_norm_ / clip_grad_value_ restate torch.nn.utils' functions of the same names on the GPU (multi-tensor HIP
launches, csrc/grad_clip.hip): the gradient clipping pl.Trainer(gradient_clip_val=...) applies before the step.

grad_accumulate_ / GradAccumulator add the gradients of the micro-batches of pl.Trainer(accumulate_grad_batches=k) with one
multi-tensor HIP launch per micro-batch (csrc/grad_accum.hip) in place of autograd's one add per parameter.

AveragedWeights keeps an EMA or the SWA mean of the trainable weights with one multi-tensor HIP launch per update
(csrc/weight_avg.hip) -- what checkpoint.WeightAveraging drives from the Trainer; update_bn is torch.optim.swa_utils.update_bn.
"""
import ctypes
import gc
import math

import torch

from . import _lib
from ._lib import check, lib, ptr, stream_ptr


def _flat_views(tensors, count=1, zeroed=True):
    """(flat, views): `count` float32 buffers shaped like every tensor of `tensors` (one device), views[i][c] = the c-th of
    tensors[i], as views of ONE buffer `flat` with 16-byte aligned slices -- one fill launch (none with zeroed=False) instead of
    `count` per tensor, and every view takes the float4 path of the multi-tensor launches.  Copy c of tensor i starts at
    c * n + off_i, n being the padded total; with zeroed=True the padding is zero and stays zero."""
    n = sum((t.numel() + 3) // 4 * 4 for t in tensors)
    flat = (torch.zeros if zeroed else torch.empty)(count * n, dtype=torch.float32, device=tensors[0].device)
    views, off = [], 0
    for t in tensors:
        m = t.numel()
        views.append([flat[c * n + off:c * n + off + m].view(t.shape) for c in range(count)])
        off += (m + 3) // 4 * 4
    return flat, views


# ---- gradient clipping (torch.nn.utils.clip_grad_norm_ / clip_grad_value_, as pl.Trainer(gradient_clip_val=...) calls them) --
# One multi-tensor launch per pass through a device table {g*, numel} per gradient (csrc/grad_clip.hip).  Eager calls stage
# the table in pinned host memory (two buffers used alternately, _PinnedTables); under stream capture the table comes
# from a pinned buffer reserved BEFORE the capture (clip_graph_prepare), is filled at capture time and copied by a copy
# node of the graph, and the clip coefficient stays on the device -- nothing is written by the host between replays.
class _PinnedTables:
    """Descriptor tables of a multi-tensor launch on their way to the device (`words` 64-bit words per record).  Eager: two
    pinned buffers used alternately, one rewritten only after the copy that last read it has completed (its event).  Under
    stream capture: a pinned buffer reserved BEFORE the capture (reserve), filled at capture time and copied by a copy node
    of the graph; it is kept alive with the process and never rewritten."""

    def __init__(self, words, what, prepare):
        self.words, self.what, self.prepare = words, what, prepare
        self.staging, self.slot = [[None, None], [None, None]], 0
        self.reserved, self.captured = [], []

    def reserve(self, n_records):
        self.reserved.append(torch.empty(self.words * max(n_records, 1), dtype=torch.int64).pin_memory())

    def upload(self, words, dev):
        """The device copy of `words`; the host buffer it is copied from is never rewritten while a copy that reads it may
        still be pending."""
        if torch.cuda.is_current_stream_capturing():
            fit = [i for i, t in enumerate(self.reserved) if t.numel() >= len(words)]
            if not fit:
                raise _lib.MsnHipError(f"{self.what} under stream capture needs optim.{self.prepare}(parameters) before the "
                                       "capture begins (the descriptor table must be pinned in advance)")
            host = self.reserved.pop(fit[0])
            self.captured.append(host)
            host[:len(words)].copy_(torch.tensor(words, dtype=torch.int64))
            return host[:len(words)].to(dev, non_blocking=True)           # a copy node of the graph (static content)
        self.slot ^= 1
        slot = self.staging[self.slot]
        if slot[1] is not None:
            slot[1].synchronize()
        if slot[0] is None or slot[0].numel() < len(words):
            slot[0] = torch.empty(max(len(words), 1024), dtype=torch.int64).pin_memory()
        slot[0][:len(words)] = torch.tensor(words, dtype=torch.int64)
        table = slot[0][:len(words)].to(dev, non_blocking=True)
        slot[1] = torch.cuda.Event()
        slot[1].record()
        return table


_CLIP_TABLES = _PinnedTables(2, "gradient clipping", "clip_graph_prepare")
_ACCUM_TABLES = _PinnedTables(4, "gradient accumulation", "accum_graph_prepare")


def clip_graph_prepare(parameters):
    """Call BEFORE a stream capture that will clip the gradients of `parameters` (eager): reserves the pinned descriptor
    table that the capture fills and its graph copies at every replay.  One reservation per clip call recorded."""
    params = [parameters] if torch.is_tensor(parameters) else list(parameters)
    _CLIP_TABLES.reserve(len(params))


def _clip_grads(parameters, what):
    params = [parameters] if torch.is_tensor(parameters) else list(parameters)
    grads = [p.grad for p in params if p.grad is not None]
    for g in grads:
        if g.device.type != "cuda":
            _lib.require_gpu()
            raise _lib.MsnHipError(f"{what}: gradients must live on the GPU (there is no CPU path)")
        if g.dtype != torch.float32 or not g.is_contiguous():
            raise _lib.MsnHipError(f"{what}: contiguous float32 gradients only (got {g.dtype}, "
                                   f"contiguous={g.is_contiguous()})")
    if grads and len({g.device for g in grads}) != 1:
        raise _lib.MsnHipError(f"{what}: all gradients must live on one GPU")
    return grads


def _clip_table(grads):
    """(device table, max_numel) of the gradients."""
    words = []
    for g in grads:
        words += [g.data_ptr(), g.numel()]
    return _CLIP_TABLES.upload(words, grads[0].device), max(g.numel() for g in grads)


@torch.no_grad()
def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None):
    """torch.nn.utils.clip_grad_norm_: scales every gradient in place by clamp(max_norm / (total_norm + 1e-6), max=1) and
    returns the total norm before clipping as a 0-dim float32 device tensor (no host synchronisation unless
    `error_if_nonfinite`).  norm_type 1, 2 or inf; `foreach` is accepted for torch's signature (always one multi-tensor
    launch per pass)."""
    norm_type = float(norm_type)
    if norm_type not in (1.0, 2.0, float("inf")):
        raise ValueError(f"clip_grad_norm_: norm_type must be one of 1, 2, inf (got {norm_type})")
    max_norm = float(max_norm)
    if not max_norm >= 0.0:
        raise ValueError(f"clip_grad_norm_: max_norm must be non-negative (got {max_norm})")
    capturing = torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()
    if error_if_nonfinite and capturing:
        raise _lib.MsnHipError("clip_grad_norm_(error_if_nonfinite=True) reads the norm on the host and cannot be recorded "
                               "in a stream capture")
    grads = _clip_grads(parameters, "clip_grad_norm_")
    if not grads:
        return torch.tensor(0.0)
    table, max_n = _clip_table(grads)
    dev = grads[0].device
    out = torch.empty(2, dtype=torch.float32, device=dev)              # {total norm, clip coefficient}
    ws = torch.empty(int(lib().msn_grad_norm_workspace_bytes(len(grads), max_n)), dtype=torch.uint8, device=dev)
    check(lib().msn_grad_norm(ptr(table), len(grads), max_n, norm_type, max_norm, ptr(out), ctypes.c_void_p(out.data_ptr() + 4),
                              ptr(ws), ws.numel(), stream_ptr()), "msn_grad_norm")
    total = out[0]
    if error_if_nonfinite and not math.isfinite(float(total)):
        raise RuntimeError(f"The total norm of order {norm_type} for gradients from `parameters` is non-finite, so it cannot "
                           "be clipped. To disable this error and scale the gradients by the non-finite norm anyway, set "
                           "`error_if_nonfinite=False`")
    check(lib().msn_grad_scale(ptr(table), len(grads), max_n, ctypes.c_void_p(out.data_ptr() + 4), stream_ptr()),
          "msn_grad_scale")
    return total


@torch.no_grad()
def clip_grad_value_(parameters, clip_value, foreach=None):
    """torch.nn.utils.clip_grad_value_: every gradient clamped in place to [-clip_value, clip_value] (NaN kept)."""
    clip_value = float(clip_value)
    if not clip_value >= 0.0:
        raise ValueError(f"clip_grad_value_: clip_value must be non-negative (got {clip_value})")
    grads = _clip_grads(parameters, "clip_grad_value_")
    if not grads:
        return None
    table, max_n = _clip_table(grads)
    check(lib().msn_grad_clamp(ptr(table), len(grads), max_n, clip_value, stream_ptr()), "msn_grad_clamp")
    return None


# ---- gradient accumulation (pl.Trainer(accumulate_grad_batches=k)) -------------------------------------------------------
# One multi-tensor launch per micro-batch through a device table {dst*, acc*, g*, numel} per gradient (csrc/grad_accum.hip)
# in place of autograd's AccumulateGrad (one stock add per parameter).  The table travels as the clipping tables do
# (_PinnedTables): staged in pinned memory when eager, reserved before a capture (accum_graph_prepare).
def accum_graph_prepare(parameters):
    """Call BEFORE a stream capture that will accumulate the gradients of `parameters` (eager): reserves the pinned
    descriptor table the capture fills.  One reservation per accumulate call recorded."""
    params = [parameters] if torch.is_tensor(parameters) else list(parameters)
    _ACCUM_TABLES.reserve(len(params))


@torch.no_grad()
def grad_accumulate_(dsts, accs, grads, add=True, add_dev=None):
    """dst = acc + g (add) or dst = g (store) for every triple, in ONE launch; fp32, bit for bit torch's add.  accs[i] None:
    that tensor is stored whatever `add` says.  dst may be acc, g or a third buffer.  `add_dev`: a device int32 tensor whose
    first word overrides `add` when the launch runs (non-zero = add) -- for a step recorded once and replayed at every position
    of an accumulation window."""
    dsts, accs, grads = list(dsts), list(accs), list(grads)
    if not (len(dsts) == len(accs) == len(grads)):
        raise ValueError("grad_accumulate_: dsts, accs and grads must have one entry per tensor")
    if not grads:
        return
    for d, a, g in zip(dsts, accs, grads):
        for t in (d, g) if a is None else (d, a, g):
            if t.device.type != "cuda":
                _lib.require_gpu()
                raise _lib.MsnHipError("grad_accumulate_: gradients must live on the GPU (there is no CPU path)")
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise _lib.MsnHipError(f"grad_accumulate_: contiguous float32 tensors only (got {t.dtype}, "
                                       f"contiguous={t.is_contiguous()})")
            if t.numel() != g.numel():
                raise _lib.MsnHipError("grad_accumulate_: dst, acc and g of a tensor must have the same number of elements")
    if len({g.device for g in grads}) != 1:
        raise _lib.MsnHipError("grad_accumulate_: all gradients must live on one GPU")
    words = []
    for d, a, g in zip(dsts, accs, grads):
        words += [d.data_ptr(), 0 if a is None else a.data_ptr(), g.data_ptr(), g.numel()]
    max_n = max(g.numel() for g in grads)
    table = _ACCUM_TABLES.upload(words, grads[0].device)
    check(lib().msn_grad_accumulate(ptr(table), len(grads), max_n, 1 if add else 0, ptr(add_dev), stream_ptr()),
          "msn_grad_accumulate")


class GradAccumulator:
    """The accumulation buffers of one optimizer's parameters (4 bytes per trainable parameter, views of ONE flat buffer with
    16-byte aligned slices, allocated at the first micro-batch that needs them) and the state of the window: which parameters
    hold a partial sum.  Usage per micro-batch, with p.grad set to None before backward so that autograd never adds:

        backward(); acc.accumulate(boundary)         # boundary: the micro-batch after which the optimizer steps

    Not at a boundary: acc = g for a parameter's first gradient of the window, acc += g afterwards.  At a boundary the same,
    and p.grad is pointed at the accumulator (the sum of the window); a window of one micro-batch leaves p.grad as it is and
    launches nothing.  A parameter without a gradient in a micro-batch contributes nothing."""

    def __init__(self, params):
        self.params = [p for p in params if p.requires_grad]
        self.flat, self.acc = None, {}
        self.have = set()                 # parameters whose accumulator holds a partial sum of the open window
        self.selector = None              # device int32 word: the store / add selector of a recorded step

    @property
    def window_open(self):
        return bool(self.have)

    def _buffers(self):
        if self.flat is None and self.params:
            self.flat, views = _flat_views(self.params, zeroed=False)
            self.acc = {p: v for p, (v,) in zip(self.params, views)}
        return self.acc

    def _check(self, p):
        if p.device.type != "cuda":
            _lib.require_gpu()
            raise _lib.MsnHipError("gradient accumulation: parameters must live on the GPU (there is no CPU path)")
        if p.dtype != torch.float32:
            raise _lib.MsnHipError(f"gradient accumulation: float32 parameters only (got {p.dtype})")

    @torch.no_grad()
    def accumulate(self, boundary):
        with_grad = [p for p in self.params if p.grad is not None]
        if boundary and not self.have:
            return                                        # a window of one: p.grad is the sum already
        for p in with_grad:
            self._check(p)
        acc = self._buffers()
        if with_grad:
            cur = torch.cuda.current_stream(with_grad[0].device)
            for p in with_grad:                           # a gradient of a tower's side stream is freed before the next backward
                p.grad.record_stream(cur)
            grad_accumulate_([acc[p] for p in with_grad], [acc[p] if p in self.have else None for p in with_grad],
                             [p.grad for p in with_grad], add=True)
            self.have.update(with_grad)
        if boundary:
            self.point_grads()
            self.have.clear()

    @torch.no_grad()
    def record(self):
        """Under stream capture: the launch of one micro-batch with the store / add selector read from the device word, over
        the parameters that have a gradient now; their .grad is pointed at the accumulators, which is what the clipping and
        the optimizer recorded behind it read.  Nothing executes while recording, so the window's state is left alone.
        Returns the parameters recorded."""
        with_grad = [p for p in self.params if p.grad is not None]
        for p in with_grad:
            self._check(p)
        acc = self._buffers()
        if with_grad:
            grad_accumulate_([acc[p] for p in with_grad], [acc[p] for p in with_grad], [p.grad for p in with_grad],
                             add=True, add_dev=self.selector)
        for p in with_grad:
            p.grad = acc[p]
        return with_grad

    def point_grads(self):
        """p.grad = the accumulator, for every parameter that holds a sum."""
        for p in self.have:
            p.grad = self.acc[p]

    @torch.no_grad()
    def flush_into(self, params, views):
        """The last add of a window written into a third buffer: views[i] = acc + p.grad for the parameters given (a gradient
        bucket's slices); a parameter without a gradient in this micro-batch hands over its partial sum as it is, one
        without either is left alone.  The parameters leave the window."""
        todo = []                                         # (dst, acc | None, g)
        for p, v in zip(params, views):
            if p.grad is not None:
                self._check(p)
                todo.append((v, self.acc[p] if p in self.have else None, p.grad))
            elif p in self.have:
                todo.append((v, None, self.acc[p]))       # no gradient now: the partial sum itself, stored
        if todo:
            grad_accumulate_([d for d, _, _ in todo], [a for _, a, _ in todo], [g for _, _, g in todo], add=True)
        self.have.difference_update(params)

    def graph_prepare(self):
        """Call BEFORE the capture (eager): the buffers, the selector word with its two pinned constants, the pinned table."""
        self._buffers()
        dev = self.params[0].device
        self.selector = torch.zeros(1, dtype=torch.int32, device=dev)
        self._consts = [torch.tensor([0], dtype=torch.int32).pin_memory(), torch.tensor([1], dtype=torch.int32).pin_memory()]
        accum_graph_prepare(self.params)

    def graph_pre_replay(self):
        """Enqueued on the replaying stream BEFORE a replay (ordered against the previous replay's read and this one's): the
        selector says whether the window is open.  The pinned constants are never rewritten."""
        self.selector.copy_(self._consts[1 if self.have else 0], non_blocking=True)

    def graph_post_replay(self, recorded, boundary):
        if boundary:
            self.have.clear()
        else:
            self.have.update(recorded)


# ---- weight averaging (pl.callbacks.WeightAveraging / StochasticWeightAveraging, torch.optim.swa_utils.AveragedModel) ----------
# One multi-tensor launch per optimizer step through a device table {avg*, p*, numel} per averaged tensor (csrc/weight_avg.hip) in
# place of torch._foreach_lerp_.  Unlike the gradient tables this one is STATIC -- parameters are updated in place by the optimizer
# and by load_state_dict, the averages are views of one buffer -- so it is uploaded at construction (again only if a parameter's
# storage has moved, as the attention's stacked q / k / v weights do at the first forward) and the same launch with the same
# table runs eagerly and under stream capture.  Whether a recorded launch averages is a device word (`active`),
# and the number of updates is counted on the device, as RAdam's step count is.
AVG_MODES = {"ema": 0, "swa": 1}      # MSN_AVG_EMA, MSN_AVG_SWA of include/msn_hip.h
_AVG_SWAP = 2                         # MSN_AVG_SWAP


def _avg_config(avg, decay):
    """(avg, decay) as given to AveragedWeights / checkpoint.WeightAveraging, checked: "ema" | "swa", 0 <= decay <= 1."""
    if avg not in AVG_MODES:
        raise ValueError(f"avg must be 'ema' or 'swa' (got {avg!r})")
    decay = float(decay)
    if not 0.0 <= decay <= 1.0:
        raise ValueError(f"decay must lie in [0, 1] (got {decay!r})")
    return avg, decay


class AveragedWeights:
    """A running average of a model's weights, updated by ONE HIP launch (msn_weight_average):

        avg="ema":  average = decay * average + (1 - decay) * weights      (torch's get_ema_multi_avg_fn(decay))
        avg="swa":  the equal-weight mean of the weights at every update   (AveragedModel's default)

    the first update copies the weights in both.  Averaged are the contiguous float32 CUDA parameters with requires_grad=True
    of `model_or_parameters` (a module, or an iterable of parameters, then named "0", "1", ...): a frozen parameter equals its
    own average and costs neither memory nor bandwidth; any other trainable parameter is refused.  use_buffers=True (a module
    only) also averages the floating-point buffers (BatchNorm's running_mean / running_var), never the integer ones
    (num_batches_tracked); with use_buffers=False the model's live buffers serve both sets of weights, which is what torch's
    AveragedModel reaches by copying the buffers at every update (optim.update_bn recomputes them for the average).

    Memory: ONE zeroed fp32 buffer with 16-byte aligned slices, 4 bytes per averaged element -- deliberately not a deep copy of
    the module as torch's is (it would double every cache and plane buffer of the towers).  To USE the average, swap(): the
    average and the live values exchange their bits in place (`swapped` says which the model holds), so every address -- the
    optimizer's, a recorded HIP graph's -- stays valid; swap() again undoes it bit for bit.

    update() may be recorded in a stream capture: the descriptor table and the two device words {n_averaged, active} are built
    here; the table is rebuilt only if a tensor's storage has moved (graph_prepare, _refresh_table), never under capture.  A
    replay averages when `active` is set (graph_pre_replay writes it on the replaying stream) and advances the device count
    itself; the host never writes n_averaged between replays."""

    def __init__(self, model_or_parameters, avg="ema", decay=0.999, use_buffers=False):
        self.avg, self.decay = _avg_config(avg, decay)
        self.use_buffers = bool(use_buffers)
        self.weight = float(torch.tensor(1.0 - self.decay, dtype=torch.float64).to(torch.float32))   # rounded ONCE from the double
        if isinstance(model_or_parameters, torch.nn.Module):
            named = [(k, p) for k, p in model_or_parameters.named_parameters() if p.requires_grad]
            if self.use_buffers:
                named += [(k, b) for k, b in model_or_parameters.named_buffers() if b.is_floating_point()]
        else:
            if self.use_buffers:
                raise ValueError("AveragedWeights(use_buffers=True) needs a module as its first argument (parameters have no buffers)")
            ps = [model_or_parameters] if torch.is_tensor(model_or_parameters) else list(model_or_parameters)
            named = [(str(i), p) for i, p in enumerate(ps) if p.requires_grad]
        if not named:
            raise ValueError("AveragedWeights: nothing to average (no parameter with requires_grad=True)")
        for k, t in named:
            if t.device.type != "cuda":
                _lib.require_gpu()
                raise _lib.MsnHipError(f"AveragedWeights: {k} must live on the GPU (there is no CPU path)")
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise _lib.MsnHipError(f"AveragedWeights supports contiguous float32 tensors only ({k}: {t.dtype}, "
                                       f"contiguous={t.is_contiguous()})")
        if len({t.device for _, t in named}) != 1:
            raise _lib.MsnHipError("AveragedWeights: all averaged tensors must live on one GPU")
        if len(named) > 65535:
            raise _lib.MsnHipError(f"AveragedWeights: at most 65535 tensors per launch (got {len(named)})")
        self.names = [k for k, _ in named]
        self._sources = [t for _, t in named]                    # the parameters / buffers themselves
        dev = self._sources[0].device
        self.numel = sum(t.numel() for t in self._sources)
        self._max_numel = max(t.numel() for t in self._sources)
        self.flat, views = _flat_views(self._sources)
        self.averages = [v for (v,) in views]
        self._ptrs, self._table, self._retired = None, None, []
        self._refresh_table()
        self._checks_left = 2             # update() looks for moved storage only this many more times (graph_prepare re-arms it)
        self._state = torch.tensor([0, 1], dtype=torch.int64).to(dev)          # {n_averaged, active}
        self._consts = [torch.tensor([0], dtype=torch.int64).pin_memory(), torch.tensor([1], dtype=torch.int64).pin_memory()]
        self._active = True
        self.n_averaged = 0               # the host's count, kept in step with the device word
        self.swapped = False              # True: the model holds the averages and the buffer the live values

    def _refresh_table(self):
        """The device table {avg*, p*, numel}: built at construction and again only when a tensor's storage has moved since --
        the optimizer and load_state_dict write in place, but SelfAttention.stacked_qkv re-points its three projection weights
        at one buffer at the first forward, and .to() moves everything.  Never under stream capture (graph_prepare first): a
        recorded launch keeps the table it was recorded with.  A replaced table stays allocated (a launch on another stream
        may still read it; 24 bytes per tensor)."""
        ptrs = [t.data_ptr() for t in self._sources]
        if ptrs == self._ptrs:
            return
        if torch.cuda.is_current_stream_capturing():
            raise _lib.MsnHipError("AveragedWeights: a parameter's storage moved since the descriptor table was built; call "
                                   "graph_prepare() before the capture begins")
        for k, t in zip(self.names, self._sources):
            if t.device != self.flat.device or t.dtype != torch.float32 or not t.is_contiguous():
                raise _lib.MsnHipError(f"AveragedWeights supports contiguous float32 tensors on {self.flat.device} only ({k}: "
                                       f"{t.dtype}, {t.device}, contiguous={t.is_contiguous()})")
        self.tensors = [t.detach() for t in self._sources]       # views of the live storage: the addresses the table holds
        words = []
        for a, t in zip(self.averages, self.tensors):
            words += [a.data_ptr(), t.data_ptr(), t.numel()]
        if self._table is not None:
            self._retired.append(self._table)
        self._table = torch.tensor(words, dtype=torch.int64).to(self.flat.device)
        self._ptrs = ptrs

    def graph_prepare(self):
        """Call BEFORE a stream capture that records update() (eager, after at least one forward of the model), and after
        anything that moves the weights later on (.to(), an assignment to .data): the descriptor table for the addresses the
        weights have now.  update() itself looks only at its first two calls after construction or after this one -- the
        first forward is what re-points the attention weights -- so that a step does not pay a data_ptr() per tensor."""
        self._refresh_table()
        self._checks_left = 2

    def _launch(self, mode, state, look=True):
        if look:
            self._refresh_table()
        check(lib().msn_weight_average(ptr(self._table), len(self.tensors), self._max_numel, mode, self.weight, ptr(state),
                                       stream_ptr()), "msn_weight_average")

    @torch.no_grad()
    def update(self):
        """One averaging step from the live weights (does nothing while `active` is off).  Eager or under stream capture."""
        if self.swapped:
            raise RuntimeError("AveragedWeights.update(): the model holds the averages (swapped); swap() back first")
        self._launch(AVG_MODES[self.avg], self._state, look=self._checks_left > 0)
        self._checks_left = max(self._checks_left - 1, 0)
        if not torch.cuda.is_current_stream_capturing():
            self.n_averaged += int(self._active)

    def set_active(self, active):
        """Whether the next launches average: the device word, written from one of two pinned constants on the current stream
        and only when it changes (the way GradAccumulator writes its store / add word)."""
        active = bool(active)
        if active != self._active:
            self._state[1:2].copy_(self._consts[int(active)], non_blocking=True)
            self._active = active

    def graph_pre_replay(self, active=True):
        """In front of the replay of a step that recorded update(), on the replaying stream: the `active` word for this
        replay, and the host count advanced by what the replay will do (the device count is the kernel's own business)."""
        self.set_active(active)
        self.n_averaged += int(self._active)

    @torch.no_grad()
    def swap(self):
        """Exchange the averages and the live values in place, bit for bit; twice is the identity."""
        if torch.cuda.is_current_stream_capturing():
            raise _lib.MsnHipError("AveragedWeights.swap() is not part of a recorded step")
        self._launch(_AVG_SWAP, None)
        self.swapped = not self.swapped

    def device_n_averaged(self):
        """The device's count (a synchronising read; for checks)."""
        return int(self._state[0])

    def averaged_state_dict(self):
        """name -> a copy of the averaged tensor (wherever it lives now)."""
        src = self._sources if self.swapped else self.averages
        return {k: t.detach().clone() for k, t in zip(self.names, src)}

    def state_dict(self):
        """Tensors and primitives only (readable with weights_only=True).  `averages` is the CONTENT OF THE BUFFER by name: the
        averages, or with `swapped` set the live values the model's own state_dict then lacks."""
        return {"avg": self.avg, "decay": self.decay, "use_buffers": self.use_buffers, "n_averaged": int(self.n_averaged),
                "swapped": bool(self.swapped), "averages": {k: a.detach().clone() for k, a in zip(self.names, self.averages)}}

    @torch.no_grad()
    def load_state_dict(self, state):
        if state["avg"] != self.avg:
            raise ValueError(f"AveragedWeights.load_state_dict: the state was made with avg={state['avg']!r}, this object "
                             f"averages with avg={self.avg!r}")
        have, want = set(state["averages"]), set(self.names)
        if have != want:
            raise ValueError("AveragedWeights.load_state_dict: the state averages another set of tensors -- missing here: "
                             f"{sorted(have - want)}; missing in the state: {sorted(want - have)}")
        for k, a in zip(self.names, self.averages):
            src = state["averages"][k]
            if tuple(src.shape) != tuple(a.shape):
                raise ValueError(f"AveragedWeights.load_state_dict: {k} has shape {tuple(src.shape)} in the state, "
                                 f"{tuple(a.shape)} here")
            a.copy_(src)
        self.n_averaged = int(state["n_averaged"])
        self._state[0:1].copy_(torch.tensor([self.n_averaged], dtype=torch.int64))
        self.swapped = bool(state["swapped"])


@torch.no_grad()
def update_bn(loader, model, device=None, forward=None):
    """torch.optim.swa_utils.update_bn: recompute the BatchNorm running statistics of `model` for the weights it holds now (the
    averaged ones after AveragedWeights.swap(), when the buffers were not averaged with them).  Under no_grad in train mode:
    every BatchNorm's statistics are reset, then one pass over `loader` averages the batches cumulatively -- momentum
    1 / (i + 1) on batch i, handed to the BatchNorm launches per call (ops.BN_MOMENTUM; no kernel changes).  Momentum and
    train / eval mode are as before afterwards.  `forward(batch, i)` runs one batch (default: model.training_step(batch, i)
    for a Lightning-style module, else model(batch), a list / tuple batch giving its first entry as torch does); `device`:
    where to move a batch's tensors first."""
    from . import ops
    bns = [m for m in model.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm) and m.running_mean is not None]
    if not bns:
        return
    was_training = model.training
    for m in bns:
        m.running_mean.zero_()
        m.running_var.fill_(1.0)
        m.num_batches_tracked.zero_()
    if forward is None:
        if callable(getattr(model, "training_step", None)):
            forward = model.training_step
        else:
            forward = lambda batch, i: model(batch[0] if isinstance(batch, (list, tuple)) else batch)    # noqa: E731
    model.train()
    try:
        for i, batch in enumerate(loader):
            if device is not None:
                if isinstance(batch, (list, tuple)):
                    batch = type(batch)(t.to(device) if torch.is_tensor(t) else t for t in batch)
                elif torch.is_tensor(batch):
                    batch = batch.to(device)
            ops.BN_MOMENTUM = 1.0 / (i + 1)
            forward(batch, i)
    finally:
        ops.BN_MOMENTUM = None
        model.train(was_training)


# ---- fused RAdam / Adam / AdamW / SGD (torch.optim's classes, csrc/optim_steps.hip) -----------------------------------------------
# One multi-tensor launch per param group, step count and device through a descriptor table staged in pinned memory
# (_PinnedTables), so the step never blocks the host on the stream.  Under stream capture the table comes from a pinned buffer
# reserved by graph_prepare(), the hyper-parameters sit in a 64-byte device block and the step-dependent terms are derived on the
# device from a device-resident step counter that every replay increments -- nothing is written by the host between replays (it
# would race with a replay still in flight) but a changed hyper-parameter, on the replaying stream (graph_pre_replay).
_IGNORED_KEYWORDS = ("foreach", "capturable", "fused")              # accepted for torch's signatures, without effect
_REFUSED_KEYWORDS = ("amsgrad", "maximize", "differentiable")       # not built: True raises


def _torch_keywords(name, kwargs):
    """The torch.optim keywords beyond the hyper-parameters: some are ignored, some refused when set, anything else is unknown."""
    for key, value in kwargs.items():
        if key in _REFUSED_KEYWORDS:
            if value:
                raise ValueError(f"optim.{name}: {key}=True is not built (the fused step has no such form)")
        elif key not in _IGNORED_KEYWORDS:
            raise TypeError(f"optim.{name}.__init__() got an unexpected keyword argument {key!r}")


class _FusedStep(torch.optim.Optimizer):
    """What every optimizer of this module shares: state interchange, the bucketing of a group into launches, the descriptor
    tables on their way to the device and the graph interface of trainer.GraphedTrainStep (graph_prepare, step() under capture,
    graph_pre_replay, graph_note_eager_step).  The state family (_MomentState, _MomentumState) says which state a parameter
    needs (_init_state, _has_state, _needs_state), what tells two launches of a group apart (_advance: the step count, SGD's
    first-step flag) and what a record holds (_record); the optimizer itself says how to launch (_launch, _launch_dev) and what
    the device block of its hyper-parameters looks like (_hyper_block)."""
    _WORDS = 5               # 64-bit words per record of the table
    _HOST_WORDS = 12         # float32 words at the start of the device block that the host owns

    def load_state_dict(self, state_dict):
        """torch.optim.Optimizer.load_state_dict on a DEEP COPY of `state_dict` (torch's `.to()` of a tensor that already has
        the parameter's device and dtype returns that very tensor: the live state of another optimizer would be shared and
        stepped twice), then every `step` as a Python int: torch.optim stores tensor(7.), a Lightning checkpoint loaded with
        map_location="cuda" a CUDA tensor, and the recorded step reads int(step) -- on a CUDA tensor a synchronisation inside
        a stream capture."""
        import copy
        super().load_state_dict(copy.deepcopy(state_dict))
        for st in self.state.values():
            if "step" in st:
                st["step"] = int(st["step"])

    def _pinned(self):
        tables = getattr(self, "_tables", None)
        if tables is None:
            tables = self._tables = _PinnedTables(self._WORDS, f"{type(self).__name__}.step()", "graph_prepare")
        return tables

    def _check(self, p):
        name = type(self).__name__
        if p.device.type != "cuda":
            _lib.require_gpu()
            raise _lib.MsnHipError(f"{name} parameters must live on the GPU")
        if p.dtype != torch.float32 or not p.is_contiguous():
            raise _lib.MsnHipError(f"{name} supports contiguous float32 parameters only")

    @torch.no_grad()
    def step(self, closure=None):
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            self._step_captured()
            return None
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        todo = []
        for group in self.param_groups:
            ps = [p for p in group["params"] if p.grad is not None]
            for p in ps:
                self._check(p)
            todo.append((group, ps))
        fresh = self._init_state(todo)
        for group, ps in todo:
            # parameters of one group that share a step count (SGD: a first step) and a device go into one launch
            buckets = {}
            for p in ps:
                buckets.setdefault((self._advance(group, p, p in fresh), p.device), []).append(p)
            for (key, dev), items in buckets.items():
                grads = [p.grad if p.grad.is_contiguous() else p.grad.contiguous() for p in items]     # alive up to the launch
                table = self._pinned().upload(self._record(group, items, grads), dev)
                self._launch(group, key, table, len(items), max(p.numel() for p in items))
        return loss

    # ---- HIP-graph capture (trainer.GraphedTrainStep) --------------------------------------------------------------
    def graph_prepare(self):
        """Call BEFORE the capture (eager): per group the device block of the hyper-parameters, the device step count and the
        pinned buffer the capture fills with the descriptor table."""
        # A CUDAGraph that is garbage in a reference cycle is destroyed by whichever collection finds it, and torch's
        # destructor is refused while a stream is capturing: the exception leaves a destructor and aborts the process.
        # Collect now, as torch.cuda.graph does on entry and GraphedTrainStep before it records.
        gc.collect()
        self._graph_ready, self._graph_hyper_captured = {}, {}
        for gi, group in enumerate(self.param_groups):
            ps = [p for p in group["params"] if p.device.type == "cuda"]
            if not ps:
                continue
            dev = ps[0].device
            hyper = self._hyper_block(group).to(dev)
            counter = torch.tensor([self._group_step(group)], dtype=torch.int64, device=dev)
            self._pinned().reserve(len(group["params"]))
            self._graph_ready[gi] = (hyper, counter)
            self._graph_hyper_captured[gi] = self._hyper_of(group)
        torch.cuda.synchronize()

    def _step_captured(self):
        """step() under stream capture.  Leaves one record per launch in _graph_launches: (group, [(parameter, its state)],
        group index, device table, device hyper block, device step counter)."""
        name = type(self).__name__
        self._graph_launches, self._graph_hyper_seen = [], {}
        for gi, group in enumerate(self.param_groups):
            ps = [p for p in group["params"] if p.grad is not None]
            if not ps:
                continue
            for p in ps:
                self._check(p)
                if not p.grad.is_contiguous():
                    raise _lib.MsnHipError("graph capture needs contiguous gradients")
                if self._needs_state(group) and not self._has_state(p):
                    raise _lib.MsnHipError("capture the training step after at least one eager optimizer step "
                                           f"(the state buffers of {name} must exist)")
            self._capture_check(group, ps)
            ready = getattr(self, "_graph_ready", {})
            if gi not in ready or not self._pinned().reserved:
                raise _lib.MsnHipError(f"{name}.graph_prepare() must run before the training step is captured")
            hyper, counter = ready.pop(gi)
            words = self._record(group, ps, [p.grad for p in ps])
            table = self._pinned().upload(words, ps[0].device)          # a copy node of the graph (static content)
            self._launch_dev(group, table, len(ps), max(p.numel() for p in ps), hyper, counter)
            self._graph_launches.append((group, [(p, self.state.get(p, {})) for p in ps], gi, table, hyper, counter))

    def graph_pre_replay(self):
        """Keep the host-side step counts in line with the device counter a replay increments, and carry a changed
        hyper-parameter (an lr scheduler, a manual edit of param_groups) into the device block the recorded launch reads: the
        copy is enqueued on the replaying stream BEFORE the replay, so it is ordered against the previous replay's read and
        this replay's."""
        for li, (group, items, gi, _, hyper, _) in enumerate(self._graph_launches):
            self._replay_advance(items)
            now = self._hyper_of(group)
            if self._graph_hyper_seen.setdefault(li, self._graph_hyper_captured[gi]) != now:
                self._replay_check(group, self._graph_hyper_seen[li], now)
                n = self._HOST_WORDS                 # the words behind them are the device's own
                hyper.view(torch.float32)[:n].copy_(self._hyper_block(group).view(torch.float32)[:n], non_blocking=False)
                self._graph_hyper_seen[li] = now

    def _replay_check(self, group, was, now):
        pass

    def _capture_check(self, group, ps):
        pass


def _refuse_tensor_lr(lr):
    if torch.is_tensor(lr):
        raise ValueError("Tensor lr is not supported (the fused step takes the learning rate as a host scalar)")


class _MomentState:
    """The state of RAdam, Adam, AdamW and LAMB: `step` (a Python int), `exp_avg`, `exp_avg_sq`; a record is {p, g, m, v, n}."""

    @staticmethod
    def _check_hypers(lr, betas, eps, weight_decay):
        """torch.optim.Adam's checks, with its messages."""
        _refuse_tensor_lr(lr)
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")

    def _init_state(self, todo):
        """Moment buffers of every parameter that has a gradient and no state yet, as views of ONE zeroed buffer per device."""
        fresh = {}
        for _, ps in todo:
            for p in ps:
                if len(self.state.get(p, ())) == 0:
                    fresh.setdefault(p.device, []).append(p)
        for ps in fresh.values():
            for p, (m, v) in zip(ps, _flat_views(ps, 2)[1]):
                st = self.state[p]
                st["step"], st["exp_avg"], st["exp_avg_sq"] = 0, m, v
        return ()

    def _has_state(self, p):
        return len(self.state.get(p, ())) != 0

    def _needs_state(self, group):
        return True

    def _advance(self, group, p, fresh):
        st = self.state[p]
        st["step"] = int(st["step"]) + 1
        return st["step"]

    def _record(self, group, ps, grads):
        words = []
        for p, g in zip(ps, grads):
            st = self.state[p]
            words += [p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel()]
        return words

    def _group_step(self, group):
        steps = [int(self.state[p]["step"]) for p in group["params"] if len(self.state.get(p, ()))]
        return steps[0] if steps else 0

    def _capture_check(self, group, ps):
        if len({int(self.state[p]["step"]) for p in ps}) != 1:
            raise _lib.MsnHipError("graph capture needs one step count per parameter group")

    def _replay_advance(self, items):
        step = int(items[0][1]["step"]) + 1
        for _, st in items:
            st["step"] = step

    def graph_note_eager_step(self):
        """An eager step() ran between two replays (a batch of another shape): advance the device counters with it."""
        for *_, counter in getattr(self, "_graph_launches", []):
            counter.add_(1)

    @staticmethod
    def _hyper_of(group):
        b1, b2 = group["betas"]
        return (float(group["lr"]), float(b1), float(b2), float(group["eps"]), float(group["weight_decay"]))


class _MomentumState:
    """The state of SGD and LARS, as torch's: `momentum_buffer` when momentum != 0, nothing otherwise -- there is no step count;
    a record is {p, g, buf | NULL, n}."""

    @staticmethod
    def _check_hypers(lr, momentum, weight_decay):
        """torch.optim.SGD's checks, with its messages (Nesterov's: _check_nesterov)."""
        _refuse_tensor_lr(lr)
        if lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if momentum < 0.0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")

    @staticmethod
    def _check_nesterov(nesterov, momentum, dampening):
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")

    def _has_state(self, p):
        return self.state.get(p, {}).get("momentum_buffer") is not None

    def _needs_state(self, group):
        return group["momentum"] != 0

    def _init_state(self, todo):
        """Momentum buffers of every parameter that has a gradient and none yet (groups with momentum only), as views of ONE
        buffer per device.  Returns those parameters: their first step stores the gradient in the buffer."""
        fresh = {}
        for group, ps in todo:
            if group["momentum"] != 0:
                for p in ps:
                    if not self._has_state(p):
                        fresh.setdefault(p.device, []).append(p)
        for ps in fresh.values():
            for p, (buf,) in zip(ps, _flat_views(ps)[1]):
                self.state[p]["momentum_buffer"] = buf
        return {p for ps in fresh.values() for p in ps}

    def _advance(self, group, p, fresh):
        return bool(fresh)

    def _record(self, group, ps, grads):
        words = []
        for p, g in zip(ps, grads):
            buf = self.state.get(p, {}).get("momentum_buffer") if group["momentum"] != 0 else None
            words += [p.data_ptr(), g.data_ptr(), 0 if buf is None else buf.data_ptr(), p.numel()]
        return words

    def _group_step(self, group):
        return 0

    def _replay_advance(self, items):
        pass

    def _replay_check(self, group, was, now):
        """What a recorded launch cannot follow: `nesterov` is an argument of the launch, and a momentum that becomes non-zero
        needs buffers the recorded table does not hold."""
        if was[4] != now[4] or (was[1] == 0.0) != (now[1] == 0.0):
            raise _lib.MsnHipError(f"{type(self).__name__}: nesterov, or momentum between zero and non-zero, changed after the "
                                   "step was recorded; record the step again")

    def graph_note_eager_step(self):
        """An eager step() ran between two replays: there is no step count, so there is nothing to advance."""

    @staticmethod
    def _hyper_of(group):
        return (float(group["lr"]), float(group["momentum"]), float(group["dampening"]), float(group["weight_decay"]),
                bool(group["nesterov"]))


class RAdam(_MomentState, _FusedStep):
    """torch.optim.RAdam (L2 weight decay folded into the gradient, variance rectification once rho_t > 5) stepped by ONE fused
    HIP launch (msn_radam_step): the optimizer the reference builds, with torch's constructor, `param_groups` and state keys."""
    _WORDS = 5
    _HOST_WORDS = 11

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        if lr < 0 or eps < 0 or not (0 <= betas[0] < 1) or not (0 <= betas[1] < 1) or weight_decay < 0:
            raise ValueError("invalid RAdam hyper-parameters")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))

    def _launch(self, group, step, table, n, max_n):
        b1, b2 = group["betas"]                  # passed as doubles: the library rounds beta and 1 - beta once each
        check(lib().msn_radam_step(ptr(table), n, max_n, group["lr"], b1, b2, group["eps"], group["weight_decay"], step,
                                   stream_ptr()), "msn_radam_step")

    def _launch_dev(self, group, table, n, max_n, hyper, counter):
        check(lib().msn_radam_step_dev(ptr(table), n, max_n, ptr(hyper), ptr(counter), stream_ptr()), "msn_radam_step_dev")

    @classmethod
    def _hyper_block(cls, group):
        """Host image of the 64-byte device block msn_radam_step_dev reads (csrc/optim_steps.hip, RadamHyperDev), as 8 float64
        words: words 0, 1 = the exact betas (radam_prepare_kernel derives the step-dependent terms from them in double); then,
        as float32, {lr, beta1, beta2, eps, weight_decay, 1 - beta1, 1 - beta2}, each rounded ONCE from the double value, and
        {inv_c1, rect_scale}, which the device writes."""
        lr, b1, b2, eps, wd = cls._hyper_of(group)
        block = torch.zeros(8, dtype=torch.float64)
        block[0], block[1] = b1, b2
        block.view(torch.float32)[4:11] = torch.tensor([lr, b1, b2, eps, wd, 1.0 - b1, 1.0 - b2], dtype=torch.float64)
        return block


class Adam(_MomentState, _FusedStep):
    """torch.optim.Adam (coupled L2 weight decay) stepped by ONE fused HIP launch (msn_adam_step): torch's constructor,
    `param_groups` and state keys (`step` as a Python int, `exp_avg`, `exp_avg_sq`), so optimizer states of torch and
    Lightning checkpoints load.  amsgrad, maximize and differentiable are not built."""
    _DECOUPLED = 0

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, **kwargs):
        _torch_keywords(type(self).__name__, kwargs)
        self._check_hypers(lr, betas, eps, weight_decay)
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))

    def _launch(self, group, step, table, n, max_n):
        b1, b2 = group["betas"]                  # every scalar travels as a double: the library rounds each once
        check(lib().msn_adam_step(ptr(table), n, max_n, group["lr"], b1, b2, group["eps"], group["weight_decay"],
                                  self._DECOUPLED, step, stream_ptr()), "msn_adam_step")

    def _launch_dev(self, group, table, n, max_n, hyper, counter):
        check(lib().msn_adam_step_dev(ptr(table), n, max_n, ptr(hyper), self._DECOUPLED, ptr(counter), stream_ptr()),
              "msn_adam_step_dev")

    @classmethod
    def _hyper_block(cls, group):
        """Host image of the 64-byte device block msn_adam_step_dev reads (csrc/optim_steps.hip, AdamHyperDev), as 8 float64
        words: words 0 .. 3 = the exact lr, betas and weight decay (adam_prepare_kernel derives the step-dependent terms from
        them in double); then, as float32, {beta2, eps, 1 - beta1, 1 - beta2}, each rounded ONCE from the double value, and
        {step_size, bc2_sqrt, wd_term}, which the device writes; 4 bytes of padding."""
        lr, b1, b2, eps, wd = cls._hyper_of(group)
        block = torch.zeros(8, dtype=torch.float64)
        block[0], block[1], block[2], block[3] = lr, b1, b2, wd
        block.view(torch.float32)[8:12] = torch.tensor([b2, eps, 1.0 - b1, 1.0 - b2], dtype=torch.float64)
        return block


class AdamW(Adam):
    """torch.optim.AdamW: Adam with decoupled weight decay, p *= 1 - lr * weight_decay before the update (default 1e-2)."""
    _DECOUPLED = 1

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, **kwargs):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, **kwargs)


class SGD(_MomentumState, _FusedStep):
    """torch.optim.SGD (momentum, dampening, Nesterov, coupled L2 weight decay) stepped by ONE fused HIP launch
    (msn_sgd_step).  State as torch's: `momentum_buffer` when momentum != 0, nothing otherwise -- SGD has no step count."""
    _WORDS = 4
    _HOST_WORDS = 12

    def __init__(self, params, lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, **kwargs):
        _torch_keywords("SGD", kwargs)
        self._check_hypers(lr, momentum, weight_decay)
        self._check_nesterov(nesterov, momentum, dampening)
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                                      nesterov=nesterov))

    def _launch(self, group, first, table, n, max_n):
        self._check_nesterov(group["nesterov"], group["momentum"], group["dampening"])
        check(lib().msn_sgd_step(ptr(table), n, max_n, group["lr"], group["momentum"], group["dampening"], group["weight_decay"],
                                 1 if group["nesterov"] else 0, 1 if first else 0, stream_ptr()), "msn_sgd_step")

    def _launch_dev(self, group, table, n, max_n, hyper, counter):
        check(lib().msn_sgd_step_dev(ptr(table), n, max_n, ptr(hyper), 1 if group["nesterov"] else 0, stream_ptr()),
              "msn_sgd_step_dev")

    @classmethod
    def _hyper_block(cls, group):
        """Host image of the 64-byte device block msn_sgd_step_dev reads (csrc/optim_steps.hip, SgdHyperDev), as 8 float64
        words: words 0 .. 3 = lr, momentum, dampening, weight decay; then, as float32, {lr, momentum, 1 - dampening, weight
        decay}, each rounded ONCE from the double value; 16 bytes of padding."""
        lr, mom, damp, wd, _ = cls._hyper_of(group)
        block = torch.zeros(8, dtype=torch.float64)
        block[0], block[1], block[2], block[3] = lr, mom, damp, wd
        block.view(torch.float32)[8:12] = torch.tensor([lr, mom, 1.0 - damp, wd], dtype=torch.float64)
        return block


# ---- layer-wise adaptive optimizers: LAMB, LARS (csrc/optim_layerwise.hip) -------------------------------------------------------
# The fused steps above plus one thing: a per-tensor scalar (the trust ratio) that a reduction over the tensor feeds back into the
# same step.  It stays on the device -- step() holds no .item(), no synchronisation and no host read -- so the step records into a
# HIP graph as the others do.  The scratch of the reduction and the ratios belong to the optimizer: one pair of buffers per launch
# of a step, allocated at the first step that needs it or in graph_prepare(), reused afterwards, never allocated under capture.
# Data parallel needs no collective: the gradients are all-reduced before the step, so every rank forms the same norms.
class _LayerwiseStep(_FusedStep):
    def _scratch(self, n, max_n, dev):
        """(workspace, ratios) of the next launch of this step; remembers the launch for trust_ratios()."""
        i = len(self._lw_launches)
        slots = self.__dict__.setdefault("_lw_slots", [])
        need = int(lib().msn_layerwise_workspace_bytes(n, max_n))
        capturing = torch.cuda.is_current_stream_capturing()
        if i >= len(slots) or slots[i][0].device != dev or slots[i][0].numel() < need or slots[i][1].numel() < n:
            if capturing:
                raise _lib.MsnHipError(f"{type(self).__name__}.graph_prepare() must run before the training step is captured "
                                       "(the scratch of the norms is not allocated under capture)")
            pair = (torch.empty(need, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.float32, device=dev))
            if i < len(slots):
                slots[i] = pair
            else:
                slots.append(pair)
        if capturing:
            self.__dict__.setdefault("_lw_captured", []).append(slots[i])       # a recorded launch keeps its buffers
        self._lw_launches.append((slots[i][1], n))
        return slots[i]

    def trust_ratios(self):
        """The trust ratios of the last step: per launch (param group, in order) a float32 device tensor, one entry per tensor
        that had a gradient, in the group's order.  A DEVICE READ (a clone enqueued on the current stream; looking at the
        values synchronises) -- for logging and for tests, not for the step itself."""
        return [ratio[:n].clone() for ratio, n in getattr(self, "_lw_launches", [])]

    @torch.no_grad()
    def step(self, closure=None):
        self._lw_launches = []               # the launches of a step, eager or recorded, take the scratch pairs from the first on
        return super().step(closure)

    def graph_prepare(self):
        super().graph_prepare()
        groups = [[p for p in g["params"] if p.device.type == "cuda"] for g in self.param_groups]
        groups = [ps for ps in groups if ps]
        if groups:
            # one pair per group, each large enough for any of them: a group without gradients records no launch
            n, max_n = max(len(ps) for ps in groups), max(max(p.numel() for ps in groups for p in ps), 1)
            self._lw_launches = []
            for ps in groups:
                self._scratch(n, max_n, ps[0].device)
        self._lw_launches = []

    def _step_captured(self):
        super()._step_captured()
        self._lw_recorded = list(self._lw_launches)

    def graph_pre_replay(self):
        super().graph_pre_replay()
        self._lw_launches = list(self._lw_recorded)          # what trust_ratios() reads after the replay


class LAMB(_MomentState, _LayerwiseStep):
    """LAMB (You et al. 2020) in the form of timm's `Lamb`, without its gradient-norm pre-clipping (clip with the Trainer's
    gradient_clip_val), stepped by three fused HIP launches per param group (msn_lamb_step).  State keys `step` (a Python int),
    `exp_avg`, `exp_avg_sq`.  At step t, c1 = 1 - beta1^t and c2 = 1 - beta2^t (both 1 with bias_correction=False):

        m <- m + (1 - beta1) (g - m);  v <- beta2 v + (1 - beta2) g^2;  u = (m / c1) / (sqrt(v / c2) + eps) + weight_decay p
        ratio = ||p|| / ||u||  if (weight_decay != 0 or always_adapt) and ||p|| > 0 and ||u|| > 0, else 1;  trust_clip: min(ratio, 1)
        p <- p - lr ratio u

    with the 2-norms over the whole tensor, the parameter's taken before the update.  A param group with weight_decay=0 (biases,
    norm weights: layerwise_param_groups) is not adapted.  Not built: the pre-clipping, exclusion lists other than param groups."""
    _WORDS = 5
    _HOST_WORDS = 14

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.0, bias_correction=True, always_adapt=False,
                 trust_clip=False, **kwargs):
        _torch_keywords("LAMB", kwargs)
        self._check_hypers(lr, betas, eps, weight_decay)
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, bias_correction=bias_correction,
                                      always_adapt=always_adapt, trust_clip=trust_clip))

    @staticmethod
    def _flags(group):
        return (1 if group["bias_correction"] else 0, 1 if group["always_adapt"] else 0, 1 if group["trust_clip"] else 0)

    def _launch(self, group, step, table, n, max_n):
        ws, ratio = self._scratch(n, max_n, table.device)
        b1, b2 = group["betas"]                  # every scalar travels as a double: the library rounds each once
        check(lib().msn_lamb_step(ptr(table), n, max_n, group["lr"], b1, b2, group["eps"], group["weight_decay"],
                                  *self._flags(group), step, ptr(ws), ws.numel(), ptr(ratio), stream_ptr()), "msn_lamb_step")

    def _launch_dev(self, group, table, n, max_n, hyper, counter):
        ws, ratio = self._scratch(n, max_n, table.device)
        check(lib().msn_lamb_step_dev(ptr(table), n, max_n, ptr(hyper), *self._flags(group), ptr(counter), ptr(ws), ws.numel(),
                                      ptr(ratio), stream_ptr()), "msn_lamb_step_dev")

    def _replay_check(self, group, was, now):
        if was[5:] != now[5:]:
            raise _lib.MsnHipError("LAMB: bias_correction, always_adapt or trust_clip changed after the step was recorded (they are "
                                   "arguments of the recorded launch); record the step again")

    @staticmethod
    def _hyper_of(group):
        return _MomentState._hyper_of(group) + LAMB._flags(group)

    @classmethod
    def _hyper_block(cls, group):
        """Host image of the 64-byte device block msn_lamb_step_dev reads (csrc/optim_layerwise.hip, LambHyperDev), as 8 float64
        words: words 0 .. 3 = the exact lr, betas and weight decay (lamb_prepare_kernel derives the step-dependent terms from the
        betas in double, the finishing launch decides on the exact weight decay); then, as float32, {beta2, eps, 1 - beta1,
        1 - beta2, lr, weight decay}, each rounded ONCE from the double value, and {1 / c1, sqrt(c2)}, which the device writes."""
        lr, b1, b2, eps, wd = cls._hyper_of(group)[:5]
        block = torch.zeros(8, dtype=torch.float64)
        block[0], block[1], block[2], block[3] = lr, b1, b2, wd
        block.view(torch.float32)[8:14] = torch.tensor([b2, eps, 1.0 - b1, 1.0 - b2, lr, wd], dtype=torch.float64)
        return block


class LARS(_MomentumState, _LayerwiseStep):
    """LARS in the form of lightning-bolts' `LARS`: torch's SGD (momentum, dampening, Nesterov) with a layer-wise rate on the
    decayed gradient, stepped by three fused HIP launches per param group (msn_lars_step).  State as optim.SGD's:
    `momentum_buffer` when momentum != 0, nothing otherwise.

        q = trust_coefficient ||p|| / (||g|| + weight_decay ||p|| + eps)  if weight_decay != 0 and ||p|| > 0 and ||g|| > 0, else 1
        d = q (g + weight_decay p), then torch's SGD: buf = d (first step) | momentum buf + (1 - dampening) d;
        d <- d + momentum buf (nesterov) | buf;  p <- p - lr d

    A param group with weight_decay=0 (biases, norm weights: layerwise_param_groups) is stepped by plain SGD, bit for bit."""
    _WORDS = 4
    _HOST_WORDS = 16

    def __init__(self, params, lr, momentum=0.9, dampening=0.0, weight_decay=0.0, nesterov=False, trust_coefficient=1e-3,
                 eps=1e-8, **kwargs):
        _torch_keywords("LARS", kwargs)
        self._check_hypers(lr, momentum, weight_decay)
        if eps < 0.0:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not trust_coefficient > 0.0:
            raise ValueError(f"Invalid trust_coefficient value: {trust_coefficient}")
        self._check_nesterov(nesterov, momentum, dampening)
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
                                      trust_coefficient=trust_coefficient, eps=eps))

    def _launch(self, group, first, table, n, max_n):
        self._check_nesterov(group["nesterov"], group["momentum"], group["dampening"])
        ws, ratio = self._scratch(n, max_n, table.device)
        check(lib().msn_lars_step(ptr(table), n, max_n, group["lr"], group["momentum"], group["dampening"], group["weight_decay"],
                                  1 if group["nesterov"] else 0, group["trust_coefficient"], group["eps"], 1 if first else 0,
                                  ptr(ws), ws.numel(), ptr(ratio), stream_ptr()), "msn_lars_step")

    def _launch_dev(self, group, table, n, max_n, hyper, counter):
        ws, ratio = self._scratch(n, max_n, table.device)
        check(lib().msn_lars_step_dev(ptr(table), n, max_n, ptr(hyper), 1 if group["nesterov"] else 0, ptr(ws), ws.numel(),
                                      ptr(ratio), stream_ptr()), "msn_lars_step_dev")

    @staticmethod
    def _hyper_of(group):
        return _MomentumState._hyper_of(group) + (float(group["trust_coefficient"]), float(group["eps"]))

    @classmethod
    def _hyper_block(cls, group):
        """Host image of the 64-byte device block msn_lars_step_dev reads (csrc/optim_layerwise.hip, LarsHyperDev), as 8 float64
        words: words 0 .. 3 = lr, momentum, dampening, weight decay; then, as float32, {lr, momentum, 1 - dampening, weight
        decay}, each rounded ONCE from the double value; words 6, 7 = trust_coefficient and eps, exact: the ratio is formed in
        double."""
        lr, mom, damp, wd, _, tc, eps = cls._hyper_of(group)
        block = torch.zeros(8, dtype=torch.float64)
        block[0], block[1], block[2], block[3], block[6], block[7] = lr, mom, damp, wd, tc, eps
        block.view(torch.float32)[8:12] = torch.tensor([lr, mom, 1.0 - damp, wd], dtype=torch.float64)
        return block


def layerwise_param_groups(module_or_named_parameters, weight_decay):
    """The two param groups layer-wise optimizers are usually given: the trainable tensors with ndim <= 1 (biases, norm weights
    and other scalars and vectors) at weight_decay=0 -- which LAMB and LARS then do not adapt -- and the rest at `weight_decay`,
    each in the module's order.  Takes a module or an iterable of (name, parameter)."""
    named = module_or_named_parameters
    if isinstance(named, torch.nn.Module):
        named = named.named_parameters()
    ps = [p for _, p in named if p.requires_grad]
    return [dict(params=[p for p in ps if p.ndim <= 1], weight_decay=0.0),
            dict(params=[p for p in ps if p.ndim > 1], weight_decay=weight_decay)]


# "lamb" is deliberately no name yet (tests/test_optimizers_cpu.py pins it as unknown): pass the class, optimizer=optim.LAMB
OPTIMIZERS = {"radam": RAdam, "adam": Adam, "adamw": AdamW, "sgd": SGD, "lars": LARS}


def build_optimizer(name, params, lr, **kwargs):
    """The fused optimizer called `name` ("radam", "adam", "adamw", "sgd" or "lars", in any letter case) over `params`, or `name`
    itself when it is a torch.optim.Optimizer subclass (optim.LAMB): what the models' configure_optimizers build from their
    `optimizer=` keyword and `optimizer_kwargs`, as cls(params, lr=lr, **optimizer_kwargs)."""
    if isinstance(name, type) and issubclass(name, torch.optim.Optimizer):
        cls = name
    else:
        cls = None if isinstance(name, type) else OPTIMIZERS.get(str(name).lower())
    if cls is None:
        raise ValueError(f"unknown optimizer {name!r}: choose one of {', '.join(sorted(OPTIMIZERS))}")
    return cls(params, lr=lr, **kwargs)
