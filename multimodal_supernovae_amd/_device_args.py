"""What metrics.py, calibration.py, probes.py and models_finetune.py hand to the evaluation kernels, checked in one place:
row matrices and their targets on the GPU, int64 accumulators, scratch, and the accumulators' life over a validation epoch.
Private: the messages name the caller (`who`), and every one of them is part of that caller's interface."""
import numpy as np
import torch

from . import _lib
from . import distributed as D

MAX_CLASSES = 1024

# How each kind of row matrix has always been described, and whether its device is looked at before its dtype.
_ROWS = {"scores": ("a float32 (N, C) tensor", False), "embeddings": ("float32 (N, D)", True)}


def ld(t):
    """Row stride of a (N, C) tensor as the kernels want it: a single row may carry any stride, also one below C."""
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])


def rows_on_gpu(t, who, noun, max_cols=None):
    """float32 (N, C) rows on the GPU as the kernels read them: any row stride >= C is kept, anything else is made dense."""
    phrase, device_first = _ROWS[noun]
    is_tensor = isinstance(t, torch.Tensor)
    wrong_kind = not is_tensor or t.dim() != 2 or t.dtype != torch.float32
    if device_first:
        _lib.require_gpu()
    if (not is_tensor or t.device.type != "cuda") and (device_first or not wrong_kind):
        raise _lib.MsnHipError(f"{who}: {noun} must live on the GPU (got {getattr(t, 'device', type(t).__name__)}); "
                               "there is no CPU path")
    if wrong_kind:
        raise ValueError(f"{who}: {noun} must be {phrase} (got {getattr(t, 'dtype', type(t).__name__)} "
                         f"{tuple(getattr(t, 'shape', ()))})")
    _lib.require_gpu()
    N, C = t.shape
    if N == 0:
        raise ValueError(f"{who}: no rows")
    if max_cols is not None and not 1 <= C <= max_cols:
        raise _lib.MsnHipError(f"{who}: 1 to {max_cols} classes (got {C})")
    t = t.detach()
    if (t.stride(1) != 1 and C > 1) or t.stride(0) < C:
        t = t.contiguous()
    return t


def targets_next_to(S, target, who):
    """int64 (N) targets on the GPU of the (N, C) rows S, contiguous."""
    N = S.shape[0]
    if not isinstance(target, torch.Tensor) or target.shape != (N,) or target.dtype != torch.int64:
        raise ValueError(f"{who}: targets must be an int64 tensor of shape ({N},) (got {getattr(target, 'dtype', type(target).__name__)} "
                         f"{tuple(getattr(target, 'shape', ()))})")
    if target.device != S.device:
        raise _lib.MsnHipError(f"{who}: targets must live on the GPU next to the scores (got {target.device}); there is no CPU path")
    return target.detach().contiguous()


def scores_and_targets(scores, target, who):
    """Scores float32 (N, C), C <= MAX_CLASSES, and targets int64 (N) on one GPU."""
    S = rows_on_gpu(scores, who, "scores", MAX_CLASSES)
    return S, targets_next_to(S, target, who)


def accumulator(t, shape, device, who):
    """The int64 accumulator a call adds to: `t` as given, or zeros."""
    if t is None:
        return torch.zeros(shape, dtype=torch.int64, device=device)
    if t.shape != shape or t.dtype != torch.int64 or t.device != device or not t.is_contiguous():
        raise ValueError(f"{who}: the accumulator must be a contiguous int64 {tuple(shape)} tensor on {device}")
    return t


def workspace(nbytes, device):
    """Scratch for an entry point that takes a pointer and a byte count (pass numel()); never empty, so the pointer is real."""
    return torch.empty(max(int(nbytes), 8), dtype=torch.uint8, device=device)


# numpy twins for the restatements and the host halves
def to_numpy(a, dtype):
    return np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a, dtype=dtype)


def reference_inputs(S, y, n_classes, who):
    """(S fp32 (N, C), y int64 (N), C, the mask of the rows whose target lies in [0, C))."""
    S = np.asarray(S, dtype=np.float32)
    y = np.asarray(y).astype(np.int64)
    if S.ndim != 2 or y.shape != (S.shape[0],):
        raise ValueError(f"{who}: scores (N, C) and targets (N,) needed (got {S.shape} and {y.shape})")
    C = S.shape[1] if n_classes is None else int(n_classes)
    if C != S.shape[1]:
        raise ValueError(f"{who}: {S.shape[1]} score columns for {C} classes")
    return S, y, C, (y >= 0) & (y < C)


class EpochCounts:
    """Integer accumulators of a validation epoch.  A subclass names them in `_counts` -- attributes that are None until
    `_buffers(device)`, which it supplies, has allocated them -- and adds to them in its update."""
    _counts = ()

    def _allocated(self):
        return [t for t in (getattr(self, name) for name in self._counts) if t is not None]

    def reset(self):
        for t in self._allocated():
            t.zero_()

    def _all_reduce_counts(self, group, device):
        """SUM of every accumulator over the ranks, which is exact.  -> the accumulators' device, None in a world of one."""
        if D.world_size(group) == 1:
            return None
        first = getattr(self, self._counts[0])
        device = first.device if first is not None else torch.device(device if device is not None
                                                                     else f"cuda:{torch.cuda.current_device()}")
        self._buffers(device)
        for t in self._allocated():
            D.all_reduce_sum(t, group, kind="metric_all_reduce")
        return device

    def all_reduce(self, group=None, device=None):
        """Every rank enters, also one whose shard was empty (pass its device then): the SUM of the integer accumulators."""
        self._all_reduce_counts(group, device)
