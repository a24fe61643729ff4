"""Supervised heads on the CLIP towers: supernova classification and redshift regression (SURVEY.md section 2 rows 3, 4,
9, 11 -- what the reference's main script and its `ClipMLP` / finetune_clip.py train the towers for), with the reference's
names where SURVEY records them.  The reference's source is not pinned line by line here: the surface is this module's,
checked against a plain-PyTorch restatement in tests/test_supervised_gpu.py.

    cross_entropy(logits, target, weight=None)      -- F.cross_entropy(..., reduction="mean") on csrc/supervised.hip
    focal_loss(logits, target, weight, gamma, label_smoothing)
                                                    -- focal loss with label smoothing on csrc/focal_loss.hip (fp64 row
                                                       arithmetic); cross_entropy(label_smoothing > 0) is its gamma = 0;
                                                       focal_loss_reference restates it in longdouble
    class_balanced_weights(counts, beta)            -- class weights from the effective number of samples (host)
    ClassificationMetrics / RegressionMetrics       -- device accumulators (confusion matrix / six fp64 sums); compute()
                                                       is the one host copy, its arithmetic a pure function
    regression_loss(pred, target, kind, delta=, quantiles=)
                                                    -- mse / l1 / huber / log_cosh / gaussian_nll / pinball over the rows
                                                       with a finite target on csrc/regression_loss.hip (fp64 rows);
                                                       regression_loss_reference restates it in longdouble
    IntervalMetrics(mode, quantiles)                -- point metrics + calibration of the predicted sigma / coverage of the
                                                       predicted quantiles from integer counts (interval_metrics on the host)
    ClipMLP(clip_model, classification=True | regression=True, ...)
                                                    -- MLP head on the concatenated unit-norm embeddings of a
                                                       LightCurveImageCLIP, optionally with a frozen backbone

Data parallel: the Trainer SUM-all-reduces parameter gradients, so every rank's loss is its numerator over the GLOBAL
denominator (rows, or class-weight sum) and the returned value is the all-reduced global loss: a 2-rank step equals the
single-process step at the doubled batch.
"""
import torch
import torch.nn as nn

from . import _lib
from . import distributed as D
from ._device_args import workspace
from ._lib import check, lib, ptr, stream_ptr
from .loss import _AllReduceSum
from .models_multimodal import MLP
from .models_pretraining import masked_mse
from .ops import _f32c

_TOWER_ORDER = ("host_galaxy", "lightcurve", "spectral")      # LightCurveImageCLIP.forward's fixed order (img, lc, sp)


# ------------------------------------------------------------------------------------------- cross-entropy
def _loss_args(who, logits, target, weight):
    """The checked (logits, target, weight) of a classification loss: float32 (N, C) logits with unit column stride on the
    GPU, contiguous int64 targets, contiguous float32 weights or None."""
    _lib.require_gpu()
    if logits.dim() != 2:
        raise ValueError(f"{who}: logits must be (N, C) (got {tuple(logits.shape)})")
    if logits.device.type != "cuda" or logits.dtype != torch.float32:
        raise _lib.MsnHipError(f"{who}: logits must be float32 on the GPU (got {logits.dtype} on {logits.device}); "
                               "there is no CPU path")
    if logits.stride(1) != 1:
        logits = logits.contiguous()
    N, C = logits.shape
    if target.shape != (N,) or target.dtype != torch.int64 or target.device != logits.device:
        raise ValueError(f"{who}: target must be int64 of shape ({N},) on {logits.device}")
    target = target.contiguous()
    if weight is not None:
        if weight.shape != (C,):
            raise ValueError(f"{who}: weight must have shape ({C},)")
        weight = _f32c(weight.detach(), "weight")
    return logits, target, weight


class _CrossEntropy(torch.autograd.Function):
    """Returns (loss, pred): loss = this process's numerator over the denominator (its own, or the ranks' sum when
    `sharded`); pred = row arg-max (int32, no gradient)."""

    @staticmethod
    def forward(ctx, logits, target, weight, group, sharded):
        logits, target, weight = _loss_args("cross_entropy", logits, target, weight)
        N, C = logits.shape
        dev = logits.device
        L = lib()
        lse = torch.empty(N, dtype=torch.float32, device=dev)
        pred = torch.empty(N, dtype=torch.int32, device=dev)
        out = torch.empty(3, dtype=torch.float32, device=dev)              # {loss, denominator, numerator}
        nb = L.msn_cross_entropy_workspace_bytes(N, C)
        ws = workspace(nb, dev) if nb else None                            # the shapes of training take one workgroup: no scratch
        check(L.msn_cross_entropy_fwd(ptr(logits), logits.stride(0), ptr(target), ptr(weight), N, C, ptr(None), ptr(lse),
                                      ptr(pred), ptr(out), ptr(ws), nb, stream_ptr()), "msn_cross_entropy_fwd")
        if sharded:
            denom = D.all_reduce_sum(out[1].clone(), group, kind="loss_denominator_all_reduce")
            loss = out[2] / denom                                          # this rank's share of the global mean
        else:
            denom, loss = out[1], out[0]
        ctx.save_for_backward(logits, target, weight, denom)
        ctx.mark_non_differentiable(pred)
        ctx.set_materialize_grads(False)        # no zero-filled "gradient" of the int32 predictions (a launch per backward)
        return loss, pred

    @staticmethod
    def backward(ctx, g, _gpred):
        if g is None:
            return None, None, None, None, None
        logits, target, weight, denom = ctx.saved_tensors
        N, C = logits.shape
        g = g.to(torch.float32).reshape(()).contiguous()
        dx = torch.empty((N, C), dtype=torch.float32, device=logits.device)
        check(lib().msn_cross_entropy_bwd(ptr(logits), logits.stride(0), ptr(target), ptr(weight), N, C, ptr(denom), ptr(g),
                                          ptr(dx), C, stream_ptr()), "msn_cross_entropy_bwd")
        return dx, None, None, None, None


def _cross_entropy(logits, target, weight=None, group=None, sharded=None):
    if sharded is None:
        sharded = D.world_size(group) > 1
    share, pred = _CrossEntropy.apply(logits, target, weight, group, bool(sharded))
    return (_AllReduceSum.apply(share, group) if sharded else share), pred


def cross_entropy(logits, target, weight=None, *, label_smoothing=0.0, group=None):
    """torch.nn.functional.cross_entropy(logits, target, weight=weight, label_smoothing=label_smoothing, reduction="mean")
    for float32 (N, C) logits on the GPU (2 <= C <= 1024), int64 targets, default ignore_index -100 (any target outside
    [0, C) is ignored likewise).  label_smoothing = 0 takes the kernels of csrc/supervised.hip, label_smoothing > 0 the
    focal-loss kernel at gamma = 0.  With torch.distributed initialised over more than one rank every rank passes its LOCAL
    rows and gets the global mean (see the module docstring); gradients of the ranks are then to be summed."""
    if float(label_smoothing) == 0.0:
        return _cross_entropy(logits, target, weight, group)[0]
    return _focal_loss(logits, target, weight, 0.0, label_smoothing, group)[0]


def argmax_rows(logits):
    """Row arg-max of (N, C) logits as int32 (first maximal index, as torch.argmax) from the cross-entropy forward kernel."""
    fake = torch.zeros(logits.shape[0], dtype=torch.int64, device=logits.device)
    return _cross_entropy(logits.detach(), fake, sharded=False)[1]


# ------------------------------------------------------------------------- focal loss and label smoothing
def _focal_params(who, gamma, label_smoothing):
    gamma, label_smoothing = float(gamma), float(label_smoothing)
    if not (0.0 <= gamma < float("inf")):
        raise ValueError(f"{who}: gamma must be finite and >= 0 (got {gamma})")
    if not (0.0 <= label_smoothing <= 1.0):
        raise ValueError(f"{who}: label_smoothing must be in [0, 1] (got {label_smoothing})")
    return gamma, label_smoothing


class _FocalLoss(torch.autograd.Function):
    """_CrossEntropy's contract on csrc/focal_loss.hip: returns (loss, pred), loss = this process's numerator over the
    denominator (its own, or the ranks' sum when `sharded`).  Backward recomputes the rows: nothing per row is saved."""

    @staticmethod
    def forward(ctx, logits, target, weight, gamma, label_smoothing, group, sharded):
        logits, target, weight = _loss_args("focal_loss", logits, target, weight)
        N, C = logits.shape
        dev = logits.device
        L = lib()
        pred = torch.empty(N, dtype=torch.int32, device=dev)
        out = torch.empty(3, dtype=torch.float32, device=dev)              # {loss, denominator, numerator}
        nb = L.msn_focal_loss_workspace_bytes(N, C)
        ws = workspace(nb, dev) if nb else None
        check(L.msn_focal_loss_fwd(ptr(logits), logits.stride(0), ptr(target), ptr(weight), N, C, gamma, label_smoothing,
                                   ptr(None), ptr(pred), ptr(out), ptr(ws), nb, stream_ptr()), "msn_focal_loss_fwd")
        if sharded:
            denom = D.all_reduce_sum(out[1].clone(), group, kind="loss_denominator_all_reduce")
            loss = out[2] / denom                                          # this rank's share of the global mean
        else:
            denom, loss = out[1], out[0]
        ctx.save_for_backward(logits, target, weight, denom)
        ctx.focal = (gamma, label_smoothing)
        ctx.mark_non_differentiable(pred)
        ctx.set_materialize_grads(False)
        return loss, pred

    @staticmethod
    def backward(ctx, g, _gpred):
        if g is None:
            return (None,) * 7
        logits, target, weight, denom = ctx.saved_tensors
        N, C = logits.shape
        g = g.to(torch.float32).reshape(()).contiguous()
        dx = torch.empty((N, C), dtype=torch.float32, device=logits.device)
        check(lib().msn_focal_loss_bwd(ptr(logits), logits.stride(0), ptr(target), ptr(weight), N, C, *ctx.focal, ptr(denom),
                                       ptr(g), ptr(dx), C, stream_ptr()), "msn_focal_loss_bwd")
        return (dx,) + (None,) * 6


def _focal_loss(logits, target, weight, gamma, label_smoothing, group=None, sharded=None):
    gamma, label_smoothing = _focal_params("focal_loss", gamma, label_smoothing)
    if sharded is None:
        sharded = D.world_size(group) > 1
    share, pred = _FocalLoss.apply(logits, target, weight, gamma, label_smoothing, group, bool(sharded))
    return (_AllReduceSum.apply(share, group) if sharded else share), pred


def focal_loss(logits, target, weight=None, gamma=2.0, label_smoothing=0.0, *, group=None):
    """Multiclass focal loss (Lin et al. 2017) with label smoothing, mean over the rows with a target in [0, C):

        sum_i sum_c q_ic w_c (1 - p_ic)^gamma (-log p_ic) / sum_i w[y_i],    q_ic = (1 - label_smoothing) [c == y_i] + label_smoothing / C

    for float32 (N, C) logits on the GPU (2 <= C <= 1024), int64 targets and optional class weights.  gamma = 0 is
    cross_entropy(..., label_smoothing=label_smoothing); label_smoothing = 0 is w_y (1 - p_y)^gamma (-log p_y).  Data parallel
    as cross_entropy.  Not built: soft targets, per-sample weights, the sigmoid (binary) form, reductions other than the mean."""
    return _focal_loss(logits, target, weight, gamma, label_smoothing, group)[0]


def focal_loss_reference(x, y, w=None, gamma=2.0, label_smoothing=0.0):
    """(loss, dlogits) of focal_loss restated in numpy longdouble, returned as a float and a float64 (N, C) array.  u = 1 - p
    and log p are formed as the kernel forms them -- from t = sum_{c != a} exp(x_c - m) with the leading 1 of the softmax
    denominator kept apart -- and the target's gradient entry takes u_y itself, so a row whose target wins by 40 keeps its
    (tiny) loss and gradient instead of rounding them to zero.  A column with coefficient q_c = 0 takes no part."""
    import numpy as np
    ld = np.longdouble
    x = np.asarray(x.detach().cpu() if torch.is_tensor(x) else x, dtype=ld)
    y = np.asarray(y.cpu() if torch.is_tensor(y) else y).astype(np.int64)
    N, C = x.shape
    w = np.ones(C, dtype=ld) if w is None else np.asarray(w.detach().cpu() if torch.is_tensor(w) else w, dtype=ld)
    gamma, eps = _focal_params("focal_loss_reference", gamma, label_smoothing)
    gamma, keep, smooth = ld(gamma), ld(1.0) - ld(eps), ld(eps) / ld(C)
    valid = (y >= 0) & (y < C)
    ys = np.where(valid, y, 0)
    rows = np.arange(N)
    with np.errstate(all="ignore"):
        a = np.argmax(x, axis=1)                                          # first maximal index
        m = x[rows, a]
        top = np.arange(C)[None, :] == a[:, None]
        d = np.where(top, ld(0), x - m[:, None])
        e = np.where(top, ld(1), np.exp(d))
        t = np.where(top, ld(0), e).sum(axis=1)
        S = (ld(1) + t)[:, None]
        nlp = np.log1p(t)[:, None] - d
        u = np.where(top, t[:, None], S - e) / S
        p = e / S
        pw = np.ones_like(u) if gamma == 0 else np.power(u, gamma)
        F = pw * (ld(1) + gamma * p * np.where(u == 0, ld(1), nlp / np.where(u == 0, ld(1), u)))
        hot = (np.arange(C)[None, :] == ys[:, None]) & valid[:, None]
        q = np.where(hot, keep, ld(0)) + smooth
        den = w[ys][valid].sum()
        terms = np.where((q != 0) & valid[:, None], q * w[None, :] * pw * nlp, ld(0))
        loss = terms.sum() / den
        b = -keep * w[ys] * F[rows, ys] if keep != 0 else np.zeros(N, dtype=ld)
        s = -smooth * w[None, :] * F if smooth != 0 else np.zeros_like(F)
        dx = b[:, None] * np.where(hot, u, -p) + s - p * s.sum(axis=1, keepdims=True)
        dx = np.where(valid[:, None], dx, ld(0)) / den
    return float(loss), dx.astype(np.float64)


def class_balanced_weights(counts, beta=0.999):
    """Class weights from the effective number of samples (Cui et al. 2019): w_c = (1 - beta) / (1 - beta^n_c), scaled to sum
    to the number of classes; a class without samples gets weight 0.  beta = 0 weighs every class that occurs alike.  Pure
    host function; returns a float64 tensor for ClipMLP(class_weights=) / focal_loss(weight=)."""
    n = torch.as_tensor(counts, dtype=torch.float64).reshape(-1)
    beta = float(beta)
    if not (0.0 <= beta < 1.0):
        raise ValueError(f"class_balanced_weights: beta must be in [0, 1) (got {beta})")
    if bool((n < 0).any()) or not bool((n > 0).any()):
        raise ValueError("class_balanced_weights: counts must be >= 0 with at least one class present")
    seen = n > 0
    w = torch.where(seen, (1.0 - beta) / (1.0 - torch.pow(torch.full_like(n, beta), n.clamp(min=1.0))), torch.zeros_like(n))
    return w * (n.numel() / w.sum())


# ------------------------------------------------------------------------------------------------- metrics
def classification_metrics(cm):
    """Pure host function of a (C, C) confusion matrix cm[true, predicted]: accuracy, per-class F1 = 2 tp / (2 tp + fp + fn),
    micro F1 from the summed counts, macro F1 = mean over the classes with tp + fp + fn > 0 (a class that neither occurs
    nor is predicted does not count as a zero: torchmetrics' macro average)."""
    cm = torch.as_tensor(cm).to(torch.float64)
    tp = cm.diagonal()
    fp = cm.sum(dim=0) - tp
    fn = cm.sum(dim=1) - tp
    den = 2 * tp + fp + fn
    seen = den > 0
    f1 = torch.where(seen, 2 * tp / den.clamp(min=1.0), torch.zeros_like(den))
    total = float(cm.sum())
    den_micro = float(den.sum())
    return {"acc": float(tp.sum()) / total if total > 0 else float("nan"),
            "f1_macro": float(f1[seen].mean()) if bool(seen.any()) else float("nan"),
            "f1_micro": 2 * float(tp.sum()) / den_micro if den_micro > 0 else float("nan"),
            "f1_per_class": [float(v) for v in f1]}


def regression_metrics(sums):
    """Pure host function of the six sums {n, sum|d|, sum d^2, sum y, sum y^2, n_out} (d = prediction - y): the keys of the
    reference's regression_metrics_list.pkl -- L1, L2 (mean absolute / squared error), R2, OLF (outlier fraction,
    |d| / (1 + y) > 0.15)."""
    n, sad, ssd, sy, syy, n_out = (float(v) for v in sums)
    if n <= 0:
        return {"L1": float("nan"), "L2": float("nan"), "R2": float("nan"), "OLF": float("nan")}
    var = syy - sy * sy / n
    return {"L1": sad / n, "L2": ssd / n, "R2": 1.0 - ssd / var if var != 0 else float("nan"), "OLF": n_out / n}


class ClassificationMetrics:
    """Confusion matrix accumulated on the device over the batches of a validation epoch (msn_confusion_matrix)."""

    def __init__(self, n_classes):
        self.n_classes = int(n_classes)
        self.cm = None

    def reset(self):
        if self.cm is not None:
            self.cm.zero_()

    def update(self, pred, target):
        """pred: int32 class per row (cross-entropy's arg-max) or (N, C) logits; target int64.  Enqueue only."""
        if pred.shape[0] == 0:             # an empty batch counts nothing
            return
        if pred.dim() == 2:
            pred = argmax_rows(pred)
        pred = pred.to(torch.int32).contiguous()
        target = target.to(torch.int64).contiguous()
        if self.cm is None or self.cm.device != pred.device:
            self.cm = torch.zeros((self.n_classes, self.n_classes), dtype=torch.int32, device=pred.device)
        check(lib().msn_confusion_matrix(ptr(target), ptr(pred), pred.numel(), self.n_classes, ptr(self.cm), stream_ptr()),
              "msn_confusion_matrix")

    def all_reduce(self, group=None):
        # NOTE: a rank that accumulated nothing skips the collective here and in RegressionMetrics (every rank of a validation
        # epoch has rows); _device_args.EpochCounts enters it on every rank.  Kept apart: joining them changes behaviour.
        if self.cm is not None and D.world_size(group) > 1:
            D.all_reduce_sum(self.cm, group, kind="metric_all_reduce")

    def compute(self):
        if self.cm is None:
            return classification_metrics(torch.zeros((self.n_classes, self.n_classes)))
        return classification_metrics(self.cm.cpu())


class RegressionMetrics:
    """The six fp64 sums accumulated on the device over the batches of a validation epoch (msn_regression_stats)."""

    def __init__(self):
        self.sums = None

    def reset(self):
        if self.sums is not None:
            self.sums.zero_()

    def update(self, pred, target):
        pred = _f32c(pred.detach().reshape(-1), "pred")
        target = _f32c(target.detach().reshape(-1).to(pred.device), "target")
        if pred.numel() != target.numel():
            raise ValueError("RegressionMetrics.update: prediction and target differ in length")
        if pred.numel() == 0:
            return
        if self.sums is None or self.sums.device != pred.device:
            self.sums = torch.zeros(6, dtype=torch.float64, device=pred.device)
        nb = lib().msn_regression_stats_workspace_bytes(pred.numel())
        ws = workspace(nb, pred.device) if nb else None
        check(lib().msn_regression_stats(ptr(pred), ptr(target), pred.numel(), ptr(self.sums), ptr(ws), nb, stream_ptr()),
              "msn_regression_stats")

    def all_reduce(self, group=None):
        if self.sums is not None and D.world_size(group) > 1:
            D.all_reduce_sum(self.sums, group, kind="metric_all_reduce")

    def compute(self):
        return regression_metrics(self.sums.cpu().tolist() if self.sums is not None else [0.0] * 6)


# ------------------------------------------------------------- robust, Gaussian-NLL and quantile regression
REGRESSION_KINDS = {"mse": 0, "l1": 1, "huber": 2, "log_cosh": 3, "gaussian_nll": 4, "pinball": 5}     # MSN_REGLOSS_*
_INTERVAL_MODES = {"point": 0, "gaussian": 1, "quantile": 2}                                           # MSN_REGSTATS_*
_MAX_LEVELS = 16
_N_CNT, _N_ACC = 3 + _MAX_LEVELS, 8
_LEVELS = {}                 # (levels, device) -> float64 device tensor, uploaded once outside graph capture


def _check_quantiles(who, quantiles):
    """The levels as a tuple of floats: 1..16 of them, strictly increasing inside (0, 1).  Checked here, on the host: the
    kernels never read them for validation."""
    try:
        q = tuple(float(v) for v in quantiles)
    except TypeError:
        raise ValueError(f"{who}: quantiles must be a sequence of levels (got {quantiles!r})") from None
    if not (1 <= len(q) <= _MAX_LEVELS):
        raise ValueError(f"{who}: quantiles must hold 1..{_MAX_LEVELS} levels (got {len(q)})")
    if not all(0.0 < v < 1.0 for v in q) or any(b <= a for a, b in zip(q, q[1:])):
        raise ValueError(f"{who}: quantiles must be strictly increasing inside (0, 1) (got {q})")
    return q


def _regression_params(who, kind, delta, quantiles):
    """-> (kind id, K, delta, levels or None), refusing what the kernels would refuse with a ValueError naming the argument."""
    if kind not in REGRESSION_KINDS:
        raise ValueError(f"{who}: kind must be one of {sorted(REGRESSION_KINDS)} (got {kind!r})")
    delta = float(delta)
    if kind == "huber" and not (0.0 < delta < float("inf")):
        raise ValueError(f"{who}: delta must be finite and > 0 (got {delta})")
    levels = None
    if kind == "pinball":
        if quantiles is None:
            raise ValueError(f"{who}: the pinball loss needs quantiles")
        levels = _check_quantiles(who, quantiles)
    elif quantiles is not None:
        raise ValueError(f"{who}: quantiles belong to the pinball loss (kind is {kind!r})")
    K = len(levels) if levels is not None else 2 if kind == "gaussian_nll" else 1
    return REGRESSION_KINDS[kind], K, delta, levels


def _levels_on(levels, device):
    """The levels as float64 on `device`, cached per (levels, device): a replayed graph must not contain the upload."""
    if levels is None:
        return None
    key = (levels, str(device))
    if key not in _LEVELS:
        if torch.cuda.is_current_stream_capturing():
            raise _lib.MsnHipError("regression_loss: the quantile levels reach the device outside graph capture -- run one eager "
                                   "step (GraphedTrainStep's warm-up does) before recording")
        _LEVELS[key] = torch.tensor(levels, dtype=torch.float64, device=device)
    return _LEVELS[key]


def _regression_args(who, pred, target, K):
    """The checked (pred, target): float32 (N, K) predictions with unit column stride on the GPU, float32 (N) targets."""
    _lib.require_gpu()
    if pred.device.type != "cuda" or pred.dtype != torch.float32:
        raise _lib.MsnHipError(f"{who}: pred must be float32 on the GPU (got {pred.dtype} on {pred.device}); there is no CPU path")
    if pred.dim() == 1 and K == 1:
        pred = pred.unsqueeze(1)
    if pred.dim() != 2 or pred.shape[1] != K:
        raise ValueError(f"{who}: pred must be (N, {K}) for this loss (got {tuple(pred.shape)})")
    N = pred.shape[0]
    if N and ((K > 1 and pred.stride(1) != 1) or pred.stride(0) < K):
        pred = pred.contiguous()
    if target.shape != (N,) or target.device != pred.device or not target.is_floating_point():
        raise ValueError(f"{who}: target must be floating point of shape ({N},) on {pred.device}")
    return pred, target.detach().to(torch.float32).contiguous()


class _RegressionLoss(torch.autograd.Function):
    """_CrossEntropy's contract on csrc/regression_loss.hip: this process's numerator over the number of valid rows (its own,
    or the ranks' sum when `sharded`).  No host read: GraphedTrainStep records it.  Backward recomputes the rows."""

    @staticmethod
    def forward(ctx, pred, target, kind, delta, taus, group, sharded):
        N, K = pred.shape
        dev = pred.device
        L = lib()
        out = torch.empty(3, dtype=torch.float32, device=dev)              # {loss, valid rows, numerator}
        nb = L.msn_regression_loss_workspace_bytes(N, K)
        ws = workspace(nb, dev) if nb else None
        check(L.msn_regression_loss_fwd(ptr(pred), pred.stride(0), ptr(target), N, K, kind, delta, ptr(taus), ptr(None), ptr(out),
                                        ptr(ws), nb, stream_ptr()), "msn_regression_loss_fwd")
        if sharded:
            denom = D.all_reduce_sum(out[1].clone(), group, kind="loss_denominator_all_reduce")
            loss = out[2] / denom                                          # this rank's share of the global mean
        else:
            denom, loss = out[1], out[0]
        ctx.save_for_backward(pred, target, taus, denom)
        ctx.reg = (kind, delta)
        return loss

    @staticmethod
    def backward(ctx, g):
        pred, target, taus, denom = ctx.saved_tensors
        N, K = pred.shape
        g = g.to(torch.float32).reshape(()).contiguous()
        dx = torch.empty((N, K), dtype=torch.float32, device=pred.device)
        check(lib().msn_regression_loss_bwd(ptr(pred), pred.stride(0), ptr(target), N, K, *ctx.reg, ptr(taus), ptr(denom), ptr(g),
                                            ptr(dx), K, stream_ptr()), "msn_regression_loss_bwd")
        return (dx,) + (None,) * 6


def _regression_loss(pred, target, kind, delta, levels, group=None, sharded=None):
    """regression_loss on checked parameters (kind id, levels tuple or None)."""
    K = len(levels) if levels is not None else 2 if kind == REGRESSION_KINDS["gaussian_nll"] else 1
    pred, target = _regression_args("regression_loss", pred, target, K)
    if pred.shape[0] == 0:
        raise ValueError("regression_loss: pred must hold at least one row")
    if sharded is None:
        sharded = D.world_size(group) > 1
    share = _RegressionLoss.apply(pred, target, kind, delta, _levels_on(levels, pred.device), group, bool(sharded))
    return _AllReduceSum.apply(share, group) if sharded else share


def regression_loss(pred, target, kind="mse", *, delta=1.0, quantiles=None, group=None):
    """Mean over the rows with a FINITE target of one of six row terms (d = pred - target), for float32 predictions on the GPU:

        "mse" d^2 | "l1" |d| | "huber" F.huber_loss(delta=delta) | "log_cosh" log cosh d          -- pred (N,) or (N, 1)
        "gaussian_nll"  (s + (mu - y)^2 exp(-s)) / 2 for pred (N, 2) = (mu, s = log variance):
                        F.gaussian_nll_loss(mu, y, var=exp(s), full=False, eps=0)
        "pinball"       (1 / K) sum_q max(tau_q e_q, (tau_q - 1) e_q), e_q = y - pred_q, for pred (N, K) and the K <= 16 levels
                        `quantiles` (strictly increasing inside (0, 1))

    A row whose target is NaN or infinite -- an object without a spectroscopic redshift -- is ignored as cross_entropy ignores
    -100: no term, no count, a gradient row of exact zeros; no valid row at all gives nan.  Subgradients at the kinks are
    torch's (0 at d = 0, d at |d| = delta, 0 at e_q = 0).  Row arithmetic is fp64 (csrc/regression_loss.hip), bitwise
    reproducible.  No host read: a graph records it.  Data parallel as cross_entropy: every rank passes its LOCAL rows and
    gets the global mean over the ranks' valid rows.  Not built: per-sample weights, smooth_l1, a beta-NLL, CRPS, K > 16."""
    kind_id, _, delta, levels = _regression_params("regression_loss", kind, delta, quantiles)
    return _regression_loss(pred, target, kind_id, delta, levels, group)


def _np_log_cosh(d):
    """log cosh d in the kernel's split: log1p(2 sinh^2(d / 2)) up to |d| = 1, |d| + log1p(exp(-2|d|)) - ln 2 beyond."""
    import numpy as np
    a = np.abs(d)
    small = a <= 1
    h = np.sinh(np.where(small, d, 0) / 2)
    big = np.where(small, 1, a)
    return np.where(small, np.log1p(2 * h * h), big + np.log1p(np.exp(-2 * big)) - np.log(np.longdouble(2)))


def regression_loss_reference(pred, target, kind, delta=1.0, quantiles=None):
    """(loss, dpred) of regression_loss restated in numpy longdouble, returned as a float and a float64 (N, K) array: the same
    valid-row rule (finite targets), the same log cosh split and the same subgradients as the kernels."""
    import numpy as np
    ld = np.longdouble
    _, K, delta, levels = _regression_params("regression_loss_reference", kind, delta, quantiles)
    p = np.asarray(pred.detach().cpu() if torch.is_tensor(pred) else pred)
    y = np.asarray(target.detach().cpu() if torch.is_tensor(target) else target)
    p = p.reshape(y.shape[0], K).astype(ld)
    valid = np.isfinite(y)
    y = np.where(valid, y, 0).astype(ld)
    delta = ld(delta)
    with np.errstate(all="ignore"):
        if kind == "pinball":
            tau = np.asarray(levels, dtype=np.float64).astype(ld)[None, :]
            e = y[:, None] - p
            rows = np.where(e > 0, tau * e, (tau - 1) * e).sum(axis=1) / K
            g = np.where(e > 0, -tau, np.where(e < 0, 1 - tau, e)) / K
        elif kind == "gaussian_nll":
            d, s = p[:, 0] - y, p[:, 1]
            w = np.exp(-s)
            rows = (s + d * d * w) / 2
            g = np.stack([d * w, (1 - d * d * w) / 2], axis=1)
        else:
            d = p[:, 0] - y
            a = np.abs(d)
            sign = np.where(d > 0, ld(1), np.where(d < 0, ld(-1), d))
            if kind == "mse":
                rows, g = d * d, 2 * d
            elif kind == "l1":
                rows, g = a, sign
            elif kind == "huber":
                rows, g = np.where(a <= delta, d * d / 2, delta * (a - delta / 2)), np.where(a <= delta, d, delta * sign)
            else:
                rows, g = _np_log_cosh(d), np.tanh(d)
            g = g[:, None]
        n = ld(int(valid.sum()))
        loss = np.where(valid, rows, ld(0)).sum() / n if n > 0 else ld("nan")
        dx = np.where(valid[:, None], g, ld(0)) / (n if n > 0 else ld(1))
    return float(loss), dx.astype(np.float64)


def interval_metrics(cnt, acc, mode, quantiles=None):
    """Pure host function of the counts and sums of msn_regression_interval_stats.  Every mode: L1, L2, R2, OLF of the point
    prediction (regression_metrics of acc[0..5]).  "gaussian": sigma_mean, z2_mean (mean squared standardised residual: 1 for
    a calibrated head) and cov1, cov2, cov3 (fractions of rows with |d| <= k sigma; 0.683, 0.954, 0.997 for a calibrated
    Gaussian).  "quantile": coverage (y inside [pred_0, pred_{K-1}]), width_mean of that interval, pinball (the mean row term),
    crossing (fraction of rows with some pred_q > pred_{q+1}) and cov_below (per level, the fraction of rows with
    y <= pred_q: tau_q for a calibrated head).  The fractions are ratios of integer counts."""
    if mode not in _INTERVAL_MODES:
        raise ValueError(f"interval_metrics: mode must be one of {sorted(_INTERVAL_MODES)} (got {mode!r})")
    cnt = [int(v) for v in cnt]
    acc = [float(v) for v in acc]
    res = regression_metrics(acc[:6])
    n = cnt[0]
    nan = float("nan")
    if mode == "gaussian":
        res.update(sigma_mean=acc[6] / n if n else nan, z2_mean=acc[7] / n if n else nan)
        for k in (1, 2, 3):
            res[f"cov{k}"] = cnt[k] / n if n else nan
    elif mode == "quantile":
        K = len(_check_quantiles("interval_metrics", quantiles))
        res.update(coverage=cnt[1] / n if n else nan, width_mean=acc[6] / n if n else nan, pinball=acc[7] / n if n else nan,
                   crossing=cnt[2] / n if n else nan, cov_below=[cnt[3 + q] / n if n else nan for q in range(K)])
    return res


class IntervalMetrics:
    """Validation statistics of a regression head over the rows with a finite target, accumulated on the device over the
    batches of an epoch (msn_regression_interval_stats): `cnt`, int64 counts, and `acc`, fp64 sums.  mode "point" (one
    prediction per row), "gaussian" ((mu, log variance) per row) or "quantile" (one column per level of `quantiles`; the
    point prediction is the column whose level is nearest 0.5, the lower index on a tie)."""

    def __init__(self, mode, quantiles=None):
        if mode not in _INTERVAL_MODES:
            raise ValueError(f"IntervalMetrics: mode must be one of {sorted(_INTERVAL_MODES)} (got {mode!r})")
        if (mode == "quantile") != (quantiles is not None):
            raise ValueError("IntervalMetrics: quantiles belong to mode 'quantile', which needs them")
        self.mode = mode
        self.quantiles = _check_quantiles("IntervalMetrics", quantiles) if quantiles is not None else None
        self.width = len(self.quantiles) if self.quantiles else 2 if mode == "gaussian" else 1
        self.mid = min(range(self.width), key=lambda q: (abs(self.quantiles[q] - 0.5), q)) if self.quantiles else 0
        self.cnt = self.acc = None

    def ensure(self, device):
        """Zeroed buffers on `device` where there are none yet (a rank whose shard was empty still enters the collectives)."""
        if self.cnt is None or self.cnt.device != torch.device(device):
            self.cnt = torch.zeros(_N_CNT, dtype=torch.int64, device=device)
            self.acc = torch.zeros(_N_ACC, dtype=torch.float64, device=device)

    def reset(self):
        if self.cnt is not None:
            self.cnt.zero_()
            self.acc.zero_()

    def update(self, pred, target):
        """pred (N, K) (or (N,) in point mode), target (N); rows with a non-finite target do not count.  Enqueue only."""
        pred, target = _regression_args("IntervalMetrics.update", pred.detach(), target.to(pred.device), self.width)
        N = pred.shape[0]
        if N == 0:
            return
        self.ensure(pred.device)
        L = lib()
        nb = L.msn_regression_interval_stats_workspace_bytes(N)
        ws = workspace(nb, pred.device) if nb else None
        check(L.msn_regression_interval_stats(ptr(pred), pred.stride(0), ptr(target), N, self.width, _INTERVAL_MODES[self.mode],
                                              self.mid, ptr(_levels_on(self.quantiles, pred.device)), ptr(self.cnt), ptr(self.acc),
                                              ptr(ws), nb, stream_ptr()), "msn_regression_interval_stats")

    def all_reduce(self, group=None):
        if self.cnt is not None and D.world_size(group) > 1:
            D.all_reduce_sum(self.cnt, group, kind="metric_all_reduce")
            D.all_reduce_sum(self.acc, group, kind="metric_all_reduce")

    def compute(self):
        if self.cnt is None:
            return interval_metrics([0] * _N_CNT, [0.0] * _N_ACC, self.mode, self.quantiles)
        return interval_metrics(self.cnt.cpu().tolist(), self.acc.cpu().tolist(), self.mode, self.quantiles)


_REGRESSION_LOSSES = ("mse", "l1", "huber", "log_cosh", "gaussian_nll", "quantile")
_DEFAULT_QUANTILES = (0.16, 0.5, 0.84)


# -------------------------------------------------------------------------------------------------- module
class ClipMLP(nn.Module):
    """MLP head on the concatenated embeddings of a (pretrained) LightCurveImageCLIP, trained for classification
    (cross-entropy against batch[8]) or redshift regression (MSE against batch[7]); Lightning hooks as plain methods,
    driven by trainer.Trainer / GraphedTrainStep.  state_dict: clip_model.*, mlp.layers.{0,3,6,...}.*, class_weights.
    ranking_metrics=True (classification only) also feeds the validation logits to a metrics.RankingMetrics and logs
    auroc_val, ap_val (macro one-vs-rest AUROC / average precision) and top2_acc_val beside f1_val, f1_micro_val and acc_val; without it the logged keys are those three and val_loss.
    calibration_metrics=True (classification only) also feeds them to a calibration.CalibrationMetrics (softmax of the logits,
    15 bins) and logs ece_val and brier_val (top-label expected calibration error, multi-class Brier score).
    loss="focal" (classification only) trains and validates on focal_loss with loss_kwargs {"gamma": 2.0, "label_smoothing": 0.0};
    loss="cross_entropy" (the default) takes loss_kwargs {"label_smoothing"}.  val_loss is the configured loss; the metrics and
    the state_dict do not depend on it.
    regression=True takes loss= "mse" | "l1" | "huber" | "log_cosh" | "gaussian_nll" | "quantile" (regression_loss on
    csrc/regression_loss.hip) with loss_kwargs {"delta"} for huber, {"quantiles"} for quantile (default (0.16, 0.5, 0.84)) and
    none otherwise.  These ignore rows whose redshift is NaN or infinite.  The head emits 1 value, (mu, log variance) for
    gaussian_nll, or one value per level for quantile -- only the last layer's shape changes; `metrics` is an IntervalMetrics
    and validation logs L1_val .. OLF_val of the point prediction (itself, mu, or the level nearest 0.5) plus sigma_val, z2_val,
    cov1_val, cov2_val (gaussian_nll) or coverage_val, width_val, crossing_val (quantile).  loss=None on a regression model is the
    masked-MSE path unchanged (same bits, keys and state_dict; a NaN target poisons it); an explicit loss="mse" takes the new
    kernel instead: it ignores non-finite targets and agrees with the default to fp32 rounding, not bit for bit."""

    def __init__(self, clip_model, learning_rate=1e-3, regression=False, classification=False, n_classes=5, hidden_dim=128,
                 num_layers=2, dropout=0.0, freeze_backbone=False, class_weights=None, optimizer_kwargs=None,
                 optimizer="radam", ranking_metrics=False, calibration_metrics=False, loss=None, loss_kwargs=None):
        super().__init__()
        if bool(regression) == bool(classification):
            raise ValueError("ClipMLP needs exactly one of regression=True / classification=True")
        self.reg_loss = None                  # regression: None = today's masked MSE, else (kind id, delta, levels or None)
        if regression:
            if loss is None and loss_kwargs is not None:
                raise ValueError("ClipMLP: loss_kwargs need a loss= on a regression model (the default trains on the MSE)")
            if loss is not None and loss not in _REGRESSION_LOSSES:
                raise ValueError(f"ClipMLP: a regression model's loss must be one of {_REGRESSION_LOSSES} (got {loss!r})")
            loss_kwargs = dict(loss_kwargs or {})
            allowed = {"huber": ("delta",), "quantile": ("quantiles",)}.get(loss, ())
            unknown = sorted(set(loss_kwargs) - set(allowed))
            if unknown:
                raise ValueError(f"ClipMLP: loss={loss!r} takes the loss_kwargs {allowed} (got {unknown})")
            if loss is not None:
                kind = "pinball" if loss == "quantile" else loss
                levels = loss_kwargs.get("quantiles", _DEFAULT_QUANTILES) if loss == "quantile" else None
                kind_id, _, delta, levels = _regression_params("ClipMLP", kind, loss_kwargs.get("delta", 1.0), levels)
                self.reg_loss = (kind_id, delta, levels)
            self.loss_name = "cross_entropy" if loss is None else loss      # (the default keeps the attribute it always had)
            self.loss_gamma, self.label_smoothing = 0.0, 0.0
        else:
            loss = "cross_entropy" if loss is None else loss
            if loss not in ("cross_entropy", "focal"):
                raise ValueError(f"ClipMLP: loss must be 'cross_entropy' or 'focal' (got {loss!r})")
            loss_kwargs = dict(loss_kwargs or {})
            allowed = ("gamma", "label_smoothing") if loss == "focal" else ("label_smoothing",)
            unknown = sorted(set(loss_kwargs) - set(allowed))
            if unknown:
                raise ValueError(f"ClipMLP: loss={loss!r} takes the loss_kwargs {allowed} (got {unknown})")
            self.loss_name = loss
            self.loss_gamma, self.label_smoothing = _focal_params("ClipMLP", loss_kwargs.get("gamma", 2.0 if loss == "focal" else 0.0),
                                                                  loss_kwargs.get("label_smoothing", 0.0))
        if "meta" in clip_model.combinations:
            raise ValueError("ClipMLP: a clip_model with the 'meta' tower reads redshift and class -- the labels; build it "
                             "without 'meta' and load the pretrained state_dict with strict=False")
        self.towers = [c for c in _TOWER_ORDER if c in clip_model.combinations]
        if not self.towers:
            raise ValueError("ClipMLP: the clip_model has no tower")
        if class_weights is not None and not classification:
            raise ValueError("ClipMLP: class_weights belong to classification")
        self.clip_model = clip_model
        self.regression, self.classification = bool(regression), bool(classification)
        self.n_classes = int(n_classes)
        self.learning_rate = learning_rate
        self.optimizer_kwargs = dict(optimizer_kwargs or {})
        self.optimizer = optimizer            # optim.build_optimizer's name ("radam", "adam", "adamw", "sgd", "lars") or an Optimizer class (optim.LAMB)
        self.freeze_backbone = bool(freeze_backbone)
        self.mlp = MLP(input_dim=len(self.towers) * clip_model.enc_dim, hidden_dim=hidden_dim,
                       output_dim=self.n_classes if classification else self._regression_width(), num_layers=num_layers,
                       dropout=dropout)
        if class_weights is not None:
            w = torch.as_tensor(class_weights, dtype=torch.float32).reshape(-1)
            if w.numel() != self.n_classes:
                raise ValueError(f"ClipMLP: {self.n_classes} classes need {self.n_classes} class weights (got {w.numel()})")
            self.register_buffer("class_weights", w.clone())
        else:
            self.class_weights = None
        if self.freeze_backbone:
            self.clip_model.requires_grad_(False)
            self.clip_model.eval()
        self.group = None
        if classification:
            self.metrics = ClassificationMetrics(self.n_classes)
        elif self.reg_loss is None:
            self.metrics = RegressionMetrics()
        else:
            mode = {"gaussian_nll": "gaussian", "quantile": "quantile"}.get(self.loss_name, "point")
            self.metrics = IntervalMetrics(mode, self.reg_loss[2])
        self.ranking = None                   # opt-in: threshold-free metrics of the logits (metrics.RankingMetrics)
        if ranking_metrics and classification:
            from .metrics import RankingMetrics
            self.ranking = RankingMetrics(self.n_classes, normalize="log_softmax", top_k=(1, 2))
        self.calibration = None               # opt-in: calibration of softmax(logits) (calibration.CalibrationMetrics)
        if calibration_metrics and classification:
            from .calibration import CalibrationMetrics
            self.calibration = CalibrationMetrics(self.n_classes, normalize="softmax")
        self._val_batches = 0
        self._ones = {}
        self.logged = {}

    def _regression_width(self):
        """Outputs of the regression head: 1, (mu, log variance) for the Gaussian NLL, or one per quantile level."""
        if self.reg_loss is None or self.loss_name not in ("gaussian_nll", "quantile"):
            return 1
        return 2 if self.loss_name == "gaussian_nll" else len(self.reg_loss[2])

    def log(self, name, value, **kwargs):
        # detached: a logged loss must not keep its autograd graph alive into the next step
        self.logged[name] = value.detach() if torch.is_tensor(value) else value

    def train(self, mode=True):
        super().train(mode)
        if self.freeze_backbone:
            self.clip_model.eval()          # frozen towers: no dropout, BatchNorm on its running statistics
        return self

    def features(self, *batch):
        """(B, M * enc_dim): the unit-norm projected embeddings side by side in the order image, light curve, spectrum."""
        if self.freeze_backbone:
            with torch.no_grad():
                embs = self.clip_model(*batch)
        else:
            embs = self.clip_model(*batch)
        return embs[0] if len(embs) == 1 else torch.cat(embs, dim=1)

    def forward(self, *batch):
        """(B, n_classes) logits, or (B, 1) redshift predictions."""
        return self.mlp(self.features(*batch))

    def configure_optimizers(self):
        """RAdam (or the optimizer named by `optimizer=`) over the parameters that take part: the head, plus towers and projections unless frozen -- never the
        contrastive logit_scale / logit_bias (no gradient here; coupled weight decay must not move them)."""
        from .optim import build_optimizer
        params = list(self.mlp.parameters())
        if not self.freeze_backbone:
            params += [p for n, p in self.clip_model.named_parameters() if n not in ("logit_scale", "logit_bias")]
        return {"optimizer": build_optimizer(self.optimizer, params, lr=self.learning_rate, **self.optimizer_kwargs)}

    # -- losses ------------------------------------------------------------------------------------------------------
    def _all_true(self, n, device):
        """The all-true selection of the masked-MSE kernels (plain MSE = every element selected)."""
        key = (n, device)
        if key not in self._ones:
            ones = torch.ones(n, dtype=torch.uint8, device=device)
            if torch.cuda.is_current_stream_capturing():
                return ones               # filled by a node of the recording only: not kept for eager use
            self._ones[key] = ones
        return self._ones[key]

    def _mse(self, pred, target, sharded):
        loss = masked_mse(pred, target, self._all_true(pred.numel(), pred.device))
        if not sharded:
            return loss
        n_local = float(pred.numel())
        n_global = D.all_reduce_sum(torch.full((), n_local, dtype=torch.float32, device=pred.device), self.group,
                                    kind="loss_denominator_all_reduce")
        return _AllReduceSum.apply(loss * (n_local / n_global), self.group)

    def _loss_out(self, batch, sharded):
        """-> (loss, prediction, target, head output): class per row (int32) / redshift per row; logits / (B, 1) predictions."""
        out = self(*batch)
        if self.classification:
            target = batch[8].to(torch.int64).reshape(-1)
            if self.loss_name == "focal" or self.label_smoothing != 0.0:
                loss, pred = _focal_loss(out, target, self.class_weights, self.loss_gamma, self.label_smoothing, self.group, sharded)
            else:
                loss, pred = _cross_entropy(out, target, self.class_weights, self.group, sharded)
            return loss, pred, target, out
        target = batch[7].to(torch.float32).reshape(-1)
        if self.reg_loss is not None:           # the head's whole output goes to the loss and to IntervalMetrics
            return _regression_loss(out, target, *self.reg_loss, self.group, sharded), out, target, out
        pred = out.squeeze(1)
        return self._mse(pred, target, sharded), pred, target, out

    def _loss(self, batch, sharded):
        """-> (loss, prediction, target)."""
        return self._loss_out(batch, sharded)[:3]

    def training_step(self, batch, batch_idx):
        loss, _, _ = self._loss(batch, D.world_size(self.group) > 1)
        self.log("train_loss", loss, on_epoch=True, on_step=False, prog_bar=True, logger=True)
        return loss

    def on_validation_start(self):
        self.metrics.reset()
        if self.ranking is not None:
            self.ranking.reset()
        if self.calibration is not None:
            self.calibration.reset()
        self._val_batches = 0

    def validation_step(self, batch, batch_idx):
        """Per shard, as the Trainer validates: no collective inside the loop, no host synchronisation."""
        loss, pred, target, out = self._loss_out(batch, False)
        self.metrics.update(pred.detach(), target)
        if self.ranking is not None:
            self.ranking.update(out.detach(), target)
        if self.calibration is not None:
            self.calibration.update(out.detach(), target)
        self._val_batches += 1
        self.log("val_loss", loss, on_epoch=True, on_step=False, prog_bar=True, logger=True)
        return loss

    def on_validation_epoch_end(self):
        world = D.world_size(self.group)
        if world == 1 and not self._val_batches:
            return
        if world > 1:
            if self._val_batches == 0:        # every rank enters the collective, also one whose shard was empty
                dev = next(self.mlp.parameters()).device
                if self.classification and self.metrics.cm is None:
                    self.metrics.cm = torch.zeros((self.n_classes, self.n_classes), dtype=torch.int32, device=dev)
                if self.regression and self.reg_loss is not None:
                    self.metrics.ensure(dev)
                elif self.regression and self.metrics.sums is None:
                    self.metrics.sums = torch.zeros(6, dtype=torch.float64, device=dev)
            self.metrics.all_reduce(self.group)
            if self.ranking is not None:
                self.ranking.all_reduce(self.group, device=next(self.mlp.parameters()).device)
            if self.calibration is not None:
                self.calibration.all_reduce(self.group, device=next(self.mlp.parameters()).device)
        res = self.metrics.compute()
        kw = dict(on_epoch=True, on_step=False, prog_bar=True, logger=True)
        if self.classification:
            self.log("f1_val", res["f1_macro"], **kw)
            self.log("f1_micro_val", res["f1_micro"], **kw)
            self.log("acc_val", res["acc"], **kw)
            if self.ranking is not None:
                rk = self.ranking.compute()
                self.log("auroc_val", rk["auroc_macro"], **kw)
                self.log("ap_val", rk["ap_macro"], **kw)
                self.log("top2_acc_val", rk["top2_acc"], **kw)
            if self.calibration is not None:
                cal = self.calibration.compute()
                self.log("ece_val", cal["ece"], **kw)
                self.log("brier_val", cal["brier"], **kw)
        else:
            for k in ("L1", "L2", "R2", "OLF"):
                self.log(f"{k}_val", res[k], **kw)
            extra = {"gaussian_nll": (("sigma_val", "sigma_mean"), ("z2_val", "z2_mean"), ("cov1_val", "cov1"), ("cov2_val", "cov2")),
                     "quantile": (("coverage_val", "coverage"), ("width_val", "width_mean"), ("crossing_val", "crossing"))}
            for name, key in extra.get(self.loss_name, ()):               # (the default model's loss_name is neither)
                self.log(name, res[key], **kw)
