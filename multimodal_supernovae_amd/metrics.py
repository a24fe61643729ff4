"""Threshold-free classification metrics on the device: one-vs-rest AUROC, average precision, binned ROC / precision-recall
curves and top-k accuracy (csrc/rank_metrics.hip).  Supernova classes are badly imbalanced; accuracy and F1 at the arg-max
(models_finetune.ClassificationMetrics) say little there, and the scores of the head (logits), of
probes.LogisticRegressionProbe.decision_function and of KNeighborsClassifierProbe.predict_proba are already on the GPU.

    rank_counts, threshold_counts, topk_ranks, log_softmax_rows
                             thin wrappers over the four entry points; enqueue only, no host synchronisation
    auroc_from_stats, average_precision_from_stats, topk_accuracy,
    roc_curve_binned, precision_recall_curve_binned, binned_auroc, binned_average_precision
                             pure host functions of the small integer outputs (the role of classification_metrics(cm))
    multiclass_auroc, multiclass_average_precision, binary_auroc, binary_average_precision
                             one call: kernel, one host copy, host function
    RankingMetrics           reset / update / all_reduce / compute over the batches of a validation epoch, exact (keeps the
                             scores, one pair count at the end) or binned (int64 accumulators per threshold)
    rank_counts_reference, threshold_counts_reference, topk_ranks_reference
                             numpy restatements, importable without a GPU: the authority for every convention

The metrics are exact: AUROC_c = U2_c / (2 P_c Nneg_c) is Mann-Whitney with ties at one half, formed from integer pair
counts; AP_c = ap_sum_c / P_c gives all positives at one score one precision (scikit-learn's rule).  A row whose target lies
outside [0, n_classes) -- -100 -- counts nowhere.  No scipy or scikit-learn at run time.
"""
import math

import numpy as np
import torch

from . import _lib
from . import distributed as D
from ._device_args import (MAX_CLASSES, EpochCounts, accumulator, ld, reference_inputs, rows_on_gpu, scores_and_targets,
                           to_numpy, workspace)
from ._lib import check, lib, ptr, stream_ptr

MAX_THRESHOLDS = 1024
IGNORE = -100


# ------------------------------------------------------------------------------------------------- host: restatements
def rank_counts_reference(S, y, n_classes=None):
    """numpy restatement of msn_rank_counts: (counts int32 (N, 3) = {n_gt, n_ge, p_ge}, istats int64 (C, 3) = {P, Nneg, U2},
    ap_sum fp64 (C)).  Compares are fp32 compares (a NaN is false both ways); every quotient p_ge / (p_ge + n_ge) is rounded
    once and a class's quotients are added by math.fsum (the correctly rounded sum: the kernel's fixed order lies within
    P_c 2^-52 ap_sum of it)."""
    S, y, C, valid = reference_inputs(S, y, n_classes, "rank_counts_reference")
    N = len(y)
    counts = np.zeros((N, 3), dtype=np.int32)
    istats = np.zeros((C, 3), dtype=np.int64)
    ap_sum = np.zeros(C, dtype=np.float64)
    n_valid = int(valid.sum())
    for c in range(C):
        pos = np.nonzero(valid & (y == c))[0]
        neg = S[valid & (y != c), c]
        own = S[pos, c]
        P, Nneg = len(pos), n_valid - len(pos)
        if P:
            counts[pos, 0] = (neg[None, :] > own[:, None]).sum(axis=1)
            counts[pos, 1] = (neg[None, :] >= own[:, None]).sum(axis=1)
            counts[pos, 2] = (own[None, :] >= own[:, None]).sum(axis=1)
        g, e, p = (counts[pos, k].astype(np.int64) for k in range(3))
        istats[c] = (P, Nneg, 2 * Nneg * P - int(g.sum()) - int(e.sum()))
        with np.errstate(invalid="ignore"):
            ap_sum[c] = math.fsum((p.astype(np.float64) / (p + e).astype(np.float64)).tolist())
    return counts, istats, ap_sum


def threshold_counts_reference(S, y, thresholds, n_classes=None):
    """numpy restatement of msn_threshold_counts for one call from zero: (acc int64 (C, T, 2), tot int64 (C, 2)) with
    acc[c, t] = {#(y = c, S[:, c] >= thr[t]), #(y != c, S[:, c] >= thr[t])} over the valid rows, tot[c] = {P_c, Nneg_c}."""
    S, y, C, valid = reference_inputs(S, y, n_classes, "threshold_counts_reference")
    thr = np.asarray(thresholds, dtype=np.float32).reshape(-1)
    acc = np.zeros((C, len(thr), 2), dtype=np.int64)
    tot = np.zeros((C, 2), dtype=np.int64)
    for c in range(C):
        pos, neg = valid & (y == c), valid & (y != c)
        acc[c, :, 0] = (S[pos, c][:, None] >= thr[None, :]).sum(axis=0)
        acc[c, :, 1] = (S[neg, c][:, None] >= thr[None, :]).sum(axis=0)
        tot[c] = (pos.sum(), neg.sum())
    return acc, tot


def topk_ranks_reference(S, y, n_classes=None):
    """numpy restatement of msn_topk_ranks: (rank int32 (N), -1 for ignored rows; hist int64 (C)).  rank = the classes scoring
    above the target class, plus the lower classes scoring the same."""
    S, y, C, valid = reference_inputs(S, y, n_classes, "topk_ranks_reference")
    rank = np.full(len(y), -1, dtype=np.int32)
    rows = np.nonzero(valid)[0]
    s = S[rows, y[rows]][:, None]
    lower = np.arange(C)[None, :] < y[rows][:, None]
    rank[rows] = ((S[rows] > s) | ((S[rows] == s) & lower)).sum(axis=1)
    return rank, np.bincount(rank[rows], minlength=C).astype(np.int64)


# ---------------------------------------------------------------------------------------------- host: the metrics
def _average(per_class, weights, average, who):
    """Mean of the defined (non-nan) entries: plain ("macro") or weighted by the classes' positives ("weighted"); None gives
    the per-class array.  nan when no class is defined -- the rule of the macro F1 of classification_metrics."""
    if average is None:
        return per_class
    if average not in ("macro", "weighted"):
        raise ValueError(f"{who}: average must be 'macro', 'weighted' or None (got {average!r})")
    ok = ~np.isnan(per_class)
    if not ok.any():
        return float("nan")
    if average == "macro":
        return float(per_class[ok].mean())
    w = weights[ok].astype(np.float64)
    return float((per_class[ok] * w).sum() / w.sum())


def _per_class_auroc(istats):
    st = to_numpy(istats, np.int64).reshape(-1, 3)
    out = np.full(len(st), np.nan)
    for c, (P, Nneg, U2) in enumerate(st.tolist()):
        if P > 0 and Nneg > 0:
            out[c] = U2 / (2 * P * Nneg)             # Python integers: the quotient is rounded once
    return out, st[:, 0]


def auroc_from_stats(istats, average="macro"):
    """One-vs-rest AUROC from istats (C, 3) = {P, Nneg, U2}: U2 / (2 P Nneg) per class, nan for a class without positives or
    without negatives; such a class is left out of the macro / weighted (by P) mean."""
    per, P = _per_class_auroc(istats)
    return _average(per, P, average, "auroc_from_stats")


def _per_class_ap(istats, ap_sum):
    st = to_numpy(istats, np.int64).reshape(-1, 3)
    s = to_numpy(ap_sum, np.float64).reshape(-1)
    out = np.full(len(st), np.nan)
    ok = st[:, 0] > 0
    out[ok] = s[ok] / st[ok, 0]
    return out, st[:, 0]


def average_precision_from_stats(istats, ap_sum, average="macro"):
    """Average precision per class, ap_sum / P: nan for a class without positives (left out of the mean); a class without
    negatives has precision 1 everywhere and scores 1.0, as scikit-learn's average_precision_score does."""
    per, P = _per_class_ap(istats, ap_sum)
    return _average(per, P, average, "average_precision_from_stats")


def topk_accuracy(hist, k):
    """Share of the counted rows whose target class is among the k best-scored: sum(hist[:k]) / sum(hist); nan without rows."""
    h = to_numpy(hist, np.int64).reshape(-1)
    if not 1 <= int(k) <= len(h):
        raise ValueError(f"topk_accuracy: k must be in 1..{len(h)} (got {k})")
    total = int(h.sum())
    return int(h[:int(k)].sum()) / total if total else float("nan")


def _binned(acc, tot):
    acc, tot = to_numpy(acc, np.int64), to_numpy(tot, np.int64)
    if acc.ndim != 3 or acc.shape[2] != 2 or tot.shape != (acc.shape[0], 2):
        raise ValueError(f"binned curves: acc (C, T, 2) and tot (C, 2) needed (got {acc.shape} and {tot.shape})")
    return acc.astype(np.float64), tot.astype(np.float64)


def roc_curve_binned(acc, tot):
    """(fpr, tpr), each (C, T), at the thresholds in their ascending order: tpr = acc[..., 0] / P, fpr = acc[..., 1] / Nneg.
    A class without positives has tpr nan everywhere, one without negatives fpr nan everywhere."""
    a, t = _binned(acc, tot)
    with np.errstate(invalid="ignore", divide="ignore"):
        tpr = np.where(t[:, None, 0] > 0, a[:, :, 0] / t[:, None, 0], np.nan)
        fpr = np.where(t[:, None, 1] > 0, a[:, :, 1] / t[:, None, 1], np.nan)
    return fpr, tpr


def precision_recall_curve_binned(acc, tot):
    """(precision, recall), each (C, T): precision = tp / (tp + fp), 1.0 where no row reaches the threshold (tp + fp = 0, the
    end point of scikit-learn's curve); recall = tp / P, nan everywhere for a class without positives."""
    a, t = _binned(acc, tot)
    reached = a[:, :, 0] + a[:, :, 1]
    with np.errstate(invalid="ignore", divide="ignore"):
        precision = np.where(reached > 0, a[:, :, 0] / reached, 1.0)
        recall = np.where(t[:, None, 0] > 0, a[:, :, 0] / t[:, None, 0], np.nan)
    return precision, recall


def binned_auroc(acc, tot, average="macro"):
    """Trapezoid area under the binned ROC curve, closed by (1, 1) below the lowest and (0, 0) above the highest threshold;
    equals the exact AUROC when every score lies on a threshold.  nan for a class without positives or negatives."""
    fpr, tpr = roc_curve_binned(acc, tot)
    C = fpr.shape[0]
    x = np.concatenate([np.ones((C, 1)), fpr, np.zeros((C, 1))], axis=1)
    y = np.concatenate([np.ones((C, 1)), tpr, np.zeros((C, 1))], axis=1)
    per = ((x[:, :-1] - x[:, 1:]) * (y[:, :-1] + y[:, 1:])).sum(axis=1) * 0.5
    return _average(per, to_numpy(tot, np.int64)[:, 0], average, "binned_auroc")


def binned_average_precision(acc, tot, average="macro"):
    """sum_t (recall[t] - recall[t + 1]) precision[t] with recall 0 above the highest threshold; equals the exact average
    precision when every score lies on a threshold.  nan for a class without positives."""
    precision, recall = precision_recall_curve_binned(acc, tot)
    r = np.concatenate([recall, np.zeros((recall.shape[0], 1))], axis=1)
    per = ((r[:, :-1] - r[:, 1:]) * precision).sum(axis=1)
    return _average(per, to_numpy(tot, np.int64)[:, 0], average, "binned_average_precision")


# ------------------------------------------------------------------------------------------------------ device halves
def rank_counts(scores, target):
    """(counts int32 (N, 3), istats int64 (C, 3), ap_sum fp64 (C)) of msn_rank_counts, all on the device.  Enqueue only."""
    S, y = scores_and_targets(scores, target, "rank_counts")
    N, C = S.shape
    counts = torch.empty((N, 3), dtype=torch.int32, device=S.device)
    istats = torch.empty((C, 3), dtype=torch.int64, device=S.device)
    ap_sum = torch.empty(C, dtype=torch.float64, device=S.device)
    L = lib()
    ws = workspace(L.msn_rank_counts_workspace_bytes(N, C), S.device)
    check(L.msn_rank_counts(ptr(S), ld(S), ptr(y), N, C, ptr(counts), ptr(istats), ptr(ap_sum), ptr(ws), ws.numel(),
                            stream_ptr()), "msn_rank_counts")
    return counts, istats, ap_sum


def threshold_counts(scores, target, thresholds, acc=None, tot=None):
    """(acc int64 (C, T, 2), tot int64 (C, 2)) of msn_threshold_counts for ascending float32 thresholds (T) on the device; acc /
    tot given are added to (the accumulators of a validation epoch), else they start from zero.  Enqueue only."""
    S, y = scores_and_targets(scores, target, "threshold_counts")
    N, C = S.shape
    if not isinstance(thresholds, torch.Tensor) or thresholds.dim() != 1 or thresholds.dtype != torch.float32:
        raise ValueError("threshold_counts: thresholds must be a float32 (T,) tensor")
    if thresholds.device != S.device:
        raise _lib.MsnHipError("threshold_counts: thresholds must live on the GPU next to the scores; there is no CPU path")
    T = thresholds.numel()
    if not 1 <= T <= MAX_THRESHOLDS:
        raise _lib.MsnHipError(f"threshold_counts: 1 to {MAX_THRESHOLDS} thresholds (got {T})")
    thr = thresholds.detach().contiguous()
    acc = accumulator(acc, (C, T, 2), S.device, "threshold_counts")
    tot = accumulator(tot, (C, 2), S.device, "threshold_counts")
    check(lib().msn_threshold_counts(ptr(S), ld(S), ptr(y), N, C, ptr(thr), T, ptr(acc), ptr(tot), stream_ptr()),
          "msn_threshold_counts")
    return acc, tot


def topk_ranks(scores, target, hist=None, return_ranks=True):
    """(rank int32 (N) or None, hist int64 (C)) of msn_topk_ranks; a hist given is added to.  Enqueue only."""
    S, y = scores_and_targets(scores, target, "topk_ranks")
    N, C = S.shape
    rank = torch.empty(N, dtype=torch.int32, device=S.device) if return_ranks else None
    hist = accumulator(hist, (C,), S.device, "topk_ranks")
    check(lib().msn_topk_ranks(ptr(S), ld(S), ptr(y), N, C, ptr(rank), ptr(hist), stream_ptr()), "msn_topk_ranks")
    return rank, hist


def log_softmax_rows(logits):
    """log_softmax over the rows of float32 (N, C) logits in one launch (msn_log_softmax_rows), a new dense tensor."""
    S = rows_on_gpu(logits, "log_softmax_rows", "scores", MAX_CLASSES)
    N, C = S.shape
    out = torch.empty((N, C), dtype=torch.float32, device=S.device)
    check(lib().msn_log_softmax_rows(ptr(S), ld(S), N, C, ptr(out), C, stream_ptr()), "msn_log_softmax_rows")
    return out


# ------------------------------------------------------------------------------------------------------ conveniences
def multiclass_auroc(scores, target, average="macro"):
    """One-vs-rest AUROC of float32 (N, C) scores against int64 targets: the pair count on the device, one host copy."""
    _, istats, _ = rank_counts(scores, target)
    return auroc_from_stats(istats.cpu(), average)


def multiclass_average_precision(scores, target, average="macro"):
    _, istats, ap_sum = rank_counts(scores, target)
    return average_precision_from_stats(istats.cpu(), ap_sum.cpu(), average)


def _binary(scores, target, who):
    if not isinstance(scores, torch.Tensor) or scores.dim() != 1 or scores.dtype != torch.float32:
        raise ValueError(f"{who}: scores must be a float32 (N,) tensor (got {getattr(scores, 'dtype', type(scores).__name__)})")
    if scores.device.type != "cuda":
        raise _lib.MsnHipError(f"{who}: scores must live on the GPU (got {scores.device}); there is no CPU path")
    s = scores.detach()
    return rank_counts(torch.stack([-s, s], dim=1), target)           # negation is exact: class 0 ranks by -s


def binary_auroc(scores, target):
    """AUROC of float32 (N,) scores of the positive class against int64 targets in {0, 1} (others are ignored)."""
    _, istats, _ = _binary(scores, target, "binary_auroc")
    return float(auroc_from_stats(istats.cpu(), None)[1])


def binary_average_precision(scores, target):
    _, istats, ap_sum = _binary(scores, target, "binary_average_precision")
    return float(average_precision_from_stats(istats.cpu(), ap_sum.cpu(), None)[1])


class RankingMetrics(EpochCounts):
    """AUROC, average precision and top-k accuracy over the batches of a validation epoch, in the shape of
    ClassificationMetrics: reset, update(scores, target), all_reduce(group), compute().

    thresholds=None is the exact mode: update keeps the detached batches, compute concatenates them and counts the pairs
    once (msn_rank_counts); under data parallel all_reduce gathers every rank's rows first.  thresholds = T (linspace(0, 1, T)
    in fp32) or a float32 tensor is the binned mode: update is one msn_threshold_counts launch into int64 accumulators,
    all_reduce their SUM, compute the one host copy; the thresholds are in the units of the scores as they are ranked (after
    `normalize`).  The top-k histogram accumulates in both modes.  normalize="log_softmax" ranks logits as log-probabilities."""

    _counts = ("hist", "acc", "tot")                            # acc and tot in the binned mode only

    def __init__(self, n_classes, thresholds=None, top_k=(1,), normalize=None):
        self.n_classes = int(n_classes)
        if not 1 <= self.n_classes <= MAX_CLASSES:
            raise ValueError(f"RankingMetrics: n_classes must be in 1..{MAX_CLASSES} (got {n_classes})")
        if normalize not in (None, "log_softmax"):
            raise ValueError(f"RankingMetrics: normalize must be None or 'log_softmax' (got {normalize!r})")
        self.top_k = tuple(int(k) for k in top_k)
        if any(not 1 <= k <= self.n_classes for k in self.top_k):
            raise ValueError(f"RankingMetrics: top_k must lie in 1..{self.n_classes} (got {top_k})")
        self.normalize = normalize
        if thresholds is None:
            self.thresholds = None
        elif isinstance(thresholds, torch.Tensor):
            self.thresholds = thresholds.detach().to(torch.float32).reshape(-1).clone()
        else:
            self.thresholds = torch.linspace(0, 1, int(thresholds), dtype=torch.float32)
        if self.thresholds is not None and not 1 <= self.thresholds.numel() <= MAX_THRESHOLDS:
            raise ValueError(f"RankingMetrics: 1 to {MAX_THRESHOLDS} thresholds (got {self.thresholds.numel()})")
        self.hist = self.acc = self.tot = None
        self.reset()

    @property
    def binned(self):
        return self.thresholds is not None

    def reset(self):
        self._scores, self._targets, self._gathered = [], [], False
        self.istats = self.ap_sum = None                       # the exact mode's last pair count, on the device
        super().reset()

    def _buffers(self, device):
        C = self.n_classes
        if self.hist is None or self.hist.device != device:
            self.hist = torch.zeros(C, dtype=torch.int64, device=device)
            if self.binned:
                self.thresholds = self.thresholds.to(device)
                self.acc = torch.zeros((C, self.thresholds.numel(), 2), dtype=torch.int64, device=device)
                self.tot = torch.zeros((C, 2), dtype=torch.int64, device=device)

    def update(self, scores, target):
        """scores float32 (N, n_classes) on the GPU, target int64 (N).  Enqueue only; an empty batch counts nothing."""
        if isinstance(scores, torch.Tensor) and scores.dim() == 2 and scores.shape[0] == 0:
            return
        if isinstance(target, torch.Tensor):
            target = target.to(torch.int64)
        S, y = scores_and_targets(scores, target, "RankingMetrics.update")
        if S.shape[1] != self.n_classes:
            raise ValueError(f"RankingMetrics.update: {S.shape[1]} score columns for {self.n_classes} classes")
        if self.normalize == "log_softmax":
            S = log_softmax_rows(S)
        self._buffers(S.device)
        topk_ranks(S, y, hist=self.hist, return_ranks=False)
        if self.binned:
            threshold_counts(S, y, self.thresholds, acc=self.acc, tot=self.tot)
        else:
            self._scores.append(S if S.is_contiguous() else S.contiguous())
            self._targets.append(y)
            self._gathered = False

    def _local(self, device):
        C = self.n_classes
        if not self._scores:
            return torch.empty((0, C), dtype=torch.float32, device=device), torch.empty(0, dtype=torch.int64, device=device)
        if len(self._scores) > 1:
            self._scores, self._targets = [torch.cat(self._scores)], [torch.cat(self._targets)]
        return self._scores[0], self._targets[0]

    def all_reduce(self, group=None, device=None):
        """Every rank enters, also one whose shard was empty (pass its device then).  Binned: SUM of the accumulators.  Exact:
        all ranks gather all rows -- all_gather_rows wants equal blocks, so a shard is padded to the largest with rows of target
        -100, which count nowhere."""
        device = self._all_reduce_counts(group, device)
        if device is None or self.binned or self._gathered:
            return
        S, y = self._local(device)
        sizes = D.all_gather_rows(torch.tensor([S.shape[0]], dtype=torch.int64, device=device), group, kind="metric_all_gather")
        n_max = int(sizes.max().item())
        self._gathered = True
        if n_max == 0:
            return
        pad = n_max - S.shape[0]
        if pad:
            S = torch.cat([S, torch.zeros((pad, self.n_classes), dtype=torch.float32, device=device)])
            y = torch.cat([y, torch.full((pad,), IGNORE, dtype=torch.int64, device=device)])
        self._scores = [D.all_gather_rows(S, group, kind="metric_all_gather")]
        self._targets = [D.all_gather_rows(y, group, kind="metric_all_gather")]

    def compute(self):
        """The one host copy: {auroc_macro, auroc_per_class, ap_macro, ap_per_class, top{k}_acc} and, binned, the curves
        (thresholds, fpr, tpr, precision, recall as numpy arrays)."""
        C = self.n_classes
        res = {}
        if self.binned:
            acc = self.acc.cpu() if self.acc is not None else torch.zeros((C, self.thresholds.numel(), 2), dtype=torch.int64)
            tot = self.tot.cpu() if self.tot is not None else torch.zeros((C, 2), dtype=torch.int64)
            au, ap = binned_auroc(acc, tot, None), binned_average_precision(acc, tot, None)
            P = tot.numpy()[:, 0]
            fpr, tpr = roc_curve_binned(acc, tot)
            precision, recall = precision_recall_curve_binned(acc, tot)
            res.update(thresholds=self.thresholds.cpu().numpy(), fpr=fpr, tpr=tpr, precision=precision, recall=recall)
        elif self._scores:
            S, y = self._local(None)
            _, self.istats, self.ap_sum = rank_counts(S, y)
            istats, ap_sum = self.istats.cpu(), self.ap_sum.cpu()
            au, ap = auroc_from_stats(istats, None), average_precision_from_stats(istats, ap_sum, None)
            P = istats.numpy()[:, 0]
        else:
            au, ap, P = np.full(C, np.nan), np.full(C, np.nan), np.zeros(C, dtype=np.int64)
        res.update(auroc_macro=_average(au, P, "macro", "RankingMetrics"), auroc_per_class=[float(v) for v in au],
                   ap_macro=_average(ap, P, "macro", "RankingMetrics"), ap_per_class=[float(v) for v in ap])
        hist = self.hist.cpu() if self.hist is not None else torch.zeros(C, dtype=torch.int64)
        for k in self.top_k:
            res[f"top{k}_acc"] = topk_accuracy(hist, k)
        return res
