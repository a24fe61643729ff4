"""Calibration of classifier probabilities on the device: expected calibration error (ECE), reliability diagram, Brier score
and post-hoc temperature scaling (Guo et al. 2017; csrc/calibration.hip).  models_finetune.ClassificationMetrics judges the
arg-max and metrics.RankingMetrics the order of the scores; this module judges the probabilities themselves -- of the head
(softmax of the logits), of probes.LogisticRegressionProbe.decision_function and of KNeighborsClassifierProbe.predict_proba,
which are already on the GPU.

    softmax_rows, calibration_counts, temperature_nll
                             thin wrappers over the entry points; enqueue only, no host synchronisation
    ece_from_counts, classwise_ece_from_counts, brier_from_counts, reliability_curve
                             pure host functions of the small integer outputs (the role of classification_metrics(cm))
    CalibrationMetrics       reset / update / all_reduce / compute over the batches of a validation epoch: int64 accumulators
    TemperatureScaling       fit(logits, target): safeguarded Newton on beta = 1 / T over msn_temperature_nll; predict_proba
    softmax_rows_reference, calibration_counts_reference, temperature_nll_reference, fit_temperature_reference
                             numpy restatements, importable without a GPU: the authority for every convention

Confidences are binned in fixed point: q(p) = rint(p 2^32) is exact in the fp32 bits of p, the bin of p is
min(B - 1, (q B) >> 32) (edges k / B, p = 1 in the last bin), and every accumulated quantity is an integer -- the counts do
not depend on the order of the adds or on how an epoch is cut into batches or ranks, and the quantisation moves ECE by at most
2^-33.  A row whose target lies outside [0, n_classes) -- -100 -- counts nowhere; a row with a target in range whose entries
do not lie in [0, 1] or do not sum to 1 within 2^-10 is a bad row: it counts in n_bad only (a kNN row that no labelled
neighbour votes for sums to 0 and is such a row).  No scipy or scikit-learn at run time.
"""
import math
import warnings

import numpy as np
import torch

from . import _lib
from . import distributed as D
from ._lib import check, lib, ptr, stream_ptr
from ._device_args import (EpochCounts, accumulator, ld, reference_inputs, rows_on_gpu, scores_and_targets, to_numpy,
                           workspace)
from .metrics import IGNORE, MAX_CLASSES  # noqa: F401 -- part of the interface

MAX_BINS = 1024
Q_ONE = 1 << 32                # the fixed-point unit of a confidence
BRIER_ONE = 1 << 30            # the fixed-point unit of a row's Brier sum
SUM_SLACK = 2.0 ** -10         # a valid row sums to 1 within this


# ------------------------------------------------------------------------------------------------- host: restatements
def _beta(temperature, beta, who):
    if beta is None:
        b = 1.0 / float(temperature) if float(temperature) != 0.0 else float("inf")
    else:
        b = float(beta)
    if not (b > 0.0 and math.isfinite(b)):
        raise ValueError(f"{who}: the temperature must be finite and > 0 (got beta = 1 / temperature = {b})")
    return b


def softmax_rows_reference(x, temperature=1.0, beta=None, dtype=np.float64):
    """numpy restatement of msn_softmax_rows BEFORE its one rounding to fp32: t = beta x in `dtype`, minus the row maximum, exp,
    the sum in column order, the quotient.  A row that holds a NaN or +inf comes out all NaN."""
    x = np.asarray(x, dtype=np.float32)
    if x.ndim != 2:
        raise ValueError(f"softmax_rows_reference: logits (N, C) needed (got {x.shape})")
    b = dtype(_beta(temperature, beta, "softmax_rows_reference"))
    with np.errstate(invalid="ignore", over="ignore"):
        t = b * x.astype(dtype)
        e = np.exp(t - t.max(axis=1, keepdims=True))
        s = np.zeros(len(x), dtype=dtype)
        for c in range(x.shape[1]):
            s = s + e[:, c]
        return e / s[:, None]


def calibration_counts_reference(P, y, n_bins=15, classwise=False, n_classes=None):
    """numpy restatement of msn_calibration_counts for one call from zero: (acc int64 (slots, B, 3), tot int64 (3)) with
    acc[s, b] = {rows, hits, sum of q(conf)} of slot s (0: the top label at its first maximal column; 1 + c: class c) in bin b
    over the valid rows, tot = {#valid, #bad, sum of rint(brier_i 2^30)}."""
    P, y, C, in_range = reference_inputs(P, y, n_classes, "calibration_counts_reference")
    B = int(n_bins)
    if not 1 <= B <= MAX_BINS:
        raise ValueError(f"calibration_counts_reference: 1 to {MAX_BINS} bins (got {n_bins})")
    P64 = P.astype(np.float64)
    with np.errstate(invalid="ignore"):
        unit = ((P >= 0) & (P <= 1)).all(axis=1)                 # a NaN fails; -0.0 passes
        s = np.zeros(len(y), dtype=np.float64)
        for c in range(C):                                       # column order
            s = s + P64[:, c]
        ok = unit & (np.abs(s - 1.0) <= SUM_SLACK)
    rows = np.nonzero(in_range & ok)[0]
    slots = 1 + C if classwise else 1
    acc = np.zeros((slots, B, 3), dtype=np.int64)
    tot = np.array([len(rows), int((in_range & ~ok).sum()), 0], dtype=np.int64)
    if not len(rows):
        return acc, tot
    Pv, yv = P[rows], y[rows]
    q = np.rint(P64[rows] * float(Q_ONE)).astype(np.int64)       # the product is exact
    bins = np.minimum(B - 1, (q * B) >> 32)

    def add(slot, col, hit):
        r = np.arange(len(rows))
        np.add.at(acc[slot, :, 0], bins[r, col], 1)
        np.add.at(acc[slot, :, 1], bins[r, col], hit.astype(np.int64))
        np.add.at(acc[slot, :, 2], bins[r, col], q[r, col])

    a = Pv.argmax(axis=1)                                        # the first maximal column
    add(0, a, a == yv)
    if classwise:
        for c in range(C):
            add(1 + c, np.full(len(rows), c), yv == c)
    br = np.zeros(len(rows), dtype=np.float64)
    for c in range(C):                                           # column order; product and add rounded apart
        d = P64[rows, c] - (yv == c)
        br = br + d * d
    tot[2] = int(np.rint(br * float(BRIER_ONE)).astype(np.int64).sum())
    return acc, tot


def temperature_nll_reference(S, y, temperature=1.0, beta=None, n_classes=None, dtype=np.float64):
    """numpy restatement of msn_temperature_nll: {n_valid, sum nll_i, sum g_i, sum h_i, n_bad} as an array of `dtype`.  The rows'
    terms are formed in `dtype` -- d = x - max x, u = beta d, nll = log(sum exp u) - u_y, mu = sum(e d) / sum e, g = mu - d_y,
    h = sum(e (d - mu)^2) / sum e -- and added by math.fsum (fp64: the correctly rounded sum) or in `dtype` (longdouble: the
    reference of the accuracy tests)."""
    S, y, C, in_range = reference_inputs(S, y, n_classes, "temperature_nll_reference")
    b = dtype(_beta(temperature, beta, "temperature_nll_reference"))
    finite = np.isfinite(S).all(axis=1)
    rows = np.nonzero(in_range & finite)[0]
    out = np.zeros(5, dtype=dtype)
    out[0], out[4] = len(rows), int((in_range & ~finite).sum())
    if not len(rows):
        return out
    X = S[rows].astype(dtype)
    d = X - X.max(axis=1, keepdims=True)
    dy = d[np.arange(len(rows)), y[rows]]
    e = np.exp(b * d)
    z = e.sum(axis=1)
    mu = (e * d).sum(axis=1) / z
    t = d - mu[:, None]
    terms = (np.log(z) - b * dy, mu - dy, (e * (t * t)).sum(axis=1) / z)
    for k, v in enumerate(terms):
        out[1 + k] = math.fsum(v.tolist()) if dtype is np.float64 else v.sum(dtype=dtype)
    return out


def _fit_beta(evaluate, max_iter, tol, bounds, who):
    """Newton on beta = 1 / T from 1 for the convex objective sum nll(beta); evaluate(beta) -> the five numbers of
    msn_temperature_nll.  Safeguard: the sign of the gradient keeps a bracket [lo, hi] around the minimum (inside
    1 / bounds[1] .. 1 / bounds[0]); a step that leaves it is replaced by the bracket's geometric mean (bisection in log beta).
    Stops when |sum g| / n <= tol; without that within max_iter evaluations, the best point seen is kept and a warning given."""
    t_lo, t_hi = float(bounds[0]), float(bounds[1])
    if not (0.0 < t_lo < t_hi and math.isfinite(t_hi)) or int(max_iter) < 1 or not tol > 0:
        raise ValueError(f"{who}: 0 < bounds[0] < bounds[1] < inf, max_iter >= 1 and tol > 0 needed")
    lo, hi = 1.0 / t_hi, 1.0 / t_lo
    beta = min(max(1.0, lo), hi)
    first = best = None
    converged = False
    for it in range(1, int(max_iter) + 1):
        n, nll, g, h, n_bad = (float(v) for v in evaluate(beta))
        if not n > 0:
            raise ValueError(f"{who}: no valid row (every target lies outside the classes or every row holds a non-finite logit)")
        if first is None:
            first = nll / n
        if best is None or nll < best[1]:
            best = (beta, nll)
        if abs(g) / n <= tol:
            converged = True
            best = (beta, nll)
            break
        if g > 0:
            hi = beta
        else:
            lo = beta
        step = beta - g / h if h > 0 else float("nan")
        beta = step if lo < step < hi else math.sqrt(lo * hi)
    if not converged:
        warnings.warn(f"{who}: |gradient| / n did not reach {tol:g} within {max_iter} evaluations (the minimum may lie outside "
                      f"the temperature bounds {bounds}); the best temperature seen is kept", RuntimeWarning, stacklevel=3)
    return {"beta": best[0], "temperature": 1.0 / best[0], "n_iter": it, "nll_before": first, "nll_after": best[1] / n,
            "converged": converged, "n": int(n), "n_bad": int(n_bad)}


def fit_temperature_reference(logits, target, max_iter=50, tol=1e-8, bounds=(1e-2, 1e2)):
    """The iteration of TemperatureScaling.fit over temperature_nll_reference (numpy fp64): a dict with beta, temperature, n_iter,
    nll_before, nll_after (means), converged, n, n_bad."""
    S = np.asarray(logits, dtype=np.float32)
    y = np.asarray(target).astype(np.int64)
    return _fit_beta(lambda b: temperature_nll_reference(S, y, beta=b), max_iter, tol, bounds, "fit_temperature_reference")


# ---------------------------------------------------------------------------------------------- host: the metrics
def _slots(acc, who):
    a = to_numpy(acc, np.int64)
    if a.ndim == 2:
        a = a[None]
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"{who}: acc (slots, B, 3) needed (got {a.shape})")
    return a


def _gaps(cells):
    """Per bin |S_b - H_b 2^32| and the rows n_b of one slot, in Python integers."""
    return [abs(s - h * Q_ONE) for _, h, s in cells], [n for n, _, _ in cells]


def _slot_ece(cells, norm):
    gaps, counts = _gaps(cells)
    n = sum(counts)
    if not n:
        return float("nan")
    if norm == "l1":
        return sum(gaps) / (n * Q_ONE)                            # Python integers: the quotient is rounded once
    return max(g / (k * Q_ONE) for g, k in zip(gaps, counts) if k)


def ece_from_counts(acc, norm="l1"):
    """Top-label calibration error from acc (slot 0 of (slots, B, 3), or (B, 3)): norm="l1" the expected calibration error
    sum_b |S_b / 2^32 - H_b| / n, norm="max" the maximum calibration error max_b |S_b / 2^32 - H_b| / n_b over the bins that
    hold a row.  The differences are formed in Python integers and divided once; nan without rows."""
    if norm not in ("l1", "max"):
        raise ValueError(f"ece_from_counts: norm must be 'l1' or 'max' (got {norm!r})")
    return _slot_ece(_slots(acc, "ece_from_counts")[0].tolist(), norm)


def classwise_ece_from_counts(acc, average="macro"):
    """Classwise ECE from the slots 1 .. C of acc (1 + C, B, 3): per class sum_b |S_b / 2^32 - H_b| / n with the class's own
    probability as the confidence and (y = c) as the hit; average="macro" their mean, None the per-class array."""
    a = _slots(acc, "classwise_ece_from_counts")
    if a.shape[0] < 2:
        raise ValueError("classwise_ece_from_counts: acc holds the top-label slot only (count with classwise=True)")
    if average not in ("macro", None):
        raise ValueError(f"classwise_ece_from_counts: average must be 'macro' or None (got {average!r})")
    per = np.array([_slot_ece(cells, "l1") for cells in a[1:].tolist()])
    return per if average is None else float(per.mean())


def brier_from_counts(tot):
    """Multi-class Brier score mean_i sum_c (p_ic - [y_i = c])^2 from tot = {n, n_bad, sum of rint(brier_i 2^30)}; nan without
    rows.  (Twice scikit-learn's brier_score_loss for two classes.)"""
    n, _, s = (int(v) for v in to_numpy(tot, np.int64).reshape(3))
    return s / (n * BRIER_ONE) if n else float("nan")


def reliability_curve(acc, slot=0):
    """(bin_confidence, bin_accuracy, bin_count) of one slot, each (B): the mean confidence S_b / (n_b 2^32) and the share of
    hits H_b / n_b of the rows in bin b (edges k / B), nan for an empty bin; bin_count int64."""
    cells = _slots(acc, "reliability_curve")[slot].tolist()
    conf = np.array([s / (n * Q_ONE) if n else float("nan") for n, _, s in cells])
    hits = np.array([h / n if n else float("nan") for n, h, _ in cells])
    return conf, hits, np.array([n for n, _, _ in cells], dtype=np.int64)


# ------------------------------------------------------------------------------------------------------ device halves
def softmax_rows(logits, temperature=1.0, beta=None):
    """softmax(logits / temperature) over the rows of float32 (N, C) logits in one launch (msn_softmax_rows: evaluated in fp64,
    rounded to fp32 once), a new dense tensor.  Enqueue only."""
    b = _beta(temperature, beta, "softmax_rows")
    S = rows_on_gpu(logits, "softmax_rows", "scores", MAX_CLASSES)
    N, C = S.shape
    out = torch.empty((N, C), dtype=torch.float32, device=S.device)
    check(lib().msn_softmax_rows(ptr(S), ld(S), N, C, b, ptr(out), C, stream_ptr()), "msn_softmax_rows")
    return out


def calibration_counts(probs, target, n_bins=15, classwise=False, acc=None, tot=None):
    """(acc int64 (slots, n_bins, 3), tot int64 (3)) of msn_calibration_counts for float32 (N, C) probabilities on the device,
    slots = 1 + C with classwise; acc / tot given are added to (the accumulators of a validation epoch), else they start from
    zero.  Enqueue only."""
    P, y = scores_and_targets(probs, target, "calibration_counts")
    N, C = P.shape
    B = int(n_bins)
    if not 1 <= B <= MAX_BINS:
        raise _lib.MsnHipError(f"calibration_counts: 1 to {MAX_BINS} bins (got {n_bins})")
    acc = accumulator(acc, (1 + C if classwise else 1, B, 3), P.device, "calibration_counts")
    tot = accumulator(tot, (3,), P.device, "calibration_counts")
    check(lib().msn_calibration_counts(ptr(P), ld(P), ptr(y), N, C, B, int(bool(classwise)), ptr(acc), ptr(tot), stream_ptr()),
          "msn_calibration_counts")
    return acc, tot


def temperature_nll(logits, target, temperature=1.0, beta=None):
    """{n_valid, sum nll, sum d nll / d beta, sum d2 nll / d beta2, n_bad} of msn_temperature_nll at beta = 1 / temperature: five
    doubles on the device.  Enqueue only."""
    b = _beta(temperature, beta, "temperature_nll")
    S, y = scores_and_targets(logits, target, "temperature_nll")
    N, C = S.shape
    out = torch.empty(5, dtype=torch.float64, device=S.device)
    L = lib()
    ws = workspace(L.msn_temperature_nll_workspace_bytes(N), S.device)
    check(L.msn_temperature_nll(ptr(S), ld(S), ptr(y), N, C, b, ptr(out), ptr(ws), ws.numel(), stream_ptr()),
          "msn_temperature_nll")
    return out


class CalibrationMetrics(EpochCounts):
    """ECE, MCE, Brier score and the reliability diagram over the batches of a validation epoch, in the shape of
    metrics.RankingMetrics in its binned mode: reset, update(scores, target), all_reduce(group), compute().

    update is one msn_calibration_counts launch into int64 accumulators (after one msn_softmax_rows launch with
    normalize="softmax", which turns logits into softmax(logits / temperature)); all_reduce their SUM, which is exact; compute
    the one host copy.  classwise=True also bins every class's own probability (classwise ECE)."""

    _counts = ("acc", "tot")

    def __init__(self, n_classes, n_bins=15, classwise=False, normalize=None, temperature=1.0):
        self.n_classes, self.n_bins = int(n_classes), int(n_bins)
        if not 1 <= self.n_classes <= MAX_CLASSES:
            raise ValueError(f"CalibrationMetrics: n_classes must be in 1..{MAX_CLASSES} (got {n_classes})")
        if not 1 <= self.n_bins <= MAX_BINS:
            raise ValueError(f"CalibrationMetrics: n_bins must be in 1..{MAX_BINS} (got {n_bins})")
        if normalize not in (None, "softmax"):
            raise ValueError(f"CalibrationMetrics: normalize must be None or 'softmax' (got {normalize!r})")
        self.temperature = float(temperature)
        _beta(self.temperature, None, "CalibrationMetrics")
        if normalize is None and self.temperature != 1.0:
            raise ValueError("CalibrationMetrics: a temperature applies to logits (normalize='softmax')")
        self.classwise, self.normalize = bool(classwise), normalize
        self.acc = self.tot = None

    def _buffers(self, device):
        if self.acc is None or self.acc.device != device:
            slots = 1 + self.n_classes if self.classwise else 1
            self.acc = torch.zeros((slots, self.n_bins, 3), dtype=torch.int64, device=device)
            self.tot = torch.zeros(3, dtype=torch.int64, device=device)

    def update(self, scores, target):
        """scores float32 (N, n_classes) on the GPU -- probabilities, or logits with normalize="softmax" -- and target int64 (N).
        Enqueue only; an empty batch counts nothing."""
        if isinstance(scores, torch.Tensor) and scores.dim() == 2 and scores.shape[0] == 0:
            return
        if isinstance(target, torch.Tensor):
            target = target.to(torch.int64)
        S, y = scores_and_targets(scores, target, "CalibrationMetrics.update")
        if S.shape[1] != self.n_classes:
            raise ValueError(f"CalibrationMetrics.update: {S.shape[1]} score columns for {self.n_classes} classes")
        if self.normalize == "softmax":
            S = softmax_rows(S, self.temperature)
        self._buffers(S.device)
        calibration_counts(S, y, self.n_bins, self.classwise, acc=self.acc, tot=self.tot)

    def compute(self):
        """The one host copy: {ece, mce, brier, n, n_bad, bin_confidence, bin_accuracy, bin_count} and, classwise,
        {classwise_ece, classwise_ece_per_class}.  Warns when rows were bad (n_bad > 0): they are in no other number."""
        if self.acc is None:
            acc = torch.zeros((1 + self.n_classes if self.classwise else 1, self.n_bins, 3), dtype=torch.int64)
            tot = torch.zeros(3, dtype=torch.int64)
        else:
            acc, tot = self.acc.cpu(), self.tot.cpu()
        n, n_bad = int(tot[0]), int(tot[1])
        if n_bad:
            warnings.warn(f"CalibrationMetrics: {n_bad} row(s) with a target in range do not hold probabilities (entries outside "
                          f"[0, 1], a NaN, or a sum away from 1); they count in n_bad only", RuntimeWarning, stacklevel=2)
        conf, hits, count = reliability_curve(acc, 0)
        res = {"ece": ece_from_counts(acc, "l1"), "mce": ece_from_counts(acc, "max"), "brier": brier_from_counts(tot), "n": n,
               "n_bad": n_bad, "bin_confidence": conf, "bin_accuracy": hits, "bin_count": count}
        if self.classwise:
            per = classwise_ece_from_counts(acc, None)
            res.update(classwise_ece=float(per.mean()), classwise_ece_per_class=[float(v) for v in per])
        return res


class TemperatureScaling:
    """Post-hoc temperature scaling (Guo et al. 2017): the one scalar T > 0 that minimises the mean negative log-likelihood of
    softmax(logits / T) on held-out rows.  fit runs a safeguarded Newton iteration on beta = 1 / T from 1 -- the objective is
    convex in beta -- with one msn_temperature_nll evaluation (value, gradient and curvature in fp64) and one host copy of
    five doubles per iteration; under data parallel the five doubles are SUM-all-reduced first, so every rank takes identical
    steps.  It stops when |d nll / d beta| / n <= tol.  Rows with a target outside the classes are ignored, rows with a
    non-finite logit are counted in n_bad_ and otherwise left out.

    After fit: temperature_, n_iter_ (evaluations), nll_before_ / nll_after_ (mean NLL at T = 1 and at temperature_),
    converged_, n_, n_bad_.  predict_proba(logits) = softmax_rows(logits, temperature_)."""

    def __init__(self, max_iter=50, tol=1e-8, bounds=(1e-2, 1e2)):
        self.max_iter, self.tol, self.bounds = int(max_iter), float(tol), (float(bounds[0]), float(bounds[1]))
        self.temperature_ = None

    def fit(self, logits, target, group=None):
        if isinstance(target, torch.Tensor):
            target = target.to(torch.int64)
        S, y = scores_and_targets(logits, target, "TemperatureScaling.fit")
        world = D.world_size(group)

        def evaluate(beta):
            out = temperature_nll(S, y, beta=beta)
            if world > 1:
                D.all_reduce_sum(out, group, kind="metric_all_reduce")
            return out.cpu().tolist()

        r = _fit_beta(evaluate, self.max_iter, self.tol, self.bounds, "TemperatureScaling.fit")
        self.beta_, self.temperature_, self.n_iter_ = r["beta"], r["temperature"], r["n_iter"]
        self.nll_before_, self.nll_after_, self.converged_ = r["nll_before"], r["nll_after"], r["converged"]
        self.n_, self.n_bad_ = r["n"], r["n_bad"]
        return self

    def predict_proba(self, logits):
        if self.temperature_ is None:
            raise RuntimeError("TemperatureScaling.predict_proba: fit first")
        return softmax_rows(logits, beta=self.beta_)
