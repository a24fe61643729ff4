"""Validation-time retrieval metric with the reference's function names (src/utils.py:256-272, 380-426):
the per-row similarity ranking runs in one fused HIP kernel instead of a Python loop over argsorts."""
import numpy as np
import torch

from . import ops
from ._lib import check, lib, ptr, stream_ptr


def retrieval_ranks(embs1, embs2):
    """rank[i] = number of rows of embs1 more similar (cosine) to embs2[i] than its partner embs1[i]."""
    if embs1.shape != embs2.shape:
        raise ValueError("retrieval ranks need two (N, D) embedding sets of equal shape")
    e1, _ = ops.l2norm_fwd(embs1.detach().float().contiguous())          # cosine_similarity normalises both, :268-269
    e2, _ = ops.l2norm_fwd(embs2.detach().float().contiguous())
    n, d = e1.shape
    rank = torch.empty(n, dtype=torch.int32, device=e1.device)
    L = lib()
    nb = L.msn_infonce_workspace_bytes(n, n, n, n, d)
    ws = torch.empty(max(nb, 16) // 4 + 1, dtype=torch.float32, device=e1.device)
    check(L.msn_retrieval_rank(ptr(e1), d, ptr(e2), d, n, d, ptr(rank), ptr(ws), nb, stream_ptr()), "msn_retrieval_rank")
    return rank


def get_ROC_data(embs1, embs2):
    """(thresholds, fraction_correct): fraction of rows whose partner is inside the top int(threshold * N)
    of the similarity ranking, for 100 thresholds in [0, 1] (ref src/utils.py:380-411)."""
    ranks = retrieval_ranks(embs1, embs2).cpu().numpy()
    n = len(ranks)
    thresholds = np.linspace(0, 1, 100)
    top = np.array([int(t * n) for t in thresholds])
    fraction_correct = (ranks[None, :] < top[:, None]).sum(axis=1) / n
    return thresholds, fraction_correct


def get_AUC(embs1, embs2):
    """Area under that curve (ref src/utils.py:414-426)."""
    thresholds, fraction_correct = get_ROC_data(embs1, embs2)
    return np.trapezoid(fraction_correct, thresholds) if hasattr(np, "trapezoid") else np.trapz(fraction_correct, thresholds)


def get_linear_predictions(X, Y, X_val=None, Y_val=None, task="regression", **probe_kwargs):
    """Fit a linear probe on the embeddings (X, Y) and return its predictions for X_val (for X when X_val is None) as a
    tensor on the device: fp32 values for task="regression" (probes.LinearRegressionProbe), int32 classes for
    task="classification" (probes.LogisticRegressionProbe); probe_kwargs go to the probe.  Named after the reference's helper
    (SURVEY.md section 2 row 7); the reference's source is not available to this build, so this is the helper's role and not
    a line-by-line port.  Y_val is accepted for the reference's call shape and is not used."""
    from .probes import LinearRegressionProbe, LogisticRegressionProbe
    if task == "regression":
        probe = LinearRegressionProbe(**probe_kwargs).fit(X, Y)
    elif task == "classification":
        probe = LogisticRegressionProbe(**probe_kwargs).fit(X, Y)
    else:
        raise ValueError(f"get_linear_predictions: task must be 'regression' or 'classification' (got {task!r})")
    return probe.predict(X if X_val is None else X_val)


def _ranking_keys(scores, Y_val):
    """auroc_macro, ap_macro and their per-class lists of (N, C) scores on the device (metrics.rank_counts: exact)."""
    from . import metrics as M
    _, istats, ap_sum = M.rank_counts(scores, Y_val.to(torch.int64))
    istats, ap_sum = istats.cpu(), ap_sum.cpu()
    return {"auroc_macro": M.auroc_from_stats(istats, "macro"), "ap_macro": M.average_precision_from_stats(istats, ap_sum, "macro"),
            "auroc_per_class": [float(v) for v in M.auroc_from_stats(istats, None)],
            "ap_per_class": [float(v) for v in M.average_precision_from_stats(istats, ap_sum, None)]}


def _calibration_keys(probs, Y_val):
    """ece, mce and brier of (N, C) probabilities on the device (calibration.calibration_counts: 15 bins, integer counts)."""
    from . import calibration as K
    acc, tot = K.calibration_counts(probs, Y_val.to(torch.int64))
    acc, tot = acc.cpu(), tot.cpu()
    return {"ece": K.ece_from_counts(acc, "l1"), "mce": K.ece_from_counts(acc, "max"), "brier": K.brier_from_counts(tot)}


def _no_calibration_of_regression(calibration, task, who):
    if calibration and task != "classification":
        raise ValueError(f"{who}: calibration=True belongs to task='classification' (got {task!r})")


def linear_probe_metrics(X, Y, X_val, Y_val, task="regression", n_classes=None, ranking=False, calibration=False,
                         **probe_kwargs):
    """The metrics of a linear probe fitted on (X, Y) and evaluated on (X_val, Y_val), with the keys of the reference's
    pickles: L1, L2, R2, OLF for task="regression" (RegressionMetrics), acc and the F1 scores for task="classification"
    (ClassificationMetrics over n_classes, by default the largest class of Y and Y_val plus one).  ranking=True adds, for
    classification, auroc_macro, ap_macro, auroc_per_class and ap_per_class of the probe's decision_function.
    calibration=True adds, for classification, ece, mce and brier of the softmax of the decision_function (regression refuses it)."""
    from .models_finetune import ClassificationMetrics, RegressionMetrics
    _no_calibration_of_regression(calibration, task, "linear_probe_metrics")
    if task == "classification":
        if n_classes is None:
            n_classes = int(max(Y.max().item(), Y_val.max().item())) + 1
        probe_kwargs = dict(probe_kwargs, n_classes=n_classes)
    if (ranking or calibration) and task == "classification":
        from .models_finetune import argmax_rows
        from .probes import LogisticRegressionProbe
        scores = LogisticRegressionProbe(**probe_kwargs).fit(X, Y).decision_function(X_val)
        metrics = ClassificationMetrics(n_classes)
        metrics.update(argmax_rows(scores), Y_val)
        res = metrics.compute()
        if ranking:
            res.update(_ranking_keys(scores, Y_val))
        if calibration:
            from .calibration import softmax_rows
            res.update(_calibration_keys(softmax_rows(scores), Y_val))
        return res
    pred = get_linear_predictions(X, Y, X_val, Y_val, task=task, **probe_kwargs)
    metrics = RegressionMetrics() if task == "regression" else ClassificationMetrics(n_classes)
    metrics.update(pred, Y_val)
    return metrics.compute()


def get_knn_predictions(X, Y, X_val=None, Y_val=None, k=5, task="regression", **probe_kwargs):
    """Fit a k-nearest-neighbour probe on the embeddings (X, Y) and return its predictions for X_val as a tensor on the
    device: fp32 values for task="regression" (probes.KNeighborsRegressorProbe), int32 classes for task="classification"
    (probes.KNeighborsClassifierProbe); probe_kwargs (weights, metric, n_classes) go to the probe.  With X_val = None the
    training set is predicted leave-one-out: no row is its own neighbour.  The kNN counterpart of get_linear_predictions;
    Y_val is accepted for the reference's call shape and is not used."""
    from .probes import KNeighborsClassifierProbe, KNeighborsRegressorProbe
    if task == "regression":
        probe = KNeighborsRegressorProbe(n_neighbors=k, **probe_kwargs).fit(X, Y)
    elif task == "classification":
        probe = KNeighborsClassifierProbe(n_neighbors=k, **probe_kwargs).fit(X, Y)
    else:
        raise ValueError(f"get_knn_predictions: task must be 'regression' or 'classification' (got {task!r})")
    return probe.predict(X_val)


def knn_probe_metrics(X, Y, X_val, Y_val, k=5, task="regression", n_classes=None, ranking=False, calibration=False,
                      **probe_kwargs):
    """The metrics of a kNN probe fitted on (X, Y) and evaluated on (X_val, Y_val), with the keys of linear_probe_metrics:
    L1, L2, R2, OLF for task="regression", acc and the F1 scores for task="classification" (over n_classes, by default the
    largest class of Y and Y_val plus one).  ranking=True adds, for classification, auroc_macro, ap_macro, auroc_per_class and
    ap_per_class of the probe's predict_proba (vote shares: coarse scores with many ties, which the metrics count at one half).
    calibration=True adds, for classification, ece, mce and brier of predict_proba (regression refuses it); a row that no
    labelled neighbour votes for sums to 0 and is a bad row of calibration.py: it is in none of the three."""
    from .models_finetune import ClassificationMetrics, RegressionMetrics
    _no_calibration_of_regression(calibration, task, "knn_probe_metrics")
    if task == "classification":
        if n_classes is None:
            n_classes = int(max(Y.max().item(), Y_val.max().item())) + 1
        probe_kwargs = dict(probe_kwargs, n_classes=n_classes)
    if (ranking or calibration) and task == "classification":
        from .probes import KNeighborsClassifierProbe
        probe = KNeighborsClassifierProbe(n_neighbors=k, **probe_kwargs).fit(X, Y)
        metrics = ClassificationMetrics(n_classes)
        metrics.update(probe.predict(X_val), Y_val)
        res, proba = metrics.compute(), probe.predict_proba(X_val)
        if ranking:
            res.update(_ranking_keys(proba, Y_val))
        if calibration:
            res.update(_calibration_keys(proba, Y_val))
        return res
    pred = get_knn_predictions(X, Y, X_val, Y_val, k=k, task=task, **probe_kwargs)
    metrics = RegressionMetrics() if task == "regression" else ClassificationMetrics(n_classes)
    metrics.update(pred, Y_val)
    return metrics.compute()
