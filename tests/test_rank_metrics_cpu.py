"""Threshold-free classification metrics without a GPU (multimodal_supernovae_amd/metrics.py): the numpy restatements against
brute-force definitions and against scikit-learn, the host functions' nan / averaging conventions, the binned curve functions
on a hand-made accumulator, and the refusals (CPU tensors, dtypes, MSN_ERR_SHAPE through the C-ABI before any launch)."""
import ctypes
import math

import numpy as np
import pytest
import torch

from multimodal_supernovae_amd import metrics as M

REL = 4 * 2.0 ** -53          # against scikit-learn: the same rationals in fp64 with a handful of roundings


def _tied_case(N=40, C=5, seed=0):
    """Integer scores in [-3, 3] (ties everywhere), class 3 empty, some targets -100 and one above the range."""
    rng = np.random.default_rng(seed)
    S = rng.integers(-3, 4, (N, C)).astype(np.float32)
    y = rng.integers(0, C, N)
    y[y == 3] = 4
    y[::7] = -100
    y[5] = C + 2
    return S, y


def test_restatements_equal_the_brute_force_definitions():
    S, y = _tied_case()
    N, C = S.shape
    valid = [0 <= y[i] < C for i in range(N)]
    counts = np.zeros((N, 3), dtype=np.int64)
    for i in range(N):
        if not valid[i]:
            continue
        c, s = y[i], S[i, y[i]]
        for j in range(N):
            if not valid[j]:
                continue
            if y[j] != c:
                counts[i, 0] += S[j, c] > s
                counts[i, 1] += S[j, c] >= s
            else:
                counts[i, 2] += S[j, c] >= s
    istats = np.zeros((C, 3), dtype=np.int64)
    ap = [[] for _ in range(C)]
    for c in range(C):
        P = sum(1 for i in range(N) if valid[i] and y[i] == c)
        Nneg = sum(1 for i in range(N) if valid[i] and y[i] != c)
        U2 = sum(2 * Nneg - counts[i, 0] - counts[i, 1] for i in range(N) if valid[i] and y[i] == c)
        istats[c] = (P, Nneg, U2)
        ap[c] = [counts[i, 2] / (counts[i, 2] + counts[i, 1]) for i in range(N) if valid[i] and y[i] == c]
    got_counts, got_istats, got_ap = M.rank_counts_reference(S, y)
    assert got_counts.dtype == np.int32 and np.array_equal(got_counts, counts)
    assert got_istats.dtype == np.int64 and np.array_equal(got_istats, istats)
    assert istats[3, 0] == 0 and (counts[::7] == 0).all() and (counts[5] == 0).all()
    assert [float(v) for v in got_ap] == [math.fsum(t) for t in ap]
    # U2 is twice the Mann-Whitney statistic with ties at one half
    for c in range(C):
        u2 = 0
        for i in range(N):
            for j in range(N):
                if valid[i] and valid[j] and y[i] == c and y[j] != c:
                    u2 += 2 * (S[i, c] > S[j, c]) + (S[i, c] == S[j, c])
        assert u2 == istats[c, 2]

    thr = np.array([-3.0, -1.0, -1.0, 0.5, 3.0, 4.0], dtype=np.float32)
    acc = np.zeros((C, len(thr), 2), dtype=np.int64)
    tot = np.zeros((C, 2), dtype=np.int64)
    for c in range(C):
        for i in range(N):
            if not valid[i]:
                continue
            k = 0 if y[i] == c else 1
            tot[c, k] += 1
            for t in range(len(thr)):
                acc[c, t, k] += S[i, c] >= thr[t]
    got_acc, got_tot = M.threshold_counts_reference(S, y, thr)
    assert np.array_equal(got_acc, acc) and np.array_equal(got_tot, tot) and np.array_equal(tot, istats[:, :2])

    rank = np.full(N, -1, dtype=np.int64)
    for i in range(N):
        if valid[i]:
            rank[i] = sum(1 for k in range(C) if S[i, k] > S[i, y[i]] or (S[i, k] == S[i, y[i]] and k < y[i]))
    got_rank, got_hist = M.topk_ranks_reference(S, y)
    assert got_rank.dtype == np.int32 and np.array_equal(got_rank, rank)
    assert np.array_equal(got_hist, np.bincount(rank[rank >= 0], minlength=C)) and got_hist.sum() == sum(valid)


def test_nan_scores_compare_false_both_ways():
    S = np.array([[0.0, np.nan], [1.0, 0.0], [np.nan, 2.0], [0.5, 1.0]], dtype=np.float32)
    y = np.array([0, 0, 1, 1])
    counts, istats, ap = M.rank_counts_reference(S, y)
    # class 0: positives 0.0, 1.0, negatives nan, 0.5; class 1: positives 2.0, 1.0, negatives nan, 0.0
    assert counts.tolist() == [[1, 1, 2], [0, 0, 1], [0, 0, 1], [0, 0, 2]]
    assert istats.tolist() == [[2, 2, 6], [2, 2, 8]]
    Sn = S.copy()
    Sn[0, 0] = np.nan                                          # a positive's own score: p_ge = 0, the class's ap_sum is nan
    counts, _, ap = M.rank_counts_reference(Sn, y)
    assert counts[0].tolist() == [0, 0, 0] and math.isnan(ap[0]) and not math.isnan(ap[1])
    rank, _ = M.topk_ranks_reference(Sn, y)
    assert rank[0] == 0
    acc, _ = M.threshold_counts_reference(Sn, y, [-np.inf, 0.0])
    assert acc[0, :, 0].tolist() == [1, 1]


@pytest.mark.parametrize("kind", ["tied", "normal"])
def test_restatements_and_host_functions_agree_with_scikit_learn(kind):
    sk = pytest.importorskip("sklearn.metrics")
    rng = np.random.default_rng(3)
    N, C = 517, 5
    S = rng.integers(-3, 4, (N, C)).astype(np.float32) if kind == "tied" else rng.standard_normal((N, C)).astype(np.float32)
    y = rng.choice(C, N, p=[0.6, 0.2, 0.1, 0.07, 0.03])
    y[::11] = -100
    keep = y >= 0
    _, istats, ap_sum = M.rank_counts_reference(S, y)
    au = M.auroc_from_stats(istats, None)
    ap = M.average_precision_from_stats(istats, ap_sum, None)
    want_au = np.array([sk.roc_auc_score(y[keep] == c, S[keep, c].astype(np.float64)) for c in range(C)])
    want_ap = np.array([sk.average_precision_score(y[keep] == c, S[keep, c].astype(np.float64)) for c in range(C)])
    print("auroc", au, "relative difference", np.abs(au - want_au) / want_au)
    print("ap", ap, "relative difference", np.abs(ap - want_ap) / want_ap)
    assert (np.abs(au - want_au) <= REL * want_au).all()
    assert (np.abs(ap - want_ap) <= REL * want_ap).all()
    assert abs(M.auroc_from_stats(istats, "macro") - want_au.mean()) <= REL * want_au.mean()
    P = istats[:, 0]
    assert abs(M.auroc_from_stats(istats, "weighted") - (want_au * P).sum() / P.sum()) <= REL
    assert abs(M.average_precision_from_stats(istats, ap_sum, "macro") - want_ap.mean()) <= REL * want_ap.mean()
    if kind == "normal":                                       # scikit-learn orders tied classes its own way: no ties here
        _, hist = M.topk_ranks_reference(S, y)
        for k in (1, 2, 3, 4):
            want = sk.top_k_accuracy_score(y[keep], S[keep].astype(np.float64), k=k, labels=np.arange(C))
            assert abs(M.topk_accuracy(hist, k) - want) <= REL * want
    # the binary form: class 1 of [-s, s]
    s, t = S[keep, 0], (y[keep] == 2).astype(np.int64)
    _, st, aps = M.rank_counts_reference(np.stack([-s, s], axis=1), t)
    want = sk.roc_auc_score(t, s.astype(np.float64)), sk.average_precision_score(t, s.astype(np.float64))
    assert abs(M.auroc_from_stats(st, None)[1] - want[0]) <= REL * want[0]
    assert abs(M.average_precision_from_stats(st, aps, None)[1] - want[1]) <= REL * want[1]


def test_nan_and_averaging_conventions():
    # class 1 has no positive, class 2 every valid row but one
    S = np.array([[0.1, 0.2, 0.3], [0.4, 0.0, 0.9], [0.3, 0.1, 0.5], [0.9, 0.9, 0.9]], dtype=np.float32)
    y = np.array([2, 2, 0, -100])
    _, istats, ap_sum = M.rank_counts_reference(S, y)
    au, ap = M.auroc_from_stats(istats, None), M.average_precision_from_stats(istats, ap_sum, None)
    assert istats[:, :2].tolist() == [[1, 2], [0, 3], [2, 1]]
    assert au[0] == 0.5 and math.isnan(au[1]) and au[2] == 0.5
    assert ap[0] == 0.5 and math.isnan(ap[1]) and ap[2] == (1.0 + 2.0 / 3.0) / 2
    assert M.auroc_from_stats(istats, "macro") == 0.5                      # the undefined class is left out of the mean
    assert M.auroc_from_stats(istats, "weighted") == 0.5
    assert M.average_precision_from_stats(istats, ap_sum, "weighted") == (0.5 * 1 + ap[2] * 2) / 3
    with pytest.raises(ValueError, match="average must be"):
        M.auroc_from_stats(istats, "micro")
    # all rows one class: no negatives anywhere -> AUROC undefined everywhere, AP 1.0 for the class that occurs
    _, istats, ap_sum = M.rank_counts_reference(S, np.array([1, 1, 1, 1]))
    assert np.isnan(M.auroc_from_stats(istats, None)).all() and math.isnan(M.auroc_from_stats(istats, "macro"))
    ap = M.average_precision_from_stats(istats, ap_sum, None)
    assert math.isnan(ap[0]) and ap[1] == 1.0 and math.isnan(ap[2]) and M.average_precision_from_stats(istats, ap_sum) == 1.0
    # N = 1, and nothing valid at all
    counts, istats, ap_sum = M.rank_counts_reference(S[:1], np.array([2]))
    assert counts.tolist() == [[0, 0, 1]] and istats.tolist() == [[0, 1, 0], [0, 1, 0], [1, 0, 0]] and ap_sum.tolist() == [0, 0, 1]
    assert math.isnan(M.auroc_from_stats(istats)) and M.average_precision_from_stats(istats, ap_sum) == 1.0
    _, istats, ap_sum = M.rank_counts_reference(S[:1], np.array([-100]))
    assert not istats.any() and math.isnan(M.average_precision_from_stats(istats, ap_sum))
    # top-k
    hist = np.array([5, 3, 0, 2])
    assert [M.topk_accuracy(hist, k) for k in (1, 2, 3, 4)] == [0.5, 0.8, 0.8, 1.0]
    assert math.isnan(M.topk_accuracy(np.zeros(4, dtype=np.int64), 1))
    with pytest.raises(ValueError, match="k must be"):
        M.topk_accuracy(hist, 5)


def test_binned_curves_on_a_hand_made_accumulator():
    """Class 0: positives at 1 and 0.5, negatives at 0.5 and 0, thresholds 0, 0.5, 1, 2; class 1 has no positive; class 2 no
    negative."""
    acc = np.array([[[2, 2], [2, 1], [1, 0], [0, 0]],
                    [[0, 4], [0, 2], [0, 1], [0, 0]],
                    [[4, 0], [3, 0], [1, 0], [0, 0]]], dtype=np.int64)
    tot = np.array([[2, 2], [0, 4], [4, 0]], dtype=np.int64)
    fpr, tpr = M.roc_curve_binned(acc, tot)
    assert fpr[0].tolist() == [1.0, 0.5, 0.0, 0.0] and tpr[0].tolist() == [1.0, 1.0, 0.5, 0.0]
    assert np.isnan(tpr[1]).all() and fpr[1].tolist() == [1.0, 0.5, 0.25, 0.0] and np.isnan(fpr[2]).all()
    precision, recall = M.precision_recall_curve_binned(torch.from_numpy(acc), torch.from_numpy(tot))
    assert precision[0].tolist() == [0.5, 2.0 / 3.0, 1.0, 1.0] and recall[0].tolist() == [1.0, 1.0, 0.5, 0.0]
    assert precision[1].tolist() == [0.0, 0.0, 0.0, 1.0] and np.isnan(recall[1]).all()
    assert precision[2].tolist() == [1.0, 1.0, 1.0, 1.0] and recall[2].tolist() == [1.0, 0.75, 0.25, 0.0]
    au = M.binned_auroc(acc, tot, None)
    ap = M.binned_average_precision(acc, tot, None)
    assert au[0] == 0.875 and math.isnan(au[1]) and math.isnan(au[2])        # the exact AUROC: 3.5 of 4 pairs
    assert ap[0] == pytest.approx(0.5 + 1.0 / 3.0, rel=1e-15) and math.isnan(ap[1]) and ap[2] == 1.0
    assert M.binned_auroc(acc, tot) == 0.875 and M.binned_average_precision(acc, tot, "macro") == pytest.approx((ap[0] + 1.0) / 2)
    # the scores lie on the thresholds, so the binned values are the exact ones
    S = np.array([[1.0], [0.5], [0.5], [0.0]], dtype=np.float32)
    _, st, aps = M.rank_counts_reference(np.concatenate([S, -S], axis=1), np.array([0, 0, 1, 1]))
    assert M.auroc_from_stats(st, None)[0] == au[0] and M.average_precision_from_stats(st, aps, None)[0] == pytest.approx(ap[0], rel=1e-15)
    got_acc, got_tot = M.threshold_counts_reference(np.concatenate([S, -S], axis=1), np.array([0, 0, 1, 1]), [0.0, 0.5, 1.0, 2.0])
    assert np.array_equal(got_acc[0], acc[0]) and np.array_equal(got_tot[0], tot[0])
    with pytest.raises(ValueError, match="acc"):
        M.roc_curve_binned(acc[:, :, 0], tot)


def test_cpu_tensors_and_wrong_dtypes_are_refused():
    from multimodal_supernovae_amd._lib import MsnHipError
    S, y = torch.zeros(4, 3), torch.zeros(4, dtype=torch.int64)
    for call in (lambda: M.rank_counts(S, y), lambda: M.threshold_counts(S, y, torch.zeros(2)), lambda: M.topk_ranks(S, y),
                 lambda: M.log_softmax_rows(S), lambda: M.multiclass_auroc(S, y), lambda: M.binary_auroc(S[:, 0], y),
                 lambda: M.RankingMetrics(3).update(S, y)):
        with pytest.raises(MsnHipError, match="must live on the GPU"):
            call()
    for call in (lambda: M.rank_counts(S.double(), y), lambda: M.topk_ranks(S.half(), y), lambda: M.log_softmax_rows(S.double()),
                 lambda: M.multiclass_average_precision(S.to(torch.bfloat16), y), lambda: M.binary_average_precision(S[:, 0].double(), y),
                 lambda: M.rank_counts(S[0], y), lambda: M.rank_counts(S.numpy(), y)):
        with pytest.raises(ValueError, match="float32"):
            call()
    with pytest.raises(ValueError, match="normalize"):
        M.RankingMetrics(3, normalize="softmax")
    with pytest.raises(ValueError, match="top_k"):
        M.RankingMetrics(3, top_k=(4,))
    with pytest.raises(ValueError, match="thresholds"):
        M.RankingMetrics(3, thresholds=2000)
    empty = M.RankingMetrics(3, top_k=(1, 2)).compute()                    # nothing seen: every metric undefined, no GPU touched
    assert math.isnan(empty["auroc_macro"]) and math.isnan(empty["ap_macro"]) and math.isnan(empty["top2_acc"])
    assert len(empty["auroc_per_class"]) == 3


def test_shape_limits_come_back_through_the_c_abi_without_a_gpu():
    import __graft_entry__ as entry
    entry.build()
    from multimodal_supernovae_amd import _lib
    L = _lib.lib()
    fake = ctypes.c_void_p(4096)          # never dereferenced: validation rejects the call before any launch
    big = 1 << 40

    def refused(rc, text):
        assert rc == 1 and text in L.msn_last_error(), (rc, L.msn_last_error())

    for C in (0, 1025):
        refused(L.msn_rank_counts(fake, 2048, fake, 8, C, fake, fake, fake, fake, big, None), b"C must be in 1..1024")
        refused(L.msn_threshold_counts(fake, 2048, fake, 8, C, fake, 4, fake, fake, None), b"C must be in 1..1024")
        refused(L.msn_topk_ranks(fake, 2048, fake, 8, C, fake, fake, None), b"C must be in 1..1024")
        refused(L.msn_log_softmax_rows(fake, 2048, 8, C, fake, 2048, None), b"C must be in 1..1024")
        assert L.msn_rank_counts_workspace_bytes(8, C) == 0
    for T in (0, 1025):
        refused(L.msn_threshold_counts(fake, 5, fake, 8, 5, fake, T, fake, fake, None), b"T must be in 1..1024")
    for N in (0, 1 << 31):
        refused(L.msn_rank_counts(fake, 5, fake, N, 5, fake, fake, fake, fake, big, None), b"N must be in")
        refused(L.msn_threshold_counts(fake, 5, fake, N, 5, fake, 4, fake, fake, None), b"N must be in")
        refused(L.msn_topk_ranks(fake, 5, fake, N, 5, fake, fake, None), b"N must be in")
        refused(L.msn_log_softmax_rows(fake, 5, N, 5, fake, 5, None), b"N must be in")
    refused(L.msn_rank_counts(fake, 4, fake, 8, 5, fake, fake, fake, fake, big, None), b"row stride")
    refused(L.msn_rank_counts(fake, 5, fake, 8, 5, fake, fake, fake, fake, 8, None), b"workspace")
    refused(L.msn_rank_counts(None, 5, fake, 8, 5, fake, fake, fake, fake, big, None), b"null pointer")
    # the workspace is 12 bytes per row and slab; the slabs are whole chunks of 128 rows, at most 16
    assert L.msn_rank_counts_workspace_bytes(1, 5) == 12
    assert L.msn_rank_counts_workspace_bytes(259, 5) == 3 * 259 * 12
    assert L.msn_rank_counts_workspace_bytes(3100, 64) == 13 * 3100 * 12
    assert L.msn_rank_counts_workspace_bytes(65536, 5) == 4 * 65536 * 12
