"""Exact kNN search and the kNN probes on the GPU (csrc/knn.hip, multimodal_supernovae_amd/probes.py): bit-exact against the numpy
fp64 restatement on integer data (exact ties included), independent of stride, alignment and of how the rows fall into tiles
and slabs, and on normal data within bounds derived from the arithmetic; then the prediction launch and the probes end to end.

Lines that start with "knn-accuracy:" carry the measured worst ratio to each bound (profiles/knn_accuracy.txt)."""
import functools

import numpy as np
import pytest
import torch

from test_probes_cpu import _regression_case, blobs

pytestmark = pytest.mark.gpu

U = 2.0 ** -52
QUERY_TILE = 64           # queries of one workgroup (kKnnTile of csrc/knn.hip)

# (Nq, Nx, D, k): the smallest case, k == Nx, odd sizes below a tile, one past a tile on both sides with D no multiple of 4,
# k at its limit, D at its limit
SHAPES = [(1, 1, 1, 1), (3, 5, 1, 5), (17, 63, 5, 3), (65, 129, 33, 16), (64, 257, 128, 64), (9, 70, 1024, 5)]


def _lib():
    from multimodal_supernovae_amd import _lib as L
    return L


def _P():
    from multimodal_supernovae_amd import probes
    return probes


@functools.lru_cache(maxsize=None)
def _shapes():
    """The fixed shapes plus one slab + 1 and two slabs + 1 training rows at D = 16, k = 8 (the slab length is the kernel's own),
    both with one query more than a query tile."""
    L = _lib().lib()
    nq = QUERY_TILE + 1
    rows = L.msn_knn_slab_rows(nq, 257, 16, 8)
    extra = [(nq, rows + 1, 16, 8), (nq, 2 * rows + 1, 16, 8)]
    assert rows >= 1 and all(L.msn_knn_slab_rows(q, n, d, k) == rows for q, n, d, k in extra)
    # more than 512 per-slab keys for one query (ten slabs at k = 64): the finishing launch keeps 512 in registers and reads the rest
    # again in every round
    many = (3, 9 * rows + 1, 4, 64)
    assert L.msn_knn_slab_rows(*many) == rows and L.msn_knn_workspace_bytes(*many) == 10 * 3 * 64 * 12
    return tuple(SHAPES + extra + [many])


def _dev(a):
    return None if a is None else (a if isinstance(a, torch.Tensor) else torch.from_numpy(a)).cuda()


def _search(Q, X, k, self_offset=-1):
    """(idx, dist2) as numpy arrays from probes.knn_search(return_squared=True)."""
    idx, d2 = _P().knn_search(_dev(Q), _dev(X), k, exclude_self=False if self_offset < 0 else self_offset, return_squared=True)
    assert idx.dtype == torch.int32 and d2.dtype == torch.float64 and idx.shape == d2.shape == (len(Q), k)
    return idx.cpu(), d2.cpu()


# ------------------------------------------------------------------------------------------------------- integer data
@functools.lru_cache(maxsize=None)
def _int_train(Nx, D, k):
    """Integers in [-8, 8] as floats, a quarter of the rows copies of other rows: exact ties, and every d^2 an integer."""
    g = torch.Generator().manual_seed(1000 * Nx + 10 * D + k)
    X = torch.randint(-8, 9, (Nx, D), generator=g).float()
    ndup = Nx // 4
    if ndup:
        dst = torch.randperm(Nx, generator=g)[:ndup]
        src = torch.randint(0, Nx, (ndup,), generator=g)
        X[dst] = X[src]
    return X, g.get_state()


@functools.lru_cache(maxsize=None)
def _int_case(Nq, Nx, D, k, offset):
    """offset < 0: queries drawn from the training rows; offset >= 0: the batch X[offset : offset + n] searched without itself
    (k lowered to Nx - 1 where the shape has k == Nx).  None where the shape leaves no such case."""
    X, state = _int_train(Nx, D, k)
    if offset < 0:
        g = torch.Generator()
        g.set_state(state)
        Q = X[torch.randint(0, Nx, (Nq,), generator=g)]
    else:
        k = min(k, Nx - 1)
        n = min(Nq, Nx - offset)
        if k < 1 or n < 1:
            return None
        Q = X[offset:offset + n]
    ref_i, ref_d = _P().knn_reference(Q.numpy(), X.numpy(), k, self_offset=offset)
    return Q, X, k, torch.from_numpy(ref_i), torch.from_numpy(ref_d)


@pytest.mark.parametrize("offset", [-1, 0, 7])
def test_search_is_exact_on_integer_data_with_ties(offset):
    """d^2 is an integer below 2^53 in the expansion and in the direct form, so both are exact and equal: indices and
    distances must be the reference's, bit for bit, ties by the lower index."""
    ran = 0
    for Nq, Nx, D, k in _shapes():
        case = _int_case(Nq, Nx, D, k, offset)
        if case is None:                      # a leave-one-out search needs k <= Nx - 1 and a batch inside the training set
            assert Nx - 1 < 1 or Nx <= offset
            continue
        Q, X, kk, ref_i, ref_d = case
        idx, d2 = _search(Q, X, kk, offset)
        assert bool(((idx >= 0) & (idx < Nx)).all()), (Nq, Nx, D, kk)
        srt = idx.sort(dim=1).values
        assert bool((srt[:, 1:] != srt[:, :-1]).all()), (Nq, Nx, D, kk)           # no row twice for one query
        if offset >= 0:
            assert not bool((idx == (torch.arange(len(Q)) + offset)[:, None]).any())
        assert torch.equal(idx, ref_i), (Nq, Nx, D, kk, offset)
        assert torch.equal(d2, ref_d), (Nq, Nx, D, kk, offset)
        ran += 1
    assert ran >= len(_shapes()) - 2


# -------------------------------------------------------------------------------------------------------- normal data
@functools.lru_cache(maxsize=None)
def _normal_case(Nq, Nx, D, k):
    """Standard normal rows with the reference's neighbours and the precondition under which the expansion cannot pick others:
    B = (D + 4) 2^-52 (|q|^2 + |x|^2) bounds the expansion's error (D exact products added in the dot product and in each
    norm, the two final additions, a factor 2 for 1 / (1 - D u)); where consecutive distances among the first k + 1 differ by
    more than 2 max B, the k-th and the (k + 1)-th candidate cannot change places, nor any two among the k."""
    rng = np.random.default_rng(1000 * Nx + 10 * D + k)
    X = rng.standard_normal((Nx, D)).astype(np.float32)
    Q = rng.standard_normal((Nq, D)).astype(np.float32)
    Q64, X64 = Q.astype(np.float64), X.astype(np.float64)
    kk = min(k + 1, Nx)
    _, first = _P().knn_reference(Q, X, kk)
    ref_i, ref_d = _P().knn_reference(Q, X, k)
    qn, xn = (Q64 ** 2).sum(axis=1), (X64 ** 2).sum(axis=1)
    maxB = (D + 4) * U * (qn + xn.max())
    gaps = np.diff(first, axis=1)
    margin = float((gaps / (2 * maxB[:, None])).min()) if kk > 1 else np.inf
    return Q, X, ref_i, ref_d, margin


def test_search_on_normal_data_matches_the_reference_within_derived_bounds():
    """Neighbours: equal to the reference's (the precondition is asserted, never skipped on).  Distances: the direct form by fma
    in column order is within (D + 2) 2^-52 ref of the reference: one rounding of each difference (which doubles in the
    square), one per fma, and as much again for numpy's own sum."""
    worst = 0.0
    for Nq, Nx, D, k in _shapes():
        Q, X, ref_i, ref_d, margin = _normal_case(Nq, Nx, D, k)
        assert margin > 1.0, (Nq, Nx, D, k, margin)
        idx, d2 = _search(Q, X, k)
        idx2, d22 = _search(Q, X, k)
        assert torch.equal(idx, idx2) and torch.equal(d2, d22), (Nq, Nx, D, k)     # repeatable
        assert np.array_equal(idx.numpy(), ref_i), (Nq, Nx, D, k)
        got = d2.numpy()
        assert (got >= 0).all() and (np.diff(got, axis=1) >= 0).all()
        ratio = float((np.abs(got - ref_d) / ((D + 2) * U * ref_d)).max())
        print(f"knn-accuracy: search normal ({Nq}, {Nx}, {D}, {k}) smallest gap / (2 max B) = {margin:.3g}, "
              f"worst |dist2 - ref| / bound = {ratio:.4f}")
        worst = max(worst, ratio)
        assert ratio <= 1.0, (Nq, Nx, D, k, ratio)
    print(f"knn-accuracy: search normal worst over shapes = {worst:.4f}")


def _layouts(A):
    """The three layouts of the Gram test: a wider parent tensor, a start 4 bytes off a 16-byte boundary, both."""
    A = _dev(A)
    N, D = A.shape
    wide = torch.zeros(N, D + 5).cuda()
    wide[:, :D] = A
    flat = torch.zeros(N * D + 8).cuda()
    assert flat.data_ptr() % 16 == 0
    off = flat[1:1 + N * D].view(N, D)
    off.copy_(A)
    assert off.data_ptr() % 16 == 4
    flat2 = torch.zeros(N * (D + 5) + 8).cuda()
    both = flat2[1:1 + N * (D + 5)].view(N, D + 5)[:, :D]
    both.copy_(A)
    assert both.data_ptr() % 16 == 4 and (both.stride(0) == D + 5 or N == 1)
    return [wide[:, :D], off, both]


@pytest.mark.parametrize("Nq,Nx,D,k", [(17, 63, 5, 3), (65, 129, 33, 16), (64, 257, 128, 64)])
def test_search_bits_do_not_depend_on_stride_or_alignment(Nq, Nx, D, k):
    P = _P()
    for data in ("normal", "integer"):
        if data == "normal":
            Q, X = _normal_case(Nq, Nx, D, k)[:2]
        else:
            Q, X = _int_case(Nq, Nx, D, k, -1)[:2]
        base_i, base_d = P.knn_search(_dev(Q), _dev(X), k, return_squared=True)
        for Ql, Xl in zip(_layouts(Q), _layouts(X)):
            for q, x in ((Ql, _dev(X)), (_dev(Q), Xl), (Ql, Xl)):
                idx, d2 = P.knn_search(q, x, k, return_squared=True)
                assert torch.equal(idx, base_i) and torch.equal(d2, base_d), (data, q.stride(), x.stride())


def test_search_does_not_depend_on_the_launch_plan():
    """A fixed permutation of the training rows moves every row to another tile and slab, and a subset of the queries changes
    the query tiles: the distances keep their bits and the indices map through the permutation."""
    Nq, Nx, D, k = _shapes()[len(SHAPES) + 1]                 # two slabs + 1 training rows, a query tile + 1 queries
    Q, X = _normal_case(Nq, Nx, D, k)[:2]
    idx, d2 = _search(Q, X, k)
    perm = np.random.default_rng(7).permutation(Nx)
    sub = np.arange(5, 40, 2)
    idx_p, d2_p = _search(Q[sub], X[perm], k)
    assert torch.equal(d2_p, d2[sub])
    assert torch.equal(torch.from_numpy(perm)[idx_p.long()], idx[sub].long())
    # fewer training rows: one slab instead of three; a (query, row) pair found by both searches has the same distance bits
    keep = 200
    idx_s, d2_s = _search(Q, X[:keep], k)
    ref_i, _ = _P().knn_reference(Q, X[:keep], k)
    assert np.array_equal(idx_s.numpy(), ref_i)
    common = 0
    for q in range(Nq):
        full = dict(zip(idx[q].tolist(), d2[q].tolist()))
        for j, d in zip(idx_s[q].tolist(), d2_s[q].tolist()):
            if j in full:
                assert full[j] == d, (q, j)
                common += 1
    assert common >= Nq


def test_search_refusals_launch_nothing():
    P, L = _P(), _lib()
    X = torch.zeros(8, 4).cuda()
    for args, kw, what in [((X, X, 65), {}, "k must be in 1..64"), ((X, X, 9), {}, "k must be at most Nx"),
                           ((X, X, 8), {"exclude_self": True}, "k must be at most Nx - 1"),
                           ((torch.zeros(4, 1025).cuda(), torch.zeros(4, 1025).cuda(), 2), {}, "D must be in 1..1024")]:
        with pytest.raises(L.MsnHipError, match=what):
            P.knn_search(*args, **kw)
    with pytest.raises(ValueError, match="columns"):
        P.knn_search(X, torch.zeros(8, 5).cuda(), 2)
    with pytest.raises(L.MsnHipError, match="must live on the GPU"):
        P.knn_search(X.cpu(), X, 2)


# --------------------------------------------------------------------------------------------------------- prediction
def _predict_regression(idx, d2, Y, weights):
    from multimodal_supernovae_amd._lib import check, lib, ptr, stream_ptr
    Nq, k = idx.shape
    K = Y.shape[1]
    out = torch.empty(Nq, K, device="cuda")
    check(lib().msn_knn_predict_regression(ptr(idx), ptr(d2), Nq, k, ptr(Y), Y.stride(0), K, weights, ptr(out), K, stream_ptr()),
          "msn_knn_predict_regression")
    return out


def _predict_classes(idx, d2, y, C, weights):
    from multimodal_supernovae_amd._lib import check, lib, ptr, stream_ptr
    Nq, k = idx.shape
    classes = torch.empty(Nq, dtype=torch.int32, device="cuda")
    proba = torch.empty(Nq, C, device="cuda")
    check(lib().msn_knn_predict_classes(ptr(idx), ptr(d2), Nq, k, ptr(y), C, weights, ptr(classes), ptr(proba), stream_ptr()),
          "msn_knn_predict_classes")
    only = torch.empty(Nq, dtype=torch.int32, device="cuda")
    check(lib().msn_knn_predict_classes(ptr(idx), ptr(d2), Nq, k, ptr(y), C, weights, ptr(only), None, stream_ptr()),
          "msn_knn_predict_classes")
    assert torch.equal(only, classes)
    return classes.cpu().numpy(), proba.cpu().numpy()


PREDICT_SHAPES = [(3, 5, 1, 5), (17, 63, 5, 3), (65, 129, 33, 16), (64, 257, 128, 64)]


@pytest.mark.parametrize("weights", ["uniform", "distance"])
def test_regression_prediction_matches_the_reference_on_the_kernels_own_neighbours(weights):
    """fp64 sums of k terms and one division, then one rounding to fp32: within (k + 3) 2^-52 sum w |y| / sum w + 2^-24 |pred|
    of the reference evaluated on the same (idx, dist2)."""
    P = _P()
    worst = 0.0
    for Nq, Nx, D, k in PREDICT_SHAPES:
        Q, X = _normal_case(Nq, Nx, D, k)[:2]
        rng = np.random.default_rng(Nx + k)
        Y = rng.standard_normal((Nx, 3)).astype(np.float32)
        idx, d2 = P.knn_search(_dev(Q), _dev(X), k, return_squared=True)
        Yw = torch.zeros(Nx, 5).cuda()
        Yw[:, :3] = _dev(Y)
        got = _predict_regression(idx, d2, Yw[:, :3], 1 if weights == "distance" else 0).cpu().numpy().astype(np.float64)
        i_np, d_np = idx.cpu().numpy(), d2.cpu().numpy()
        ref = P.knn_predict_reference(i_np, d_np, Y, weights=weights)
        w = 1.0 / np.sqrt(d_np) if weights == "distance" else np.ones_like(d_np)
        scale = (w[:, :, None] * np.abs(Y.astype(np.float64))[i_np]).sum(axis=1) / w.sum(axis=1)[:, None]
        bound = (k + 3) * U * scale + 2.0 ** -24 * np.abs(ref)
        ratio = float((np.abs(got - ref) / bound).max())
        print(f"knn-accuracy: regression {weights} ({Nq}, {Nx}, {D}, {k}) worst |pred - ref| / bound = {ratio:.4f}")
        worst = max(worst, ratio)
        assert ratio <= 1.0, (Nq, Nx, D, k, ratio)
    print(f"knn-accuracy: regression {weights} worst over shapes = {worst:.4f}")


def test_class_prediction_matches_the_reference_on_the_kernels_own_neighbours():
    """Uniform weights: the votes are small integers, exact in fp64, so classes and vote fractions must be the reference's.
    Distance weights: the classes must agree wherever the reference's two largest votes differ by more than k 2^-52 of the total."""
    P = _P()
    for Nq, Nx, D, k in PREDICT_SHAPES:
        Q, X = _normal_case(Nq, Nx, D, k)[:2]
        rng = np.random.default_rng(Nx + k + 1)
        for C in (3, 1024):
            y = rng.integers(0, min(C, 6), Nx)
            if C == 1024:
                y[::3] = 1023
            idx, d2 = P.knn_search(_dev(Q), _dev(X), k, return_squared=True)
            i_np, d_np = idx.cpu().numpy(), d2.cpu().numpy()
            cls, proba = _predict_classes(idx, d2, _dev(y), C, 0)
            ref_c, votes = P.knn_predict_reference(i_np, d_np, y, task="classification", n_classes=C)
            assert np.array_equal(cls, ref_c), (Nq, Nx, D, k, C)
            assert np.array_equal(proba, (votes / votes.sum(axis=1, keepdims=True)).astype(np.float32))
            cls, proba = _predict_classes(idx, d2, _dev(y), C, 1)
            ref_c, votes = P.knn_predict_reference(i_np, d_np, y, weights="distance", task="classification", n_classes=C)
            top = np.sort(votes, axis=1)
            sure = top[:, -1] - (top[:, -2] if C > 1 else 0) > k * U * votes.sum(axis=1)
            assert sure.mean() >= 0.9 and np.array_equal(cls[sure], ref_c[sure]), (Nq, Nx, D, k, C)
            want = votes / votes.sum(axis=1, keepdims=True)
            assert (np.abs(proba - want) <= (k + 3) * U + 2.0 ** -24 * want).all()


def test_zero_distance_rule_returns_the_matching_row():
    """weights="distance" with a query equal to a training row: that row's target or class, exactly."""
    P = _P()
    Nq, Nx, D, k = 65, 129, 33, 16
    X = _normal_case(Nq, Nx, D, k)[1]
    rng = np.random.default_rng(3)
    Y = rng.standard_normal((Nx, 2)).astype(np.float32)
    y = rng.integers(0, 5, Nx)
    rows = np.arange(0, Nx, 2)
    Xd = _dev(X)
    reg = P.KNeighborsRegressorProbe(n_neighbors=k, weights="distance").fit(Xd, _dev(Y))
    assert torch.equal(reg.predict(Xd[rows]).cpu(), torch.from_numpy(Y[rows]))
    clf = P.KNeighborsClassifierProbe(n_neighbors=k, weights="distance", n_classes=5).fit(Xd, _dev(y))
    assert np.array_equal(clf.predict(Xd[rows]).cpu().numpy(), y[rows])
    proba = clf.predict_proba(Xd[rows]).cpu().numpy()
    assert np.array_equal(proba, np.eye(5, dtype=np.float32)[y[rows]])
    dist, idx = reg.kneighbors(Xd[rows])
    assert bool((dist[:, 0] == 0).all()) and np.array_equal(idx[:, 0].cpu().numpy(), rows)


def test_a_label_out_of_range_counts_for_no_class():
    P = _P()
    Nq, Nx, D, k = 17, 63, 5, 3
    Q, X = _normal_case(Nq, Nx, D, k)[:2]
    y = np.random.default_rng(9).integers(0, 4, Nx)
    y[::2] = 9                                      # past C = 4
    y[1::5] = -3
    idx, d2 = P.knn_search(_dev(Q), _dev(X), k, return_squared=True)
    cls, proba = _predict_classes(idx, d2, _dev(y), 4, 0)
    ref_c, votes = P.knn_predict_reference(idx.cpu().numpy(), d2.cpu().numpy(), y, task="classification", n_classes=4)
    total = votes.sum(axis=1, keepdims=True)
    assert (total == 0).any() and (total > 0).any()
    assert np.array_equal(cls, ref_c)               # no vote at all: class 0
    assert np.array_equal(proba, np.where(total > 0, votes / np.maximum(total, 1), 0).astype(np.float32))
    with pytest.raises(_lib().MsnHipError, match="labels must lie in"):
        P.KNeighborsClassifierProbe(n_classes=4).fit(_dev(X), _dev(y))


# --------------------------------------------------------------------------------------------------------- end to end
def test_knn_probe_metrics_equal_the_metrics_of_the_reference_predictions():
    from multimodal_supernovae_amd import utils
    from multimodal_supernovae_amd.models_finetune import ClassificationMetrics, RegressionMetrics
    P = _P()
    X, y, X2, y2 = blobs(500, 64, 5, 0.3, seed=500, fresh=True)
    Xd, yd, X2d, y2d = (_dev(a) for a in (X, y, X2, y2))
    for weights in ("uniform", "distance"):
        pred = utils.get_knn_predictions(Xd, yd, X2d, y2d, k=5, task="classification", weights=weights)
        ref_i, ref_d = P.knn_reference(X2, X, 5)
        ref_c, _ = P.knn_predict_reference(ref_i, ref_d, y, weights=weights, task="classification", n_classes=5)
        assert pred.dtype == torch.int32 and np.array_equal(pred.cpu().numpy(), ref_c)
        got = utils.knn_probe_metrics(Xd, yd, X2d, y2d, k=5, task="classification", weights=weights)
        m = ClassificationMetrics(5)
        m.update(_dev(ref_c), y2d)
        assert got == m.compute() and set(got) >= {"acc", "f1_macro", "f1_micro"}
    loo = utils.get_knn_predictions(Xd, yd, k=5, task="classification")
    ref_i, ref_d = P.knn_reference(X, X, 5, self_offset=0)
    assert np.array_equal(loo.cpu().numpy(), P.knn_predict_reference(ref_i, ref_d, y, task="classification", n_classes=5)[0])

    Xr, Yr = _regression_case(1000, 128, 1, seed=3)
    Xt, Yt, Xv, Yv = Xr[:700], Yr[:700, 0], Xr[700:], Yr[700:, 0]
    pred = utils.get_knn_predictions(_dev(Xt), _dev(Yt), _dev(Xv), k=5, task="regression")
    ref_i, ref_d = P.knn_reference(Xv, Xt, 5)
    ref = P.knn_predict_reference(ref_i, ref_d, Yt).astype(np.float32)          # uniform weights: the same sums in the same order
    assert pred.dtype == torch.float32 and pred.shape == (300,) and np.array_equal(pred.cpu().numpy(), ref)
    got = utils.knn_probe_metrics(_dev(Xt), _dev(Yt), _dev(Xv), _dev(Yv), k=5, task="regression")
    m = RegressionMetrics()
    m.update(_dev(ref), _dev(Yv))
    assert got == m.compute() and set(got) == {"L1", "L2", "R2", "OLF"}
    with pytest.raises(ValueError, match="task must be"):
        utils.get_knn_predictions(_dev(Xt), _dev(Yt), task="linear")


def test_cosine_metric():
    """Rows of +-1/4 at D = 16 have norm exactly 1 and normalise to themselves: cosine must find what euclidean finds, at
    1 - cos = d^2 / 2.  On normal data: the reference's neighbours on the normalised rows."""
    P = _P()
    g = torch.Generator().manual_seed(4)
    X = (torch.randint(0, 2, (300, 16), generator=g).float() - 0.5) / 2
    Q = (torch.randint(0, 2, (40, 16), generator=g).float() - 0.5) / 2
    Xd, Qd = X.cuda(), Q.cuda()
    idx_e, d2_e = P.knn_search(Qd, Xd, 5, return_squared=True)
    idx_c, d_c = P.knn_search(Qd, Xd, 5, metric="cosine")
    assert torch.equal(idx_c, idx_e) and torch.equal(d_c, d2_e * 0.5)
    _, d_e = P.knn_search(Qd, Xd, 5)
    assert torch.equal(d_e, d2_e.sqrt())
    from multimodal_supernovae_amd import ops
    Qn, Xn = _normal_case(64, 257, 128, 64)[:2]                        # (l2norm_fwd takes row lengths that are multiples of 4)
    qn, xn = ops.l2norm_fwd(_dev(Qn))[0], ops.l2norm_fwd(_dev(Xn))[0]
    ref_i, ref_d = P.knn_reference(qn.cpu().numpy(), xn.cpu().numpy(), 16)
    idx, d = P.knn_search(_dev(Qn), _dev(Xn), 16, metric="cosine")
    assert np.array_equal(idx.cpu().numpy(), ref_i)
    assert (np.abs(d.cpu().numpy() - ref_d / 2) <= (128 + 2) * U * ref_d / 2).all()
    with pytest.raises(_lib().MsnHipError, match="multiple of 4"):
        P.knn_search(torch.ones(4, 6).cuda(), torch.ones(4, 6).cuda(), 2, metric="cosine")
    probe = P.KNeighborsRegressorProbe(n_neighbors=16, metric="cosine").fit(_dev(Xn), _dev(Xn[:, 0].copy()))
    dist, ind = probe.kneighbors(_dev(Qn))
    assert torch.equal(ind, idx) and torch.equal(dist, d)


def test_kneighbors_without_queries_is_leave_one_out():
    P = _P()
    Nq, Nx, D, k = 65, 129, 33, 16
    X = _dev(_normal_case(Nq, Nx, D, k)[1])
    probe = P.KNeighborsRegressorProbe(n_neighbors=k).fit(X, X[:, 0])
    assert probe._X.data_ptr() == X.data_ptr()                         # a reference, not a copy
    dist, idx = probe.kneighbors()
    want_i, want_d2 = P.knn_search(X, X, k, exclude_self=0, return_squared=True)
    assert torch.equal(idx, want_i) and torch.equal(dist, want_d2.sqrt())
    assert not bool((idx == torch.arange(Nx, device="cuda")[:, None]).any())
    assert torch.equal(probe.kneighbors(n_neighbors=3, return_distance=False), want_i[:, :3])
    batch_i, batch_d2 = P.knn_search(X[7:40], X, k, exclude_self=7, return_squared=True)
    assert torch.equal(batch_i, want_i[7:40]) and torch.equal(batch_d2, want_d2[7:40])
    pred = probe.predict()
    ref = P.knn_predict_reference(want_i.cpu().numpy(), want_d2.cpu().numpy(), X[:, 0].cpu().numpy()).astype(np.float32)
    assert np.array_equal(pred.cpu().numpy(), ref)
