"""The host halves of the kNN probes (multimodal_supernovae_amd/probes.py: knn_reference, knn_predict_reference) against a plain
double loop and against scikit-learn, and the argument validation of the msn_knn_* entry points, which runs before any launch."""
import ctypes

import numpy as np
import pytest
import torch

from multimodal_supernovae_amd import probes as P


def _loop_knn(Q, X, k, self_offset=-1):
    """The definition, one pair at a time: sort the (distance, index) pairs."""
    out_i, out_d = [], []
    for i in range(len(Q)):
        keys = []
        for j in range(len(X)):
            if self_offset >= 0 and j == i + self_offset:
                continue
            d = 0.0
            for c in range(X.shape[1]):
                d += (float(Q[i, c]) - float(X[j, c])) ** 2
            keys.append((d, j))
        keys.sort()
        out_i.append([j for _, j in keys[:k]])
        out_d.append([d for d, _ in keys[:k]])
    return np.array(out_i, dtype=np.int32), np.array(out_d)


def _tiny():
    rng = np.random.default_rng(5)
    X = rng.integers(-3, 4, (12, 3)).astype(np.float32)
    X[7] = X[2]                                   # duplicated rows: equal distances to every query
    X[9] = X[2]
    X[4] = X[11]
    return X


def test_reference_equals_the_double_loop_with_duplicates():
    X = _tiny()
    Q = np.concatenate([X[[2, 4, 0]], np.zeros((1, 3), np.float32)])
    for k in (1, 5, 12):
        idx, d2 = P.knn_reference(Q, X, k)
        want_i, want_d = _loop_knn(Q, X, k)
        assert idx.dtype == np.int32 and d2.dtype == np.float64
        assert np.array_equal(idx, want_i) and np.array_equal(d2, want_d), k
    idx, d2 = P.knn_reference(X[[2]], X, 3)
    assert idx.tolist() == [[2, 7, 9]] and d2.tolist() == [[0.0, 0.0, 0.0]]          # stable: the lower index first


def test_reference_self_offset():
    X = _tiny()
    for off, n in ((0, 12), (7, 5)):
        Q = X[off:off + n]
        idx, d2 = P.knn_reference(Q, X, 4, self_offset=off)
        want_i, want_d = _loop_knn(Q, X, 4, self_offset=off)
        assert np.array_equal(idx, want_i) and np.array_equal(d2, want_d)
        assert not (idx == (np.arange(n) + off)[:, None]).any()
    idx, _ = P.knn_reference(X[[2]], X, 2, self_offset=2)
    assert idx.tolist() == [[7, 9]]                                                   # its duplicates stay candidates
    with pytest.raises(ValueError, match="outside"):
        P.knn_reference(X, X, 12, self_offset=0)
    with pytest.raises(ValueError, match="outside"):
        P.knn_reference(X, X, 13)


def test_predict_reference_weighting_rules():
    idx = np.array([[0, 1, 2], [2, 1, 0]])
    d2 = np.array([[1.0, 4.0, 16.0], [0.0, 0.0, 9.0]])
    Y = np.array([1.0, 2.0, 6.0])
    assert P.knn_predict_reference(idx, d2, Y).tolist() == [3.0, 3.0]
    got = P.knn_predict_reference(idx, d2, Y, weights="distance")
    assert got[0] == (1.0 + 2.0 / 2 + 6.0 / 4) / (1 + 0.5 + 0.25) and got[1] == 4.0  # zero distances: only they count
    y = np.array([2, 0, 2])
    cls, votes = P.knn_predict_reference(idx, d2, y, task="classification", n_classes=4)
    assert cls.dtype == np.int32 and cls.tolist() == [2, 2] and votes[0].tolist() == [1.0, 0.0, 2.0, 0.0]
    cls, votes = P.knn_predict_reference(idx[:, :2], d2[:, :2], y, task="classification", n_classes=4)
    assert cls.tolist() == [0, 0]                                                     # equal votes: the lowest class
    cls, votes = P.knn_predict_reference(idx, d2, np.array([7, -1, 1]), task="classification", n_classes=4)
    assert cls.tolist() == [1, 1] and votes.sum(axis=1).tolist() == [1.0, 1.0]        # out of range: no vote
    two = P.knn_predict_reference(idx, d2, np.stack([Y, -Y], axis=1))
    assert two.shape == (2, 2) and two[:, 1].tolist() == [-3.0, -3.0]
    with pytest.raises(ValueError, match="weights must be"):
        P.knn_predict_reference(idx, d2, Y, weights="rank")


@pytest.mark.parametrize("weights", ["uniform", "distance"])
def test_predict_reference_agrees_with_scikit_learn(weights):
    nb = pytest.importorskip("sklearn.neighbors")
    rng = np.random.default_rng(11)
    X = rng.standard_normal((200, 8)).astype(np.float32)
    Q = rng.standard_normal((40, 8)).astype(np.float32)
    Q[3] = X[17]                                                  # a query identical to a training row
    Y = rng.standard_normal((200, 2))
    y = rng.integers(0, 4, 200)
    k = 7
    idx, d2 = P.knn_reference(Q, X, k)
    # scikit-learn's own brute force takes the distances from the expansion; given the direct form's distances
    # (metric="precomputed") it sees what the reference sees, and only the order of the sums is left to differ
    X64, Q64 = X.astype(np.float64), Q.astype(np.float64)
    train = np.sqrt(((X64[:, None, :] - X64[None, :, :]) ** 2).sum(axis=2))
    query = np.sqrt(((Q64[:, None, :] - X64[None, :, :]) ** 2).sum(axis=2))
    assert query[3, 17] == 0.0
    reg = nb.KNeighborsRegressor(n_neighbors=k, weights=weights, metric="precomputed").fit(train, Y)
    dist, ind = reg.kneighbors(query)
    assert np.array_equal(ind, idx) and np.array_equal(dist, np.sqrt(d2))             # tie-free data: the neighbours agree
    got = P.knn_predict_reference(idx, d2, Y, weights=weights)
    scale = np.abs(Y[idx]).max(axis=1)
    assert (np.abs(got - reg.predict(query)) <= 8 * 2.0 ** -52 * scale).all()         # a few ulps of the largest target among the k
    clf = nb.KNeighborsClassifier(n_neighbors=k, weights=weights, metric="precomputed").fit(train, y)
    cls, votes = P.knn_predict_reference(idx, d2, y, weights=weights, task="classification", n_classes=4)
    assert np.array_equal(cls, clf.predict(query))
    assert np.abs(votes / votes.sum(axis=1, keepdims=True) - clf.predict_proba(query)).max() <= 1e-12
    if weights == "distance":
        assert np.array_equal(got[3], Y[17]) and cls[3] == y[17]                      # the zero-distance rule


def _knn_lib():
    from multimodal_supernovae_amd import _lib
    return _lib.lib()


def test_knn_shape_errors_are_reported_without_a_gpu():
    """Validation happens before any launch: the pointers are never dereferenced."""
    lib = _knn_lib()
    fake = ctypes.c_void_p(4096)

    def search(Nq, Nx, D, k, self_offset=-1, ws_bytes=None):
        if ws_bytes is None:
            ws_bytes = max(lib.msn_knn_workspace_bytes(Nq, Nx, D, k), 8)
        return lib.msn_knn_search(fake, D, Nq, fake, D, Nx, D, k, self_offset, fake, fake, fake, ws_bytes, None)

    assert search(8, 100, 16, 65) == 1 and b"k must be in 1..64" in lib.msn_last_error()
    assert search(8, 4, 16, 5) == 1 and b"k must be at most Nx (" in lib.msn_last_error()
    assert search(4, 5, 16, 5, self_offset=0) == 1 and b"k must be at most Nx - 1" in lib.msn_last_error()
    assert search(8, 100, 1025, 5) == 1 and b"D must be in 1..1024" in lib.msn_last_error()
    need = lib.msn_knn_workspace_bytes(8, 100, 16, 5)
    assert need == 8 * 5 * 12                                      # one slab: k keys of 12 bytes per query
    assert search(8, 100, 16, 5, ws_bytes=need - 1) == 1 and b"workspace of 480 bytes needed, 479 given" in lib.msn_last_error()
    assert search(0, 100, 16, 5) == 1 and b"Nq must be at least 1" in lib.msn_last_error()
    assert search(8, 1 << 31, 16, 5) == 1 and b"Nx must be in" in lib.msn_last_error()
    assert search(8, 100, 16, 0) == 1 and b"k must be in 1..64" in lib.msn_last_error()
    assert lib.msn_knn_workspace_bytes(8, 100, 16, 65) == 0 and lib.msn_knn_slab_rows(8, 100, 1025, 5) == 0
    # the plan: slabs of at least 256 rows, the same length one row and two slabs further on
    rows = lib.msn_knn_slab_rows(65, 257, 16, 8)
    assert rows == 256 and lib.msn_knn_slab_rows(65, 2 * rows + 1, 16, 8) == rows
    assert lib.msn_knn_workspace_bytes(65, 2 * rows + 1, 16, 8) == 3 * 65 * 8 * 12
    rc = lib.msn_knn_predict_regression(fake, fake, 8, 5, fake, 17, 17, 0, fake, 17, None)
    assert rc == 1 and b"K must be in 1..16" in lib.msn_last_error()
    rc = lib.msn_knn_predict_regression(fake, fake, 8, 5, fake, 1, 1, 2, fake, 1, None)
    assert rc == 1 and b"weights must be 0 (uniform) or 1 (distance)" in lib.msn_last_error()
    rc = lib.msn_knn_predict_classes(fake, fake, 8, 5, fake, 1025, 0, fake, None, None)
    assert rc == 1 and b"C must be in 1..1024" in lib.msn_last_error()


def test_cpu_tensors_are_refused():
    from multimodal_supernovae_amd import _lib, utils
    X, Y = torch.zeros(8, 4), torch.zeros(8)
    with pytest.raises(_lib.MsnHipError):
        P.knn_search(X, X, 3)
    with pytest.raises(_lib.MsnHipError):
        P.KNeighborsRegressorProbe().fit(X, Y)
    with pytest.raises(_lib.MsnHipError):
        P.KNeighborsClassifierProbe().fit(X, Y.long())
    with pytest.raises(_lib.MsnHipError):
        utils.get_knn_predictions(X, Y, X, k=3)
    with pytest.raises(ValueError, match="metric must be"):
        P.knn_search(X, X, 3, metric="manhattan")
    with pytest.raises(ValueError, match="n_neighbors must be in 1..64"):
        P.KNeighborsRegressorProbe(n_neighbors=65)
    with pytest.raises(ValueError, match="weights must be"):
        P.KNeighborsClassifierProbe(weights="rank")
