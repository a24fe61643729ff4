"""The host halves of embedding_metrics.py and the refusals of csrc/embedding_metrics.hip, without a GPU: retrieval figures
against double loops, the spectrum from a Gram matrix against numpy's SVD of the rows, the modality gap against the direct means,
and the two numpy restatements against plain double loops."""
import ctypes
import math

import numpy as np
import pytest
import torch


def _E():
    from multimodal_supernovae_amd import embedding_metrics
    return embedding_metrics


def _gram(X):
    """probe_gram's matrix without targets, restated in numpy fp64: Z^T Z of Z = [X | 1]."""
    Z = np.concatenate([np.asarray(X, dtype=np.float64), np.ones((len(X), 1))], axis=1)
    return Z.T @ Z


def _unit_rows_plus_offset(n, d, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d))
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    return (X + 0.5 * rng.standard_normal(d) / math.sqrt(d)).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_are_reported_without_a_gpu():
    from multimodal_supernovae_amd import _lib
    lib = _lib.lib()
    fake = ctypes.c_void_p(4096)          # never dereferenced: validation rejects the call before any launch
    big = ctypes.c_size_t(1 << 20)

    def pot(nx, ny, d, t, mode, x=fake, y=fake, ws_bytes=big):
        return lib.msn_pair_potential(x, d, nx, y, d, ny, d, t, mode, fake, fake, ws_bytes, None)

    for args, what in [((8, 8, 0, 2.0, 0), b"D must be in 1..1024"), ((8, 8, 1025, 2.0, 0), b"D must be in 1..1024"),
                       ((0, 8, 4, 2.0, 0), b"Nx must be in"), ((8, 0, 4, 2.0, 0), b"Ny must be in"),
                       ((8, 0, 4, 2.0, 1), b"Ny must be in"), ((8, 9, 4, 2.0, 1), b"Nx == Ny"),
                       ((1 << 31, 8, 4, 2.0, 0), b"Nx must be in"), ((8, 1 << 31, 4, 2.0, 0), b"Ny must be in"),
                       ((8, 8, 4, 0.0, 0), b"finite and positive"), ((8, 8, 4, -1.0, 0), b"finite and positive"),
                       ((8, 8, 4, float("inf"), 0), b"finite and positive"), ((8, 8, 4, float("nan"), 0), b"finite and positive"),
                       ((8, 8, 4, 2.0, 3), b"mode must be"), ((8, 8, 4, 2.0, -1), b"mode must be")]:
        assert pot(*args) == 1 and what in lib.msn_last_error(), (args, lib.msn_last_error())
    assert pot(1, 0, 4, 2.0, 2, y=None) == 1 and b"Nx >= 2" in lib.msn_last_error()
    assert pot(8, 0, 4, 2.0, 2) == 1 and b"Y must be NULL" in lib.msn_last_error()               # Y given
    assert pot(8, 8, 4, 2.0, 2, y=None) == 1 and b"Y must be NULL" in lib.msn_last_error()       # Ny given
    assert pot(8, 8, 4, 2.0, 0, ws_bytes=ctypes.c_size_t(8)) == 1 and b"workspace" in lib.msn_last_error()
    assert pot(8, 0, 4, 2.0, 2, y=None, ws_bytes=ctypes.c_size_t(8)) == 1 and b"workspace" in lib.msn_last_error()
    # the plan is a function of the shape: one partial pair of doubles per workgroup, at most 1024 workgroups
    wb = lib.msn_pair_potential_workspace_bytes
    assert wb(8, 8, 4, 0) == 16 and wb(65, 130, 4, 0) == 6 * 16 and wb(1100, 0, 4, 2) == 171 * 16
    assert wb(65536, 0, 128, 2) == 1024 * 16          # 524800 tile pairs, 513 per workgroup (the last one owns a single pair)
    assert wb(8, 8, 4, 2) == 0 and wb(8, 9, 4, 1) == 0 and wb(8, 8, 1025, 0) == 0 and wb(1, 0, 4, 2) == 0

    def ali(n, d, ws_bytes=big):
        return lib.msn_pair_alignment(fake, d, fake, d, n, d, fake, None, fake, ws_bytes, None)

    for args, what in [((8, 0), b"D must be in 1..1024"), ((8, 1025), b"D must be in 1..1024"), ((0, 4), b"N must be in"),
                       ((1 << 31, 4), b"N must be in")]:
        assert ali(*args) == 1 and what in lib.msn_last_error(), (args, lib.msn_last_error())
    assert ali(8, 4, ctypes.c_size_t(8)) == 1 and b"workspace" in lib.msn_last_error()
    assert lib.msn_pair_alignment_workspace_bytes(3100, 33) == 13 * 16
    assert lib.msn_pair_alignment_workspace_bytes(0, 4) == 0 and lib.msn_pair_alignment_workspace_bytes(4, 1025) == 0


def test_cpu_tensors_are_refused():
    from multimodal_supernovae_amd import _lib
    E = _E()
    X = torch.randn(8, 4)
    for call in (lambda: E.pair_potential(X), lambda: E.pair_potential(X, X, pairs="all"), lambda: E.pair_alignment(X, X),
                 lambda: E.uniformity(X), lambda: E.cross_uniformity(X, X), lambda: E.alignment(X, X),
                 lambda: E.EmbeddingMetrics().update(X, X)):
        with pytest.raises(_lib.MsnHipError):
            call()


# ----------------------------------------------------------------------------------------------------------- retrieval
def test_retrieval_figures_match_double_loops():
    E = _E()
    n = 12
    for ranks in ([0] * n, [n - 1] * n, [0, n - 1, 3, 3, 3, 0, 5, 11, 11, 2, 7, 3], [4], [0, 1]):
        r = np.asarray(ranks, dtype=np.int32)
        for k in (1, 3, 5, 10, 50):
            hits = 0
            for v in ranks:
                hits += 1 if v < k else 0
            assert E.recall_at_k(r, k) == hits / len(ranks)
            assert E.recall_at_k(torch.from_numpy(r), k) == hits / len(ranks)
        acc = 0.0
        for v in ranks:
            acc += 1.0 / (v + 1)
        assert abs(E.mean_reciprocal_rank(r) - acc / len(ranks)) <= 1e-15
        one_based = sorted(v + 1 for v in ranks)
        m = len(one_based)
        med = one_based[m // 2] if m % 2 else 0.5 * (one_based[m // 2 - 1] + one_based[m // 2])
        assert E.median_rank(r) == med
    assert E.recall_at_k([0] * n, 1) == 1.0 and E.mean_reciprocal_rank([0] * n) == 1.0 and E.median_rank([0] * n) == 1.0
    assert E.recall_at_k([n - 1] * n, n - 1) == 0.0 and E.recall_at_k([n - 1] * n, n) == 1.0
    with pytest.raises(ValueError):
        E.recall_at_k([0, 1], 0)
    with pytest.raises(ValueError):
        E.median_rank(np.array([0.5, 1.0]))


# ------------------------------------------------------------------------------------------------------------ spectrum
def _svd_spectrum(X, center):
    X = np.asarray(X, dtype=np.float64)
    return np.linalg.svd(X - X.mean(axis=0) if center else X, compute_uv=False)


@pytest.mark.parametrize("center", [True, False])
@pytest.mark.parametrize("n,d", [(500, 16), (300, 128)])
def test_spectrum_and_effective_rank_match_the_svd_of_the_rows(n, d, center):
    E = _E()
    X = _unit_rows_plus_offset(n, d, 3 * n + d)
    s = E.covariance_spectrum(_gram(X), d, center=center)
    ref = _svd_spectrum(X, center)
    assert s.shape == (d,) and np.all(np.diff(s) <= 0)
    assert np.max(np.abs(s - ref)) <= 1e-10
    assert abs(E.effective_rank(s) - E.effective_rank(ref)) <= 1e-10
    p = ref / ref.sum() + 1e-7
    assert abs(E.effective_rank(ref) - math.exp(-float(np.sum(p * np.log(p))))) <= 1e-12
    assert abs(E.participation_ratio(s) - float(np.sum(ref ** 2) ** 2 / np.sum(ref ** 4))) <= 1e-10 * d


@pytest.mark.parametrize("center", [True, False])
def test_effective_rank_of_rank_3_data(center):
    """Thirteen singular values are 0 in exact arithmetic; from a Gram matrix they come out as sqrt of eigenvalues of size
    2^-52 lambda_max, about 1e-8 of the largest, which moves exp(entropy) by about 1e-6."""
    E = _E()
    rng = np.random.default_rng(11)
    X = (rng.standard_normal((400, 3)) @ rng.standard_normal((3, 16))).astype(np.float32).astype(np.float64)
    if center:
        X = X - X.mean(axis=0)            # (keeps the rank at 3; an offset outside the span would add a direction)
    X = X.astype(np.float32)
    # the fp32 rounding of the entries adds directions of relative size 2^-24: the reference is the SVD of the same fp32 rows
    ref = E.effective_rank(_svd_spectrum(X, center))
    got = E.effective_rank(E.covariance_spectrum(_gram(X), 16, center=center))
    assert abs(got - ref) <= 1e-4
    assert got <= 3 + 1e-4


def test_modality_gap_matches_the_direct_means():
    E = _E()
    X, Y = _unit_rows_plus_offset(300, 33, 5), _unit_rows_plus_offset(200, 33, 6)
    ref = float(np.linalg.norm(X.astype(np.float64).mean(axis=0) - Y.astype(np.float64).mean(axis=0)))
    assert abs(E.modality_gap(_gram(X), _gram(Y), 33) - ref) <= 1e-14
    assert E.modality_gap(_gram(X), _gram(X), 33) == 0.0
    with pytest.raises(ValueError):
        E.modality_gap(_gram(X), _gram(Y), 40)


# -------------------------------------------------------------------------------------------------------- restatements
def test_references_match_plain_double_loops():
    E = _E()
    rng = np.random.default_rng(2)
    X = rng.standard_normal((7, 3)).astype(np.float32)
    Y = rng.standard_normal((7, 3)).astype(np.float32)
    t = 1.5

    def d2(a, b):
        s = 0.0
        for c in range(3):
            s += (float(a[c]) - float(b[c])) ** 2
        return s

    for pairs, other in (("within", None), ("all", Y), ("offdiag", Y)):
        se = sd = 0.0
        for i in range(7):
            for j in range(7):
                keep = j > i if pairs == "within" else (i != j if pairs == "offdiag" else True)
                if keep:
                    v = d2(X[i], (X if other is None else other)[j])
                    se += math.exp(-t * v)
                    sd += v
        got = E.pair_potential_reference(X, other, t, pairs)
        assert abs(float(got[0]) - se) <= 1e-13 * se and abs(float(got[1]) - sd) <= 1e-13 * sd
    s2 = s1 = 0.0
    rows = []
    for i in range(7):
        v = d2(X[i], Y[i])
        rows.append(v)
        s2 += v
        s1 += math.sqrt(v)
    got = E.pair_alignment_reference(X, Y)
    assert abs(float(got[0]) - s2) <= 1e-13 * s2 and abs(float(got[1]) - s1) <= 1e-13 * s1
    assert np.max(np.abs(got[2].astype(np.float64) - np.asarray(rows))) <= 1e-14
    assert float(E.pair_alignment_reference(X, X)[0]) == 0.0
    with pytest.raises(ValueError):
        E.pair_potential_reference(X, Y, t, "within")
