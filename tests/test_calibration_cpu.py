"""Calibration metrics without a GPU (calibration.py): the numpy restatements against plain double loops, the host functions of
the integer counts against the floating formulas, scikit-learn and scipy as yardsticks, and the refusals of the C-ABI."""
import ctypes
import functools
import math

import numpy as np
import pytest


def _K():
    from multimodal_supernovae_amd import calibration
    return calibration


# ----------------------------------------------------------------------------------------------------- shared cases
@functools.lru_cache(maxsize=None)
def fit_case():
    """The temperature-scaling case of the CPU and the GPU tests: z ~ 2 normal (4096, 5), labels drawn from softmax(z), logits
    2.5 z in fp32 -- an over-confident head whose best temperature is about 2.5.  Read-only arrays."""
    rng = np.random.default_rng(20240)
    z = 2.0 * rng.standard_normal((4096, 5))
    p = np.exp(z - z.max(axis=1, keepdims=True))
    p /= p.sum(axis=1, keepdims=True)
    y = (rng.random(4096)[:, None] > np.cumsum(p, axis=1)).sum(axis=1).clip(0, 4).astype(np.int64)
    logits = (2.5 * z).astype(np.float32)
    logits.setflags(write=False)
    y.setflags(write=False)
    return logits, y


@functools.lru_cache(maxsize=None)
def fit_reference():
    return _K().fit_temperature_reference(*fit_case())


def reference_ece(logits, y, beta):
    """Top-label ECE (15 bins) of softmax(beta logits), by the restatements alone."""
    K = _K()
    P = K.softmax_rows_reference(logits, beta=beta).astype(np.float32)
    return K.ece_from_counts(K.calibration_counts_reference(P, y)[0])


# ------------------------------------------------------------------------------------------------------ double loops
def _loop_counts(P, y, B, classwise):
    N, C = P.shape
    acc = np.zeros((1 + C if classwise else 1, B, 3), dtype=np.int64)
    tot = [0, 0, 0]
    for i in range(N):
        yi = int(y[i])
        if not 0 <= yi < C:
            continue
        row = [float(P[i, c]) for c in range(C)]
        ok, s = True, 0.0
        for p in row:
            ok = ok and (0.0 <= p <= 1.0)
            s = s + p
        if not (ok and abs(s - 1.0) <= 2.0 ** -10):
            tot[1] += 1
            continue
        tot[0] += 1
        q = [round(p * 2.0 ** 32) for p in row]                  # exact product; round() is ties-to-even
        a = 0
        for c in range(C):
            if row[c] > row[a]:
                a = c
        pairs = [(0, a)] + ([(1 + c, c) for c in range(C)] if classwise else [])
        for slot, c in pairs:
            b = min(B - 1, (q[c] * B) >> 32)
            acc[slot, b] += (1, int(c == yi), q[c])
        br = 0.0
        for c in range(C):
            d = row[c] - (1.0 if c == yi else 0.0)
            br = br + d * d
        tot[2] += round(br * 2.0 ** 30)
    return acc, np.array(tot, dtype=np.int64)


def _edge_case():
    """B = 8: probabilities exactly on the edges k / 8, p = 1, -0.0, a NaN, 1.5, a row summing to 0.5, targets -100 and >= C."""
    P = np.array([[0.125, 0.375, 0.5, 0.0],
                  [0.25, 0.25, 0.25, 0.25],                      # four maxima: the first one is the top label
                  [1.0, -0.0, 0.0, -0.0],
                  [0.0, 0.0, 0.0, 1.0],
                  [0.875, 0.125, 0.0, 0.0],
                  [np.nan, 0.5, 0.25, 0.25],                     # bad
                  [1.5, -0.5, 0.0, 0.0],                         # bad
                  [0.125, 0.125, 0.125, 0.125],                  # sums to 0.5: bad
                  [0.625, 0.125, 0.125, 0.125],
                  [0.5, 0.5, 0.0, 0.0],
                  [np.nan, np.nan, np.nan, np.nan],              # ignored: the target is -100
                  [0.7, 0.1, 0.1, 0.1],
                  [0.5, 0.25, 0.125, 0.125 + 2.0 ** -11],        # the sum lies 2^-11 above 1: valid
                  [0.5, 0.25, 0.125, 0.125 + 2.0 ** -9]], dtype=np.float32)   # 2^-9 above: bad
    y = np.array([2, 3, 0, 0, 1, 1, 0, 2, 0, 1, -100, 4, 3, 3], dtype=np.int64)
    return P, y


@pytest.mark.parametrize("classwise", [False, True])
def test_counts_restatement_equals_a_double_loop_on_the_edges(classwise):
    K = _K()
    P, y = _edge_case()
    acc, tot = K.calibration_counts_reference(P, y, n_bins=8, classwise=classwise)
    wa, wt = _loop_counts(P, y, 8, classwise)
    assert np.array_equal(acc, wa) and np.array_equal(tot, wt)
    assert tot.tolist()[:2] == [8, 4] and acc.dtype == np.int64 and acc.shape == ((5 if classwise else 1), 8, 3)
    # 0.125 on the edge 1 / 8 belongs to bin 1, p = 1 to the last bin, four equal maxima to the first column
    assert acc[0, 7, 0] == 3 and acc[0, 7, 2] == 2 * 2 ** 32 + 7 * 2 ** 29 and acc[0, 2, 0] == 1 and acc[0, 2, 1] == 0
    conf, hits, count = K.reliability_curve(acc)
    assert count.tolist() == acc[0, :, 0].tolist() and conf[2] == 0.25 and hits[2] == 0.0 and math.isnan(conf[0])


@pytest.mark.parametrize("N,C,B,classwise", [(40, 1, 3, True), (200, 3, 1, False), (150, 7, 10, True), (90, 20, 1024, True)])
def test_counts_restatement_equals_a_double_loop_on_softmax_rows(N, C, B, classwise):
    K = _K()
    rng = np.random.default_rng(N + C)
    P = K.softmax_rows_reference(3 * rng.standard_normal((N, C)).astype(np.float32)).astype(np.float32)
    y = rng.integers(0, C, N)
    P[::11, 0] = 0.5 if C > 1 else 0.25                          # rows that do not sum to 1
    y[5::13], y[7::17] = -100, C
    acc, tot = K.calibration_counts_reference(P, y, n_bins=B, classwise=classwise)
    wa, wt = _loop_counts(P, y, B, classwise)
    assert np.array_equal(acc, wa) and np.array_equal(tot, wt) and tot[1] > 0 and tot[0] > 0
    if C == 1:
        assert acc[0, B - 1, 0] == tot[0] == acc[0, B - 1, 1] and tot[2] == 0        # p = 1 in the last bin, always a hit


def test_counts_of_two_halves_add_up_to_the_counts_of_the_whole():
    K = _K()
    rng = np.random.default_rng(3)
    P = K.softmax_rows_reference(3 * rng.standard_normal((501, 6)).astype(np.float32)).astype(np.float32)
    y = rng.integers(0, 7, 501)
    P[::17, 2] = np.nan
    whole = K.calibration_counts_reference(P, y, classwise=True)
    a, b = K.calibration_counts_reference(P[:200], y[:200], classwise=True), K.calibration_counts_reference(P[200:], y[200:], classwise=True)
    assert np.array_equal(a[0] + b[0], whole[0]) and np.array_equal(a[1] + b[1], whole[1])


# ------------------------------------------------------------------------------------------------ ECE from integers
@pytest.mark.parametrize("N,C,B", [(5000, 5, 15), (3100, 1024, 10), (70000, 16, 100)])
def test_ece_from_integers_meets_the_floating_formula(N, C, B):
    """floor(conf B) bins and fp64 sums on rows none of which lies within 2^-30 of a bin edge (asserted for every row): the
    fixed-point quantisation moves ECE by at most 2^-33, the fp64 sums by less; the two agree within 2^-32."""
    K = _K()
    rng = np.random.default_rng(7 * N + C)
    P = K.softmax_rows_reference(3 * rng.standard_normal((N, C)).astype(np.float32)).astype(np.float32)
    y = rng.integers(0, C, N)
    acc, tot = K.calibration_counts_reference(P, y, n_bins=B)
    assert tot.tolist()[:2] == [N, 0]                            # no row is left out
    a = P.argmax(axis=1)
    conf = P[np.arange(N), a].astype(np.float64)
    edges = np.arange(B + 1) / B
    assert np.abs(conf[:, None] - edges[None, :]).min() > 2.0 ** -30          # the precondition, every row
    b = np.minimum(B - 1, np.floor(conf * B).astype(np.int64))
    hit = (a == y).astype(np.float64)
    gap = np.abs(np.bincount(b, conf, B) - np.bincount(b, hit, B))
    n_b = np.bincount(b, minlength=B)
    ece, mce = gap.sum() / N, (gap[n_b > 0] / n_b[n_b > 0]).max()
    d_ece, d_mce = abs(K.ece_from_counts(acc) - ece), abs(K.ece_from_counts(acc, "max") - mce)
    print(f"calibration: ({N}, {C}, B {B}): ece {ece:.6f}, |integer - floating| = {d_ece:.3e} (mce {d_mce:.3e})")
    assert d_ece <= 2.0 ** -32 and d_mce <= 2.0 ** -32
    assert np.array_equal(acc[0, :, 0], n_b)


def test_classwise_ece_and_empty_accumulators():
    K = _K()
    rng = np.random.default_rng(11)
    P = K.softmax_rows_reference(2 * rng.standard_normal((900, 4)).astype(np.float32)).astype(np.float32)
    y = rng.integers(0, 4, 900)
    acc, tot = K.calibration_counts_reference(P, y, n_bins=10, classwise=True)
    per = K.classwise_ece_from_counts(acc, None)
    for c in range(4):
        conf = P[:, c].astype(np.float64)
        b = np.minimum(9, np.floor(conf * 10).astype(np.int64))
        want = np.abs(np.bincount(b, conf, 10) - np.bincount(b, (y == c).astype(np.float64), 10)).sum() / 900
        assert per[c] == pytest.approx(want, abs=2.0 ** -32)
    assert K.classwise_ece_from_counts(acc) == pytest.approx(per.mean(), rel=1e-15)
    with pytest.raises(ValueError, match="classwise"):
        K.classwise_ece_from_counts(acc[:1])
    with pytest.raises(ValueError, match="norm"):
        K.ece_from_counts(acc, "l2")
    zero = np.zeros((1, 10, 3), dtype=np.int64)
    assert math.isnan(K.ece_from_counts(zero)) and math.isnan(K.ece_from_counts(zero, "max"))
    assert math.isnan(K.brier_from_counts(np.zeros(3, dtype=np.int64)))
    assert np.isnan(K.reliability_curve(zero)[0]).all()


# ---------------------------------------------------------------------------------------------------- Brier and NLL
def test_brier_at_two_classes_is_twice_scikit_learns():
    from sklearn.metrics import brier_score_loss
    K = _K()
    rng = np.random.default_rng(5)
    p1 = rng.integers(0, 2 ** 20 + 1, 3000) / 2.0 ** 20          # on a grid: p0 = 1 - p1 is exact in fp32
    P = np.stack([1.0 - p1, p1], axis=1).astype(np.float32)
    assert np.array_equal(P.astype(np.float64).sum(axis=1), np.ones(3000))
    y = (rng.random(3000) < p1).astype(np.int64)
    _, tot = K.calibration_counts_reference(P, y)
    got, want = K.brier_from_counts(tot), 2.0 * brier_score_loss(y, P[:, 1].astype(np.float64))
    assert tot[0] == 3000 and abs(got - want) <= 2.0 ** -31 + 4 * 2.0 ** -53


@pytest.mark.parametrize("T", [1.0, 0.5, 2.5])
def test_reference_nll_is_scikit_learns_log_loss(T):
    from sklearn.metrics import log_loss
    K = _K()
    logits, y = fit_case()
    out = K.temperature_nll_reference(logits, y, T)
    assert out[0] == 4096 and out[4] == 0 and out[3] > 0
    P = K.softmax_rows_reference(logits, T)
    assert out[1] / 4096 == pytest.approx(log_loss(y, P, labels=list(range(5))), rel=1e-12)
    # the derivatives are the derivatives: central differences of the value in beta
    b, eps = 1.0 / T, 1e-5
    up, dn = K.temperature_nll_reference(logits, y, beta=b + eps), K.temperature_nll_reference(logits, y, beta=b - eps)
    assert out[2] == pytest.approx((up[1] - dn[1]) / (2 * eps), rel=1e-6, abs=1e-4)
    assert out[3] == pytest.approx((up[2] - dn[2]) / (2 * eps), rel=1e-6)


def test_reference_nll_counts_bad_and_ignored_rows():
    K = _K()
    S = np.array([[1.0, 2.0, 0.5], [np.nan, 0.0, 0.0], [np.inf, 0.0, 0.0], [0.0, -np.inf, 1.0], [3.0, 1.0, 2.0], [np.nan, 1, 1]],
                 dtype=np.float32)
    y = np.array([1, 0, 2, 2, 5, -100])
    out = K.temperature_nll_reference(S, y, 2.0)
    assert out[0] == 1 and out[4] == 3
    t = S[0].astype(np.float64) / 2.0
    assert out[1] == pytest.approx(math.log(np.exp(t).sum()) - t[1], rel=1e-15)
    wide = K.temperature_nll_reference(S, y, 2.0, dtype=np.longdouble)
    assert wide.dtype == np.longdouble and float(wide[1]) == pytest.approx(float(out[1]), rel=1e-15)


# ---------------------------------------------------------------------------------------------------- reference fit
def test_reference_fit_meets_scipy_and_lowers_the_ece():
    from scipy.optimize import minimize_scalar
    K = _K()
    logits, y = fit_case()
    r = fit_reference()
    print(f"calibration: reference fit: T = {r['temperature']:.6f} in {r['n_iter']} evaluations, mean nll {r['nll_before']:.6f} -> "
          f"{r['nll_after']:.6f}")
    assert r["converged"] and r["n_iter"] <= 12 and r["n"] == 4096 and r["n_bad"] == 0
    assert abs(K.temperature_nll_reference(logits, y, beta=r["beta"])[2]) / 4096 <= 1e-8
    assert r["nll_after"] < r["nll_before"] and 2.0 < r["temperature"] < 3.0
    ms = minimize_scalar(lambda b: float(K.temperature_nll_reference(logits, y, beta=b)[1]), bounds=(1e-2, 1e2), method="bounded",
                         options={"xatol": 1e-10})
    assert ms.success and abs(ms.x - r["beta"]) <= 1e-6 * r["beta"]
    before, after = reference_ece(logits, y, 1.0), reference_ece(logits, y, r["beta"])
    print(f"calibration: reference ECE {before:.6f} -> {after:.6f}")
    assert after < before


def test_fit_safeguards():
    K = _K()
    logits, y = fit_case()
    with pytest.raises(ValueError, match="no valid row"):
        K.fit_temperature_reference(logits[:8], np.full(8, -100))
    # labels that are always the arg-max: the likelihood grows with beta without end, the bracket runs into the bound
    with pytest.warns(RuntimeWarning, match="did not reach"):
        r = K.fit_temperature_reference(logits[:64], logits[:64].argmax(axis=1), max_iter=30)
    assert not r["converged"] and r["temperature"] < 0.02 and r["nll_after"] <= r["nll_before"]
    # a start far from the minimum: an under-confident head (T about 0.1) is reached through the safeguard
    r = K.fit_temperature_reference((logits / 25).astype(np.float32), y)
    assert r["converged"] and r["temperature"] == pytest.approx(fit_reference()["temperature"] / 25, rel=1e-5)


# -------------------------------------------------------------------------------------------------------- refusals
def test_cpu_tensors_are_refused():
    import torch
    from multimodal_supernovae_amd import _lib
    K = _K()
    with pytest.raises(_lib.MsnHipError, match="GPU"):
        K.softmax_rows(torch.zeros(4, 3))
    with pytest.raises(_lib.MsnHipError, match="GPU"):
        K.calibration_counts(torch.zeros(4, 3), torch.zeros(4, dtype=torch.int64))
    with pytest.raises(_lib.MsnHipError, match="GPU"):
        K.temperature_nll(torch.zeros(4, 3), torch.zeros(4, dtype=torch.int64), 1.0)
    with pytest.raises(ValueError, match="temperature"):
        K.softmax_rows(torch.zeros(4, 3), temperature=0.0)
    with pytest.raises(ValueError):
        K.CalibrationMetrics(5, n_bins=0)
    with pytest.raises(ValueError):
        K.CalibrationMetrics(5, normalize="sigmoid")
    with pytest.raises(ValueError, match="logits"):
        K.CalibrationMetrics(5, temperature=2.0)
    empty = K.CalibrationMetrics(3, classwise=True).compute()
    assert math.isnan(empty["ece"]) and empty["n"] == 0 and len(empty["classwise_ece_per_class"]) == 3


def test_shape_and_temperature_errors_are_reported_without_a_gpu():
    import __graft_entry__ as entry
    entry.build()
    from multimodal_supernovae_amd import _lib
    lib = _lib.lib()
    fake = ctypes.c_void_p(4096)                                 # never dereferenced: validation rejects the call before any launch

    def refused(rc, text):
        return rc == 1 and text in lib.msn_last_error()

    assert refused(lib.msn_softmax_rows(fake, 1025, 8, 1025, 1.0, fake, 1025, None), b"C must be in 1..1024")
    assert refused(lib.msn_softmax_rows(fake, 5, 0, 5, 1.0, fake, 5, None), b"N must be in")
    assert refused(lib.msn_softmax_rows(fake, 5, 8, 5, 1.0, fake, 4, None), b"output row stride")
    assert refused(lib.msn_calibration_counts(fake, 1025, fake, 8, 1025, 15, 0, fake, fake, None), b"C must be in 1..1024")
    assert refused(lib.msn_calibration_counts(fake, 5, fake, 8, 5, 0, 0, fake, fake, None), b"B must be in 1..1024")
    assert refused(lib.msn_calibration_counts(fake, 5, fake, 8, 5, 1025, 1, fake, fake, None), b"B must be in 1..1024")
    assert refused(lib.msn_calibration_counts(fake, 4, fake, 8, 5, 15, 1, fake, fake, None), b"row stride")
    assert refused(lib.msn_calibration_counts(fake, 5, fake, 1 << 31, 5, 15, 1, fake, fake, None), b"N must be in")
    for beta in (0.0, -1.0, float("nan"), float("inf")):
        assert refused(lib.msn_softmax_rows(fake, 5, 8, 5, beta, fake, 5, None), b"beta must be finite and > 0")
        assert refused(lib.msn_temperature_nll(fake, 5, fake, 8, 5, beta, fake, fake, 1 << 20, None), b"beta must be finite and > 0")
    assert refused(lib.msn_temperature_nll(fake, 1025, fake, 8, 1025, 1.0, fake, fake, 1 << 20, None), b"C must be in 1..1024")
    assert lib.msn_temperature_nll_workspace_bytes(0) == 0 and lib.msn_temperature_nll_workspace_bytes(1 << 31) == 0
    assert lib.msn_temperature_nll_workspace_bytes(1) == 64
    need = lib.msn_temperature_nll_workspace_bytes(100000)
    assert need == 391 * 64 and lib.msn_temperature_nll_workspace_bytes(1 << 30) == 512 * 64
    assert refused(lib.msn_temperature_nll(fake, 5, fake, 100000, 5, 1.0, fake, fake, need - 1, None), b"workspace")
    assert refused(lib.msn_temperature_nll(fake, 5, fake, 100000, 5, 1.0, fake, None, 0, None), b"workspace")
