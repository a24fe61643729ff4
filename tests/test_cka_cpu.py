"""Centred kernel alignment without a GPU: the host halves of embedding_metrics (hsic_from_sums, cka_from_sums) over the longdouble
restatement of the kernel's sums against the matrix definitions (tr(KHLH), Song et al.'s debiased estimator), the feature-space
form of linear CKA, the invariances, the nan rules and the minibatch combination of the CKA class.

Everything here is longdouble, every rational factor included: formed as a Python float, 2 / n alone costs 2.6e-14 of an RBF
HSIC, whose three terms are some hundred times their sum."""
import numpy as np
import pytest
import torch

SHAPES = [(4, 1, 3), (5, 33, 1), (65, 33, 7), (130, 100, 64)]
KERNELS = ["linear", "rbf"]
LD = np.longdouble


def _E():
    from multimodal_supernovae_amd import embedding_metrics
    return embedding_metrics


def _pair(n, dx, dy, offset=0.0, seed=0):
    """Two fp32 sets that share their first columns; `offset` is added to every entry of X before the rounding to fp32."""
    rng = np.random.default_rng(1000 * n + dx + seed)
    X = rng.standard_normal((n, dx))
    Y = rng.standard_normal((n, dy))
    k = min(dx, dy)
    Y[:, :k] += X[:, :k]
    return (X + offset).astype(np.float32), Y.astype(np.float32)


def _terms(sums, n, pair, debiased):
    """The magnitudes of the three terms of hsic_from_sums, divided as the estimator divides them."""
    ip, ir, ia, ib = {"KL": (0, 3, 6, 7), "KK": (1, 4, 6, 6), "LL": (2, 5, 7, 7)}[pair]
    s = sums[0 if debiased else 1]
    n = LD(n)
    if debiased:
        return (abs(s[ip]) + abs(s[ia] * s[ib]) / ((n - 1) * (n - 2)) + 2 / (n - 2) * abs(s[ir])) / (n * (n - 3))
    return (abs(s[ip]) + 2 / n * abs(s[ir]) + abs(s[ia] * s[ib]) / (n * n)) / ((n - 1) * (n - 1))


@pytest.mark.parametrize("n,dx,dy", SHAPES)
@pytest.mark.parametrize("kernel", KERNELS)
def test_the_sums_give_the_matrix_definitions(n, dx, dy, kernel):
    E = _E()
    for offset in (0.0, 100.0):
        X, Y = _pair(n, dx, dy, offset)
        sums = E.hsic_sums_reference(X, Y, kernel)
        assert sums.dtype == LD and sums.shape == (2, 8)
        for debiased in (False, True):
            want = E.hsic_reference(X, Y, kernel, debiased)
            for pair, w in zip(("KL", "KK", "LL"), want):
                got = E.hsic_from_sums(sums, n, pair, debiased)
                assert got.dtype == LD
                assert abs(got - w) <= LD(1e-15) * _terms(sums, n, pair, debiased), (offset, debiased, pair, float(got), float(w))
            a, b = E.cka_from_sums(sums, n, debiased), E.cka_reference(X, Y, kernel, debiased)
            # a quotient of figures that agree to 1e-15 of their terms, the terms up to 1e3 times their sum
            assert (np.isnan(a) and np.isnan(b)) or abs(a - b) <= 1e-12, (offset, debiased, a, b)
        # an explicit bandwidth, one per set
        if kernel == "rbf":
            sums = E.hsic_sums_reference(X, Y, kernel, sigma=(1.5, 0.75))
            for pair, w in zip(("KL", "KK", "LL"), E.hsic_reference(X, Y, kernel, False, sigma=(1.5, 0.75))):
                assert abs(E.hsic_from_sums(sums, n, pair) - w) <= LD(1e-15) * _terms(sums, n, pair, False)


def test_the_derived_bandwidth_is_the_mean_squared_distance():
    """sigma=None equals the explicit sigma^2 = sigma_scale^2 (2 / (N - 1)) sum_i |xc_i|^2: what the kernel forms."""
    E = _E()
    X, Y = _pair(65, 33, 7)
    for scale in (1.0, 0.5):
        sig = []
        for Z in (X, Y):
            Zc = Z.astype(LD) - Z.astype(LD).sum(axis=0) / LD(len(Z))
            sig.append(float(scale * np.sqrt(LD(2) / LD(len(Z) - 1) * (Zc * Zc).sum())))
        a = E.hsic_sums_reference(X, Y, "rbf", sigma=None, sigma_scale=scale)
        b = E.hsic_sums_reference(X, Y, "rbf", sigma=tuple(sig))
        assert np.all(np.abs(a - b) <= 1e-12 * np.abs(b))               # the explicit sigma went through fp64: 1.1e-16 times exponents < 1e3


@pytest.mark.parametrize("n,dx,dy", SHAPES[1:])
def test_biased_linear_cka_is_the_feature_space_form(n, dx, dy):
    E = _E()
    X, Y = _pair(n, dx, dy)
    Xc, Yc = X.astype(LD) - X.astype(LD).mean(axis=0), Y.astype(LD) - Y.astype(LD).mean(axis=0)
    fro = lambda A: np.sqrt((A * A).sum())
    want = fro(Yc.T @ Xc) ** 2 / (fro(Xc.T @ Xc) * fro(Yc.T @ Yc))
    assert abs(E.cka_from_sums(E.hsic_sums_reference(X, Y), n) - float(want)) <= 1e-12
    assert abs(E.cka_reference(X, Y) - float(want)) <= 1e-12


def _exact_sets(n=37):
    """Multiples of 1/16 in sixteen columns: an orthogonal map with entries +-1/4, a scale of 3 and an integer translation are
    exact in fp32, so the invariances are checked on the inputs the map really produces."""
    rng = np.random.default_rng(5)
    X = np.round(rng.standard_normal((n, 16)) * 16) / 16
    Y = np.round((0.5 * X[:, :5] + rng.standard_normal((n, 5))) * 16) / 16
    H = np.array([[1.0]])
    for _ in range(4):
        H = np.block([[H, H], [H, -H]])
    Q = (H / 4)[rng.permutation(16)] * rng.choice([-1.0, 1.0], size=16)
    assert np.array_equal(Q @ Q.T, np.eye(16))
    for A in (X, Y, 3 * X @ Q, X + 37, Y - 12):
        assert np.array_equal(A.astype(np.float32).astype(np.float64), A)
    return X, Y, Q


def test_invariances_of_the_reference():
    E = _E()
    X, Y, Q = _exact_sets()
    shift_x, shift_y = np.arange(16) * 3.0 - 20, np.array([37.0, -5, 0, 11, -64])
    for debiased in (False, True):
        base = E.cka_reference(X, Y, "linear", debiased)
        assert abs(E.cka_reference(3 * X @ Q, Y, "linear", debiased) - base) <= 1e-12        # an orthogonal map and a scale of X
        assert abs(E.cka_reference(X, 0.5 * Y, "linear", debiased) - base) <= 1e-12
        for kernel in KERNELS:
            base = E.cka_reference(X, Y, kernel, debiased)
            assert abs(E.cka_reference(X + shift_x, Y + shift_y, kernel, debiased) - base) <= 1e-12   # translation
            assert abs(E.cka_from_sums(E.hsic_sums_reference(X + shift_x, Y + shift_y, kernel), len(X), debiased) - base) <= 1e-12
            assert abs(E.cka_reference(X, X, kernel, debiased) - 1.0) <= 1e-12
            assert abs(E.cka_reference(X, Y, kernel, debiased) - E.cka_reference(Y, X, kernel, debiased)) <= 1e-12
        # the RBF kernel with a derived bandwidth does not see the scale either; the map keeps every distance
        assert abs(E.cka_reference(3 * X @ Q, Y, "rbf", debiased) - E.cka_reference(X, Y, "rbf", debiased)) <= 1e-12
    assert 0.0 < E.cka_reference(X, Y) < 1.0


def test_nan_rules():
    E = _E()
    X, Y = _pair(9, 5, 3)
    same = np.full((9, 4), 2.5, dtype=np.float32)
    for kernel in KERNELS:
        for debiased in (False, True):
            assert np.isnan(E.cka_reference(same, Y, kernel, debiased)) and np.isnan(E.cka_reference(X, same, kernel, debiased))
            assert np.isnan(E.cka_from_sums(E.hsic_sums_reference(same, Y, kernel), 9, debiased))
            assert np.isfinite(E.cka_reference(X, Y, kernel, debiased))
        for n in (2, 3):
            sums = E.hsic_sums_reference(X[:n], Y[:n], kernel)
            assert np.isnan(E.cka_from_sums(sums, n, True)) and np.isnan(E.cka_reference(X[:n], Y[:n], kernel, True))
            assert np.isnan(E.hsic_from_sums(sums, n, "KL", True)) and np.isfinite(E.hsic_from_sums(sums, n, "KL", False))
    # a set of equal rows has no derived bandwidth: every RBF sum is nan; with the linear kernel its sums are zero
    assert np.isnan(E.hsic_sums_reference(same, Y, "rbf")[:, [0, 1, 3, 4, 6]]).all()
    assert (E.hsic_sums_reference(same, Y, "linear")[:, [0, 1, 3, 4, 6]] == 0).all()
    nonfinite = E.hsic_sums_reference(X, Y).astype(np.float64)
    nonfinite[1, 1] = np.inf
    assert np.isnan(E.cka_from_sums(nonfinite, 9))
    for bad in (dict(kernel="poly"), dict(sigma=0.0), dict(sigma=(1.0, -1.0)), dict(sigma=float("inf")), dict(sigma_scale=0.0),
                dict(sigma=(1.0, 2.0, 3.0))):
        with pytest.raises(ValueError):
            E.hsic_sums_reference(X, Y, **{"kernel": "rbf", **bad})
    with pytest.raises(ValueError):
        E.hsic_from_sums(np.zeros((2, 8)), 9, "LK")
    with pytest.raises(ValueError):
        E.hsic_from_sums(np.zeros((2, 7)), 9)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("debiased", [True, False])
def test_the_cka_class_combines_the_batches(monkeypatch, kernel, debiased):
    """The device half replaced by its restatement rounded to fp64: compute() is sum_b HSIC(K_b, L_b) over the root of the two
    other sums, each HSIC from the matrix definition of its own batch.  fp64 sums under a cancellation of up to 1e3: 1e-10."""
    E = _E()
    calls = []

    def fake(X, Y, kernel="linear", sigma=None, sigma_scale=1.0, out=None):
        calls.append((kernel, sigma, sigma_scale))
        return torch.from_numpy(E.hsic_sums_reference(X.numpy(), Y.numpy(), kernel, sigma, sigma_scale).astype(np.float64))

    monkeypatch.setattr(E, "hsic_sums", fake)
    batches = [_pair(n, 12, 5, seed=s) for s, n in enumerate((17, 33, 8))]
    m = E.CKA(kernel, debiased=debiased, sigma_scale=0.75)
    assert E.CKA().debiased is True
    for X, Y in batches:
        assert m.update(torch.from_numpy(X), torch.from_numpy(Y)) is m
    h = [E.hsic_reference(X, Y, kernel, debiased, None, 0.75) for X, Y in batches]
    want = float(sum(v[0] for v in h) / np.sqrt(sum(v[1] for v in h) * sum(v[2] for v in h)))
    assert abs(m.compute() - want) <= 1e-10 and calls == [(kernel, None, 0.75)] * 3
    assert abs(m.compute() - E.cka_reference(*batches[0], kernel, debiased, None, 0.75)) > 1e-6       # not the first batch alone
    with pytest.raises(ValueError, match="widths changed"):
        m.update(torch.zeros(8, 12), torch.zeros(8, 6))
    m.reset()
    with pytest.raises(ValueError, match="nothing added"):
        m.compute()
    m.update(torch.from_numpy(batches[0][0][:3]), torch.from_numpy(batches[0][1][:3]))             # widths are free after a reset
    assert np.isnan(m.compute()) == debiased


def test_cpu_tensors_are_refused():
    E = _E()
    from multimodal_supernovae_amd._lib import MsnHipError
    X = torch.zeros(8, 4)
    for call in (lambda: E.hsic_sums(X, X), lambda: E.cka(X, X), lambda: E.CKA().update(X, X), lambda: E.cka_matrix([X], [X])):
        with pytest.raises(MsnHipError):
            call()
