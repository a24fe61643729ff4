"""The host halves of the linear probes (multimodal_supernovae_amd/probes.py), pure numpy fp64: solve_normal_equations against
numpy.linalg.lstsq of the centred problem, lbfgs on the numpy restatement of the logistic objective.  No GPU."""
import numpy as np
import pytest

from multimodal_supernovae_amd import probes as P


def _unit_rows(rng, N, D):
    X = rng.standard_normal((N, D))
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    return X.astype(np.float32)


def _regression_case(N, D, K, seed, dup=False):
    rng = np.random.default_rng(seed)
    X = _unit_rows(rng, N, D)
    if dup:
        X[:, D - 1] = X[:, 0]
    Y = (X.astype(np.float64) @ rng.standard_normal((D, K)) + 0.3 + 0.05 * rng.standard_normal((N, K))).astype(np.float32)
    return X, Y


def _gram(X, Y):
    Z = np.concatenate([X, np.ones((len(X), 1), np.float32), Y], axis=1).astype(np.float64)
    return Z.T @ Z


def _centred(X, Y):
    X, Y = X.astype(np.float64), Y.astype(np.float64)
    return X - X.mean(axis=0), Y - Y.mean(axis=0)


def _coef_bound(X, Y, ref):
    Xc, _ = _centred(X, Y)
    cond = np.linalg.cond(Xc.T @ Xc)
    return cond * X.shape[1] * 2.0 ** -50 * np.abs(ref).max(), cond


SHAPES = [(1000, 128, 1), (300, 32, 2), (2000, 512, 1)]


@pytest.mark.parametrize("N,D,K", SHAPES)
def test_normal_equations_match_lstsq_of_the_centred_problem(N, D, K):
    X, Y = _regression_case(N, D, K, seed=N + D)
    Xc, Yc = _centred(X, Y)
    ref = np.linalg.lstsq(Xc, Yc, rcond=None)[0].T                    # (K, D)
    coef, intercept = P.solve_normal_equations(_gram(X, Y), D, K)
    bound, cond = _coef_bound(X, Y, ref)
    err = np.abs(coef - ref).max()
    print(f"({N}, {D}, {K}): cond(A) {cond:.3g}, max|coef - lstsq| {err:.3e}, bound {bound:.3e}")
    assert coef.shape == (K, D) and intercept.shape == (K,)
    assert err <= bound
    ref_b = Y.astype(np.float64).mean(axis=0) - ref @ X.astype(np.float64).mean(axis=0)
    assert np.abs(intercept - ref_b).max() <= bound * np.sqrt(D)     # |x_mean| <= 1: the intercept inherits the coefficients' error


@pytest.mark.parametrize("N,D,K", SHAPES)
def test_ridge_matches_the_closed_form(N, D, K):
    alpha = 1e-2
    X, Y = _regression_case(N, D, K, seed=7 * N + D)
    Xc, Yc = _centred(X, Y)
    ref = np.linalg.solve(Xc.T @ Xc + alpha * np.eye(D), Xc.T @ Yc).T
    coef, _ = P.solve_normal_equations(_gram(X, Y), D, K, alpha=alpha)
    bound, _ = _coef_bound(X, Y, ref)
    assert np.abs(coef - ref).max() <= bound


@pytest.mark.parametrize("N", [50, 100])
def test_rank_deficient_problems_take_the_minimum_norm_solution(N):
    D = 128
    X, Y = _regression_case(N, D, 1, seed=N, dup=True)
    Xc, Yc = _centred(X, Y)
    ref = np.linalg.lstsq(Xc, Yc, rcond=None)[0].T
    coef, intercept = P.solve_normal_equations(_gram(X, Y), D, 1)
    fit = X.astype(np.float64) @ coef.T + intercept
    fit_ref = Xc @ ref.T + Y.astype(np.float64).mean(axis=0)
    err = np.abs(fit - fit_ref).max()
    print(f"({N}, {D}) duplicated column: max|fit - lstsq fit| {err:.3e}")
    assert err <= 1e-10 * np.abs(Y).max()
    assert np.abs(coef - ref).max() <= 1e-8 * np.abs(ref).max()      # the minimum-norm solution itself, not just its fit


def test_near_square_problem():
    N, D = 129, 128
    X, Y = _regression_case(N, D, 1, seed=129)
    Xc, Yc = _centred(X, Y)
    ref = np.linalg.lstsq(Xc, Yc, rcond=None)[0].T
    coef, _ = P.solve_normal_equations(_gram(X, Y), D, 1)
    rel = np.abs(coef - ref).max() / np.abs(ref).max()
    print(f"(129, 128): cond(A) {np.linalg.cond(Xc.T @ Xc):.3g}, relative coefficient error {rel:.3e}")
    assert rel <= 1e-8


def test_without_intercept():
    N, D, K = 300, 32, 2
    X, Y = _regression_case(N, D, K, seed=5)
    ref = np.linalg.lstsq(X.astype(np.float64), Y.astype(np.float64), rcond=None)[0].T
    coef, intercept = P.solve_normal_equations(_gram(X, Y), D, K, fit_intercept=False)
    Xd = X.astype(np.float64)
    bound = np.linalg.cond(Xd.T @ Xd) * D * 2.0 ** -50 * np.abs(ref).max()
    assert np.abs(coef - ref).max() <= bound
    assert np.array_equal(intercept, np.zeros(K))


def test_a_gram_matrix_without_targets_is_refused():
    X = _unit_rows(np.random.default_rng(0), 20, 4)
    Z = np.concatenate([X, np.ones((20, 1), np.float32)], axis=1).astype(np.float64)
    with pytest.raises(ValueError, match="K must be at least 1"):
        P.solve_normal_equations(Z.T @ Z, 4, 0)
    with pytest.raises(ValueError, match="G must be"):
        P.solve_normal_equations(Z.T @ Z, 4, 1)


@pytest.mark.parametrize("N,D,K", SHAPES)
def test_normal_equations_against_scikit_learn(N, D, K):
    lm = pytest.importorskip("sklearn.linear_model")
    X, Y = _regression_case(N, D, K, seed=N + D)
    Xd, Yd = X.astype(np.float64), Y.astype(np.float64)
    ols = lm.LinearRegression().fit(Xd, Yd)
    coef, intercept = P.solve_normal_equations(_gram(X, Y), D, K)
    bound, _ = _coef_bound(X, Y, ols.coef_)
    assert np.abs(coef - ols.coef_.reshape(K, D)).max() <= bound
    assert np.abs(intercept - np.reshape(ols.intercept_, K)).max() <= bound * np.sqrt(D)
    ridge = lm.Ridge(alpha=1e-2, solver="cholesky").fit(Xd, Yd)
    coef, _ = P.solve_normal_equations(_gram(X, Y), D, K, alpha=1e-2)
    assert np.abs(coef - ridge.coef_.reshape(K, D)).max() <= bound


# ------------------------------------------------------------------------------------------------------------ L-BFGS
def blobs(N, D, C, spread, seed, fresh=False):
    """Gaussian class blobs: class means drawn with standard deviation `spread`, unit noise (fp32, as embeddings are).
    fresh=True returns a second draw of the same size around the same means behind the first: (X, y, X2, y2)."""
    rng = np.random.default_rng(seed)
    mu = rng.standard_normal((C, D)) * spread
    out = []
    for _ in range(2 if fresh else 1):
        y = rng.integers(0, C, N)
        out += [(mu[y] + rng.standard_normal((N, D))).astype(np.float32), y]
    return tuple(out)


def fit_numpy(X, y, C, **kw):
    D = X.shape[1]

    def f(w):
        v, g = P.logistic_objective(X, y, w.reshape(C, D + 1))
        return v, g.reshape(-1)
    return P.lbfgs(f, np.zeros(C * (D + 1)), **kw)


BLOBS = [(300, 20, 3, 0.5), (500, 64, 5, 0.3), (2000, 128, 5, 0.15)]


@pytest.mark.parametrize("N,D,C,spread", BLOBS)
def test_lbfgs_on_the_logistic_objective(N, D, C, spread):
    X, y = blobs(N, D, C, spread, seed=N)
    res = fit_numpy(X, y, C)
    print(f"({N}, {D}, {C}): {res.n_iter} iterations, {res.n_evals} evaluations, max|g| {np.abs(res.grad).max():.3e}, "
          f"objective {res.fun:.12g}")
    assert res.converged and res.status == "gtol"
    assert np.abs(res.grad).max() <= 1e-4
    assert res.n_iter < 200
    W = res.x.reshape(C, D + 1)
    assert abs(W[:, -1].sum()) <= 1e-10
    v, g = P.logistic_objective(X, y, W)
    assert v == res.fun and np.array_equal(g.reshape(-1), res.grad)


@pytest.mark.parametrize("N,D,C,spread", BLOBS)
def test_lbfgs_reaches_scikit_learns_optimum(N, D, C, spread):
    lm = pytest.importorskip("sklearn.linear_model")
    X, y = blobs(N, D, C, spread, seed=N)
    res = fit_numpy(X, y, C)
    sk = lm.LogisticRegression(tol=1e-6, max_iter=1000).fit(X.astype(np.float64), y)
    v_sk, _ = P.logistic_objective(X, y, np.concatenate([sk.coef_, sk.intercept_[:, None]], axis=1))
    print(f"({N}, {D}, {C}): ours {res.fun:.12g}, scikit-learn {v_sk:.12g}, relative {(v_sk - res.fun) / v_sk:.3e}")
    assert res.fun <= v_sk * (1 + 1e-6)


def test_logistic_objective_gradient_is_the_derivative():
    X, y = blobs(40, 6, 3, 0.5, seed=1)
    y[::7] = -100
    rng = np.random.default_rng(2)
    W = rng.standard_normal((3, 7)) * 0.5
    cw = np.array([0.5, 1.0, 2.0])
    _, g = P.logistic_objective(X, y, W, C=2.0, class_weight=cw)
    h = 1e-6
    for idx in [(0, 0), (1, 3), (2, 6)]:
        Wp, Wm = W.copy(), W.copy()
        Wp[idx] += h
        Wm[idx] -= h
        num = (P.logistic_objective(X, y, Wp, C=2.0, class_weight=cw)[0] - P.logistic_objective(X, y, Wm, C=2.0, class_weight=cw)[0]) / (2 * h)
        assert abs(num - g[idx]) <= 1e-6 * max(1.0, abs(g[idx]))


def test_a_line_search_without_decrease_ends_as_converged_to_precision():
    calls = []

    def f(x):
        calls.append(1)
        return 1.0 + np.abs(x).sum(), -np.ones_like(x)           # the "gradient" points uphill: no step decreases f

    res = P.lbfgs(f, np.zeros(3))
    assert res.status == "precision" and res.converged
    assert np.array_equal(res.x, np.zeros(3)) and res.fun == 1.0 and res.n_iter == 0
    assert len(calls) == res.n_evals <= 100


def test_lbfgs_stops_at_max_iter():
    X, y = blobs(300, 20, 3, 0.5, seed=300)
    res = fit_numpy(X, y, 3, max_iter=3)
    assert res.status == "max_iter" and not res.converged and res.n_iter == 3
