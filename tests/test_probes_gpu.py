"""Linear probes on the GPU (csrc/probes.hip, multimodal_supernovae_amd/probes.py): the fp64 Gram kernel against exact integer
sums and against numpy fp64 within the bound exact products leave, the logistic loss-and-gradient kernel against the numpy fp64
restatement within a bound derived from the arithmetic, and the probes end to end against the host solvers.

Lines that start with "probes-accuracy:" carry the measured worst ratio to each bound (profiles/probes_accuracy.txt)."""
import functools

import numpy as np
import pytest
import torch

from test_probes_cpu import _coef_bound, _regression_case, blobs, fit_numpy

pytestmark = pytest.mark.gpu

U = 2.0 ** -52


def _lib():
    from multimodal_supernovae_amd import _lib as L
    return L


def _P():
    from multimodal_supernovae_amd import probes
    return probes


GRAM_SHAPES = [(1, 1, 1), (63, 5, 1), (257, 33, 2), (1000, 128, 1), (300, 1024, 1), (40, 7, 16)]


def _gram_shapes_with_slabs():
    """The fixed shapes plus one slab + 1 and two slabs + 1 rows at D = 16 (the slab length is the kernel's own)."""
    L = _lib().lib()
    rows = L.msn_probe_gram_slab_rows(257, 16, 1)
    extra = [(rows + 1, 16, 1), (2 * rows + 1, 16, 1)]
    assert all(L.msn_probe_gram_slab_rows(n, 16, 1) == rows for n, _, _ in extra)
    return GRAM_SHAPES + extra


@functools.lru_cache(maxsize=None)
def _int_case(N, D, K):
    g = torch.Generator().manual_seed(1000 * N + 10 * D + K)
    X = torch.randint(-8, 9, (N, D), generator=g).float()
    Y = torch.randint(-8, 9, (N, K), generator=g).float() if K else None
    Z = torch.cat([X, torch.ones(N, 1)] + ([Y] if K else []), dim=1).long()
    return X, Y, (Z.T @ Z).double()


@functools.lru_cache(maxsize=None)
def _normal_case(N, D, K):
    rng = np.random.default_rng(1000 * N + 10 * D + K)
    X = rng.standard_normal((N, D)).astype(np.float32)
    Y = rng.standard_normal((N, K)).astype(np.float32)
    Z = np.concatenate([X, np.ones((N, 1), np.float32), Y], axis=1).astype(np.float64)
    return X, Y, Z.T @ Z, N * U * (np.abs(Z).T @ np.abs(Z))


def _dev(a):
    return None if a is None else (a if isinstance(a, torch.Tensor) else torch.from_numpy(a)).cuda()


# ---------------------------------------------------------------------------------------------------------- Gram, exact
def test_gram_is_exact_on_integer_data():
    P = _P()
    for N, D, K in _gram_shapes_with_slabs():
        X, Y, ref = _int_case(N, D, K)
        G = P.probe_gram(_dev(X), _dev(Y))
        assert torch.equal(G.cpu(), ref), (N, D, K)


@pytest.mark.parametrize("N,D,K", [(63, 5, 1), (257, 33, 2), (1000, 128, 1), (40, 7, 16)])
def test_gram_bits_do_not_depend_on_stride_or_alignment(N, D, K):
    P = _P()
    X, Y, ref = _int_case(N, D, K)
    wide = torch.zeros(N, D + 5).cuda()
    wide[:, :D] = X.cuda()
    assert torch.equal(P.probe_gram(wide[:, :D], _dev(Y)).cpu(), ref)
    flat = torch.zeros(N * D + 8).cuda()
    assert flat.data_ptr() % 16 == 0
    off = flat[1:1 + N * D].view(N, D)                    # starts 4 bytes off a 16-byte boundary
    off.copy_(X.cuda())
    assert off.data_ptr() % 16 == 4
    assert torch.equal(P.probe_gram(off, _dev(Y)).cpu(), ref)
    Yw = torch.zeros(N, K + 3).cuda()
    Yw[:, :K] = Y.cuda()
    assert torch.equal(P.probe_gram(off, Yw[:, :K]).cpu(), ref)


def test_gram_without_targets():
    P = _P()
    for N, D in [(63, 5), (1000, 128)]:
        X, _, ref = _int_case(N, D, 0)
        G = P.probe_gram(_dev(X), None)
        assert G.shape == (D + 1, D + 1) and torch.equal(G.cpu(), ref)


# --------------------------------------------------------------------------------------------------------- Gram, random
def test_gram_on_normal_data_is_within_the_summation_bound():
    """Products are exact, so any order of the N additions is within gamma_N of the true sum: N 2^-52 (|Z|^T |Z|) leaves a
    factor 2 over N 2^-53 for 1 / (1 - N u) and the add into a running G."""
    P = _P()
    worst = 0.0
    for N, D, K in _gram_shapes_with_slabs():
        X, Y, ref, bound = _normal_case(N, D, K)
        G = P.probe_gram(_dev(X), _dev(Y))
        G2 = P.probe_gram(_dev(X), _dev(Y))
        assert torch.equal(G, G.T), (N, D, K)
        assert torch.equal(G, G2), (N, D, K)
        ratio = float((np.abs(G.cpu().numpy() - ref) / bound).max())
        print(f"probes-accuracy: gram normal ({N}, {D}, {K}) worst |G - ref| / bound = {ratio:.4f}")
        worst = max(worst, ratio)
        assert ratio <= 1.0, (N, D, K, ratio)
    print(f"probes-accuracy: gram normal worst over shapes = {worst:.4f}")


@pytest.mark.parametrize("N,D,K", [(257, 33, 2), (1000, 128, 1)])
def test_partial_fit_in_uneven_chunks(N, D, K):
    P = _P()
    X, Y, ref, bound = _normal_case(N, D, K)
    Xd, Yd = _dev(X), _dev(Y)
    probe = P.LinearRegressionProbe()
    cuts = [0, N // 7, N // 7 + N // 2 + 1, N]
    for a, b in zip(cuts[:-1], cuts[1:]):
        probe.partial_fit(Xd[a:b], Yd[a:b])
    G = probe.gram
    assert torch.equal(G, G.T)
    ratio = float((np.abs(G.cpu().numpy() - ref) / bound).max())
    print(f"probes-accuracy: gram partial_fit x3 ({N}, {D}, {K}) worst |G - ref| / bound = {ratio:.4f}")
    assert ratio <= 1.0
    probe.reset()
    assert probe.gram is None


def test_a_nan_stays_in_its_row_and_column():
    P = _P()
    N, D, K = 257, 33, 2
    X, Y, ref, bound = _normal_case(N, D, K)
    X = X.copy()
    X[3, 2] = np.nan
    G = P.probe_gram(_dev(X), _dev(Y)).cpu().numpy()
    assert np.isnan(G[2, :]).all() and np.isnan(G[:, 2]).all()
    keep = np.ones(D + 1 + K, bool)
    keep[2] = False
    rest = G[np.ix_(keep, keep)]
    assert np.isfinite(rest).all()
    assert (np.abs(rest - ref[np.ix_(keep, keep)]) <= bound[np.ix_(keep, keep)]).all()


# ------------------------------------------------------------------------------------------------------------- logistic
def _lr_block_boundary():
    """One block + 1 and two blocks + 1 rows of whatever a workgroup owns at (D, C) = (16, 3)."""
    L = _lib().lib()
    rows = L.msn_logreg_block_rows(65, 16, 3)
    shapes = [(rows + 1, 16, 3), (2 * rows + 1, 16, 3)]
    assert all(L.msn_logreg_block_rows(n, 16, 3) == rows for n, _, _ in shapes)
    return shapes


LR_SHAPES = [(1, 1, 2), (65, 7, 3), (500, 64, 5), (300, 1024, 16), (257, 128, 127)]


@functools.lru_cache(maxsize=None)
def _lr_case(N, D, C, weighted, ignored):
    P = _P()
    rng = np.random.default_rng(100000 * N + 100 * D + C + (7 if weighted else 0) + (13 if ignored else 0))
    X = rng.standard_normal((N, D)).astype(np.float32)
    y = rng.integers(0, C, N)
    if ignored:
        y[rng.random(N) < 0.1] = -100
    W = rng.standard_normal((C, D + 1)) * 0.5
    cw = rng.random(C) + 0.25 if weighted else None
    loss, grad = P.logistic_objective(X, y, W, C=np.inf, class_weight=cw)
    Xa = np.abs(X.astype(np.float64))
    A = Xa @ np.abs(W[:, :D]).max(axis=0) + np.abs(W[:, D]).max()
    eps = (N + D + 32) * U
    wmax = float(cw.max()) if weighted else 1.0
    loss_tol = eps * wmax * np.sum(1 + A)
    col = np.concatenate([Xa, np.ones((N, 1))], axis=1)
    grad_tol = eps * wmax * (col.T @ (1 + A))                        # per column d; the same for every class
    return X, y, W, cw, loss, grad, loss_tol, grad_tol


def _lr_check(shape, weighted, ignored, strided=False):
    P = _P()
    N, D, C = shape
    X, y, W, cw, loss, grad, loss_tol, grad_tol = _lr_case(N, D, C, weighted, ignored)
    Xd = _dev(X)
    if strided:
        wide = torch.zeros(N, D + 3).cuda()
        wide[:, :D] = Xd
        Xd = wide[:, :D]
    args = (Xd, _dev(y), _dev(W), _dev(cw))
    out = P.logreg_loss_grad(*args)
    assert torch.equal(out, P.logreg_loss_grad(*args)), shape
    o = out.cpu().numpy()
    rl = abs(o[0] - loss) / loss_tol
    rg = float((np.abs(o[1:].reshape(C, D + 1) - grad) / grad_tol[None, :]).max())
    tag = f"({N}, {D}, {C}){' weighted' if weighted else ''}{' 10% ignored' if ignored else ''}{' strided' if strided else ''}"
    print(f"probes-accuracy: logistic {tag} loss ratio {rl:.4f} gradient ratio {rg:.4f}")
    assert rl <= 1.0 and rg <= 1.0, (tag, rl, rg)
    return max(rl, rg)


@pytest.mark.parametrize("weighted,ignored", [(False, False), (True, False), (False, True), (True, True)])
def test_logistic_loss_and_gradient_match_numpy_fp64(weighted, ignored):
    """Bound: a logit is off by at most (D + 1) u A_r with A_r = sum_d |x_rd| max_c |w_cd| + max_c |b_c|; softmax and lse pass an
    absolute error of the logits on one to one; exp and log add a few ulp; the sum over the rows adds N u.  Hence
    eps = (N + D + 32) 2^-52, loss within eps wmax sum_r (1 + A_r), gradient (c, d) within eps wmax sum_r |x_rd| (1 + A_r)."""
    worst = 0.0
    for shape in LR_SHAPES + _lr_block_boundary():
        worst = max(worst, _lr_check(shape, weighted, ignored))
    worst = max(worst, _lr_check((65, 7, 3), weighted, ignored, strided=True))
    worst = max(worst, _lr_check((300, 1024, 16), weighted, ignored, strided=True))
    print(f"probes-accuracy: logistic worst ratio (weighted={weighted}, ignored={ignored}) = {worst:.4f}")


def test_logistic_refusals_launch_nothing():
    P, L = _P(), _lib()
    for D, C, what in [(1024, 17, "above 16400"), (1025, 2, "D must be in 1..1024"), (8, 1, "C must be at least 2")]:
        X = torch.zeros(4, D).cuda()
        y = torch.zeros(4, dtype=torch.int64).cuda()
        W = torch.zeros(C, D + 1, dtype=torch.float64).cuda()
        out = torch.full((1 + C * (D + 1),), -7.0, dtype=torch.float64).cuda()
        with pytest.raises(L.MsnHipError, match=what):
            P.logreg_loss_grad(X, y, W, out=out)
        assert bool((out == -7.0).all())
    with pytest.raises(L.MsnHipError, match="D must be in 1..1024"):
        P.probe_gram(torch.zeros(4, 1025).cuda(), torch.zeros(4, 1).cuda())
    with pytest.raises(L.MsnHipError, match="K must be in 0..16"):
        P.probe_gram(torch.zeros(4, 8).cuda(), torch.zeros(4, 17).cuda())


def test_cpu_tensors_are_refused():
    P, L = _P(), _lib()
    X, Y = torch.zeros(8, 4), torch.zeros(8)
    with pytest.raises(L.MsnHipError, match="no CPU path"):
        P.LinearRegressionProbe().partial_fit(X, Y)
    with pytest.raises(L.MsnHipError, match="no CPU path"):
        P.LinearRegressionProbe().partial_fit(X.cuda(), Y)
    with pytest.raises(L.MsnHipError, match="no CPU path"):
        P.LogisticRegressionProbe().fit(X, Y.long())
    with pytest.raises(L.MsnHipError, match="no CPU path"):
        P.LogisticRegressionProbe().fit(X.cuda(), Y.long())


# ----------------------------------------------------------------------------------------------------------- end to end
def test_linear_regression_probe_end_to_end():
    P = _P()
    N, D, K = 1000, 128, 1
    X, Y = _regression_case(N, D, K, seed=N + D)
    Xd64, Yd64 = X.astype(np.float64), Y.astype(np.float64)
    Xc, Yc = Xd64 - Xd64.mean(axis=0), Yd64 - Yd64.mean(axis=0)
    ref = np.linalg.lstsq(Xc, Yc, rcond=None)[0].T
    probe = P.LinearRegressionProbe().fit(_dev(X), _dev(Y[:, 0]))
    bound, _ = _coef_bound(X, Y, ref)
    assert probe.coef_.shape == (D,) and isinstance(probe.intercept_, float)
    assert np.abs(probe.coef_ - ref[0]).max() <= bound
    pred = probe.predict(_dev(X))
    assert pred.shape == (N,) and pred.dtype == torch.float32 and pred.is_cuda
    want = Xd64 @ probe.coef_ + probe.intercept_
    err = np.abs(pred.cpu().numpy().astype(np.float64) - want).max()
    print(f"probes-accuracy: LinearRegressionProbe predict max error {err:.3e} (gate {1e-5 * np.abs(Y).max():.3e})")
    assert err <= 1e-5 * np.abs(Y).max()
    two = P.LinearRegressionProbe(alpha=1e-2).fit(_dev(X), _dev(np.concatenate([Y, -Y], axis=1)))
    assert two.coef_.shape == (2, D) and two.predict(_dev(X)).shape == (N, 2)
    assert np.abs(two.coef_[0] + two.coef_[1]).max() <= bound


@pytest.mark.parametrize("N,D,C,spread", [(500, 64, 5, 0.3), (2000, 128, 5, 0.15)])
def test_logistic_regression_probe_end_to_end(N, D, C, spread):
    P = _P()
    X, y, X2, _ = blobs(N, D, C, spread, seed=N, fresh=True)
    cpu = fit_numpy(X, y, C)
    probe = P.LogisticRegressionProbe(n_classes=C).fit(_dev(X), _dev(y))
    W = np.concatenate([probe.coef_, probe.intercept_[:, None]], axis=1)
    obj = P.logistic_objective(X, y, W)[0]
    rel = abs(obj - cpu.fun) / cpu.fun
    print(f"probes-accuracy: LogisticRegressionProbe ({N}, {D}, {C}): {probe.n_iter_} iterations, {probe.n_evals_} evaluations, "
          f"objective {obj:.12g} vs host {cpu.fun:.12g} (relative {rel:.3e})")
    assert probe.converged_ and probe.n_iter_ < 200
    assert rel <= 1e-6
    Wc = cpu.x.reshape(C, D + 1)
    Z = X2.astype(np.float64) @ Wc[:, :D].T + Wc[:, D]
    top = np.sort(Z, axis=1)
    sure = top[:, -1] - top[:, -2] >= 1e-3
    assert (~sure).mean() <= 0.02
    pred = probe.predict(_dev(X2))
    assert pred.dtype == torch.int32 and pred.shape == (N,)
    assert np.array_equal(pred.cpu().numpy()[sure], Z.argmax(axis=1)[sure])
    assert probe.decision_function(_dev(X2)).shape == (N, C)


def test_linear_probe_metrics_equal_the_metrics_fed_by_hand():
    from multimodal_supernovae_amd import utils
    from multimodal_supernovae_amd.models_finetune import ClassificationMetrics, RegressionMetrics
    X, y, X2, y2 = (_dev(a) for a in blobs(500, 64, 5, 0.3, seed=500, fresh=True))
    got = utils.linear_probe_metrics(X, y, X2, y2, task="classification")
    pred = utils.get_linear_predictions(X, y, X2, y2, task="classification", n_classes=5)
    m = ClassificationMetrics(5)
    m.update(pred, y2)
    assert got == m.compute() and set(got) >= {"acc", "f1_macro", "f1_micro"} and got["acc"] > 0.5
    Xr, Yr = _regression_case(1000, 128, 1, seed=3)
    Xr, Yr = _dev(Xr), _dev(Yr[:, 0])
    got = utils.linear_probe_metrics(Xr[:700], Yr[:700], Xr[700:], Yr[700:], task="regression")
    pred = utils.get_linear_predictions(Xr[:700], Yr[:700], Xr[700:], task="regression")
    m = RegressionMetrics()
    m.update(pred, Yr[700:])
    assert got == m.compute() and set(got) == {"L1", "L2", "R2", "OLF"} and got["R2"] > 0.5
    with pytest.raises(ValueError, match="task must be"):
        utils.get_linear_predictions(Xr, Yr, task="knn")
