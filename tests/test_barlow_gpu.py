"""Barlow Twins on the GPU (csrc/barlow.hip): the cross covariance with its means and biased variances
(embedding_metrics.cross_correlation) exactly on integer data and within bounds derived from the addition depths of
include/msn_hip.h, the orientation of the D x D matrices, the loss and its gradients (loss.barlow_twins_loss) against the
longdouble reference within bounds derived the same way, the structure (poisoned outputs and workspace, rows it must not write,
the same bits for every run, stride and alignment), the refusals, and the model end to end.

Every bound comes from the arithmetic, with MARGIN = 2 over the first-order derivation (as tests/test_vicreg_gpu.py uses it);
none is tuned to what was measured.  Lines that start with "barlow-accuracy:" carry the measured worst ratio to each bound
(profiles/barlow_accuracy.txt)."""
import copy
import functools
import gc
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -53            # unit roundoff of fp64
MARGIN = 2
LAMBD, EPS = 5e-3, 1e-5   # the main setting

SHAPES = [(2, 1), (3, 2), (5, 3), (33, 12), (63, 31), (64, 32), (65, 33), (129, 64), (130, 128), (200, 256), (300, 100), (300, 130),
          (1100, 4), (2100, 256)]
ONCE = (2100, 256)        # the largest case runs the main setting on one family only
STRUCTURE = [(65, 33), (130, 128), (1100, 4)]
FAMILIES = ["unit", "offset", "same", "const"]


def _E():
    from multimodal_supernovae_amd import embedding_metrics
    return embedding_metrics


def _Lo():
    from multimodal_supernovae_amd import loss
    return loss


def _lib():
    from multimodal_supernovae_amd import _lib as L
    return L


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------- the plan and the depths of the header
def xcov_plan(N, D):
    """(mrows, mslabs, pairs, per, slabs) of msn_cross_cov (include/msn_hip.h)."""
    mrows = max(64, cdiv(N, 64))
    T = cdiv(D, 64)
    pairs = T * T
    chunks = cdiv(N, 32)
    per = max(4, cdiv(chunks, cdiv(512, pairs)))
    return mrows, cdiv(N, mrows), pairs, per, cdiv(chunks, per)


def a_mean(N):
    mrows, mslabs, _, _, _ = xcov_plan(N, 1)
    return mrows + mslabs


def a_var(N, D):
    _, _, _, per, slabs = xcov_plan(N, D)
    return 8 * per + 4 + slabs


def a_cov(N, D):
    _, _, _, per, slabs = xcov_plan(N, D)
    return 32 * per + slabs


def a_dd(D):
    blocks = min(cdiv(D * D, 256), 64)
    return cdiv(D * D, 256 * blocks) + 9 + cdiv(blocks, 256) + 9


def a_rq(D):
    return D


def a_p(D):
    return 32 * cdiv(D, 32)


def test_the_plan_cuts_the_test_shapes_into_slabs_tile_pairs_and_a_ragged_tile():
    assert xcov_plan(129, 64)[2:] == (1, 4, 2) and xcov_plan(300, 130)[2:] == (9, 4, 3) and xcov_plan(1100, 4)[2:] == (1, 4, 9)
    assert xcov_plan(2100, 256) == (64, 33, 16, 4, 17) and xcov_plan(65, 33)[4] == 1 and xcov_plan(200, 256)[2:] == (16, 4, 2)
    assert xcov_plan(10 ** 6, 256)[3] == cdiv(cdiv(10 ** 6, 32), 32)          # beyond 512 workgroups the slabs grow
    assert xcov_plan(2100, 256)[1] > 1 and xcov_plan(5000, 4)[0] == 79         # several slabs of the means; slabs beyond 64 rows
    shapes = SHAPES + [(300, 200)]
    assert any(cdiv(d, 64) > 1 and d % 64 for _, d in shapes) and any(d % 64 == 0 for _, d in shapes)    # ragged and full last tiles
    assert any(xcov_plan(n, d)[4] > 1 and xcov_plan(n, d)[2] > 1 for n, d in shapes)                     # slabs x tile pairs
    L = _lib().lib()
    for n, d in shapes + [(4096, 128), (10 ** 6, 256)]:
        _, mslabs, pairs, _, slabs = xcov_plan(n, d)
        assert L.msn_cross_cov_workspace_bytes(n, d) == 8 * (2 * mslabs * d + 2 * slabs * d + 4096 * slabs * pairs), (n, d)
        assert L.msn_barlow_workspace_bytes(d) == 16 * min(cdiv(d * d, 256), 64), d


# ----------------------------------------------------------------------------------------------------------- the inputs
def _unit(n, d, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d))
    return X / np.linalg.norm(X, axis=1, keepdims=True)


@functools.lru_cache(maxsize=None)
def _pair(family, n, d):
    """unit    unit-norm rows and a unit-norm partner (the rows plus noise of relative size 0.3): what the model's towers give
       offset  unnormalised rows with a large common offset (mean >> spread: what the centring is for), the columns' spreads
               alternating between 0.25 and 4; the partner has another offset and scale
       same    Y = X (the rows of "offset"): c_aa is next to 1
       const   "unit" with one constant column in X: v = 0 there, its row of c is 0"""
    seed = 11 * n + d
    if family in ("unit", "const"):
        X = _unit(n, d, seed)
        Y = X + 0.3 * _unit(n, d, seed + 5)
        Y /= np.linalg.norm(Y, axis=1, keepdims=True)
        X, Y = X.astype(np.float32), Y.astype(np.float32)
        if family == "const":
            X[:, min(1, d - 1)] = 0.75
        return X, Y
    rng = np.random.default_rng(seed + 1)
    scale = np.where(np.arange(d) % 2 == 0, 0.25, 4.0)
    X = (100.0 + rng.standard_normal((n, d)) * scale).astype(np.float32)
    if family == "same":
        return X, X.copy()
    Y = (-40.0 + 0.5 * (X.astype(np.float64) - 100.0) + 0.5 * rng.standard_normal((n, d)) * scale).astype(np.float32)
    return X, Y


def _ratio(err, bound):
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    return float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err == 0, 0.0, np.inf))))


# ----------------------------------------------------------------------------------------------------------- the bounds
def _derive(X, Y, lambd, eps):
    """The longdouble reference of one pair and what fp64 may do to every quantity on the kernels' way, first order, from the
    depths of the header and the reference's absolute sums (float64 arrays; u = 2^-53):
        dmean_c  = (A_mean + 1) u sum_i |x_ic| / N                         the column sum's additions and the division
        E_ic     = dmean_c + u (|xc_ic| + dmean_c)                          a staged centred value: the mean's error, one subtraction
        dvar_a   = (2 |Xc|^T E + E^T E)_aa-wise / N + (A_var + 3) u v_a     the factors' errors; the squares, the additions, the division
        dcov_ab  = (|Xc|^T E_y + E_x^T |Yc| + E_x^T E_y)_ab / N + (A_cov + 3) u (|Xc|^T |Yc|)_ab / N
        ds_a     = dvar_a / s_a + 2 u s_a                                   s = sqrt(v + eps): 1 / s covers either sign; the addition, the root
        dss_ab   = ds_x[a] s_y[b] + s_x[a] ds_y[b] + ds_x[a] ds_y[b] + u ss_ab
        dc_ab    = dcov_ab / ss_ab + |c_ab| dss_ab / ss_ab + 2 u |c_ab|
        dcm1_a   = dc_aa + u |c_aa - 1|
        don      = sum_a (2 |c_aa - 1| dcm1_a + dcm1_a^2) + (A_dd + 2) u on;   doff likewise over a != b with dc
        dL       = don + lambd doff + 3 u (on + lambd off)
        dG_ab    = 2 dcm1_a on the diagonal, 2 lambd (dc_ab + 2 u |c_ab|) off it
        dA_ab    = dG_ab / (N ss_ab) + |A_ab| (dss_ab / ss_ab + 3 u)
        dr_a     = sum_b (dG |c| + |G| dc + dG dc)_ab + (A_rq + 2) u sum_b |G c|_ab;   dq_b likewise over a
        dd_x[a]  = dr_a / (N w_a) + |d_x[a]| (dw_a / w_a + 3 u),  w = v + eps, dw = dvar + u w
        dP_x     = |Yc| dA^T + E_y |A|^T + (A_p + 2) u |Yc| |A|^T            the factors' errors; the products and the additions
        omit_x[a] = sum_b |A_ab| dmean_y[b]                                  the omitted mean_i(dL/dxhat): -sum_b A_ab mean_i(yc_ib),
                                                                            zero for exact means, the means' rounding otherwise
        B_x      = dP_x + dd_x |Xc| + |d_x| E_x + dd_x E_x + 4 u (|Yc| |A|^T + |d_x| |Xc|) + omit_x   (the fma, the product with g)
    and B_y with the towers exchanged and A for A^T."""
    n, d = X.shape
    loss, grads, terms = _Lo().barlow_twins_reference([X, Y], lambd, eps, return_terms=True)
    mx, my, vx, vy, cov, corr = _E().cross_correlation_reference(X, Y, eps)
    f = lambda a: np.asarray(a, dtype=np.float64)
    Xl, Yl = X.astype(np.longdouble), Y.astype(np.longdouble)
    dmx = f((a_mean(n) + 1) * U * np.abs(Xl).sum(axis=0) / n)
    dmy = f((a_mean(n) + 1) * U * np.abs(Yl).sum(axis=0) / n)
    aXc, aYc = f(np.abs(Xl - mx)), f(np.abs(Yl - my))
    Ex, Ey = dmx[None, :] + U * (aXc + dmx[None, :]), dmy[None, :] + U * (aYc + dmy[None, :])
    v_x, v_y, c = f(vx), f(vy), f(corr)
    dvx = (2 * (aXc * Ex).sum(axis=0) + (Ex * Ex).sum(axis=0)) / n + (a_var(n, d) + 3) * U * v_x
    dvy = (2 * (aYc * Ey).sum(axis=0) + (Ey * Ey).sum(axis=0)) / n + (a_var(n, d) + 3) * U * v_y
    dcov = (aXc.T @ Ey + Ex.T @ aYc + Ex.T @ Ey) / n + (a_cov(n, d) + 3) * U * (aXc.T @ aYc) / n
    sx, sy = np.sqrt(v_x + eps), np.sqrt(v_y + eps)
    dsx, dsy = dvx / sx + 2 * U * sx, dvy / sy + 2 * U * sy
    ss = np.outer(sx, sy)
    dss = np.outer(dsx, sy) + np.outer(sx, dsy) + np.outer(dsx, dsy) + U * ss
    dc = dcov / ss + np.abs(c) * dss / ss + 2 * U * np.abs(c)
    diag = np.eye(d, dtype=bool)
    cm1 = np.diag(c) - 1.0
    dcm1 = np.diag(dc) + U * np.abs(cm1)
    on, off = float((cm1 ** 2).sum()), float((np.where(diag, 0.0, c) ** 2).sum())
    don = float((2 * np.abs(cm1) * dcm1 + dcm1 ** 2).sum()) + (a_dd(d) + 2) * U * on
    doff = float(np.where(diag, 0.0, 2 * np.abs(c) * dc + dc ** 2).sum()) + (a_dd(d) + 2) * U * off
    dL = don + lambd * doff + 3 * U * (on + lambd * off)
    G = np.where(diag, 2 * (c - 1.0), 2 * lambd * c)
    dG = np.where(diag, np.diag(2 * dcm1), 2 * lambd * (dc + 2 * U * np.abs(c)))
    A = G / (n * ss)
    aA = np.abs(A)
    dA = dG / (n * ss) + aA * (dss / ss + 3 * U)
    dterm = dG * np.abs(c) + np.abs(G) * dc + dG * dc
    aGc = np.abs(G * c)
    dr = dterm.sum(axis=1) + (a_rq(d) + 2) * U * aGc.sum(axis=1)
    dq = dterm.sum(axis=0) + (a_rq(d) + 2) * U * aGc.sum(axis=0)
    wx, wy = v_x + eps, v_y + eps
    d_x, d_y = -(G * c).sum(axis=1) / (n * wx), -(G * c).sum(axis=0) / (n * wy)
    ddx = dr / (n * wx) + np.abs(d_x) * ((dvx + U * wx) / wx + 3 * U)
    ddy = dq / (n * wy) + np.abs(d_y) * ((dvy + U * wy) / wy + 3 * U)
    spread_x, spread_y = aYc @ aA.T, aXc @ aA
    dPx = aYc @ dA.T + Ey @ aA.T + (a_p(d) + 2) * U * spread_x
    dPy = aXc @ dA + Ex @ aA + (a_p(d) + 2) * U * spread_y
    omit_x, omit_y = (aA @ dmy)[None, :], (aA.T @ dmx)[None, :]
    Bx = dPx + ddx * aXc + np.abs(d_x) * Ex + ddx * Ex + 4 * U * (spread_x + np.abs(d_x) * aXc) + omit_x
    By = dPy + ddy * aYc + np.abs(d_y) * Ey + ddy * Ey + 4 * U * (spread_y + np.abs(d_y) * aYc) + omit_y
    return dict(loss=loss, grads=grads, on=terms["on"][(0, 1)], off=terms["off"][(0, 1)], mean=(mx, my), var=(vx, vy), cov=cov,
                corr=corr, dmean=(dmx, dmy), dvar=(dvx, dvy), dcov=dcov, dcorr=dc, don=don, doff=doff, dL=dL, B=(Bx, By))


@functools.lru_cache(maxsize=None)
def _derived(family, n, d, lambd, eps):
    return _derive(*_pair(family, n, d), lambd, eps)


WORST = {}


def _note(key, value):
    WORST[key] = max(WORST.get(key, 0.0), value)
    return value


def _err(got, ref):
    return np.abs(got.detach().cpu().numpy().astype(np.longdouble) - ref).astype(np.float64)


def _check_statistics(X, Y, R, eps, label):
    E = _E()
    mx, my, vx, vy, cov, corr = E.cross_correlation(torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda(), eps)
    n, d = X.shape
    for t in (mx, my, vx, vy):
        assert t.dtype == torch.float64 and t.shape == (d,)
    for t in (cov, corr):
        assert t.dtype == torch.float64 and t.shape == (d, d)
    r = {"mean": max(_ratio(_err(mx, R["mean"][0]), MARGIN * R["dmean"][0]), _ratio(_err(my, R["mean"][1]), MARGIN * R["dmean"][1])),
         "var": max(_ratio(_err(vx, R["var"][0]), MARGIN * R["dvar"][0]), _ratio(_err(vy, R["var"][1]), MARGIN * R["dvar"][1])),
         "cov": _ratio(_err(cov, R["cov"]), MARGIN * R["dcov"]),
         "corr": _ratio(_err(corr, R["corr"]), MARGIN * R["dcorr"])}
    print(f"barlow-accuracy: statistics {label}: A_mean = {a_mean(n)}, A_var = {a_var(n, d)}, A_cov = {a_cov(n, d)}; error / bound: "
          + ", ".join(f"{k} {v:.4f}" for k, v in r.items()))
    for k, v in r.items():
        _note(k, v)
        assert v <= 1.0, (label, k, v)


def _check_loss(X, Y, R, lambd, eps, g, label):
    Lo = _Lo()
    e1 = torch.from_numpy(X).cuda().requires_grad_(True)
    e2 = torch.from_numpy(Y).cuda().requires_grad_(True)
    loss, comps = Lo.barlow_twins_loss_multimodal([e1, e2], lambd, eps, return_components=True)
    assert loss.dtype == torch.float32 and loss.dim() == 0
    assert len(comps) == 1 and comps[0].dtype == torch.float64 and comps[0].shape == (2,)
    (loss * g).backward()
    ref = R["loss"]
    bound = 2.0 ** -24 * abs(float(ref)) + MARGIN * R["dL"] + 2.0 ** -149
    err = abs(float(np.longdouble(float(loss.detach())) - ref))
    c = comps[0].cpu().numpy()
    r = {"loss": err / bound,
         "on": abs(float(np.longdouble(c[0]) - R["on"])) / (MARGIN * R["don"] + 2.0 ** -1074),
         "off": abs(float(np.longdouble(c[1]) - R["off"])) / (MARGIN * R["doff"] + 2.0 ** -1074)}
    worst = 0.0
    for got, w, b in ((e1.grad, R["grads"][0], R["B"][0]), (e2.grad, R["grads"][1], R["B"][1])):
        assert got.dtype == torch.float32 and got.shape == X.shape
        w = g * w
        bnd = 2.0 ** -24 * np.abs(w.astype(np.float64)) + MARGIN * abs(g) * b + 2.0 ** -149
        worst = max(worst, _ratio(_err(got, w), bnd))
    r["gradient"] = worst
    print(f"barlow-accuracy: loss {label} lambd = {lambd} eps = {eps} g = {g}: L = {float(ref):.6f}, error / bound: "
          + ", ".join(f"{k} {v:.4f}" for k, v in r.items()))
    for k, v in r.items():
        _note(k, v)
        assert v <= 1.0, (label, lambd, eps, k, v)
    return loss, comps[0], e1.grad, e2.grad


# --------------------------------------------------------------------------------------------------- statistics: exact
def _integers(n, d, seed):
    """Integers in -8 .. 8 whose column sums are multiples of N: the last row is adjusted (to the multiple nearest 0)."""
    rng = np.random.default_rng(seed)
    X = rng.integers(-8, 9, size=(n, d)).astype(np.int64)
    s = X[:-1].sum(axis=0)
    X[-1] = -s + n * np.round(s / n).astype(np.int64)
    assert (X.sum(axis=0) % n == 0).all() and np.abs(X).max() <= max(8, n // 2 + 1)
    return X


@pytest.mark.parametrize("n", [2, 3, 64, 129, 1024])
def test_statistics_of_integer_data_are_exact(n):
    """Integer data with integer means: the sums, the means, the centred values, their products and every partial sum are exact
    in fp64 in any order, so the only rounding is the one division by N -- which the restatement makes too."""
    E = _E()
    for d in (1, 3, 17, 64, 65, 130, 256):
        Xi, Yi = _integers(n, d, 1000 * n + d), _integers(n, d, 1000 * n + d + 500)
        X, Y = torch.from_numpy(Xi.astype(np.float32)).cuda(), torch.from_numpy(Yi.astype(np.float32)).cuda()
        mx, my, vx, vy, cov, _ = E.cross_correlation(X, Y)
        sx, sy = Xi.sum(axis=0) // n, Yi.sum(axis=0) // n
        Xc, Yc = Xi - sx, Yi - sy
        want = [sx.astype(np.float64), sy.astype(np.float64), (Xc * Xc).sum(axis=0).astype(np.float64) / float(n),
                (Yc * Yc).sum(axis=0).astype(np.float64) / float(n), (Xc.T @ Yc).astype(np.float64) / float(n)]
        for name, got, w in zip(("mean_x", "mean_y", "var_x", "var_y", "cov"), (mx, my, vx, vy, cov), want):
            assert torch.equal(got.cpu(), torch.from_numpy(w)), (n, d, name)


# ------------------------------------------------------------------------------------------------------- orientation
@pytest.mark.parametrize("d", [130, 200])
def test_the_matrices_are_not_transposed(d):
    """Y is X with its columns rolled by one, plus small noise: c is large at (a, a + 1 mod D) only.  A transposed tile, a
    transposed M or a swapped (a, b) puts the ridge at (a + 1, a) and fails here and in the gradients."""
    n = 300
    rng = np.random.default_rng(d)
    X = rng.standard_normal((n, d)).astype(np.float32)
    Y = (np.roll(X.astype(np.float64), 1, axis=1) + 0.05 * rng.standard_normal((n, d))).astype(np.float32)
    corr = _E().cross_correlation(torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda(), EPS)[5].cpu().numpy()
    ridge = (np.arange(d)[:, None] + 1) % d == np.arange(d)[None, :]
    assert corr[ridge].min() > 0.95 and np.abs(corr[~ridge]).max() < 0.5
    R = _derive(X, Y, LAMBD, EPS)
    _check_statistics(X, Y, R, EPS, f"rolled ({n}, {d})")
    _check_loss(X, Y, R, LAMBD, EPS, 1.0, f"rolled ({n}, {d})")
    _check_loss(X, Y, _derive(X, Y, 1.0, EPS), 1.0, EPS, 1.0, f"rolled ({n}, {d})")


# ------------------------------------------------------------------------------------------- float data: derived bounds
@pytest.mark.parametrize("n,d", SHAPES)
def test_statistics_loss_and_gradients_within_the_derived_bounds(n, d):
    families = ["offset"] if (n, d) == ONCE else FAMILIES
    for family in families:
        X, Y = _pair(family, n, d)
        label = f"{family} ({n}, {d})"
        R = _derived(family, n, d, LAMBD, EPS)
        _check_statistics(X, Y, R, EPS, label)
        _, comp, _, _ = _check_loss(X, Y, R, LAMBD, EPS, 1.0, label)
        if d == 1:
            assert float(comp[1]) == 0.0                          # one column: no off-diagonal term
    if (n, d) == ONCE:
        return
    for family, lambd, eps in (("offset", 0.0, EPS), ("offset", 1.0, 1e-2), ("unit", 1.0, EPS), ("unit", LAMBD, 1e-2), ("same", 0.0, 1e-2)):
        X, Y = _pair(family, n, d)
        R = _derived(family, n, d, lambd, eps)
        if eps != EPS:
            _check_statistics(X, Y, R, eps, f"{family} ({n}, {d}) eps = {eps}")
        _check_loss(X, Y, R, lambd, eps, 1.0, f"{family} ({n}, {d})")


def test_an_upstream_gradient_scales_the_result():
    _check_loss(*_pair("offset", 130, 128), _derived("offset", 130, 128, LAMBD, EPS), LAMBD, EPS, -3.5, "offset (130, 128)")
    _check_loss(*_pair("unit", 65, 33), _derived("unit", 65, 33, LAMBD, EPS), LAMBD, EPS, 0.125, "unit (65, 33)")


def test_three_towers_against_the_reference():
    """Each pair's loss is rounded to fp32 and the three are added in fp32; each tower's gradient is the fp32 sum of the
    gradients of its two pairs, each within the pair's own bound: 2^-24 of every partial figure and of the sum, and the fp64
    bounds of both pairs."""
    Lo = _Lo()
    n, d = 65, 33
    X, Y = _pair("offset", n, d)
    Z = (30.0 + 0.25 * X.astype(np.float64) - 0.5 * Y.astype(np.float64) + _unit(n, d, 99)).astype(np.float32)
    Xs = [X, Y, Z]
    embs = [torch.from_numpy(x).cuda().requires_grad_(True) for x in Xs]
    loss, comps = Lo.barlow_twins_loss_multimodal(embs, LAMBD, EPS, return_components=True)
    loss.backward()
    ref, grads = Lo.barlow_twins_reference(Xs, LAMBD, EPS)
    order = ((0, 1), (0, 2), (1, 2))
    R = {p: _derive(Xs[p[0]], Xs[p[1]], LAMBD, EPS) for p in order}
    assert len(comps) == 3 and all(c.dtype == torch.float64 and c.shape == (2,) for c in comps)
    for p, c in zip(order, comps):
        c = c.cpu().numpy()
        assert abs(float(np.longdouble(c[0]) - R[p]["on"])) <= MARGIN * R[p]["don"]
        assert abs(float(np.longdouble(c[1]) - R[p]["off"])) <= MARGIN * R[p]["doff"]
    sum_abs = sum(abs(float(R[p]["loss"])) for p in order)
    fp64 = MARGIN * sum(R[p]["dL"] for p in order)
    assert abs(float(np.longdouble(float(loss.detach())) - ref)) <= 2.0 ** -24 * (3 * sum_abs + abs(float(ref))) + fp64
    for k in range(3):
        mine = [p for p in order if k in p]
        parts = sum(np.abs(R[p]["grads"][p.index(k)].astype(np.float64)) for p in mine)
        b = 2.0 ** -24 * (parts + np.abs(grads[k].astype(np.float64))) + MARGIN * sum(R[p]["B"][p.index(k)] for p in mine) + 2.0 ** -149
        ratio = _ratio(_err(embs[k].grad, grads[k]), b)
        print(f"barlow-accuracy: three towers, tower {k}: worst |dX - ref| / bound = {ratio:.4f}")
        assert ratio <= 1.0, (k, ratio)


def test_zz_the_worst_ratios_of_this_run():
    """Printed last: the worst measured error / bound per quantity over the tests above that ran in this process."""
    print("barlow-accuracy: worst error / bound over this run: " + ", ".join(f"{k} {v:.4f}" for k, v in sorted(WORST.items())))
    assert all(v <= 1.0 for v in WORST.values())


# ----------------------------------------------------------------------------------------------------------- structure
def _strided(X, pad, shift):
    """The same rows with row stride D + pad, starting `shift` floats into a buffer: a padded stride and a base misaligned by
    4 bytes against the allocation."""
    n, d = X.shape
    buf = torch.full((n * (d + pad) + shift + 8,), float("nan"), device=X.device)
    view = buf[shift:shift + n * (d + pad)].view(n, d + pad)[:, :d]
    view.copy_(X)
    assert view.stride(0) == d + pad and view.data_ptr() % 8 == 4 * (shift % 2)
    return view


def _raw(X, Y, lambd, eps, g, pad=0, extra=5):
    """The whole pipeline through the C-ABI with every output and workspace poisoned with NaN before its launch; dX and dY carry
    `extra` sentinel rows past N and row stride D + pad."""
    L = _lib()
    lib, p, s = L.lib(), L.ptr, L.stream_ptr()
    n, d = X.shape
    nan = float("nan")
    f64 = dict(dtype=torch.float64, device="cuda")
    mx, my, vx, vy = (torch.full((d,), nan, **f64) for _ in range(4))
    cov = torch.full((d, d), nan, **f64)
    ws = torch.full((lib.msn_cross_cov_workspace_bytes(n, d) // 8,), nan, **f64)
    assert lib.msn_cross_cov(p(X), X.stride(0), p(Y), Y.stride(0), n, d, p(mx), p(my), p(vx), p(vy), p(cov), p(ws), ws.numel() * 8, s) == 0
    loss, comp = torch.full((), nan, device="cuda"), torch.full((2,), nan, **f64)
    corr, Mx, My = (torch.full((d, d), nan, **f64) for _ in range(3))
    dx, dy = torch.full((d,), nan, **f64), torch.full((d,), nan, **f64)
    ws2 = torch.full((lib.msn_barlow_workspace_bytes(d) // 8,), nan, **f64)
    assert lib.msn_barlow_fwd(p(vx), p(vy), p(cov), n, d, lambd, eps, p(loss), p(comp), p(corr), p(Mx), p(My), p(dx), p(dy), p(ws2),
                              ws2.numel() * 8, s) == 0
    gt = torch.tensor(g, dtype=torch.float32, device="cuda")
    dX = torch.full((n + extra, d + pad), -7.0, device="cuda")
    dY = torch.full((n + extra, d + pad), -7.0, device="cuda")
    assert lib.msn_barlow_bwd(p(X), X.stride(0), p(Y), Y.stride(0), n, d, p(mx), p(my), p(Mx), p(My), p(dx), p(dy), p(gt), p(dX), d + pad,
                              p(dY), d + pad, s) == 0
    return (mx, my, vx, vy, cov, loss, comp, corr, Mx, My, dx, dy), (dX, dY)


@pytest.mark.parametrize("n,d", STRUCTURE)
def test_poisoned_buffers_sentinel_rows_and_the_same_bits_for_every_stride_and_alignment(n, d):
    Lo = _Lo()
    Xn, Yn = _pair("offset", n, d)
    X, Y = torch.from_numpy(Xn).cuda(), torch.from_numpy(Yn).cuda()
    first, fgrads = _raw(X, Y, LAMBD, EPS, -1.5)
    for t in first:
        assert bool(torch.isfinite(t).all())                  # nothing of the poison is left, nothing poisoned was added up
    for dA in fgrads:
        assert bool((dA[n:] == -7.0).all()) and bool(torch.isfinite(dA[:n]).all())
    assert torch.equal(first[8], first[9].T.contiguous())     # M_x is M_y transposed, bit for bit
    runs = [_raw(X, Y, LAMBD, EPS, -1.5), _raw(_strided(X, 3, 1), _strided(Y, 7, 3), LAMBD, EPS, -1.5, pad=3, extra=2)]
    for again, agrads in runs:
        for a, b in zip(first, again):
            assert torch.equal(a, b)
        for a, b in zip(fgrads, agrads):
            assert bool((b[n:] == -7.0).all()) and bool((b[:, d:] == -7.0).all())
            assert torch.equal(a[:n, :d], b[:n, :d])
    # the autograd node gives the same bits as the raw pipeline
    e1, e2 = X.clone().requires_grad_(True), Y.clone().requires_grad_(True)
    loss = Lo.barlow_twins_loss(e1, e2, LAMBD, EPS)
    (loss * -1.5).backward()
    assert torch.equal(loss.detach(), first[5]) and torch.equal(e1.grad, fgrads[0][:n, :d]) and torch.equal(e2.grad, fgrads[1][:n, :d])
    # cross_correlation from strided rows
    got = _E().cross_correlation(_strided(X, 5, 1), _strided(Y, 2, 3), EPS)
    for a, b in zip(got, first[:5] + (first[7],)):
        assert torch.equal(a, b)


def test_non_finite_inputs_propagate():
    Xn, Yn = _pair("unit", 65, 33)
    X, Y = torch.from_numpy(Xn.copy()).cuda(), torch.from_numpy(Yn).cuda()
    X[7, 5] = float("nan")
    e1, e2 = X.requires_grad_(True), Y.clone().requires_grad_(True)
    loss = _Lo().barlow_twins_loss(e1, e2, LAMBD, EPS)
    loss.backward()
    assert math.isnan(float(loss.detach())) and bool(torch.isnan(e1.grad[7, 5])) and bool(torch.isnan(e1.grad[:, 5]).all())
    corr = _E().cross_correlation(X.detach(), Y, EPS)[5]
    assert bool(torch.isnan(corr[5]).all()) and bool(torch.isfinite(corr[4]).all())


# ----------------------------------------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing(monkeypatch):
    E, Lo, L = _E(), _Lo(), _lib()
    X = torch.from_numpy(_pair("unit", 8, 4)[0]).cuda()
    wide = torch.zeros(4, 257).cuda()
    for call, what in [(lambda: E.cross_correlation(wide, wide), r"D must be in 1\.\.256"),
                       (lambda: E.cross_correlation(X[:1], X[:1]), "N must be at least 2"),
                       (lambda: E.cross_correlation(X.cpu(), X), "must live on the GPU"),
                       (lambda: Lo.barlow_twins_loss(wide, wide), r"D must be in 1\.\.256"),
                       (lambda: Lo.barlow_twins_loss(X[:1], X[:1]), "N must be at least 2"),
                       (lambda: Lo.barlow_twins_loss(X.cpu(), X.cpu()), "must live on the GPU"),
                       (lambda: Lo.barlow_twins_loss(X, X.cpu()), "must live on the GPU")]:
        with pytest.raises(L.MsnHipError, match=what):
            call()
    for call, what in [(lambda: Lo.barlow_twins_loss(X, X, lambd=-1.0), "lambd"),
                       (lambda: Lo.barlow_twins_loss(X, X, lambd=float("inf")), "lambd"),
                       (lambda: Lo.barlow_twins_loss(X, X, lambd=float("nan")), "lambd"),
                       (lambda: Lo.barlow_twins_loss(X, X, eps=0.0), "eps"),
                       (lambda: Lo.barlow_twins_loss(X, X, eps=float("inf")), "eps"),
                       (lambda: E.cross_correlation(X, X, eps=-1.0), "eps"),
                       (lambda: E.cross_correlation(X, X[:7]), "one shape"),
                       (lambda: Lo.barlow_twins_loss(X, X[:7]), "one shape"),
                       (lambda: Lo.barlow_twins_loss_multimodal([X]), "at least two")]:
        with pytest.raises(ValueError, match=what):
            call()
    # the C-ABI itself: MSN_ERR_SHAPE (1) and nothing enqueued
    lib = L.lib()
    f64 = dict(dtype=torch.float64, device="cuda")
    mean, var, cov, M, corr = torch.zeros(2, 4, **f64), torch.zeros(2, 4, **f64), torch.zeros(4, 4, **f64), torch.zeros(2, 4, 4, **f64), torch.zeros(4, 4, **f64)
    dd = torch.zeros(2, 4, **f64)
    loss, comp = torch.zeros((), device="cuda"), torch.zeros(2, **f64)
    dX = torch.zeros(8, 4, device="cuda")
    ws = torch.zeros(1 << 16, dtype=torch.uint8).cuda()
    p, s = L.ptr, L.stream_ptr()

    def xc(n=8, d=4, ldx=4, mx=mean[0], nb=ws.numel()):
        return lib.msn_cross_cov(p(X), ldx, p(X), 4, n, d, None if mx is None else p(mx), p(mean[1]), p(var[0]), p(var[1]), p(cov), p(ws), nb, s)

    assert xc(nb=8) == 1 and xc(n=1) == 1 and xc(ldx=3) == 1 and xc(d=0) == 1 and xc(mx=None) == 1

    def fwd(n=8, lambd=5e-3, eps=1e-5, nb=ws.numel(), comp_=comp):
        return lib.msn_barlow_fwd(p(var[0]), p(var[1]), p(cov), n, 4, lambd, eps, p(loss), None if comp_ is None else p(comp_), p(corr),
                                  p(M[0]), p(M[1]), p(dd[0]), p(dd[1]), p(ws), nb, s)

    assert fwd(n=1) == 1 and fwd(lambd=-1.0) == 1 and fwd(lambd=float("nan")) == 1 and fwd(eps=0.0) == 1 and fwd(nb=8) == 1
    assert fwd(comp_=None) == 1

    def bwd(lddx=4, g=loss, n=8):
        return lib.msn_barlow_bwd(p(X), 4, p(X), 4, n, 4, p(mean[0]), p(mean[1]), p(M[0]), p(M[1]), p(dd[0]), p(dd[1]),
                                  None if g is None else p(g), p(dX), lddx, p(dX), 4, s)

    assert bwd(lddx=3) == 1 and bwd(g=None) == 1 and bwd(n=1) == 1
    assert lib.msn_cross_cov_workspace_bytes(8, 257) == 0 and lib.msn_barlow_workspace_bytes(0) == 0
    torch.cuda.synchronize()
    for t in (mean, var, cov, M, corr, dd, comp, dX):
        assert float(t.abs().sum()) == 0.0
    assert float(loss) == 0.0
    # sharded: statistics over gathered rows are not built
    monkeypatch.setattr(Lo, "_is_sharded", lambda global_negatives, group: bool(global_negatives))
    with pytest.raises(NotImplementedError, match="global_negatives=False"):
        Lo.barlow_twins_loss(X, X)
    assert Lo.barlow_twins_loss(X, X.flip(0), global_negatives=False).dim() == 0


# ------------------------------------------------------------------------------------------------------------ the model
TK = dict(n_out=16, emb=16, heads=2, depth=1, dropout=0.0, time_norm=20583.37, agg="mean")
SK = dict(n_out=16, emb=16, heads=2, depth=1, dropout=0.0, time_norm=17945.14, agg="mean")


def _clip(loss="barlow", **kw):
    from multimodal_supernovae_amd.models_multimodal import LightCurveImageCLIP
    torch.manual_seed(0)
    return LightCurveImageCLIP(enc_dim=32, nband=2, transformer_kwargs=TK, transformer_spectral_kwargs=SK,
                               combinations=["lightcurve", "spectral"], loss=loss, **kw).cuda().train()


def _batch(g, B, T=12, Ts=16):
    t = torch.sort(torch.rand(B, T // 2, generator=g) * 100, dim=1)[0].repeat(1, 2)
    return tuple(x.cuda() if x is not None else None for x in (
        None, torch.randn(B, T, generator=g), t, torch.ones(B, T, dtype=torch.bool), torch.randn(B, Ts, generator=g),
        torch.sort(torch.rand(B, Ts, generator=g) * 6000 + 3000, dim=1)[0], torch.ones(B, Ts, dtype=torch.bool),
        torch.rand(B, generator=g), torch.randint(0, 5, (B,), generator=g)))


def test_one_eager_step_reaches_every_trainable_parameter():
    model = _clip(loss_kwargs={"lambd": 5e-3})
    loss = model.training_step(_batch(torch.Generator().manual_seed(5), 16), 0)
    assert loss.dtype == torch.float32 and bool(torch.isfinite(loss))
    loss.backward()
    for k, p in model.named_parameters():
        if k in ("logit_scale", "logit_bias"):
            assert p.grad is None and not p.requires_grad, k
        else:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
    assert any(float(p.grad.abs().max()) > 0 for k, p in model.named_parameters() if p.grad is not None)
    assert torch.equal(model.logged["train_loss"], loss.detach())


def test_twenty_radam_steps_on_one_batch_lower_the_loss():
    model = _clip(lr=3e-3)
    batch = _batch(torch.Generator().manual_seed(6), 16)
    opt = model.configure_optimizers()["optimizer"]
    before = copy.deepcopy(model.state_dict())
    losses = []
    for _ in range(20):
        opt.zero_grad(set_to_none=True)
        loss = model.training_step(batch, 0)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    with torch.no_grad():
        losses.append(float(model.training_step(batch, 0)))
    assert all(math.isfinite(v) for v in losses) and losses[-1] < losses[0], losses
    after = model.state_dict()
    assert torch.equal(before["logit_scale"], after["logit_scale"]) and torch.equal(before["logit_bias"], after["logit_bias"])


def test_graphed_step_equals_eager_steps():
    """The step has no host read: it records into a graph and replays to what the eager steps give (the tolerance of
    tests/test_vicreg_gpu.py for the same model)."""
    from multimodal_supernovae_amd.trainer import GraphedTrainStep
    steps = 9
    g = torch.Generator().manual_seed(7)
    batches = [_batch(g, 16) for _ in range(steps)]
    eager = _clip(lr=3e-3, optimizer_kwargs={"weight_decay": 1e-3})
    graphed = copy.deepcopy(eager)
    opt_e = eager.configure_optimizers()["optimizer"]
    losses_e = []
    for b in batches:
        opt_e.zero_grad(set_to_none=True)
        loss = eager.training_step(b, 0)
        loss.backward()
        opt_e.step()
        losses_e.append(float(loss.detach()))
    step = GraphedTrainStep(graphed, graphed.configure_optimizers()["optimizer"], warmup=3)
    losses_g = [float(step(b).detach()) for b in batches]
    assert step.graph is not None and step.calls == steps
    torch.cuda.synchronize()
    for a, b in zip(losses_e, losses_g):
        assert abs(a - b) <= 1e-5 * abs(a), (losses_e, losses_g)
    for (k, p), (_, q) in zip(eager.named_parameters(), graphed.named_parameters()):
        torch.testing.assert_close(q, p, rtol=1e-5, atol=1e-7, msg=lambda m: f"{k}: {m}")
    del step, graphed, losses_g                         # the recorded graph is destroyed here, not by a later collection
    gc.collect()


def test_the_softmax_and_vicreg_objectives_are_what_they_were():
    """loss="softmax" still launches clip_loss_multimodal on the model's embeddings with its two trainable scalars, and
    loss="vicreg" vicreg_loss_multimodal with gamma = 1 / sqrt(enc_dim): the same bits as the free functions give, before and
    after a Barlow Twins step has run in the process."""
    from multimodal_supernovae_amd.loss import clip_loss_multimodal, vicreg_loss_multimodal
    batch = _batch(torch.Generator().manual_seed(8), 16)
    soft, vic = _clip(loss="softmax"), _clip(loss="vicreg")

    def both():
        a, b = soft.training_step(batch, 0), vic.training_step(batch, 0)
        with torch.no_grad():
            wa = clip_loss_multimodal(soft(*batch), soft.logit_scale, soft.logit_bias)
            wb = vicreg_loss_multimodal(vic(*batch), gamma=1.0 / math.sqrt(32))
        assert torch.equal(a.detach(), wa) and torch.equal(b.detach(), wb)
        return a, b

    a0, b0 = both()
    _clip().training_step(batch, 0).backward()
    a1, b1 = both()
    assert torch.equal(a0.detach(), a1.detach()) and torch.equal(b0.detach(), b1.detach())
    a1.backward()
    assert soft.logit_scale.grad is not None and soft.logit_bias.grad is not None
    assert list(soft.state_dict()) == list(_clip().state_dict()) == list(vic.state_dict())
