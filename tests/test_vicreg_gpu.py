"""VICReg on the GPU (csrc/vicreg.hip): the centred column covariance (embedding_metrics.column_covariance) exactly on
integer data and within a bound derived from the addition depths of include/msn_hip.h, the loss and its gradients
(loss.vicreg_loss) against the longdouble reference within bounds derived the same way, the structure (poisoned outputs and
workspace, rows it must not write, the same bits for every run, stride and alignment), the refusals, and the model end to end.

Every bound comes from the arithmetic, with MARGIN = 2 over the first-order derivation (as tests/infonce_refs.py and
tests/supcon_refs.py use it); none is tuned to what was measured.  Lines that start with "vicreg-accuracy:" carry the measured
worst ratio to each bound (profiles/vicreg_accuracy.txt)."""
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
EPS = 1e-4

SHAPES = [(2, 1), (3, 2), (5, 3), (33, 12), (63, 31), (64, 32), (65, 33), (129, 64), (130, 128), (200, 256), (300, 100), (300, 130),
          (1100, 4), (2100, 256)]
ONCE = (2100, 256)        # the largest case runs the main setting only
STRUCTURE = [(65, 33), (130, 128), (1100, 4)]


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
def cov_plan(N, D):
    """(mrows, mslabs, pairs, per, slabs) of msn_column_cov (include/msn_hip.h)."""
    mrows = max(64, cdiv(N, 64))
    T = cdiv(D, 64)
    pairs = T * (T + 1) // 2
    chunks = cdiv(N, 32)
    per = max(4, cdiv(chunks, cdiv(512, pairs)))
    return mrows, cdiv(N, mrows), pairs, per, cdiv(chunks, per)


def a_mean(N):
    mrows, mslabs, _, _, _ = cov_plan(N, 1)
    return mrows + mslabs


def a_cov(N, D):
    _, _, _, per, slabs = cov_plan(N, D)
    return 32 * per + slabs


def a_dd(D):
    blocks = min(cdiv(D * D, 256), 64)
    return cdiv(D * D, 256 * blocks) + 9 + cdiv(blocks, 256) + 9


def a_p(D):
    return 32 * cdiv(D, 32)


def rows_depth(N):
    """The sum over the rows in the order of msn_pair_alignment: a thread's rows, 6 + 3 in the workgroup, the finishing thread's
    partials, 6 + 3 again."""
    blocks = min(cdiv(N, 256), 1024)
    return cdiv(N, 256 * blocks) + 9 + cdiv(blocks, 256) + 9


# ----------------------------------------------------------------------------------------------------------- the inputs
def _unit(n, d, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d))
    return X / np.linalg.norm(X, axis=1, keepdims=True)


def _scaled(n, d, seed, base=None):
    """Unit-norm normal rows whose even columns are scaled by 0.25 and odd columns by 4; with `base`, that set plus noise of
    relative size 0.1 with the same column scaling."""
    scale = np.where(np.arange(d) % 2 == 0, 0.25, 4.0)
    if base is None:
        return (_unit(n, d, seed) * scale).astype(np.float32)
    return (base.astype(np.float64) + 0.1 * _unit(n, d, seed) * scale).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _pair(n, d):
    X = _scaled(n, d, 11 * n + d)
    return X, _scaled(n, d, 11 * n + d + 5, base=X)


@functools.lru_cache(maxsize=None)
def _cov_ref(n, d, which=0):
    """(mean, cov) in longdouble and the derived bounds (dmean (D), E (N, D), dcov (D, D)) in float64:
        dmean_c  = (A_mean + 1) u sum_i |x_ic| / N                       the column sum's additions and the division
        E_ic     = dmean_c + u (|xc_ic| + dmean_c)                        a staged centred value: the mean's error, one subtraction
        dcov_cc' = (|Xc|^T E + E^T |Xc| + E^T E)_cc' / (N - 1) + (A_cov + 3) u (|Xc|^T |Xc|)_cc' / (N - 1)
                                                                          the factors' errors; the products, the additions, the division."""
    X = _pair(n, d)[which]
    mean, cov = _E().column_covariance_reference(X)
    Xl = X.astype(np.longdouble)
    dmean = ((a_mean(n) + 1) * U * np.abs(Xl).sum(axis=0) / n).astype(np.float64)
    aXc = np.abs(Xl - mean).astype(np.float64)
    E = dmean[None, :] + U * (aXc + dmean[None, :])
    dcov = (aXc.T @ E + E.T @ aXc + E.T @ E) / (n - 1) + (a_cov(n, d) + 3) * U * (aXc.T @ aXc) / (n - 1)
    return mean, cov, dmean, E, dcov


def _ratio(err, bound):
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    return float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err == 0, 0.0, np.inf))))


# --------------------------------------------------------------------------------------------------- covariance: exact
@pytest.mark.parametrize("n", [2, 4, 64, 128, 1024])
def test_covariance_of_integer_data_is_exact(n):
    """Integer values in [-8, 8], every row present twice, N a power of two: the column sums, the means, the centred values,
    their products and every partial sum are exact in fp64 in any order, so the only rounding is the division by N - 1."""
    E = _E()
    for d in (1, 3, 16, 17, 33, 64, 130, 256):
        rng = np.random.default_rng(1000 * n + d)
        half = rng.integers(-8, 9, size=(n // 2, d))
        X = np.concatenate([half, half], axis=0)[rng.permutation(n)].astype(np.float32)
        mean, cov = E.column_covariance(torch.from_numpy(X).cuda())
        assert mean.dtype == torch.float64 and cov.dtype == torch.float64 and mean.shape == (d,) and cov.shape == (d, d)
        X64 = X.astype(np.float64)
        want_mean = X64.sum(axis=0) / n
        Xc = X64 - want_mean
        want_cov = (Xc.T @ Xc) / (n - 1)
        assert torch.equal(mean.cpu(), torch.from_numpy(want_mean)), (n, d)
        assert torch.equal(cov.cpu(), torch.from_numpy(want_cov)), (n, d)
        assert torch.equal(cov, cov.T.contiguous()), (n, d)


# --------------------------------------------------------------------------------------------------- covariance: bound
@pytest.mark.parametrize("n,d", SHAPES)
def test_covariance_within_the_derived_bound(n, d):
    E = _E()
    worst = [0.0, 0.0]
    for which in (0, 1):
        X = _pair(n, d)[which]
        mean_ref, cov_ref, dmean, _, dcov = _cov_ref(n, d, which)
        mean, cov = E.column_covariance(torch.from_numpy(X).cuda())
        assert torch.equal(cov, cov.T.contiguous())
        em = np.abs(mean.cpu().numpy().astype(np.longdouble) - mean_ref)
        ec = np.abs(cov.cpu().numpy().astype(np.longdouble) - cov_ref)
        rm, rc = _ratio(em, MARGIN * dmean), _ratio(ec, MARGIN * dcov)
        worst = [max(worst[0], rm), max(worst[1], rc)]
    print(f"vicreg-accuracy: covariance ({n}, {d}): A_mean = {a_mean(n)}, A_cov = {a_cov(n, d)}, |mean - ref| / bound = {worst[0]:.4f}, "
          f"|cov - ref| / bound = {worst[1]:.4f}")
    assert worst[0] <= 1.0 and worst[1] <= 1.0, (n, d, worst)


def test_the_plan_cuts_the_test_shapes_into_slabs_and_tile_pairs():
    assert cov_plan(129, 64)[4] == 2 and cov_plan(300, 130)[2:] == (6, 4, 3) and cov_plan(1100, 4)[4] == 9
    assert cov_plan(2100, 256) == (64, 33, 10, 4, 17) and cov_plan(65, 33)[4] == 1
    assert cov_plan(10 ** 6, 256)[3] == cdiv(cdiv(10 ** 6, 32), 52)          # beyond 512 workgroups the slabs grow
    L = _lib().lib()
    for n, d in SHAPES + [(4096, 128), (10 ** 6, 256)]:
        _, mslabs, pairs, _, slabs = cov_plan(n, d)
        assert L.msn_column_cov_workspace_bytes(n, d) == 8 * (mslabs * d + 4096 * slabs * pairs), (n, d)
        assert L.msn_vicreg_workspace_bytes(n, d) == 8 * (min(cdiv(n, 256), 1024) + 4 * min(cdiv(d * d, 256), 64)), (n, d)


# ------------------------------------------------------------------------------------------------------------- the loss
def _tower_bounds(n, d, which, std, covc, gamma, eps):
    """What fp64 may do to one tower's terms, from the longdouble reference and the bounds of _cov_ref:
        ds_c  = dcov_cc / s_c + 2 u s_c                 s_c = sqrt(C_cc + eps): the entry's error through the root (1 / s_c covers
                                                        either sign of it), the addition and the root
        dh_c  = ds_c + u |gamma - s_c|                  one term of the hinge (the branch is the reference's: asserted below)
        dvar  = (sum_c dh_c + (A_dd + 2) u sum_c h_c) / D
        dcovt = (sum_{c != c'} (2 |C| dcov + dcov^2) + (A_dd + 3) u sum_{c != c'} C^2) / D
        dM    = kcov (dcov + 3 u |C|) off the diagonal, a_c (ds_c / s_c + 4 u) on it, a_c = std / (D (N - 1) s_c) where active
    Returns (var, covt, dvar, dcovt, |Xc|, E, M, dM)."""
    X = _pair(n, d)[which]
    mean, C, _, E, dcov = _cov_ref(n, d, which)
    C64 = C.astype(np.float64)
    s = np.sqrt(np.diag(C64) + eps)
    ds = np.diag(dcov) / s + 2 * U * s
    assert (np.abs(s - gamma) > MARGIN * ds).all(), "a column's s_c sits within the arithmetic's reach of gamma"
    h = np.maximum(gamma - s, 0.0)
    dh = ds + U * np.abs(gamma - s)
    add = a_dd(d)
    dvar = (dh.sum() + (add + 2) * U * h.sum()) / d
    offmask = ~np.eye(d, dtype=bool)
    off = np.where(offmask, C64, 0.0)
    dcovt = (np.where(offmask, 2 * np.abs(C64) * dcov + dcov ** 2, 0.0).sum() + (add + 3) * U * (off ** 2).sum()) / d
    dn = d * (n - 1.0)
    a = np.where(s < gamma, std / (dn * s), 0.0)
    M = 4 * covc / dn * off - np.diag(a)
    dM = np.where(offmask, 4 * covc / dn * (dcov + 3 * U * np.abs(C64)), 0.0) + np.diag(a * (ds / s + 4 * U))
    aXc = np.abs(X.astype(np.longdouble) - mean).astype(np.float64)
    return h.sum() / d, (off ** 2).sum() / d, dvar, dcovt, aXc, E, M, dM


def _pair_bounds(n, d, coeffs, gamma, eps, g=1.0):
    """(B_loss, B_x, B_y) of one pair:
        B_loss = sim inv (D + rows + 4) u + std (dvar_x + dvar_y) + covc (dcovt_x + dcovt_y) + 6 u (the terms' sum)
        dP_ic  = (|Xc| dM + E |M|)_ic + (A_p + 2) u (|Xc| |M|)_ic        the factors' errors; the products and the additions
        B_ic   = |g| (dP_ic + 6 u (k |x_ic - y_ic| + (|Xc| |M|)_ic))     the difference, k times it, the fma, the product with g."""
    sim, std, covc = coeffs
    X, Y = _pair(n, d)
    tx = _tower_bounds(n, d, 0, std, covc, gamma, eps)
    ty = _tower_bounds(n, d, 1, std, covc, gamma, eps)
    diff = np.abs(X.astype(np.float64) - Y.astype(np.float64))
    inv = (diff ** 2).sum() / (n * d)
    terms = sim * inv + std * (tx[0] + ty[0]) + covc * (tx[1] + ty[1])
    b_loss = sim * inv * (d + rows_depth(n) + 4) * U + std * (tx[2] + ty[2]) + covc * (tx[3] + ty[3]) + 6 * U * terms
    k = 2 * sim / (n * d)
    out = [b_loss]
    for _, _, _, _, aXc, E, M, dM in (tx, ty):
        aM = np.abs(M)
        spread = aXc @ aM
        dP = aXc @ dM + E @ aM + (a_p(d) + 2) * U * spread
        out.append(abs(g) * (dP + 6 * U * (k * diff + spread)))
    return out


@functools.lru_cache(maxsize=None)
def _ref(n, d, coeffs, gamma, eps):
    X, Y = _pair(n, d)
    return _Lo().vicreg_reference([X, Y], *coeffs, gamma, eps, return_terms=True)


def _check_pair(n, d, coeffs, gamma, eps=EPS, g=1.0, label="", precondition=False):
    Lo = _Lo()
    X, Y = _pair(n, d)
    ref, grads, terms = _ref(n, d, coeffs, gamma, eps)
    if precondition:
        for x in (X, Y):
            s = np.sqrt(np.diag(_E().column_covariance_reference(x)[1]).astype(np.float64) + eps)
            assert np.abs(s - gamma).min() >= 0.01 * gamma, (n, d)
            if d >= 2:
                assert (s < gamma).any() and (s > gamma).any(), "both branches of the hinge are to be taken"
    e1 = torch.from_numpy(X).cuda().requires_grad_(True)
    e2 = torch.from_numpy(Y).cuda().requires_grad_(True)
    loss, comps = Lo.vicreg_loss_multimodal([e1, e2], *coeffs, gamma, eps, return_components=True)
    assert loss.dtype == torch.float32 and loss.dim() == 0
    assert len(comps) == 1 and comps[0].dtype == torch.float64 and comps[0].shape == (5,)
    (loss * g).backward()
    b_loss, b_x, b_y = _pair_bounds(n, d, coeffs, gamma, eps, g)
    bound = 2.0 ** -24 * abs(float(ref)) + MARGIN * b_loss + 2.0 ** -149
    err = abs(float(np.longdouble(float(loss.detach())) - ref))
    r_loss = err / bound
    # the components against the reference's terms, each within its part of the fp64 bound (the whole of it: simpler, and wider)
    c = comps[0].cpu().numpy()
    want = [terms["inv"][(0, 1)], terms["var"][0], terms["var"][1], terms["cov"][0], terms["cov"][1]]
    tx = _tower_bounds(n, d, 0, coeffs[1], coeffs[2], gamma, eps)
    ty = _tower_bounds(n, d, 1, coeffs[1], coeffs[2], gamma, eps)
    cb = [float(want[0]) * (d + rows_depth(n) + 4) * U, tx[2], ty[2], tx[3], ty[3]]
    for k in range(5):
        assert abs(float(np.longdouble(c[k]) - want[k])) <= MARGIN * cb[k] + 2 * U * abs(float(want[k])), (label, k, c[k], float(want[k]))
    worst = 0.0
    for got, w, b in ((e1.grad, grads[0], b_x), (e2.grad, grads[1], b_y)):
        assert got.dtype == torch.float32 and got.shape == X.shape
        w = g * w
        bnd = 2.0 ** -24 * np.abs(w.astype(np.float64)) + MARGIN * b + 2.0 ** -149
        e = np.abs(got.cpu().numpy().astype(np.longdouble) - w).astype(np.float64)
        worst = max(worst, _ratio(e, bnd))
    print(f"vicreg-accuracy: loss {label} coefficients {coeffs} gamma = {gamma:.4g} g = {g}: L = {float(ref):.6f}, "
          f"|L - ref| / bound = {r_loss:.4f}, worst |dX - ref| / bound = {worst:.4f}")
    assert err <= bound, (label, float(loss), float(ref))
    assert worst <= 1.0, (label, coeffs, gamma, worst)
    return loss, comps[0], e1.grad, e2.grad


@pytest.mark.parametrize("n,d", SHAPES)
def test_loss_and_gradient_against_the_reference(n, d):
    """gamma = 1 / sqrt(D): the columns scaled by 0.25 lie below it, those scaled by 4 above -- both branches of the hinge."""
    gamma = 1.0 / math.sqrt(d)
    _check_pair(n, d, (25.0, 25.0, 1.0), gamma, label=f"({n}, {d})", precondition=True)
    if (n, d) == ONCE:
        return
    for coeffs in ((0.0, 25.0, 1.0), (25.0, 0.0, 1.0), (25.0, 25.0, 0.0)):
        _check_pair(n, d, coeffs, gamma, label=f"({n}, {d})")
    # the hinge never active: the variance term is exactly 0 and M has an empty diagonal; always active
    _, comp, _, _ = _check_pair(n, d, (25.0, 25.0, 1.0), 0.0, label=f"({n}, {d})")
    assert float(comp[1]) == 0.0 and float(comp[2]) == 0.0
    _check_pair(n, d, (25.0, 25.0, 1.0), 10.0, label=f"({n}, {d})")
    if d == 1:
        assert float(comp[3]) == 0.0 and float(comp[4]) == 0.0           # one column: no covariance term


def test_an_upstream_gradient_scales_the_result():
    _check_pair(130, 128, (25.0, 25.0, 1.0), 1.0 / math.sqrt(128), g=-3.5, label="(130, 128)")
    _check_pair(65, 33, (25.0, 25.0, 1.0), 1.0 / math.sqrt(33), g=0.125, label="(65, 33)")


def test_three_towers_against_the_reference():
    """Each pair's loss is rounded to fp32 and the three are added in fp32; each tower's gradient is the fp32 sum of the
    gradients of its two pairs, each within the pair's own bound: 2^-24 of every partial figure and of the sum, and the fp64
    bounds of both pairs."""
    Lo = _Lo()
    n, d = 65, 33
    coeffs, gamma = (25.0, 25.0, 1.0), 1.0 / math.sqrt(d)
    X, Y = _pair(n, d)
    Xs = [X, Y, _scaled(n, d, 99, base=X)]
    embs = [torch.from_numpy(x).cuda().requires_grad_(True) for x in Xs]
    loss, comps = Lo.vicreg_loss_multimodal(embs, *coeffs, gamma, EPS, return_components=True)
    loss.backward()
    ref, grads, terms = Lo.vicreg_reference(Xs, *coeffs, gamma, EPS, return_terms=True)
    order = ((0, 1), (0, 2), (1, 2))
    pair_refs = {p: Lo.vicreg_reference([Xs[p[0]], Xs[p[1]]], *coeffs, gamma, EPS) for p in order}
    assert len(comps) == 3 and all(c.dtype == torch.float64 and c.shape == (5,) for c in comps)
    for (i, j), c in zip(order, comps):
        c = c.cpu().numpy()
        want = [terms["inv"][(i, j)], terms["var"][i], terms["var"][j], terms["cov"][i], terms["cov"][j]]
        for k in range(5):
            assert abs(c[k] - float(want[k])) <= 1e-12 * max(abs(float(want[k])), 1e-3), (i, j, k)
        got = coeffs[0] * c[0] + coeffs[1] * (c[1] + c[2]) + coeffs[2] * (c[3] + c[4])
        assert abs(got - float(pair_refs[(i, j)][0])) <= 1e-12 * abs(float(pair_refs[(i, j)][0]))
    sum_abs = sum(abs(float(v[0])) for v in pair_refs.values())
    assert abs(float(np.longdouble(float(loss.detach())) - ref)) <= 2.0 ** -24 * (3 * sum_abs + abs(float(ref))) + 1e-12 * sum_abs
    # fp64 part: the pair (0, 1) is the cached case; the other pairs' bounds have its size (the same rows plus the same noise),
    # and all of it lies six orders below the fp32 part: three times the cached pair's covers the two pairs of a tower
    _, b_x, b_y = _pair_bounds(n, d, coeffs, gamma, EPS)
    fp64 = 3 * np.maximum(b_x, b_y).max()
    for k in range(3):
        parts = [np.abs(pair_refs[p][1][p.index(k)].astype(np.float64)) for p in order if k in p]
        b = 2.0 ** -24 * (sum(parts) + np.abs(grads[k].astype(np.float64))) + MARGIN * fp64 + 2.0 ** -149
        e = np.abs(embs[k].grad.cpu().numpy().astype(np.longdouble) - grads[k]).astype(np.float64)
        ratio = _ratio(e, b)
        print(f"vicreg-accuracy: three towers, tower {k}: worst |dX - ref| / bound = {ratio:.4f}")
        assert ratio <= 1.0, (k, ratio)


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


def _raw(X, Y, coeffs, gamma, eps, g, pad=0, extra=5):
    """The whole pipeline through the C-ABI with every output and workspace poisoned with NaN before its launch; dX and dY carry
    `extra` sentinel rows past N and row stride D + pad."""
    L = _lib()
    lib, p, s = L.lib(), L.ptr, L.stream_ptr()
    n, d = X.shape
    nan = float("nan")
    f64 = dict(dtype=torch.float64, device="cuda")
    stats = []
    for A in (X, Y):
        mean, cov = torch.full((d,), nan, **f64), torch.full((d, d), nan, **f64)
        ws = torch.full((lib.msn_column_cov_workspace_bytes(n, d) // 8,), nan, **f64)
        assert lib.msn_column_cov(p(A), A.stride(0), n, d, p(mean), p(cov), p(ws), ws.numel() * 8, s) == 0
        stats.append((mean, cov))
    loss, comp = torch.full((), nan, device="cuda"), torch.full((5,), nan, **f64)
    Mx, My = torch.full((d, d), nan, **f64), torch.full((d, d), nan, **f64)
    ws = torch.full((lib.msn_vicreg_workspace_bytes(n, d) // 8,), nan, **f64)
    assert lib.msn_vicreg_fwd(p(X), X.stride(0), p(Y), Y.stride(0), n, d, p(stats[0][1]), p(stats[1][1]), *coeffs, gamma, eps, p(loss),
                              p(comp), p(Mx), p(My), p(ws), ws.numel() * 8, s) == 0
    gt = torch.tensor(g, dtype=torch.float32, device="cuda")
    dX = torch.full((n + extra, d + pad), -7.0, device="cuda")
    dY = torch.full((n + extra, d + pad), -7.0, device="cuda")
    assert lib.msn_vicreg_bwd(p(X), X.stride(0), p(Y), Y.stride(0), n, d, p(stats[0][0]), p(stats[1][0]), p(Mx), p(My), p(gt),
                              coeffs[0], p(dX), d + pad, p(dY), d + pad, s) == 0
    return stats[0] + stats[1] + (loss, comp, Mx, My, dX, dY)


@pytest.mark.parametrize("n,d", STRUCTURE)
def test_poisoned_buffers_sentinel_rows_and_the_same_bits_for_every_stride_and_alignment(n, d):
    Lo = _Lo()
    Xn, Yn = _pair(n, d)
    X, Y = torch.from_numpy(Xn).cuda(), torch.from_numpy(Yn).cuda()
    coeffs, gamma = (25.0, 25.0, 1.0), 1.0 / math.sqrt(d)
    first = _raw(X, Y, coeffs, gamma, EPS, -1.5)
    for t in first[:8]:
        assert bool(torch.isfinite(t).all())                  # nothing of the poison is left, nothing poisoned was added up
    for dA in first[8:]:
        assert bool((dA[n:] == -7.0).all()) and bool(torch.isfinite(dA[:n]).all())
    runs = [_raw(X, Y, coeffs, gamma, EPS, -1.5), _raw(_strided(X, 3, 1), _strided(Y, 7, 3), coeffs, gamma, EPS, -1.5, pad=3, extra=2)]
    for again in runs:
        for a, b in zip(first[:8], again[:8]):
            assert torch.equal(a, b)
        for a, b in zip(first[8:], again[8:]):
            assert bool((b[n:] == -7.0).all()) and bool((b[:, d:] == -7.0).all())
            assert torch.equal(a[:n, :d], b[:n, :d])
    # the autograd node gives the same bits as the raw pipeline
    e1, e2 = X.clone().requires_grad_(True), Y.clone().requires_grad_(True)
    loss = Lo.vicreg_loss(e1, e2, *coeffs, gamma, EPS)
    (loss * -1.5).backward()
    assert torch.equal(loss.detach(), first[4]) and torch.equal(e1.grad, first[8][:n, :d]) and torch.equal(e2.grad, first[9][:n, :d])
    # column_covariance into given outputs, from strided rows
    mean, cov = torch.full((d,), float("nan"), dtype=torch.float64).cuda(), torch.full((d, d), float("nan"), dtype=torch.float64).cuda()
    got = _E().column_covariance(_strided(X, 5, 1), out=(mean, cov))
    assert got[0] is mean and got[1] is cov and torch.equal(mean, first[0]) and torch.equal(cov, first[1])


def test_non_finite_inputs_propagate():
    Xn, Yn = _pair(65, 33)
    X, Y = torch.from_numpy(Xn.copy()).cuda(), torch.from_numpy(Yn).cuda()
    X[7, 5] = float("nan")
    e1, e2 = X.requires_grad_(True), Y.clone().requires_grad_(True)
    loss = _Lo().vicreg_loss(e1, e2, 25.0, 25.0, 1.0, 1.0 / math.sqrt(33), EPS)
    loss.backward()
    assert math.isnan(float(loss.detach())) and bool(torch.isnan(e1.grad[7, 5])) and bool(torch.isnan(e1.grad[:, 5]).all())


# ----------------------------------------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing(monkeypatch):
    E, Lo, L = _E(), _Lo(), _lib()
    X = torch.from_numpy(_scaled(8, 4, 1)).cuda()
    wide = torch.zeros(4, 257).cuda()
    for call, what in [(lambda: E.column_covariance(wide), r"D must be in 1\.\.256"),
                       (lambda: E.column_covariance(X[:1]), "N must be at least 2"),
                       (lambda: E.column_covariance(X.cpu()), "must live on the GPU"),
                       (lambda: Lo.vicreg_loss(wide, wide), r"D must be in 1\.\.256"),
                       (lambda: Lo.vicreg_loss(X[:1], X[:1]), "N must be at least 2"),
                       (lambda: Lo.vicreg_loss(X.cpu(), X.cpu()), "must live on the GPU"),
                       (lambda: Lo.vicreg_loss(X, X.cpu()), "must live on the GPU")]:
        with pytest.raises(L.MsnHipError, match=what):
            call()
    for call, what in [(lambda: Lo.vicreg_loss(X, X, sim_coeff=-1.0), "sim_coeff"),
                       (lambda: Lo.vicreg_loss(X, X, std_coeff=float("inf")), "std_coeff"),
                       (lambda: Lo.vicreg_loss(X, X, cov_coeff=float("nan")), "cov_coeff"),
                       (lambda: Lo.vicreg_loss(X, X, gamma=-1.0), "gamma"),
                       (lambda: Lo.vicreg_loss(X, X, gamma=float("nan")), "gamma"),
                       (lambda: Lo.vicreg_loss(X, X, eps=0.0), "eps"),
                       (lambda: Lo.vicreg_loss(X, X, eps=float("inf")), "eps"),
                       (lambda: Lo.vicreg_loss(X, X[:7]), "one shape"),
                       (lambda: Lo.vicreg_loss_multimodal([X]), "at least two")]:
        with pytest.raises(ValueError, match=what):
            call()
    # the C-ABI itself: MSN_ERR_SHAPE (1) and nothing enqueued
    lib = L.lib()
    f64 = dict(dtype=torch.float64, device="cuda")
    mean, cov, M = torch.zeros(4, **f64), torch.zeros(4, 4, **f64), torch.zeros(4, 4, **f64)
    loss, comp = torch.zeros((), device="cuda"), torch.zeros(5, **f64)
    dX = torch.zeros(8, 4, device="cuda")
    ws = torch.zeros(1 << 16, dtype=torch.uint8).cuda()
    p, s = L.ptr, L.stream_ptr()
    assert lib.msn_column_cov(p(X), 4, 8, 4, p(mean), p(cov), p(ws), 8, s) == 1                              # workspace too small
    assert lib.msn_column_cov(p(X), 4, 1, 4, p(mean), p(cov), p(ws), ws.numel(), s) == 1
    assert lib.msn_column_cov(p(X), 3, 8, 4, p(mean), p(cov), p(ws), ws.numel(), s) == 1
    assert lib.msn_column_cov(p(X), 4, 8, 0, p(mean), p(cov), p(ws), ws.numel(), s) == 1
    assert lib.msn_column_cov(p(X), 4, 8, 4, None, p(cov), p(ws), ws.numel(), s) == 1

    def fwd(n=8, sim=25.0, gamma=1.0, eps=1e-4, nb=ws.numel(), comp_=comp):
        return lib.msn_vicreg_fwd(p(X), 4, p(X), 4, n, 4, p(cov), p(cov), sim, 25.0, 1.0, gamma, eps, p(loss), p(comp_), p(M), p(M), p(ws), nb, s)

    assert fwd(n=1) == 1 and fwd(sim=-1.0) == 1 and fwd(gamma=float("nan")) == 1 and fwd(eps=0.0) == 1 and fwd(nb=8) == 1
    assert fwd(comp_=None) == 1
    assert lib.msn_vicreg_bwd(p(X), 4, p(X), 4, 8, 4, p(mean), p(mean), p(M), p(M), p(loss), float("inf"), p(dX), 4, p(dX), 4, s) == 1
    assert lib.msn_vicreg_bwd(p(X), 4, p(X), 4, 8, 4, p(mean), p(mean), p(M), p(M), p(loss), 25.0, p(dX), 3, p(dX), 4, s) == 1
    assert lib.msn_vicreg_bwd(p(X), 4, p(X), 4, 8, 4, p(mean), p(mean), p(M), p(M), None, 25.0, p(dX), 4, p(dX), 4, s) == 1
    assert lib.msn_column_cov_workspace_bytes(8, 257) == 0 and lib.msn_vicreg_workspace_bytes(1, 4) == 0
    torch.cuda.synchronize()
    for t in (mean, cov, M, comp, dX):
        assert float(t.abs().sum()) == 0.0
    assert float(loss) == 0.0
    # sharded: statistics over gathered rows are not built
    monkeypatch.setattr(Lo, "_is_sharded", lambda global_negatives, group: bool(global_negatives))
    with pytest.raises(NotImplementedError, match="global_negatives=False"):
        Lo.vicreg_loss(X, X)
    assert Lo.vicreg_loss(X, X.flip(0), global_negatives=False).dim() == 0


# ------------------------------------------------------------------------------------------------------------ the model
TK = dict(n_out=16, emb=16, heads=2, depth=1, dropout=0.0, time_norm=20583.37, agg="mean")
SK = dict(n_out=16, emb=16, heads=2, depth=1, dropout=0.0, time_norm=17945.14, agg="mean")


def _clip(loss="vicreg", **kw):
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
    model = _clip(loss_kwargs={"sim_coeff": 25.0, "std_coeff": 25.0, "cov_coeff": 1.0})
    assert model.loss_kwargs["gamma"] == 1.0 / math.sqrt(32)
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
    tests/test_align_uniform_gpu.py for the same model)."""
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


def test_the_softmax_objective_is_what_it_was():
    """loss="softmax" still launches clip_loss_multimodal on the model's embeddings with its two trainable scalars: the same
    bits as the free function gives, and gradients for both scalars."""
    from multimodal_supernovae_amd.loss import clip_loss_multimodal
    model = _clip(loss="softmax")
    batch = _batch(torch.Generator().manual_seed(8), 16)
    loss = model.training_step(batch, 0)
    with torch.no_grad():
        want = clip_loss_multimodal(model(*batch), model.logit_scale, model.logit_bias)
    assert torch.equal(loss.detach(), want)
    loss.backward()
    assert model.logit_scale.grad is not None and model.logit_bias.grad is not None
    assert list(model.state_dict()) == list(_clip().state_dict())
