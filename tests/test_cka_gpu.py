"""Centred kernel alignment on the GPU (csrc/cka.hip): the sixteen sums of embedding_metrics.hsic_sums exactly on integer data and
within bounds derived from the addition depths of include/msn_hip.h, cka / CKA / cka_matrix / EmbeddingMetrics(cka=True) against
the longdouble references within the bounds carried through the formulas, the structure (poisoned output and workspace, rows
past N, the same bits for every run, stride and alignment, non-finite inputs) and the refusals.

Every bound comes from the arithmetic, with MARGIN = 2 over the first-order derivation (as tests/test_barlow_gpu.py uses it);
none is tuned to what was measured.  Lines that start with "cka-accuracy:" carry the measured worst ratio to each bound
(profiles/cka_accuracy.txt)."""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -53            # unit roundoff of fp64
MARGIN = 2
NS = [2, 3, 4, 5, 63, 64, 65, 129, 200]
DS = [(1, 1), (3, 1), (31, 33), (32, 64), (100, 7), (256, 256), (1024, 36)]
SLABS = (1030, 33, 7)     # T = 17 tile rows, per = 2: nine slabs, the last of one tile
FAMILIES = ["unit", "offset", "same", "indep", "const"]
SETTINGS = [("linear", False), ("rbf", False), ("rbf", True)]       # (kernel, explicit bandwidth)
NAMES = ("KL", "KK", "LL", "rKL", "rKK", "rLL", "sK", "sL")


def _E():
    from multimodal_supernovae_amd import embedding_metrics
    return embedding_metrics


def _lib():
    from multimodal_supernovae_amd import _lib as L
    return L


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------- the plan and the depths of the header
def hsic_plan(N):
    """(mrows, mslabs, nparts, T, per, slabs) of msn_hsic_sums (include/msn_hip.h)."""
    mrows = max(64, cdiv(N, 64))
    T = cdiv(N, 64)
    per = max(2, cdiv(T, cdiv(1024, T)))
    return mrows, cdiv(N, mrows), cdiv(N, 256), T, per, cdiv(T, per)


def depths(N):
    mrows, mslabs, nparts, T, per, slabs = hsic_plan(N)
    return dict(mean=mrows + mslabs, sigma=9 + cdiv(nparts, 256) + 9, row=2 + 4 + per + 1 + slabs + 1,
                scalar=16 * per + 9 + cdiv(T * slabs, 256) + 9 + 1, finish=cdiv(N, 256) + 9)


def a_norm(D):
    return D


def a_dot(D):
    return 32 * cdiv(D, 32)


def test_the_plan_cuts_the_test_shapes_into_slabs_with_a_ragged_last_one():
    assert hsic_plan(SLABS[0])[3:] == (17, 2, 9) and 17 % 2 == 1
    assert hsic_plan(200)[3:] == (4, 2, 2) and hsic_plan(129)[3:] == (3, 2, 2) and hsic_plan(64)[3:] == (1, 2, 1)
    assert hsic_plan(4096)[3:] == (64, 4, 16) and hsic_plan(8192)[3:] == (128, 16, 8)
    assert hsic_plan(10 ** 6)[4:] == (15625, 1) and hsic_plan(5000)[:3] == (79, 64, 20)
    L = _lib().lib()
    for n, dx, dy in [(n, *d) for n in NS for d in DS] + [SLABS, (4096, 128, 128), (10 ** 6, 1024, 1)]:
        _, mslabs, nparts, T, _, slabs = hsic_plan(n)
        assert L.msn_hsic_workspace_bytes(n, dx, dy) == 8 * (mslabs * (dx + dy) + dx + dy + 2 * n + 2 * nparts + 2 + 2 * slabs * n
                                                            + 3 * T * slabs), (n, dx, dy)


# ----------------------------------------------------------------------------------------------------------- the inputs
def _unit(n, d, rng):
    X = rng.standard_normal((n, d))
    return X / np.linalg.norm(X, axis=1, keepdims=True)


@functools.lru_cache(maxsize=None)
def _pair(family, n, dx, dy):
    """unit    unit-norm rows; Y shares its first columns with X, plus noise
       offset  a common offset of 100 times the spread in X, of -40 times in Y: what the centring is for
       same    Y = X (its columns repeated or cut where the widths differ)
       indep   independent normal sets
       const   "unit" with one constant column in X (the only column when Dx = 1: a set of equal rows)"""
    rng = np.random.default_rng(7 * n + 131 * dx + dy)
    k = min(dx, dy)
    if family in ("unit", "const"):
        X, Y = _unit(n, dx, rng), 0.3 * _unit(n, dy, rng)
        Y[:, :k] += X[:, :k]
        Y /= np.linalg.norm(Y, axis=1, keepdims=True)
        if family == "const":
            X[:, min(1, dx - 1)] = 0.75
    elif family == "offset":
        X = rng.standard_normal((n, dx))
        Y = 0.5 * rng.standard_normal((n, dy))
        Y[:, :k] += 0.5 * X[:, :k]
        X, Y = X + 100.0, Y - 40.0
    elif family == "same":
        X = rng.standard_normal((n, dx))
        Y = X[:, np.arange(dy) % dx]
    else:
        X, Y = rng.standard_normal((n, dx)), rng.standard_normal((n, dy))
    return np.ascontiguousarray(X, dtype=np.float32), np.ascontiguousarray(Y, dtype=np.float32)


def _explicit_sigma(X, Y):
    """A bandwidth per set near 0.7 of the root mean squared distance, as a Python float both sides receive."""
    out = []
    for Z in (X, Y):
        Zc = Z.astype(np.float64) - Z.astype(np.float64).mean(axis=0)
        out.append(float(0.7 * np.sqrt(max(2.0 * (Zc * Zc).sum() / (len(Z) - 1), 1e-3))))
    return tuple(out)


# ----------------------------------------------------------------------------------------------------------- the bounds
def _kernel_bound(Z, kernel, sigma, scale, A):
    """(K, dK): one set's kernel matrix with its diagonal and what fp64 may do to each entry on the kernels' way, first order,
    from the depths of the header (float64 arrays: a bound needs its magnitudes to a few digits only; u = 2^-53):
        dmean_c = (A_mean + 1) u sum_i |z_ic| / N                         the column sum's additions and the division
        E_ic    = dmean_c + u (|zc_ic| + dmean_c)                          a centred value: the mean's error, one subtraction
        dn_i    = sum_c (2 |zc_ic| E_ic + E_ic^2) + (A_norm + 1) u n_i     the norm: the factors' errors; the fma chain
        dg_ij   = sum_c (|zc_ic| E_jc + E_ic |zc_jc| + E_ic E_jc) + (A_dot + 1) u sum_c |zc_ic zc_jc|     the dot product
      linear:  K_ij = g_ij, dK_ij = dg_ij;  K_ii = n_i, dK_ii = dn_i
      RBF:     v = (n_i + n_j) - 2 g:  dv = dn_i + dn_j + 2 dg + 3 u (n_i + n_j + 2 |g|);  max(0, .) moves nothing further
               inv = 1 / (2 sigma^2): relative error 3 u for an explicit sigma (the square, the doubling, the quotient);
                 derived, S = sum_i n_i: dS = sum_i dn_i + A_sigma u S, relative error dS / S + 6 u
               e = d2 inv:  de = dv inv + e (rel + u);   K = exp(-e), the device's exp within 1 ulp = 2 u:
               dK = K (expm1(de) + 2 u);   K_ii = 1 exactly"""
    n, D = Z.shape
    Zd = Z.astype(np.float64)
    Zc = Zd - Zd.sum(axis=0) / n
    a = np.abs(Zc)
    dmean = (A["mean"] + 1) * U * np.abs(Zd).sum(axis=0) / n
    Er = dmean[None, :] + U * (a + dmean[None, :])
    nrm = (Zc * Zc).sum(axis=1)
    dn = (2 * a * Er + Er * Er).sum(axis=1) + (a_norm(D) + 1) * U * nrm
    G = Zc @ Zc.T
    cross = a @ Er.T
    dG = cross + cross.T + Er @ Er.T + (a_dot(D) + 1) * U * (a @ a.T)
    if kernel == "linear":
        np.fill_diagonal(G, nrm)
        np.fill_diagonal(dG, dn)
        return G, dG
    pair = nrm[:, None] + nrm[None, :]
    d2 = np.maximum(pair - 2 * G, 0.0)
    dv = dn[:, None] + dn[None, :] + 2 * dG + 3 * U * (pair + 2 * np.abs(G))
    with np.errstate(invalid="ignore", divide="ignore"):
        if sigma is None:
            S = nrm.sum()
            s2, rel = scale * scale * 2 * S / (n - 1), (dn.sum() + A["sigma"] * U * S) / S + 6 * U
        else:
            s2, rel = sigma * sigma, 3 * U
        inv = 1 / (2 * s2)
        e = d2 * inv
        K = np.exp(-e)
        dK = K * (np.expm1(dv * inv + e * (rel + U)) + 2 * U)
    np.fill_diagonal(K, 1.0)
    np.fill_diagonal(dK, 0.0)
    return K, dK


def _sum_bounds(K, dK, L, dL, A):
    """(2, 8) bounds of the sums from the entries' bounds:
        P = sum A_ij B_ij:  sum (|A| dB + dA |B| + dA dB) + (A_scalar + 1) u sum_{i != j} |A B|, with the diagonal also
                            (A_finish + 2) u sum_i |A_ii B_ii|  (its own chain, one fma each, the final addition)
        r_i = sum_j A_ij:   dr_i = sum_j dA_ij + (A_row - 1 + c) u sum_j |A_ij|      (c = 1: the addition of the diagonal)
        R = sum_i r_i r'_i: sum (|r| dr' + dr |r'| + dr dr') + (A_finish + 1) u sum |r r'|;   S = sum_i r_i: sum dr + A_finish u sum |r|"""
    n = K.shape[0]
    eye = np.eye(n, dtype=bool)
    out = np.zeros((2, 8))
    for c in (0, 1):
        M = [np.where(eye, 0.0, m) if c == 0 else m for m in (K, dK, L, dL)]

        def prod(a, da, b, db):
            ab = np.abs(a * b)
            bound = (np.abs(a) * db + da * np.abs(b) + da * db).sum() + (A["scalar"] + 1) * U * ab[~eye].sum()
            return bound + ((A["finish"] + 2) * U * ab[eye].sum() if c else 0.0)

        def rows(a, da):
            return a.sum(axis=1), da.sum(axis=1) + (A["row"] - 1 + c) * U * np.abs(a).sum(axis=1)

        def rowprod(r, dr, s, ds):
            return (np.abs(r) * ds + dr * np.abs(s) + dr * ds).sum() + (A["finish"] + 1) * U * np.abs(r * s).sum()

        (rk, drk), (rl, drl) = rows(M[0], M[1]), rows(M[2], M[3])
        out[c] = [prod(*M), prod(M[0], M[1], M[0], M[1]), prod(M[2], M[3], M[2], M[3]), rowprod(rk, drk, rl, drl),
                  rowprod(rk, drk, rk, drk), rowprod(rl, drl, rl, drl), drk.sum() + A["finish"] * U * np.abs(rk).sum(),
                  drl.sum() + A["finish"] * U * np.abs(rl).sum()]
    return out


_PAIRS = {"KL": (0, 3, 6, 7), "KK": (1, 4, 6, 6), "LL": (2, 5, 7, 7)}


def _hsic_bound(s, B, n, pair, debiased):
    """What the sums' bounds B and the host's fp64 (six roundings of the three terms) may do to hsic_from_sums."""
    ip, ir, ia, ib = _PAIRS[pair]
    c = 0 if debiased else 1
    P, R, Sa, Sb = (abs(float(s[c, k])) for k in (ip, ir, ia, ib))
    bP, bR, ba, bb = (B[c, k] for k in (ip, ir, ia, ib))
    ss, bss = Sa * Sb, Sa * bb + ba * Sb + ba * bb
    if debiased:
        f_r, f_s, div = 2.0 / (n - 2), 1.0 / ((n - 1) * (n - 2)), n * (n - 3)
    else:
        f_r, f_s, div = 2.0 / n, 1.0 / (n * n), (n - 1) * (n - 1)
    return (bP + f_r * bR + f_s * bss + 6 * U * (P + f_r * R + f_s * ss)) / div


def _cka_bound(hs, dhs):
    """CKA = h_kl / sqrt(h_kk h_ll) over the intervals h +- dh; None where a denominator's interval reaches zero (the quotient
    is not determined there)."""
    (kl, kk, ll), (dkl, dkk, dll) = (tuple(float(v) for v in hs), dhs)
    lo_k, lo_l = kk - dkk, ll - dll
    if not (lo_k > 0 and lo_l > 0):
        return None
    den, den_lo = math.sqrt(kk * ll), math.sqrt(lo_k * lo_l)
    return dkl / den_lo + abs(kl) * (1 / den_lo - 1 / den) + 8 * U * abs(kl) / den


def _derive(X, Y, kernel, sigma, scale=1.0):
    E = _E()
    n = len(X)
    A = depths(n)
    sx, sy = sigma if sigma is not None else (None, None)
    ref = E.hsic_sums_reference(X, Y, kernel, sigma, scale)
    bounds = MARGIN * _sum_bounds(*_kernel_bound(X, kernel, sx, scale, A), *_kernel_bound(Y, kernel, sy, scale, A), A)
    return ref, bounds


@functools.lru_cache(maxsize=None)
def _derived(family, n, dx, dy, kernel, explicit):
    X, Y = _pair(family, n, dx, dy)
    return _derive(X, Y, kernel, _explicit_sigma(X, Y) if explicit else None)


def _cka_figures(ref, bounds, n, debiased):
    """(the reference CKA through the longdouble formulas, its bound or None)."""
    E = _E()
    hs = [E.hsic_from_sums(ref, n, p, debiased) for p in ("KL", "KK", "LL")]
    want = E.cka_from_sums(ref, n, debiased)
    if not all(np.isfinite(float(h)) for h in hs):
        return want, None
    return want, _cka_bound(hs, [_hsic_bound(ref, bounds, n, p, debiased) for p in ("KL", "KK", "LL")])


WORST = {}


def _note(key, value):
    WORST[key] = max(WORST.get(key, 0.0), value)
    return value


def _sum_ratios(got, ref, bounds):
    """error / bound per sum; a sum the reference has as nan must be nan, one it has finite must be finite."""
    got = np.asarray(got, dtype=np.float64)
    out = np.zeros((2, 8))
    for idx in np.ndindex(2, 8):
        r = ref[idx]
        if np.isnan(r):
            out[idx] = 0.0 if np.isnan(got[idx]) else np.inf
        else:
            err = abs(float(np.longdouble(got[idx]) - r)) if np.isfinite(got[idx]) else np.inf
            out[idx] = 0.0 if err == 0 else (err / bounds[idx] if bounds[idx] > 0 else np.inf)
    return out


def _check(X, Y, kernel, sigma, ref, bounds, label, unit):
    E = _E()
    n = len(X)
    Xg, Yg = torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda()
    sums = E.hsic_sums(Xg, Yg, kernel, sigma)
    assert sums.dtype == torch.float64 and sums.shape == (2, 8)
    got = sums.cpu().numpy()
    ratios = _sum_ratios(got, ref, bounds)
    line = ", ".join(f"{name} {max(ratios[0, k], ratios[1, k]):.4f}" for k, name in enumerate(NAMES))
    figures = []
    for debiased in (False, True):
        want, bound = _cka_figures(ref, bounds, n, debiased)
        value = E.cka_from_sums(got, n, debiased)
        key = "cka_debiased" if debiased else "cka"
        if debiased and n < 4:
            assert np.isnan(value) and np.isnan(want)
        elif bound is not None:
            assert np.isfinite(want)
            if unit:
                # not vacuous: depth ~1e3, cancellation ~1e3, 2^-53 put it near 1e-10
                assert bound < 1e-6, (label, key, bound)
            r = abs(value - want) / bound if np.isfinite(value) else np.inf
            figures.append((key, r, bound))
            line += f", {key} {r:.4f} (bound {bound:.1e})"
    print(f"cka-accuracy: {label}: error / bound: {line}")
    for k, name in enumerate(NAMES):
        _note(name, float(max(ratios[0, k], ratios[1, k])))
        assert ratios[0, k] <= 1.0 and ratios[1, k] <= 1.0, (label, name, ratios[:, k], got[:, k], ref[:, k], bounds[:, k])
    for key, r, bound in figures:
        _note(key, r)
        assert r <= 1.0, (label, key, r, bound)
    return sums


# ----------------------------------------------------------------------------------------------------- integers: exact
def _integer_sums(X, Y):
    """The sixteen sums of the linear kernel in int64, for integer data whose column sums are zero."""
    K, L = X @ X.T, Y @ Y.T
    out = np.zeros((2, 8), dtype=np.int64)
    eye = np.eye(len(X), dtype=np.int64)
    for c in (0, 1):
        A, B = (K * (1 - eye), L * (1 - eye)) if c == 0 else (K, L)
        ra, rb = A.sum(axis=1), B.sum(axis=1)
        out[c] = [(A * B).sum(), (A * A).sum(), (B * B).sum(), ra @ rb, ra @ ra, rb @ rb, ra.sum(), rb.sum()]
        # every sum of magnitudes stays below 2^53: each partial sum in any order is exact in fp64
        assert max((np.abs(A) * np.abs(B)).sum(), (A * A).sum(), (B * B).sum(), np.abs(ra) @ np.abs(rb), ra @ ra, rb @ rb,
                   np.abs(A).sum(), np.abs(B).sum()) < 2 ** 53
    return out


@pytest.mark.parametrize("n", [2, 5, 64, 65, 200])
def test_the_sums_of_integer_data_are_exact(n):
    """A - A[perm] of integers in -8 .. 8: the column sums are exactly zero, so the means are, the centred values are the
    integers, and every product and partial sum is an integer below 2^53: all sixteen sums equal the int64 restatement."""
    E = _E()
    for dx, dy in ((1, 1), (33, 7), (64, 64)):
        rng = np.random.default_rng(100 * n + dx)
        perm = np.roll(np.arange(n), 1)
        A, B = rng.integers(-8, 9, size=(n, dx)), rng.integers(-8, 9, size=(n, dy))
        Xi, Yi = (A - A[perm]).astype(np.int64), (B - B[perm]).astype(np.int64)
        assert not Xi.sum(axis=0).any() and not Yi.sum(axis=0).any()
        want = _integer_sums(Xi, Yi)
        got = E.hsic_sums(torch.from_numpy(Xi.astype(np.float32)).cuda(), torch.from_numpy(Yi.astype(np.float32)).cuda())
        assert torch.equal(got.cpu(), torch.from_numpy(want.astype(np.float64))), (n, dx, dy, got.cpu().numpy(), want)


# ------------------------------------------------------------------------------------------- float data: derived bounds
@pytest.mark.parametrize("dx,dy", DS)
@pytest.mark.parametrize("n", NS)
def test_sums_and_cka_within_the_derived_bounds(n, dx, dy):
    for family in FAMILIES:
        X, Y = _pair(family, n, dx, dy)
        for kernel, explicit in SETTINGS:
            sigma = _explicit_sigma(X, Y) if explicit else None
            ref, bounds = _derived(family, n, dx, dy, kernel, explicit)
            _check(X, Y, kernel, sigma, ref, bounds, f"{family} ({n}, {dx}, {dy}) {kernel}{' explicit' if explicit else ''}",
                   family == "unit")


def test_several_slabs_with_a_ragged_last_one():
    """The largest case: its longdouble references take the time, so two families carry it (the structure test below adds the
    NaN poison, the strides and the rows past N at this size)."""
    n, dx, dy = SLABS
    for family in ("unit", "offset"):
        X, Y = _pair(family, n, dx, dy)
        for kernel, explicit in SETTINGS:
            sigma = _explicit_sigma(X, Y) if explicit else None
            ref, bounds = _derived(family, n, dx, dy, kernel, explicit)
            _check(X, Y, kernel, sigma, ref, bounds, f"{family} ({n}, {dx}, {dy}) {kernel}{' explicit' if explicit else ''}",
                   family == "unit")


def test_a_sigma_scale_and_the_matrix_definitions():
    """sigma_scale reaches the derived bandwidth; cka against cka_reference (tr(KHLH) and Song et al.'s formula), which does not
    go through the sums."""
    E = _E()
    X, Y = _pair("unit", 65, 31, 33)
    Xg, Yg = torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda()
    ref, bounds = _derive(X, Y, "rbf", None, 0.5)
    got = E.hsic_sums(Xg, Yg, "rbf", sigma_scale=0.5).cpu().numpy()
    assert _sum_ratios(got, ref, bounds).max() <= 1.0
    assert not np.array_equal(got, E.hsic_sums(Xg, Yg, "rbf").cpu().numpy())
    for kernel, scale in (("linear", 1.0), ("rbf", 0.5)):
        ref, bounds = _derive(X, Y, kernel, None, scale)
        for debiased in (False, True):
            _, bound = _cka_figures(ref, bounds, 65, debiased)
            want = E.cka_reference(X, Y, kernel, debiased, None, scale)
            value = E.cka(Xg, Yg, kernel, debiased, None, scale)
            assert bound < 1e-6 and abs(value - want) <= bound + 1e-15, (kernel, debiased, value, want, bound)


def test_the_cka_class_combines_the_batches_within_the_bound():
    E = _E()
    batches = [_pair("unit", n, 100, 7) for n in (63, 129, 5)]
    for kernel in ("linear", "rbf"):
        for debiased in (True, False):
            m = E.CKA(kernel, debiased=debiased)
            hs, dhs = np.zeros(3, dtype=np.longdouble), np.zeros(3)
            for X, Y in batches:
                m.update(torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda())
                ref, bounds = _derive(X, Y, kernel, None)
                for k, p in enumerate(("KL", "KK", "LL")):
                    hs[k] += E.hsic_from_sums(ref, len(X), p, debiased)
                    dhs[k] += _hsic_bound(ref, bounds, len(X), p, debiased)
            dhs += 3 * U * np.abs(hs.astype(np.float64))                                  # the host's additions over the batches
            bound = _cka_bound(hs, list(dhs))
            want = float(hs[0] / np.sqrt(hs[1] * hs[2]))
            value = m.compute()
            r = abs(value - want) / bound
            print(f"cka-accuracy: CKA class {kernel} debiased={debiased}: error / bound {r:.4f} (bound {bound:.1e})")
            assert bound < 1e-6 and _note("cka_class", r) <= 1.0, (kernel, debiased, value, want, bound)


def test_zz_the_worst_ratios_of_this_run():
    """Printed last: the worst measured error / bound per quantity over the tests above that ran in this process."""
    assert callable(_E().hsic_sums)
    print("cka-accuracy: worst error / bound over this run: " + ", ".join(f"{k} {v:.4f}" for k, v in sorted(WORST.items())))
    assert all(v <= 1.0 for v in WORST.values())


# ----------------------------------------------------------------------------------------------------------- structure
def _strided(X, pad, shift):
    """The same rows with row stride D + pad, starting `shift` floats into a buffer filled with NaN: a padded stride and a base
    misaligned by 4 bytes against the allocation."""
    n, d = X.shape
    buf = torch.full((n * (d + pad) + shift + 8,), float("nan"), device=X.device)
    view = buf[shift:shift + n * (d + pad)].view(n, d + pad)[:, :d]
    view.copy_(X)
    assert view.stride(0) == d + pad and view.data_ptr() % 8 == 4 * (shift % 2)
    return view


def _raw(X, Y, kernel, sigma=(0.0, 0.0), scale=1.0, n=None):
    """msn_hsic_sums through the C-ABI with the output and the workspace poisoned with NaN."""
    L = _lib()
    lib, p = L.lib(), L.ptr
    n = X.shape[0] if n is None else n
    dx, dy = X.shape[1], Y.shape[1]
    out = torch.full((2, 8), float("nan"), dtype=torch.float64, device="cuda")
    ws = torch.full((lib.msn_hsic_workspace_bytes(n, dx, dy) // 8,), float("nan"), dtype=torch.float64, device="cuda")
    assert lib.msn_hsic_sums(p(X), X.stride(0), dx, p(Y), Y.stride(0), dy, n, kernel, sigma[0], sigma[1], scale, p(out), p(ws),
                             ws.numel() * 8, L.stream_ptr()) == 0
    return out


@pytest.mark.parametrize("n,dx,dy", [(65, 31, 33), (200, 100, 7), SLABS])
def test_poisoned_buffers_rows_past_n_and_the_same_bits_for_every_stride_and_alignment(n, dx, dy):
    E = _E()
    Xn, Yn = _pair("offset", n, dx, dy)
    X, Y = torch.from_numpy(Xn).cuda(), torch.from_numpy(Yn).cuda()
    for kid, kernel in ((0, "linear"), (1, "rbf")):
        first = _raw(X, Y, kid)
        assert bool(torch.isfinite(first).all())               # nothing of the poison is left, nothing poisoned was added up
        assert torch.equal(first, E.hsic_sums(X, Y, kernel))
        assert torch.equal(first, _raw(X, Y, kid))             # a second run
        assert torch.equal(first, _raw(_strided(X, 3, 1), _strided(Y, 7, 3), kid))
        assert torch.equal(first, E.hsic_sums(_strided(X, 5, 3), _strided(Y, 2, 1), kernel))
        # NaN rows behind row N of a larger buffer are never read
        Xb = torch.full((n + 70, dx), float("nan"), device="cuda")
        Yb = torch.full((n + 70, dy), float("nan"), device="cuda")
        Xb[:n], Yb[:n] = X, Y
        assert torch.equal(first, _raw(Xb, Yb, kid, n=n))
        ref, bounds = _derived("offset", n, dx, dy, kernel, False)
        assert _sum_ratios(first.cpu().numpy(), ref, bounds).max() <= 1.0
    sig = _explicit_sigma(Xn, Yn)
    assert torch.equal(_raw(X, Y, 1, sig), E.hsic_sums(X, Y, "rbf", sig))
    assert torch.equal(_raw(X, Y, 1, (sig[0], 0.0)), E.hsic_sums(X, Y, "rbf", (sig[0], None)))     # one explicit, one derived


def test_non_finite_inputs_and_equal_rows_give_non_finite_sums_and_no_fault():
    E = _E()
    Xn, Yn = _pair("unit", 65, 31, 33)
    for bad in (float("nan"), float("inf")):
        X, Y = torch.from_numpy(Xn.copy()).cuda(), torch.from_numpy(Yn).cuda()
        X[7, 5] = bad
        for kernel in ("linear", "rbf"):
            s = E.hsic_sums(X, Y, kernel).cpu()
            assert not bool(torch.isfinite(s[:, [0, 1, 3, 4, 6]]).any()), (bad, kernel, s)
            assert bool(torch.isfinite(s[:, [2, 5, 7]]).all())                       # Y's own sums are untouched
            assert math.isnan(E.cka(X, Y, kernel)) and math.isnan(E.cka(X, Y, kernel, debiased=True))
    same = torch.full((65, 4), 2.5, device="cuda")
    Y = torch.from_numpy(Yn).cuda()
    s = E.hsic_sums(same, Y, "rbf").cpu()
    assert bool(torch.isnan(s[:, [0, 1, 3, 4, 6]]).all()) and bool(torch.isfinite(s[:, [2, 5, 7]]).all())
    assert float(E.hsic_sums(same, Y, "linear")[:, [0, 1, 3, 4, 6]].abs().sum()) == 0.0
    for kernel in ("linear", "rbf"):
        for debiased in (False, True):
            assert math.isnan(E.cka(same, Y, kernel, debiased)) and math.isnan(E.cka(Y, same, kernel, debiased))
    assert math.isnan(E.cka(Y[:3], Y[:3], debiased=True)) and abs(E.cka(Y[:3], Y[:3]) - 1.0) < 1e-12


# ----------------------------------------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing():
    E, L = _E(), _lib()
    lib, p, s = L.lib(), L.ptr, L.stream_ptr()
    X = torch.from_numpy(_pair("unit", 8, 3, 1)[0]).cuda()
    wide = torch.zeros(4, 1025, device="cuda")
    for call, what in [(lambda: E.hsic_sums(wide, X[:4]), r"must be in 1\.\.1024"), (lambda: E.hsic_sums(X[:4], wide), r"must be in 1\.\.1024"),
                       (lambda: E.hsic_sums(X[:1], X[:1]), "N must be at least 2"), (lambda: E.hsic_sums(X.cpu(), X), "must live on the GPU"),
                       (lambda: E.cka(X, X.cpu()), "must live on the GPU"), (lambda: E.CKA().update(X.cpu(), X), "must live on the GPU"),
                       (lambda: E.cka_matrix([X], [X.cpu()]), "must live on the GPU")]:
        with pytest.raises(L.MsnHipError, match=what):
            call()
    for call, what in [(lambda: E.hsic_sums(X, X[:7]), "same number of rows"), (lambda: E.hsic_sums(X, X, "poly"), "kernel"),
                       (lambda: E.hsic_sums(X, X, "rbf", sigma=-1.0), "sigma"), (lambda: E.hsic_sums(X, X, "rbf", sigma=0.0), "sigma"),
                       (lambda: E.hsic_sums(X, X, "rbf", sigma=(1.0, float("nan"))), "sigma"),
                       (lambda: E.hsic_sums(X, X, "rbf", sigma_scale=float("inf")), "sigma_scale"),
                       (lambda: E.hsic_sums(X, X, out=torch.zeros(16, dtype=torch.float64, device="cuda")), "out must be"),
                       (lambda: E.cka_matrix([X], [X[:7]]), "same 8 rows"), (lambda: E.cka_matrix([], [X]), "non-empty")]:
        with pytest.raises(ValueError, match=what):
            call()
    # the C-ABI itself: MSN_ERR_SHAPE (1) and nothing enqueued
    out = torch.zeros(2, 8, dtype=torch.float64, device="cuda")
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    nan, inf = float("nan"), float("inf")

    def call(n=8, dx=3, dy=3, ldx=3, ldy=3, kernel=1, sx=0.0, sy=0.0, scale=1.0, x=X, o=out, w=ws, nb=ws.numel()):
        return lib.msn_hsic_sums(p(x), ldx, dx, p(X), ldy, dy, n, kernel, sx, sy, scale, p(o), p(w), nb, s)

    assert call(dx=0) == 1 and call(dy=0) == 1 and call(dx=1025, ldx=1025) == 1 and call(dy=1025, ldy=1025) == 1
    assert call(n=1) == 1 and call(n=2 ** 31) == 1 and call(ldx=2) == 1 and call(ldy=2) == 1
    assert call(kernel=2) == 1 and call(kernel=-1) == 1
    assert call(sx=-1.0) == 1 and call(sy=-0.5) == 1 and call(sx=nan) == 1 and call(sy=inf) == 1
    assert call(scale=0.0) == 1 and call(scale=-1.0) == 1 and call(scale=nan) == 1 and call(scale=inf) == 1
    assert call(kernel=0, scale=0.0) == 1 and call(kernel=0, sx=-1.0) == 1           # checked for the linear kernel too
    assert call(x=None) == 1 and call(o=None) == 1 and call(w=None) == 1 and call(nb=8) == 1
    assert call(nb=lib.msn_hsic_workspace_bytes(8, 3, 3) - 1) == 1
    for n, dx, dy in ((8, 0, 3), (8, 3, 0), (8, 1025, 3), (8, 3, 1025), (1, 3, 3), (0, 3, 3), (2 ** 31, 3, 3)):
        assert lib.msn_hsic_workspace_bytes(n, dx, dy) == 0, (n, dx, dy)
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0.0 and int(ws.sum()) == 0
    assert call(nb=lib.msn_hsic_workspace_bytes(8, 3, 3)) == 0                        # and the smallest workspace is enough
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and float(out.abs().sum()) > 0


# -------------------------------------------------------------------------------------------------------- Python layer
def test_cka_matrix_is_the_pairwise_calls():
    E = _E()
    n = 65
    feats_a = [torch.from_numpy(_pair("unit", n, d, 7)[0]).cuda() for d in (31, 100)]
    feats_b = [torch.from_numpy(_pair("indep", n, 3, d)[1]).cuda() for d in (1, 33, 64)]
    feats_b[1] = feats_a[0][:, :20] + 0.1 * feats_b[1][:, :20]
    for kw in (dict(), dict(kernel="rbf", debiased=True, sigma_scale=0.5), dict(kernel="rbf", sigma=(1.0, 2.0))):
        M = E.cka_matrix(feats_a, feats_b, **kw)
        assert isinstance(M, np.ndarray) and M.shape == (2, 3) and M.dtype == np.float64
        for i, a in enumerate(feats_a):
            for j, b in enumerate(feats_b):
                assert M[i, j] == E.cka(a, b, **kw), (kw, i, j)
        assert M[0, 1] > M[0, 0]                               # the set built from feats_a[0] against an independent one


def test_embedding_metrics_adds_exactly_two_keys():
    E = _E()
    g = torch.Generator().manual_seed(3)
    batches = [(torch.randn(n, 32, generator=g).cuda(), torch.randn(n, 32, generator=g).cuda()) for n in (40, 25)]
    results = []
    for flag in (False, True):
        m = E.EmbeddingMetrics(cka=flag) if flag else E.EmbeddingMetrics()
        for a, b in batches:
            m.update(a, a + 0.5 * b)
        results.append(m.compute())
    plain, with_cka = results
    assert set(with_cka) - set(plain) == {"cka", "cka_debiased"} and set(plain) <= set(with_cka)
    assert list(with_cka)[:len(plain)] == list(plain)
    for k, v in plain.items():
        assert with_cka[k] == v or (np.isnan(v) and np.isnan(with_cka[k])), k
    A = torch.cat([E._unit_rows(a, "test") for a, _ in batches])
    B = torch.cat([E._unit_rows(a + 0.5 * b, "test") for a, b in batches])
    assert with_cka["cka"] == E.cka(A, B) and with_cka["cka_debiased"] == E.cka(A, B, debiased=True)
    assert 0.0 < with_cka["cka_debiased"] < 1.0 and 0.0 < with_cka["cka"] < 1.0
