"""The row field of csrc/uniformity_loss.hip (embedding_metrics.pair_field) and the alignment + uniformity loss built on it
(loss.align_uniform_loss, LightCurveImageCLIP(loss="align_uniform")) on the GPU: the field within a bound derived from the
arithmetic, its structure (the potential it sums to, rows it must not write, the same bits for every run, stride and
alignment), the loss and its gradients against the longdouble reference, the refusals, and the model end to end.

Lines that start with "align-uniform-accuracy:" carry the measured worst ratio to each bound
(profiles/align_uniform_accuracy.txt)."""
import copy
import functools
import gc
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TILE = 64                 # rows of a tile (kFieldTile of csrc/uniformity_loss.hip)
BLOCKS = 512              # workgroups aimed at (kFieldBlocks)
TS = (0.5, 2.0, 8.0)

# one pair of rows, a tile less a row, a tile, a tile and a row with a chunk and a column, three tiles at four chunks, four tiles at
# the widest D (the accumulator's eight chunks), 18 x 18 tiles in 18 slabs
SYMMETRIC = [(2, 1), (63, 3), (64, 32), (65, 33), (130, 128), (200, 256), (1100, 4)]
# (Nx, Ny, D, self_offset): nothing left out; the pair (i, i + 64) left out
RECT = [(70, 130, 40, -1), (64, 192, 16, 64)]


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


def field_plan(Nx, Ny):
    ti, tj = cdiv(Nx, TILE), cdiv(Ny, TILE)
    per = cdiv(tj, min(tj, cdiv(BLOCKS, ti)))
    return ti, per, cdiv(tj, per)


def addition_depth(Nx, Ny):
    """A_f(Nx, Ny) of include/msn_hip.h: 4 additions per matrix instruction, 16 instructions per column tile of a slab, then the
    slabs one after the other."""
    _, per, slabs = field_plan(Nx, Ny)
    return 64 * per + slabs


def loss_depth(N):
    """The additions of the loss's sums over the rows: a thread's rows, 6 + 3 in the workgroup, the finishing thread's
    partials, 6 + 3 again."""
    blocks = min(cdiv(N, 256), 1024)
    return cdiv(N, 256 * blocks) + 9 + cdiv(blocks, 256) + 9


def e_w(t, D, R):
    """What the rounding of d2 (D products added, three more operations) does to exp(-t d2), and two ulps for exp: the
    relative error of one w_ij, as tests/test_embedding_metrics_gpu.py derives it; R = max |x|^2 + max |y|^2."""
    return t * (D + 4) * 2.0 ** -52 * R + 2.0 ** -51


def _unit_rows(n, d, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d))
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    return (scale * X).astype(np.float32)


def _R(X, Y):
    return float((X.astype(np.float64) ** 2).sum(axis=1).max() + (Y.astype(np.float64) ** 2).sum(axis=1).max())


@functools.lru_cache(maxsize=None)
def _case(nx, ny, d, offset):
    """(X, Y): Y is X for a symmetric case."""
    X = _unit_rows(nx, d, 3 * nx + d)
    return (X, X) if ny is None else (X, _unit_rows(ny, d, 5 * ny + d + 1))


@functools.lru_cache(maxsize=None)
def _field_ref(nx, ny, d, offset, t):
    """(r, F, B) in longdouble: B_ic = sum_j w_ij (|x_ic| + |y_jc|), the scale the r x - M form cancels against."""
    X, Y = _case(nx, ny, d, offset)
    r, F = _E().pair_field_reference(X, None if Y is X else Y, t, self_offset=offset)
    Xl, Yl = np.abs(X.astype(np.longdouble)), np.abs(Y.astype(np.longdouble))
    B = np.zeros(X.shape, dtype=np.longdouble)
    for i in range(len(X)):
        w = np.exp(-np.longdouble(t) * ((X[i].astype(np.longdouble) - Y.astype(np.longdouble)) ** 2).sum(axis=1))
        if offset >= 0 and i + offset < len(Y):
            w[i + offset] = 0
        B[i] = w.sum() * Xl[i] + w @ Yl
    return r, F, B


def _field(X, Y, t, offset, **kw):
    E = _E()
    Xd = torch.from_numpy(X).cuda()
    r, F = E.pair_field(Xd, None if Y is X else torch.from_numpy(Y).cuda(), t, self_offset=offset, **kw)
    assert r.dtype == torch.float64 and F.dtype == torch.float64
    return r, F


# ------------------------------------------------------------------------------------------------------ field: accuracy
@pytest.mark.parametrize("nx,ny,d,offset", [(n, None, d, 0) for n, d in SYMMETRIC] + RECT)
def test_field_within_the_derived_bound(nx, ny, d, offset):
    """|r_i - r_ref| <= r_ref (e_w + A_f 2^-53): non-negative terms, each within e_w, added through at most A_f additions.
    |F_ic - F_ref| <= B_ic (e_w + (A_f + 2) 2^-53): r_i x_ic and M_ic each carry their sum's error at the scale of their terms,
    and the fma that joins them rounds once more (the bound allows two)."""
    X, Y = _case(nx, ny, d, offset)
    A = addition_depth(len(X), len(Y))
    R = _R(X, Y)
    worst_r = worst_f = 0.0
    for t in TS:
        r, F = _field(X, Y, t, offset)
        assert r.shape == (len(X),) and F.shape == X.shape
        r_ref, F_ref, B = _field_ref(nx, ny, d, offset, t)
        rg, Fg = r.cpu().numpy().astype(np.longdouble), F.cpu().numpy().astype(np.longdouble)
        br = r_ref * (e_w(t, d, R) + A * 2.0 ** -53)
        bf = B * (e_w(t, d, R) + (A + 2) * 2.0 ** -53)
        er, ef = np.abs(rg - r_ref), np.abs(Fg - F_ref)
        ratio_r = float(np.max(np.where(br > 0, er / np.where(br > 0, br, 1), np.where(er == 0, 0.0, np.inf))))
        ratio_f = float(np.max(np.where(bf > 0, ef / np.where(bf > 0, bf, 1), np.where(ef == 0, 0.0, np.inf))))
        print(f"align-uniform-accuracy: field ({nx}, {ny or nx}, {d}) offset {offset} t = {t}: A_f = {A}, "
              f"|r - ref| / bound = {ratio_r:.4f}, |F - ref| / bound = {ratio_f:.4f}")
        worst_r, worst_f = max(worst_r, ratio_r), max(worst_f, ratio_f)
        assert ratio_r <= 1.0, (nx, ny, d, t, ratio_r)
        assert ratio_f <= 1.0, (nx, ny, d, t, ratio_f)
    print(f"align-uniform-accuracy: field ({nx}, {ny or nx}, {d}) worst over t: r {worst_r:.4f}, F {worst_f:.4f}")


def test_the_plan_cuts_a_small_shape_into_slabs_and_row_tiles():
    ti, per, slabs = field_plan(1100, 1100)
    assert ti >= 2 and slabs >= 2
    L = _lib().lib()
    for nx, ny, d in [(1100, 1100, 4), (200, 200, 256), (64, 192, 16), (2, 2, 1), (5000, 70, 9)]:
        assert L.msn_pair_field_workspace_bytes(nx, ny, d) == 8 * field_plan(nx, ny)[2] * nx * (d + 1)


# ----------------------------------------------------------------------------------------------------- field: structure
def potential_depth(Nx, Ny, mode):
    """A(Nx, Ny, mode) of msn_pair_potential (include/msn_hip.h), as tests/test_embedding_metrics_gpu.py states it."""
    ti = cdiv(Nx, TILE)
    pairs = ti * (ti + 1) // 2 if mode == 2 else ti * cdiv(Ny, TILE)
    per = cdiv(pairs, 1024)
    return 16 * per + 9 + cdiv(cdiv(pairs, per), 256) + 9


def potential_bound(S, t, D, R, A):
    return S * (e_w(t, D, R) + A * 2.0 ** -53)



@pytest.mark.parametrize("n,d", [(2, 1), (65, 33), (200, 256), (1100, 4)])
def test_rows_sum_to_twice_the_potential(n, d):
    """sum_i r_i over Y = X without the pairs (i, i) counts every unordered pair twice: 2 pair_potential(X, 'within')[0], each
    side within its own bound (the sum over i is formed exactly here)."""
    E = _E()
    X, _ = _case(n, None, d, 0)
    R = _R(X, X)
    for t in TS:
        r, _ = _field(X, X, t, 0)
        total = math.fsum(r.cpu().tolist())
        within = float(E.pair_potential(torch.from_numpy(X).cuda(), None, t, "within").cpu()[0])
        ref = float(_field_ref(n, None, d, 0, t)[0].sum())
        slack = ref * (e_w(t, d, R) + addition_depth(n, n) * 2.0 ** -53) + 2.0 * potential_bound(ref / 2, t, d, R, potential_depth(n, 0, 2))
        assert abs(total - 2.0 * within) <= slack, (n, d, t, total, within)


def test_rows_past_nx_are_never_written():
    E = _E()
    X, Y = _case(70, 130, 40, -1)
    Xd, Yd = torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda()
    r = torch.full((70 + 5,), -7.0, dtype=torch.float64, device="cuda")
    F = torch.full((70 + 60, 40), -7.0, dtype=torch.float64, device="cuda")
    got = E.pair_field(Xd, Yd, 2.0, self_offset=-1, out=(r, F))
    assert got[0] is r and got[1] is F
    assert bool((r[70:] == -7.0).all()) and bool((F[70:] == -7.0).all())
    want = E.pair_field(Xd, Yd, 2.0, self_offset=-1)
    assert torch.equal(r[:70], want[0]) and torch.equal(F[:70], want[1])


def _strided(X, pad, shift):
    """The same rows with row stride D + pad, starting `shift` floats into a buffer: a padded stride and a base misaligned by
    4 bytes against the allocation."""
    n, d = X.shape
    buf = torch.full((n * (d + pad) + shift + 8,), float("nan"), device=X.device)
    view = buf[shift:shift + n * (d + pad)].view(n, d + pad)[:, :d]
    view.copy_(X)
    assert view.stride(0) == d + pad and view.data_ptr() % 8 == 4 * (shift % 2)
    return view


@pytest.mark.parametrize("n,d", [(65, 33), (130, 128), (1100, 4)])
def test_same_bits_for_every_run_stride_and_alignment(n, d):
    E = _E()
    X, Y = torch.from_numpy(_unit_rows(n, d, 1)).cuda(), torch.from_numpy(_unit_rows(n + 7, d, 2)).cuda()
    Xs, Ys = _strided(X, 3, 1), _strided(Y, 7, 3)
    first = E.pair_field(X)
    for again in (E.pair_field(X), E.pair_field(Xs), E.pair_field(X, X), E.pair_field(Xs, _strided(X, 5, 3))):
        assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    first = E.pair_field(X, Y, 0.5, exclude_self=False)
    for again in (E.pair_field(X, Y, 0.5, exclude_self=False), E.pair_field(Xs, Ys, 0.5, self_offset=-1)):
        assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])


# ------------------------------------------------------------------------------------------------------------- the loss
def _partners(n, d, seed):
    """Two unit-norm sets whose partners are correlated, as trained towers' are."""
    a, b = _unit_rows(n, d, seed), _unit_rows(n, d, seed + 1)
    b = (0.8 * a.astype(np.float64) + 0.6 * b.astype(np.float64))
    b /= np.linalg.norm(b, axis=1, keepdims=True)
    return a, b.astype(np.float32)


def _fp64_bounds(X, alpha, t, lam, weight):
    """What the fp64 arithmetic may do, from the longdouble reference: eS, the relative error of S = sum r / 2 (every w within
    e_w, A_f additions in the field, the loss's own sums after it); dU, the error of U = log(2 S / (N (N - 1))) (a quotient and
    a log on top); and per element dG, the error of weight lam t F_ic / S: F within B_ic (e_w + (A_f + 2) 2^-53), S within eS, a
    quotient and two products on top."""
    E = _E()
    n, d = X.shape
    R = _R(X, X)
    r, F = E.pair_field_reference(X, None, t, True)
    absX = np.abs(X.astype(np.longdouble))
    B = np.zeros(X.shape, dtype=np.longdouble)
    for i in range(n):
        w = np.exp(-np.longdouble(t) * ((X[i].astype(np.longdouble) - X.astype(np.longdouble)) ** 2).sum(axis=1))
        w[i] = 0
        B[i] = w.sum() * absX[i] + w @ absX
    S = r.sum() / 2
    A = addition_depth(n, n)
    eS = e_w(t, d, R) + (A + loss_depth(n)) * 2.0 ** -53
    U = np.log(S / (np.longdouble(n) * (n - 1) / 2))
    dU = float(eS + 2.0 ** -51 * (1 + abs(U)))
    dG = (weight * lam * t / S) * (B * (e_w(t, d, R) + (A + 2) * 2.0 ** -53) + np.abs(F) * (eS + 2.0 ** -50))
    return dU, dG.astype(np.float64)


def _align_fp64(X, Y, alpha):
    """Error of (x_ic - y_ic) k_i in fp64: the difference is exact to an ulp, d2_i a chain of D, a root, a quotient, products."""
    n, d = X.shape
    diff = np.abs(X.astype(np.float64) - Y.astype(np.float64))
    if alpha == 2:
        return diff * (2.0 / n) * 2.0 ** -50
    d2 = (diff ** 2).sum(axis=1, keepdims=True)
    k = np.where(d2 > 0, 1.0 / (n * np.sqrt(np.where(d2 > 0, d2, 1.0))), 0.0)
    return diff * k * (d + 6) * 2.0 ** -52


def _check_pair(X, Y, alpha, t, lam, g=1.0, label=""):
    Lo = _Lo()
    e1 = torch.from_numpy(X).cuda().requires_grad_(True)
    e2 = torch.from_numpy(Y).cuda().requires_grad_(True)
    loss = Lo.align_uniform_loss(e1, e2, alpha, t, lam)
    assert loss.dtype == torch.float32 and loss.dim() == 0
    (loss * g).backward()
    ref, grads = Lo.align_uniform_reference([X, Y], alpha, t, lam)
    n, d = X.shape
    diff = X.astype(np.float64) - Y.astype(np.float64)
    align = float(((diff ** 2).sum(axis=1) ** (alpha / 2)).mean())
    worst = 0.0
    dUx, dGx = _fp64_bounds(X, alpha, t, lam, 1)
    dUy, dGy = _fp64_bounds(Y, alpha, t, lam, 1)
    # the loss: one rounding to fp32 of a sum whose terms carry align (D + the sums' additions) 2^-52 and lam / 2 (dU_x + dU_y)
    bound = 2.0 ** -24 * abs(float(ref)) + (align * (d + loss_depth(n) + 2) * 2.0 ** -52 + lam / 2 * (dUx + dUy)
                                           + 2.0 ** -51 * abs(float(ref))) * (1 + 2.0 ** -24)
    err = abs(float(np.longdouble(float(loss.detach())) - ref))
    print(f"align-uniform-accuracy: loss {label} alpha = {alpha} t = {t} lam = {lam}: L = {float(ref):.6f}, |L - ref| / bound = {err / bound:.4f}")
    assert err <= bound, (label, float(loss), float(ref))
    for got, want, dG in ((e1.grad, grads[0], dGx), (e2.grad, grads[1], dGy)):
        assert got.dtype == torch.float32 and got.shape == X.shape
        want = g * want
        fp64 = abs(g) * (dG + _align_fp64(X, Y, alpha)) + 2.0 ** -52 * np.abs(want.astype(np.float64))
        b = 2.0 ** -24 * np.abs(want.astype(np.float64)) + fp64 * (1 + 2.0 ** -24) + 2.0 ** -149
        e = np.abs(got.cpu().numpy().astype(np.longdouble) - want).astype(np.float64)
        ratio = float((e / b).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, (label, alpha, t, lam, ratio)
    print(f"align-uniform-accuracy: gradient {label} alpha = {alpha} t = {t} lam = {lam} g = {g}: worst |dX - ref| / bound = {worst:.4f}")
    return e1.grad, e2.grad


@pytest.mark.parametrize("n,d", SYMMETRIC)
def test_loss_and_gradient_against_the_reference(n, d):
    X, Y = _partners(n, d, 7 * n + d) if d > 1 else (_unit_rows(n, d, 7 * n), _unit_rows(n, d, 7 * n + 3))
    for alpha, t, lam in ((2, 2.0, 1.0), (1, 2.0, 1.0), (2, 0.5, 0.0), (1, 8.0, 1.0)):
        _check_pair(X, Y, alpha, t, lam, label=f"({n}, {d})")


def test_identical_partners_under_alpha_one_get_no_alignment_gradient():
    X, Y = _partners(65, 33, 5)
    Y[3] = X[3]
    g1, g2 = _check_pair(X, Y, 1, 2.0, 0.0, label="(65, 33) e1[3] == e2[3]")
    assert bool((g1[3] == 0).all()) and bool((g2[3] == 0).all()) and bool(torch.isfinite(g1).all())
    _check_pair(X, Y, 1, 2.0, 1.0, label="(65, 33) e1[3] == e2[3]")


def test_an_upstream_gradient_scales_the_result():
    X, Y = _partners(130, 128, 9)
    _check_pair(X, Y, 2, 2.0, 1.0, g=-3.5, label="(130, 128)")
    _check_pair(X, Y, 1, 2.0, 1.0, g=0.125, label="(130, 128)")


@pytest.mark.parametrize("alpha", [2, 1])
def test_three_towers_against_the_reference(alpha):
    """Each pair's loss is rounded to fp32 and the three are added in fp32; each tower's gradient is the fp32 sum of the
    gradients of its two pairs, each within the pair's own bound: 2^-24 of every partial figure and of the sum, and the fp64
    bounds at the weight m - 1 = 2."""
    Lo = _Lo()
    n, d, t, lam = 65, 33, 2.0, 1.0
    Xs = [_unit_rows(n, d, 40), None, None]
    Xs[1], Xs[2] = _partners(n, d, 41)[1], _partners(n, d, 40)[1]
    embs = [torch.from_numpy(x).cuda().requires_grad_(True) for x in Xs]
    loss, comps = Lo.align_uniform_loss_multimodal(embs, alpha, t, lam, return_components=True)
    loss.backward()
    ref, grads = Lo.align_uniform_reference(Xs, alpha, t, lam)
    pair_refs = {(i, j): Lo.align_uniform_reference([Xs[i], Xs[j]], alpha, t, lam) for i, j in ((0, 1), (0, 2), (1, 2))}
    assert len(comps) == 3 and all(c.dtype == torch.float64 and c.shape == (5,) for c in comps)
    for (i, j), c in zip(((0, 1), (0, 2), (1, 2)), comps):
        c = c.cpu().numpy()
        want = float(pair_refs[(i, j)][0])
        assert abs(c[0] + lam / 2 * (c[1] + c[2]) - want) <= 1e-12 * abs(want)
    sum_abs = sum(abs(float(v[0])) for v in pair_refs.values())
    assert abs(float(np.longdouble(float(loss.detach())) - ref)) <= 2.0 ** -24 * (3 * sum_abs + abs(float(ref))) + 1e-12
    for k in range(3):
        parts = [np.abs((pair_refs[p][1][p.index(k)]).astype(np.float64)) for p in pair_refs if k in p]
        dG = _fp64_bounds(Xs[k], alpha, t, lam, 2)[1]
        others = [x for q, x in enumerate(Xs) if q != k]
        fp64 = dG + sum(_align_fp64(Xs[k], o, alpha) for o in others)
        b = 2.0 ** -24 * (sum(parts) + np.abs(grads[k].astype(np.float64))) + fp64 * (1 + 2.0 ** -23) + 2.0 ** -149
        e = np.abs(embs[k].grad.cpu().numpy().astype(np.longdouble) - grads[k]).astype(np.float64)
        ratio = float((e / b).max())
        print(f"align-uniform-accuracy: three towers alpha = {alpha} tower {k}: worst |dX - ref| / bound = {ratio:.4f}")
        assert ratio <= 1.0, (k, ratio)


# ----------------------------------------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing(monkeypatch):
    E, Lo, L = _E(), _Lo(), _lib()
    X = torch.from_numpy(_unit_rows(8, 4, 1)).cuda()
    wide = torch.zeros(4, 257).cuda()
    for call, what in [(lambda: E.pair_field(wide), "D must be in 1..256"),
                       (lambda: E.pair_field(X, t=0.0), "finite and positive"),
                       (lambda: E.pair_field(X, t=float("nan")), "finite and positive"),
                       (lambda: E.pair_field(X.cpu()), "must live on the GPU"),
                       (lambda: E.pair_field(X, X.cpu()), "must live on the GPU"),
                       (lambda: Lo.align_uniform_loss(wide, wide), "D must be in 1..256"),
                       (lambda: Lo.align_uniform_loss(X[:1], X[:1]), "N must be at least 2"),
                       (lambda: Lo.align_uniform_loss(X.cpu(), X.cpu()), "must live on the GPU"),
                       (lambda: Lo.align_uniform_loss(X, X.cpu()), "must live on the GPU")]:
        with pytest.raises(L.MsnHipError, match=what):
            call()
    for call, what in [(lambda: Lo.align_uniform_loss(X, X, t=0.0), "finite and positive"),
                       (lambda: Lo.align_uniform_loss(X, X, t=float("inf")), "finite and positive"),
                       (lambda: Lo.align_uniform_loss(X, X, alpha=3), "alpha must be 2 or 1"),
                       (lambda: Lo.align_uniform_loss(X, X, lam=-1.0), "lam"),
                       (lambda: Lo.align_uniform_loss(X, X[:7]), "one shape"),
                       (lambda: Lo.align_uniform_loss_multimodal([X]), "at least two"),
                       (lambda: E.pair_field(X, torch.zeros(8, 5).cuda()), "columns"),
                       (lambda: E.pair_field(X, self_offset=-2), "self_offset")]:
        with pytest.raises(ValueError, match=what):
            call()
    # the C-ABI itself: MSN_ERR_SHAPE (1) and nothing enqueued
    lib = L.lib()
    r, F = torch.zeros(8, dtype=torch.float64).cuda(), torch.zeros(8, 4, dtype=torch.float64).cuda()
    ws = torch.zeros(1 << 12, dtype=torch.uint8).cuda()
    p, s = L.ptr, L.stream_ptr()
    assert lib.msn_pair_field(p(X), 4, 8, p(X), 4, 8, 4, 2.0, 0, p(r), p(F), p(ws), 8, s) == 1             # workspace too small
    assert lib.msn_pair_field(p(X), 4, 8, p(X), 4, 1 << 31, 4, 2.0, 0, p(r), p(F), p(ws), ws.numel(), s) == 1
    assert lib.msn_pair_field(p(X), 4, 0, p(X), 4, 8, 4, 2.0, 0, p(r), p(F), p(ws), ws.numel(), s) == 1
    loss, comp = torch.zeros((), device="cuda"), torch.zeros(5, dtype=torch.float64).cuda()
    assert lib.msn_align_uniform_fwd(p(X), 4, p(X), 4, 1, 4, p(r), p(r), 2, 1.0, p(loss), p(comp), p(r), p(ws), ws.numel(), s) == 1
    assert lib.msn_align_uniform_fwd(p(X), 4, p(X), 4, 8, 4, p(r), p(r), 3, 1.0, p(loss), p(comp), p(r), p(ws), ws.numel(), s) == 1
    assert lib.msn_align_uniform_fwd(p(X), 4, p(X), 4, 8, 4, p(r), p(r), 2, 1.0, p(loss), p(comp), p(r), p(ws), 8, s) == 1
    assert lib.msn_align_uniform_bwd(p(X), 4, p(X), 4, 8, 4, p(F), p(F), p(r), p(comp), p(loss), 2, 0.0, 1.0, p(F), 4, p(F), 4, s) == 1
    assert lib.msn_pair_field_workspace_bytes(8, 8, 257) == 0 and lib.msn_align_uniform_workspace_bytes(1) == 0
    torch.cuda.synchronize()
    assert float(r.abs().sum()) == 0.0 and float(F.abs().sum()) == 0.0 and float(loss) == 0.0
    # sharded: uniformity over gathered rows is not built
    monkeypatch.setattr(Lo, "_is_sharded", lambda global_negatives, group: bool(global_negatives))
    with pytest.raises(NotImplementedError, match="global_negatives=False"):
        Lo.align_uniform_loss(X, X)
    assert Lo.align_uniform_loss(X, X.flip(0), global_negatives=False).dim() == 0


# ------------------------------------------------------------------------------------------------------------ the model
TK = dict(n_out=16, emb=16, heads=2, depth=1, dropout=0.0, time_norm=20583.37, agg="mean")
SK = dict(n_out=16, emb=16, heads=2, depth=1, dropout=0.0, time_norm=17945.14, agg="mean")


def _clip(**kw):
    from multimodal_supernovae_amd.models_multimodal import LightCurveImageCLIP
    torch.manual_seed(0)
    return LightCurveImageCLIP(enc_dim=32, nband=2, transformer_kwargs=TK, transformer_spectral_kwargs=SK,
                               combinations=["lightcurve", "spectral"], loss="align_uniform", **kw).cuda().train()


def _batch(g, B, T=12, Ts=16):
    t = torch.sort(torch.rand(B, T // 2, generator=g) * 100, dim=1)[0].repeat(1, 2)
    return tuple(x.cuda() if x is not None else None for x in (
        None, torch.randn(B, T, generator=g), t, torch.ones(B, T, dtype=torch.bool), torch.randn(B, Ts, generator=g),
        torch.sort(torch.rand(B, Ts, generator=g) * 6000 + 3000, dim=1)[0], torch.ones(B, Ts, dtype=torch.bool),
        torch.rand(B, generator=g), torch.randint(0, 5, (B,), generator=g)))


def test_one_eager_step_reaches_every_trainable_parameter():
    model = _clip(loss_kwargs={"alpha": 2, "t": 2.0, "lam": 1.0})
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
    tests/test_graph_gpu.py for its own model)."""
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
