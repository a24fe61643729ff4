"""The pair kernels of csrc/embedding_metrics.hip and embedding_metrics.py on the GPU: coverage pinned bit for bit on integer
data (every pair once, no padded row, no diagonal), the Gaussian potential on unit-norm data within a bound derived from the
arithmetic, the same bits for every run, stride and alignment, the alignment sums, the refusals, and the host figures, the
accumulator and the model's opt-in log end to end.

Lines that start with "embedding-metrics-accuracy:" carry the measured worst ratio to each bound
(profiles/embedding_metrics_accuracy.txt)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TILE = 64                 # rows of a tile (kPairTile of csrc/embedding_metrics.hip)
BLOCKS = 1024             # workgroups aimed at (kPairBlocks)
MODES = {"all": 0, "offdiag": 1, "within": 2}

# N: one row (modes 0 / 1), the smallest triangle, one below / at / one past a tile, two tiles and a row, three tiles and a part.
# D: one column, no multiple of 4, one chunk, one chunk and a column, four chunks.
GRID = [(n, d) for n in (1, 2, 63, 64, 65, 129, 200) for d in (1, 5, 32, 33, 128)]
# more than 16 partials over many workgroups (171 tile pairs within); D at its limit
EXTRA = [(1100, 4), (70, 1024)]
RECT = (65, 130, 33)      # (Nx, Ny, D) in mode 0: two tiles by three


def _E():
    from multimodal_supernovae_amd import embedding_metrics
    return embedding_metrics


def _lib():
    from multimodal_supernovae_amd import _lib as L
    return L


def cdiv(a, b):
    return -(-a // b)


def addition_depth(Nx, Ny, mode):
    """A(Nx, Ny, mode) of include/msn_hip.h: 16 per tile pair of a workgroup in a lane, 6 + 3 in the workgroup's reduction,
    ceil(blocks / 256) in a finishing thread, 6 + 3 in its reduction."""
    ti = cdiv(Nx, TILE)
    pairs = ti * (ti + 1) // 2 if mode == 2 else ti * cdiv(Ny, TILE)
    per = cdiv(pairs, BLOCKS)
    blocks = cdiv(pairs, per)
    return 16 * per + 9 + cdiv(blocks, 256) + 9


def potential_bound(S, t, D, R, A):
    """t (D + 4) 2^-52 R for what the rounding of d2 (D products added, three more operations) does to exp(-t d2), two ulps for
    exp, A 2^-53 for the sums of non-negative terms."""
    return S * (t * (D + 4) * 2.0 ** -52 * R + 2.0 ** -51 + A * 2.0 ** -53)


def _integer_rows(n, d, seed):
    """Entries in [-3, 3], every third row a copy of the row before it: every d2 and every sum of them is exact in fp64."""
    rng = np.random.default_rng(seed)
    X = rng.integers(-3, 4, size=(n, d)).astype(np.float32)
    X[2::3] = X[1::3][:len(X[2::3])]
    return X


def _unit_rows(n, d, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d))
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    return (scale * X).astype(np.float32)


def _d2_exact(X, Y):
    X, Y = X.astype(np.float64), Y.astype(np.float64)
    return ((X[:, None, :] - Y[None, :, :]) ** 2).sum(axis=2) if X.shape[1] <= 128 else \
        np.stack([((Y - x) ** 2).sum(axis=1) for x in X])


def _sum_d2_exact(X, Y, pairs):
    d2 = _d2_exact(X, X if Y is None else Y)
    if pairs == "within":
        return float(np.triu(d2, 1).sum())
    return float(d2.sum() - (np.trace(d2) if pairs == "offdiag" else 0.0))


def _pot(X, Y, t, pairs):
    E = _E()
    out = E.pair_potential(torch.from_numpy(X).cuda(), None if Y is None else torch.from_numpy(Y).cuda(), t, pairs)
    assert out.dtype == torch.float64 and out.shape == (2,)
    return out.cpu()


# ------------------------------------------------------------------------------------------------- potential: coverage
@pytest.mark.parametrize("n,d", GRID + EXTRA)
def test_integer_data_pins_the_pair_set(n, d):
    E = _E()
    X, Y = _integer_rows(n, d, 7 * n + d), _integer_rows(n, d, 11 * n + d)
    t = 0.125
    for pairs, other in (("all", Y), ("offdiag", Y), ("within", None)):
        if pairs == "within" and n < 2:
            continue
        got = _pot(X, other, t, pairs)
        assert float(got[1]) == _sum_d2_exact(X, other, pairs), (pairs, n, d)
    # the same set against itself: the diagonal of `all` is exactly N terms of exp(0), offdiag drops terms that are exactly 0
    a = _pot(X, X, t, "all")
    o = _pot(X, X, t, "offdiag")
    assert torch.equal(o[1], a[1])
    if n >= 2:
        w = _pot(X, None, t, "within")
        assert float(a[1]) == 2.0 * float(w[1])
        R = 2.0 * float((X.astype(np.float64) ** 2).sum(axis=1).max())
        sa, sw = (float(v[0]) for v in (E.pair_potential_reference(X, X, t, "all"), E.pair_potential_reference(X, None, t)))
        slack = potential_bound(sa, t, d, R, addition_depth(n, n, 0)) + 2.0 * potential_bound(sw, t, d, R, addition_depth(n, 0, 2))
        assert abs(float(a[0]) - 2.0 * float(w[0]) - n) <= slack
        assert abs(float(a[0]) - float(o[0]) - n) <= 2.0 * potential_bound(sa, t, d, R, addition_depth(n, n, 0))


def test_integer_data_rectangular_all_pairs():
    nx, ny, d = RECT
    X, Y = _integer_rows(nx, d, 1), _integer_rows(ny, d, 2)
    assert float(_pot(X, Y, 0.125, "all")[1]) == _sum_d2_exact(X, Y, "all")
    assert float(_pot(Y, X, 0.125, "all")[1]) == _sum_d2_exact(X, Y, "all")


# ------------------------------------------------------------------------------------------------- potential: accuracy
def _normal_cases():
    """(X, Y, D, label): the grid, the extras, the rectangle (mode 0 only), and one case of norm 3 with two identical rows."""
    cases = []
    for n, d in GRID + EXTRA:
        cases.append((_unit_rows(n, d, 3 * n + d), _unit_rows(n, d, 5 * n + d + 1), f"({n}, {d})"))
    X3 = _unit_rows(200, 64, 77, scale=3.0)
    X3[17] = X3[120]
    Y3 = _unit_rows(200, 64, 78, scale=3.0)
    Y3[5] = X3[5]
    cases.append((X3, Y3, "(200, 64) scale 3"))
    return cases


@pytest.mark.parametrize("pairs", ["within", "all", "offdiag"])
def test_potential_on_unit_norm_data_within_the_derived_bound(pairs):
    """|out[0] - S_ref| <= S_ref (t (D + 4) 2^-52 R + 2^-51 + A 2^-53), R = max |x|^2 + max |y|^2, against the longdouble
    restatement in the direct form; out[1], a sum of non-negative d2 each within (D + 4) 2^-52 R of the direct form, within
    (D + 4) 2^-52 R per pair + A 2^-53 of the sum."""
    E = _E()
    mode = MODES[pairs]
    cases = _normal_cases()
    if pairs == "all":
        nx, ny, d = RECT
        cases.append((_unit_rows(nx, d, 31), _unit_rows(ny, d, 32), f"({nx}, {ny}, {d})"))
    worst = 0.0
    for X, Y, label in cases:
        if pairs == "within":
            if len(X) < 2:
                continue
            Y = None
        d = X.shape[1]
        other = X if Y is None else Y
        R = float((X.astype(np.float64) ** 2).sum(axis=1).max() + (other.astype(np.float64) ** 2).sum(axis=1).max())
        A = addition_depth(len(X), 0 if Y is None else len(Y), mode)
        npairs = {"within": len(X) * (len(X) - 1) // 2, "all": len(X) * len(other), "offdiag": len(X) * (len(X) - 1)}[pairs]
        for t in (0.5, 2.0, 8.0):
            got = _pot(X, Y, t, pairs)
            se, sd = E.pair_potential_reference(X, Y, t, pairs)
            bound = potential_bound(float(se), t, d, R, A)
            err = abs(float(np.longdouble(float(got[0])) - se))
            ratio = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
            print(f"embedding-metrics-accuracy: potential {pairs} {label} t = {t}: |out[0] - ref| / bound = {ratio:.4f}")
            worst = max(worst, ratio)
            assert err <= bound, (pairs, label, t, float(got[0]), float(se))
            err1 = abs(float(np.longdouble(float(got[1])) - sd))
            assert err1 <= npairs * (d + 4) * 2.0 ** -52 * R + float(sd) * A * 2.0 ** -53, (pairs, label)
    print(f"embedding-metrics-accuracy: potential {pairs} worst over shapes and t = {worst:.4f}")


# ------------------------------------------------------------------------------------------------------------- bits
def _strided(X, pad, shift):
    """The same rows with row stride D + pad, starting `shift` floats into a buffer: a padded stride and a base misaligned by
    4 bytes against the allocation."""
    n, d = X.shape
    buf = torch.full((n * (d + pad) + shift + 8,), float("nan"), device=X.device)
    view = buf[shift:shift + n * (d + pad)].view(n, d + pad)[:, :d]
    view.copy_(X)
    assert view.stride(0) == d + pad and view.data_ptr() % 8 == 4 * (shift % 2)
    return view


@pytest.mark.parametrize("n,d", [(129, 33), (200, 128), (65, 5)])
def test_same_bits_for_every_run_stride_and_alignment(n, d):
    E = _E()
    X, Y = torch.from_numpy(_unit_rows(n, d, 1)).cuda(), torch.from_numpy(_unit_rows(n, d, 2)).cuda()
    Xs, Ys = _strided(X, 3, 1), _strided(Y, 7, 3)
    for pairs in ("within", "all", "offdiag"):
        other = (None, None) if pairs == "within" else (Y, Ys)
        first = E.pair_potential(X, other[0], 2.0, pairs)
        assert torch.equal(first, E.pair_potential(X, other[0], 2.0, pairs))
        assert torch.equal(first, E.pair_potential(Xs, other[1], 2.0, pairs))
    first, rows = E.pair_alignment(X, Y, rows=True)
    again, rows2 = E.pair_alignment(X, Y, rows=True)
    strided, rows3 = E.pair_alignment(Xs, Ys, rows=True)
    assert torch.equal(first, again) and torch.equal(first, strided) and torch.equal(rows, rows2) and torch.equal(rows, rows3)
    assert torch.equal(first, E.pair_alignment(X, Y))
    out = torch.zeros(2, dtype=torch.float64, device="cuda")
    assert E.pair_alignment(X, Y, out=out) is out and torch.equal(out, first)


# -------------------------------------------------------------------------------------------------------- alignment
ALIGN_SHAPES = [(n, d) for n in (1, 63, 64, 65, 3100) for d in (1, 33)] + [(65, 1024)]


@pytest.mark.parametrize("n,d", ALIGN_SHAPES)
def test_alignment_sums(n, d):
    """Integer data: out[0] and the rows equal numpy exactly, identical rows give exactly 0.  Normal data: non-negative terms,
    a chain of D for a row and at most N additions over the rows, so both sums lie within (D + N) 2^-52 of the longdouble value
    (sqrt is correctly rounded: half an ulp more per row, inside the same count)."""
    E = _E()
    X, Y = _integer_rows(n, d, n + d), _integer_rows(n, d, 2 * n + d)
    Y[::5] = X[::5]
    out, rows = E.pair_alignment(torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda(), rows=True)
    ref = ((X.astype(np.float64) - Y.astype(np.float64)) ** 2).sum(axis=1)
    assert rows.dtype == torch.float64 and torch.equal(rows.cpu(), torch.from_numpy(ref))
    assert float(out[0]) == float(ref.sum()) and bool((rows[::5] == 0).all())
    same = E.pair_alignment(torch.from_numpy(X).cuda(), torch.from_numpy(X).cuda())
    assert float(same[0]) == 0.0 and float(same[1]) == 0.0
    X, Y = _unit_rows(n, d, 3 * n + d), _unit_rows(n, d, 4 * n + d)
    out = E.pair_alignment(torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda()).cpu()
    s2, s1, _ = E.pair_alignment_reference(X, Y)
    worst = 0.0
    for got, ref in ((out[0], s2), (out[1], s1)):
        bound = (d + n) * 2.0 ** -52 * float(ref)
        err = abs(float(np.longdouble(float(got)) - ref))
        assert err <= bound, (n, d, float(got), float(ref))
        worst = max(worst, err / bound if bound > 0 else 0.0)          # (two equal rows of one column: 0 against 0)
    print(f"embedding-metrics-accuracy: alignment ({n}, {d}) worst |sum - ref| / bound = {worst:.4f}")


# ----------------------------------------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing():
    E, L = _E(), _lib()
    X = torch.zeros(8, 4).cuda()
    wide = torch.zeros(4, 1025).cuda()
    for call, what in [(lambda: E.pair_potential(wide), "D must be in 1..1024"),
                       (lambda: E.pair_potential(X[:1]), "Nx >= 2"),
                       (lambda: E.pair_potential(X, X[:7], pairs="offdiag"), "Nx == Ny"),
                       (lambda: E.pair_potential(X, t=0.0), "finite and positive"),
                       (lambda: E.pair_potential(X, t=float("inf")), "finite and positive"),
                       (lambda: E.pair_potential(X, t=float("nan")), "finite and positive"),
                       (lambda: E.pair_alignment(wide, wide), "D must be in 1..1024"),
                       (lambda: E.uniformity(torch.zeros(8, 5).cuda()), "multiple of 4"),
                       (lambda: E.pair_potential(X.cpu()), "must live on the GPU"),
                       (lambda: E.pair_alignment(X, X.cpu()), "must live on the GPU")]:
        with pytest.raises(L.MsnHipError, match=what):
            call()
    for call, what in [(lambda: E.pair_potential(X, X), "pass no Y"), (lambda: E.pair_potential(X, pairs="all"), "needs Y"),
                       (lambda: E.pair_potential(X, pairs="some"), "pairs must be"),
                       (lambda: E.pair_potential(X, torch.zeros(8, 5).cuda(), pairs="all"), "columns"),
                       (lambda: E.pair_alignment(X, X[:7]), "equal shape"), (lambda: E.alignment(X, X, alpha=3), "alpha")]:
        with pytest.raises(ValueError, match=what):
            call()


# ------------------------------------------------------------------------------------------------------- host figures
def test_one_copy_figures_match_their_definitions():
    E = _E()
    X, Y = _unit_rows(130, 32, 1, scale=2.0), _unit_rows(130, 32, 2, scale=0.5)
    Xd, Yd = torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda()
    Xu = X.astype(np.float64) / np.linalg.norm(X.astype(np.float64), axis=1, keepdims=True)
    Yu = Y.astype(np.float64) / np.linalg.norm(Y.astype(np.float64), axis=1, keepdims=True)
    n = len(X)
    # normalised in fp32 on the device: a coordinate moves by 2^-24, a distance d <= 2 by 2^-22 at most, d^2 by 2^-20, and the log
    # of a mean of exp(-t d^2) by t 2^-20 = 2e-6 at t = 2; the means of d^2 and of d by less
    se, _ = E.pair_potential_reference(Xu.astype(np.float32), None, 2.0, "within")
    assert abs(E.uniformity(Xd) - float(np.log(se / (n * (n - 1) / 2)))) <= 2e-6
    se, _ = E.pair_potential_reference(X, None, 0.5, "within")
    assert abs(E.uniformity(Xd, t=0.5, normalize=False) - float(np.log(se / (n * (n - 1) / 2)))) <= 1e-12
    for pairs, count in (("offdiag", n * (n - 1)), ("all", n * n)):
        se, _ = E.pair_potential_reference(X, Y, 2.0, pairs)
        assert abs(E.cross_uniformity(Xd, Yd, normalize=False, pairs=pairs) - float(np.log(se / count))) <= 1e-12
    d2 = ((Xu - Yu) ** 2).sum(axis=1)
    assert abs(E.alignment(Xd, Yd) - d2.mean()) <= 2e-6 and abs(E.alignment(Xd, Yd, alpha=1) - np.sqrt(d2).mean()) <= 2e-6
    s2, s1, _ = E.pair_alignment_reference(X, Y)
    assert abs(E.alignment(Xd, Yd, normalize=False) - float(s2) / n) <= 1e-12
    assert abs(E.alignment(Xd, Yd, alpha=1, normalize=False) - float(s1) / n) <= 1e-12


def test_retrieval_metrics():
    from multimodal_supernovae_amd.utils import retrieval_ranks
    E = _E()
    e1, e2 = torch.from_numpy(_unit_rows(70, 16, 1)).cuda(), torch.from_numpy(_unit_rows(70, 16, 2)).cuda()
    e2 = e1 * 0.5 + e2 * 0.87                          # partners correlated: ranks spread over a range
    got = E.retrieval_metrics(e1, e2, top_k=(1, 5, 10))
    a2b, b2a = retrieval_ranks(e2, e1).cpu().numpy(), retrieval_ranks(e1, e2).cpu().numpy()
    assert set(got) == {f"{k}{s}" for k in ("recall1", "recall5", "recall10", "mrr", "medr") for s in ("", "_a2b", "_b2a")}
    for sfx, r in (("_a2b", a2b), ("_b2a", b2a)):
        for k in (1, 5, 10):
            assert got[f"recall{k}{sfx}"] == E.recall_at_k(r, k)
        assert got[f"mrr{sfx}"] == E.mean_reciprocal_rank(r) and got[f"medr{sfx}"] == E.median_rank(r)
    for key in ("recall1", "recall5", "recall10", "mrr", "medr"):
        assert got[key] == 0.5 * (got[key + "_a2b"] + got[key + "_b2a"])
    assert 0.0 < got["recall1"] <= got["recall5"] <= got["recall10"] <= 1.0 and got["recall1"] < 1.0
    # well separated: every partner is the most similar row
    g = torch.Generator().manual_seed(3)
    e1 = torch.randn(64, 16, generator=g).cuda()
    e2 = e1 + 1e-3 * torch.randn(64, 16, generator=g).cuda()
    got = E.retrieval_metrics(e1, e2)
    assert all(got[k + s] == 1.0 for k in ("recall1", "mrr", "medr") for s in ("", "_a2b", "_b2a"))


# -------------------------------------------------------------------------------------------------------- accumulator
def _svd_erank(X, center):
    E = _E()
    X = X.astype(np.float64)
    return E.effective_rank(np.linalg.svd(X - X.mean(axis=0) if center else X, compute_uv=False))


def test_accumulator_over_uneven_batches_equals_one_call():
    """Entries on a grid of 1 / 8 and normalize=False: every product and every sum of the Gram matrices is exact in fp64, so
    the accumulated matrices equal the one-call matrices bit for bit however the rows were cut; everything else is computed
    from the concatenated rows either way."""
    E = _E()
    rng = np.random.default_rng(4)
    A = (rng.integers(-8, 9, size=(150, 32)) / 8.0).astype(np.float32)
    B = (A + rng.integers(-2, 3, size=(150, 32)) / 8.0).astype(np.float32)
    Ad, Bd = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()
    acc = E.EmbeddingMetrics(normalize=False)
    for lo, hi in ((0, 70), (70, 71), (71, 150)):
        acc.update(Ad[lo:hi], Bd[lo:hi])
    one = E.EmbeddingMetrics(normalize=False).update(Ad, Bd)
    assert torch.equal(acc.gram_a, one.gram_a) and torch.equal(acc.gram_b, one.gram_b)
    got, want = acc.compute(), one.compute()
    assert got == want and got["n"] == 150
    assert set(got) == {"n", "alignment", "uniformity_a", "uniformity_b", "uniformity", "uniformity_cross", "modality_gap",
                        "erank_a", "erank_b", "erank"} | set(E.retrieval_metrics(Ad, Bd))
    assert got["uniformity"] == 0.5 * (got["uniformity_a"] + got["uniformity_b"]) and got["erank"] == min(got["erank_a"], got["erank_b"])
    # each figure against its one-call function on the concatenation
    assert got["alignment"] == E.alignment(Ad, Bd, normalize=False)
    assert got["uniformity_a"] == E.uniformity(Ad, normalize=False) and got["uniformity_b"] == E.uniformity(Bd, normalize=False)
    assert got["uniformity_cross"] == E.cross_uniformity(Ad, Bd, normalize=False)
    assert abs(got["modality_gap"] - float(np.linalg.norm(A.astype(np.float64).mean(0) - B.astype(np.float64).mean(0)))) <= 1e-14
    assert abs(got["erank_a"] - _svd_erank(A, True)) <= 1e-8 and abs(got["erank_b"] - _svd_erank(B, True)) <= 1e-8
    assert {k: v for k, v in got.items() if k.startswith(("recall", "mrr", "medr"))} == E.retrieval_metrics(Ad, Bd)
    acc.reset()
    assert acc.gram_a is None
    with pytest.raises(ValueError):
        acc.compute()


@pytest.mark.parametrize("center", [True, False])
def test_accumulator_on_normalised_rows(center):
    """The defaults: rows normalised on the device, three uneven batches.  The normalisation is row-wise, so the concatenated
    rows are the same bits either way and every figure but the Gram-derived ones is equal; the Gram matrices differ by the
    order of N additions of terms of magnitude at most 1: (N - 1) 2^-53 N for either order, N^2 2^-52 between them."""
    E = _E()
    A = _unit_rows(150, 64, 5, scale=2.0) + 0.3
    B = _unit_rows(150, 64, 6, scale=0.7) + _unit_rows(1, 64, 7)
    Ad, Bd = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()
    acc = E.EmbeddingMetrics(center=center)
    for lo, hi in ((0, 33), (33, 130), (130, 150)):
        acc.update(Ad[lo:hi], Bd[lo:hi])
    one = E.EmbeddingMetrics(center=center).update(Ad, Bd)
    assert float((acc.gram_a - one.gram_a).abs().max()) <= 150 * 150 * 2.0 ** -52
    got, want = acc.compute(), one.compute()
    for k in want:
        if k.startswith("erank") or k == "modality_gap":
            assert abs(got[k] - want[k]) <= 1e-10, k
        else:
            assert got[k] == want[k], k
    Au = A.astype(np.float64) / np.linalg.norm(A.astype(np.float64), axis=1, keepdims=True)
    Bu = B.astype(np.float64) / np.linalg.norm(B.astype(np.float64), axis=1, keepdims=True)
    # the device normalises in fp32: the rows differ from the fp64 unit rows by 2^-24 relative, the entropy of 64 values likewise
    assert abs(got["erank_a"] - _svd_erank(Au, center)) <= 1e-4 and abs(got["erank_b"] - _svd_erank(Bu, center)) <= 1e-4
    assert abs(got["modality_gap"] - float(np.linalg.norm(Au.mean(0) - Bu.mean(0)))) <= 1e-6
    # the spectrum of the device's own unit rows, copied back: the Gram route itself within 1e-8
    from multimodal_supernovae_amd import ops
    own = ops.l2norm_fwd(Ad.contiguous())[0].cpu().numpy()
    assert abs(got["erank_a"] - _svd_erank(own, center)) <= 1e-8


# ------------------------------------------------------------------------------------------------------------ the log
TK = dict(n_out=16, emb=16, heads=2, depth=1, dropout=0.0, time_norm=20583.37, agg="mean")
SK = dict(n_out=16, emb=16, heads=2, depth=1, dropout=0.0, time_norm=17945.14, agg="mean")


def _clip(**kw):
    from multimodal_supernovae_amd.models_multimodal import LightCurveImageCLIP
    torch.manual_seed(0)
    return LightCurveImageCLIP(enc_dim=32, nband=2, transformer_kwargs=TK, transformer_spectral_kwargs=SK,
                               combinations=["lightcurve", "spectral"], loss="softmax", **kw).cuda().eval()


def _batch(g, B, T=12, Ts=16):
    t = torch.sort(torch.rand(B, T // 2, generator=g) * 100, dim=1)[0].repeat(1, 2)
    return tuple(x.cuda() if x is not None else None for x in (
        None, torch.randn(B, T, generator=g), t, torch.ones(B, T, dtype=torch.bool), torch.randn(B, Ts, generator=g),
        torch.sort(torch.rand(B, Ts, generator=g) * 6000 + 3000, dim=1)[0], torch.ones(B, Ts, dtype=torch.bool),
        torch.rand(B, generator=g), torch.randint(0, 5, (B,), generator=g)))


def _validate(model, val):
    with torch.no_grad():
        model.on_validation_start()
        for i, b in enumerate(val):
            model.validation_step(b, i)
        embs = [torch.cat(e, dim=0) for e in model.embs_list]
        model.on_validation_epoch_end()
    return embs


def test_the_model_logs_the_embedding_metrics_only_when_asked():
    E = _E()
    g = torch.Generator().manual_seed(5)
    val = [_batch(g, 24), _batch(g, 9)]
    plain = _clip()
    _validate(plain, val)
    assert set(plain.logged) == {"val_loss", "AUC_val"}
    model = _clip(embedding_metrics=True)
    embs = _validate(model, val)
    assert embs[0].shape == (33, 32) and model.embs_list is None
    assert set(model.logged) == {"val_loss", "AUC_val", "align_val", "uniform_val", "gap_val", "erank_val", "recall1_val"}
    assert model.logged["AUC_val"] == plain.logged["AUC_val"] and torch.equal(model.logged["val_loss"], plain.logged["val_loss"])
    want = E.EmbeddingMetrics().update(embs[0], embs[1]).compute()
    for key, name in (("align_val", "alignment"), ("uniform_val", "uniformity"), ("gap_val", "modality_gap"),
                      ("erank_val", "erank"), ("recall1_val", "recall1")):
        assert model.logged[key] == want[name], key
