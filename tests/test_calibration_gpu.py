"""Calibration metrics on the GPU (csrc/calibration.hip, calibration.py): the binned counts bit for bit against their numpy
restatement, softmax_rows against the fp64 restatement within half an fp32 ulp, the temperature objective against a longdouble
reference with the fp64 restatement as the yardstick, TemperatureScaling.fit, CalibrationMetrics, the opt-in integration into
ClipMLP and the probe metrics, and two ranks against one process.  Lines that begin with "calibration-accuracy:" are the
measurements of profiles/calibration_accuracy.txt."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NARROW_C = 16             # up to here a lane owns a row (kCalNarrowC of csrc/calibration.hip); wider C: a wave owns a row
NS = [1, 63, 257, 1025, 3100]
CS = [1, 2, 5, NARROW_C, NARROW_C + 1, 64]
SHAPES = [(n, c) for n in NS for c in CS] + [(64, 1024)]
BINS = [1, 10, 15, 1024]  # 1024: two slots per workgroup; 10 and 15: every slot of C = 64 in one workgroup
KINDS = ["grid", "softmax"]


def _K():
    from multimodal_supernovae_amd import calibration
    return calibration


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()            # a copy: the cached cases are read-only


def _strided(x):
    """The same rows under a row stride of C + 3 and a base pointer off by one float (NaN in between)."""
    N, C = x.shape
    flat = torch.full((N * (C + 3) + 1,), float("nan"), device="cuda")
    view = flat[1:].view(N, C + 3)[:, :C]
    view.copy_(x)
    assert view.data_ptr() % 8 == 4 and (N == 1 or view.stride(0) == C + 3)
    return view


@functools.lru_cache(maxsize=None)
def _logits(N, C, scale=3.0):
    x = (scale * np.random.default_rng(1009 * N + C).standard_normal((N, C))).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _targets(N, C):
    """int64 targets: some -100, some >= C."""
    rng = np.random.default_rng(77 * N + C)
    y = rng.integers(0, C, N)
    u = rng.random(N)
    y[u < 0.08] = -100
    y[(u >= 0.08) & (u < 0.12)] = C + 1
    if N >= 8:
        y[3], y[6] = -100, C
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def _probs(N, C, kind):
    """(P fp32 (N, C), y int64 (N)), read-only: probabilities on the grid k / 8 (every confidence on a bin edge of B = 1024, p = 1
    and -0.0 among them) or the softmax of 3 x normal logits; bad rows of every sort among them."""
    rng = np.random.default_rng(31 * N + C + (kind == "grid"))
    if kind == "grid":
        P = (rng.multinomial(8, np.full(C, 1.0 / C), N) / 8.0).astype(np.float32)
        P = np.where((P == 0) & (rng.random((N, C)) < 0.5), np.float32(-0.0), P)
    else:
        P = _K().softmax_rows_reference(_logits(N, C)).astype(np.float32)
    u = rng.random(N)
    P[u < 0.05, 0] = np.nan
    P[(u >= 0.05) & (u < 0.08)] *= 0.5                           # sums to 0.5
    if C > 1:
        rows = (u >= 0.08) & (u < 0.11)
        P[rows, 0], P[rows, 1] = 1.5, -0.5                       # sums to 1 + the rest, entries outside [0, 1]
    P.setflags(write=False)
    return P, _targets(N, C)


def _equal(got, want):
    return all(g.dtype == torch.int64 and torch.equal(g.cpu(), torch.from_numpy(w)) for g, w in zip(got, want))


# ------------------------------------------------------------------------------------------------------------ counts
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N,C", SHAPES)
def test_calibration_counts_equal_the_restatement(N, C, kind):
    K = _K()
    P, y = _probs(N, C, kind)
    Pd, yd = _dev(P), _dev(y)
    Ps = _strided(Pd)
    for B in BINS:
        for classwise in (False, True):
            if classwise and C == 1024 and B != 10:
                continue
            want = K.calibration_counts_reference(P, y, n_bins=B, classwise=classwise)
            got = K.calibration_counts(Pd, yd, n_bins=B, classwise=classwise)
            assert got[0].shape == ((1 + C if classwise else 1), B, 3) and got[1].shape == (3,)
            assert _equal(got, want), (N, C, kind, B, classwise)
            assert _equal(K.calibration_counts(Ps, yd, n_bins=B, classwise=classwise), want), ("strided", N, C, kind, B, classwise)
            if N > 1:                                            # two calls into the same accumulators
                cut = N // 3 + 1
                acc, tot = K.calibration_counts(Pd[:cut], yd[:cut], n_bins=B, classwise=classwise)
                acc2, tot2 = K.calibration_counts(Ps[cut:], yd[cut:], n_bins=B, classwise=classwise, acc=acc, tot=tot)
                assert acc2 is acc and tot2 is tot and _equal((acc, tot), want), ("two calls", N, C, kind, B, classwise)
    if N >= 257:
        assert want[1][1] > 0 and want[1][0] > 0                 # the case holds bad rows and valid ones
    with pytest.raises(ValueError, match="accumulator"):
        K.calibration_counts(Pd, yd, acc=torch.zeros((1, 15, 3), dtype=torch.int32, device="cuda"))


def test_calibration_counts_repeat_and_follow_a_permutation_of_the_rows():
    K = _K()
    P, y = _probs(3100, NARROW_C + 1, "softmax")
    Pd, yd = _dev(P), _dev(y)
    a = K.calibration_counts(Pd, yd, classwise=True)
    perm = torch.from_numpy(np.random.default_rng(1).permutation(3100)).cuda()
    b = K.calibration_counts(Pd[perm], yd[perm], classwise=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(a[0][:1], K.calibration_counts(Pd, yd)[0])                   # slot 0 does not depend on classwise


# ----------------------------------------------------------------------------------------------------------- softmax
@pytest.mark.parametrize("N,C", [(1, 1), (63, 2), (1025, 5), (257, NARROW_C), (257, NARROW_C + 1), (1025, 64), (64, 1024)])
def test_softmax_rows_lie_within_half_an_ulp_of_the_fp64_restatement(N, C):
    """|got - ref| <= 2^-24 |ref| (1 + 2^-20) + 2^-150: half an fp32 ulp of the fp64 value plus slack for the fp64 evaluation
    (relative error of the order (C + 10) 2^-52, far below 2^-44).  Measured worst ratios: profiles/calibration_accuracy.txt."""
    K = _K()
    x = _logits(N, C)
    xd = _dev(x)
    xs = _strided(xd)
    for beta in (1.0, 0.4, 3.0):
        ref = K.softmax_rows_reference(x, beta=beta)
        got = K.softmax_rows(xd, beta=beta)
        assert got.dtype == torch.float32 and got.is_contiguous() and got.shape == (N, C)
        err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
        bound = 2.0 ** -24 * np.abs(ref) * (1 + 2.0 ** -20) + 2.0 ** -150
        print(f"calibration-accuracy: softmax_rows ({N}, {C}) beta {beta:g}: worst |got - fp64| / bound = {float((err / bound).max()):.4f}")
        assert (err <= bound).all(), (N, C, beta, float((err / bound).max()))
        assert torch.equal(K.softmax_rows(xs, beta=beta), got)                      # bits under stride and misalignment
        assert torch.equal(K.softmax_rows(xd, temperature=1.0 / beta), K.softmax_rows(xd, beta=1.0 / (1.0 / beta)))
        # every output row is a valid row of the counts kernel
        tot = K.calibration_counts(got, torch.zeros(N, dtype=torch.int64, device="cuda"))[1]
        assert tot.tolist()[:2] == [N, 0]
    half = K.softmax_rows(xd[: N // 2 + 1], beta=3.0)
    assert torch.equal(half, got[: N // 2 + 1])                                     # a row's bits depend on the row, C and beta only


def test_softmax_rows_of_non_finite_logits():
    K = _K()
    x = torch.tensor([[0.0, float("-inf"), 1.0], [float("nan"), 0.0, 0.0], [float("inf"), 0.0, 0.0], [1e30, -1e30, 0.0]], device="cuda")
    out = K.softmax_rows(x, 0.5)
    assert out[0, 1] == 0 and float(out[0].sum()) == pytest.approx(1.0, abs=1e-6)
    assert bool(out[1].isnan().all()) and bool(out[2].isnan().all()) and out[3].tolist() == [1.0, 0.0, 0.0]
    wide = torch.zeros(2, 40, device="cuda")
    wide[0, 7], wide[1, 39] = float("nan"), -1e4
    out = K.softmax_rows(wide)
    assert bool(out[0].isnan().all()) and out[1, 39] == 0 and float(out[1, 0]) == pytest.approx(1 / 39, rel=1e-6)


# ------------------------------------------------------------------------------------------------ temperature objective
NLL_SHAPES = [(n, c) for n in NS for c in CS if (n, c) not in ((1, 1), (63, 1), (257, 1), (1025, 1), (3100, 1))] + [(63, 1), (64, 1024)]
BETAS = [0.25, 1.0, 4.0]


@functools.lru_cache(maxsize=None)
def _nll_case(N, C):
    """Logits 2 x normal with bad rows (a NaN, +-inf) and ignored targets among them."""
    x = np.array(_logits(N, C, 2.0))
    u = np.random.default_rng(N * C).random(N)
    if N >= 63:
        x[u < 0.03, 0] = np.nan
        x[(u >= 0.03) & (u < 0.05), C - 1] = np.inf
        x[(u >= 0.05) & (u < 0.07), C // 2] = -np.inf
    x.setflags(write=False)
    return x, _targets(N, C)


@functools.lru_cache(maxsize=None)
def _nll_errors():
    """Per case and sum (nll, g, h): the error of the kernel and of the fp64 restatement against the longdouble restatement,
    relative to the sum of the absolute per-row terms.  One pass over all cases, shared by the tests below."""
    K = _K()
    rows = []
    for N, C in NLL_SHAPES:
        x, y = _nll_case(N, C)
        xd, yd = _dev(x), _dev(y)
        xs = _strided(xd)
        for beta in BETAS:
            got_d = K.temperature_nll(xd, yd, beta=beta)
            assert got_d.dtype == torch.float64 and got_d.shape == (5,)
            again, strided = K.temperature_nll(xd, yd, beta=beta), K.temperature_nll(xs, yd, beta=beta)
            got = got_d.cpu().numpy()
            same = torch.equal(got_d, again) and torch.equal(got_d, strided)
            yard = K.temperature_nll_reference(x, y, beta=beta)
            ref = K.temperature_nll_reference(x, y, beta=beta, dtype=np.longdouble)
            # the scale: sum of |term| per row; nll and h are non-negative, g is not
            valid = (y >= 0) & (y < C) & np.isfinite(x).all(axis=1)
            X = x[valid].astype(np.float64)
            d = X - X.max(axis=1, keepdims=True)
            e = np.exp(beta * d)
            g_abs = float(np.abs((e * d).sum(axis=1) / e.sum(axis=1) - d[np.arange(len(d)), y[valid]]).sum())
            scale = np.array([float(ref[1]), g_abs, float(ref[3])])
            scale[scale == 0] = 1.0
            rows.append({"case": (N, C, beta), "same": same, "counts": (got[0], got[4], float(yard[0]), float(yard[4])),
                         "kernel": np.abs((got[1:4].astype(np.longdouble) - ref[1:4]).astype(np.float64)) / scale,
                         "yard": np.abs((yard[1:4].astype(np.longdouble) - ref[1:4]).astype(np.float64)) / scale})
    return rows


def test_temperature_nll_counts_are_exact_and_results_repeat_bit_for_bit():
    rows = _nll_errors()
    assert len(rows) >= 64
    for r in rows:
        assert r["same"], r["case"]                              # two calls, and stride / misalignment: the same bits
        assert r["counts"][0] == r["counts"][2] and r["counts"][1] == r["counts"][3], r["case"]
    assert any(r["counts"][1] > 0 for r in rows)


@pytest.mark.parametrize("k,name", [(0, "nll"), (1, "g"), (2, "h")])
def test_temperature_nll_sums_against_longdouble_with_the_fp64_restatement_as_the_yardstick(k, name):
    """The project's margins: the RMS of the kernel's error over the cases is at most 1.5 x that of the numpy fp64 restatement
    (per-row terms in fp64, added by math.fsum), its max at most 2.5 x.  Measured: profiles/calibration_accuracy.txt."""
    rows = _nll_errors()
    ker, yard = np.array([r["kernel"][k] for r in rows]), np.array([r["yard"][k] for r in rows])
    rms, yrms, mx, ymx = np.sqrt((ker ** 2).mean()), np.sqrt((yard ** 2).mean()), ker.max(), yard.max()
    print(f"calibration-accuracy: temperature_nll sum {name} over {len(rows)} cases: rms {rms:.3e} (fp64 restatement {yrms:.3e}, "
          f"ratio {rms / yrms:.3f}), max {mx:.3e} (restatement {ymx:.3e}, ratio {mx / ymx:.3f})")
    assert rms <= 1.5 * yrms and mx <= 2.5 * ymx


# -------------------------------------------------------------------------------------------------- temperature scaling
def test_temperature_scaling_fit_meets_the_reference_fit():
    from test_calibration_cpu import fit_case, fit_reference, reference_ece
    K = _K()
    logits, y = fit_case()
    xd, yd = _dev(logits), _dev(y)
    ts = K.TemperatureScaling().fit(xd, yd)
    ref = fit_reference()
    n = 4096
    at_dev = K.temperature_nll_reference(logits, y, beta=ts.beta_)
    print(f"calibration-accuracy: TemperatureScaling.fit (4096, 5): T = {ts.temperature_:.9f} in {ts.n_iter_} evaluations (reference "
          f"{ref['temperature']:.9f} in {ref['n_iter']}), |g_ref| / n at the device's beta = {abs(at_dev[2]) / n:.2e}, "
          f"|beta - beta_ref| = {abs(ts.beta_ - ref['beta']):.2e} (bound {2 * ts.tol * n / at_dev[3]:.2e})")
    assert ts.converged_ and ts.n_ == n and ts.n_bad_ == 0
    assert abs(at_dev[2]) / n <= 2 * ts.tol
    assert abs(ts.beta_ - ref["beta"]) <= 2 * ts.tol * n / at_dev[3]
    assert ts.n_iter_ <= ts.max_iter and ts.nll_after_ <= ts.nll_before_
    assert ts.nll_before_ == pytest.approx(ref["nll_before"], rel=1e-13) and ts.nll_after_ == pytest.approx(ref["nll_after"], rel=1e-13)
    P = ts.predict_proba(xd)
    assert torch.equal(P, K.softmax_rows(xd, beta=ts.beta_))
    before = K.ece_from_counts(K.calibration_counts(K.softmax_rows(xd), yd)[0].cpu())
    after = K.ece_from_counts(K.calibration_counts(P, yd)[0].cpu())
    print(f"calibration-accuracy: ECE through predict_proba {before:.6f} -> {after:.6f} (reference {reference_ece(logits, y, 1.0):.6f} -> "
          f"{reference_ece(logits, y, ref['beta']):.6f})")
    assert after < before
    with pytest.raises(ValueError, match="no valid row"):
        K.TemperatureScaling().fit(xd[:8], torch.full((8,), -100, device="cuda"))
    with pytest.raises(RuntimeError, match="fit first"):
        K.TemperatureScaling().predict_proba(xd)


# ------------------------------------------------------------------------------------------------- CalibrationMetrics
def test_calibration_metrics_over_uneven_batches_equal_one_batch():
    K = _K()
    x, y = _logits(1025, 5), _targets(1025, 5)
    xd, yd = _dev(x), _dev(y)
    one, three = (K.CalibrationMetrics(5, classwise=True, normalize="softmax", temperature=1.7) for _ in range(2))
    one.update(xd, yd)
    for a, b in ((0, 7), (7, 7), (7, 600), (600, 1025)):         # an empty batch among them
        three.update(xd[a:b], yd[a:b].int())
    assert torch.equal(one.acc, three.acc) and torch.equal(one.tot, three.tot)
    want = K.calibration_counts_reference(K.softmax_rows(xd, 1.7).cpu().numpy(), y, classwise=True)
    assert _equal((three.acc, three.tot), want)
    res = three.compute()
    assert set(res) == {"ece", "mce", "brier", "n", "n_bad", "bin_confidence", "bin_accuracy", "bin_count", "classwise_ece",
                        "classwise_ece_per_class"}
    assert res["ece"] == K.ece_from_counts(want[0]) and res["mce"] == K.ece_from_counts(want[0], "max")
    assert res["brier"] == K.brier_from_counts(want[1]) and res["n"] == int(want[1][0]) and res["n_bad"] == 0
    assert res["classwise_ece"] == K.classwise_ece_from_counts(want[0]) and len(res["classwise_ece_per_class"]) == 5
    assert res["bin_count"].sum() == res["n"] and 0 < res["ece"] <= res["mce"] < 1
    three.reset()
    assert int(three.acc.sum()) == 0 and three.compute()["n"] == 0
    plain = K.CalibrationMetrics(5)                              # probabilities given; a bad row warns
    Pd = K.softmax_rows(xd)
    Pd[int(np.nonzero((y >= 0) & (y < 5))[0][0])] *= 0.5
    plain.update(Pd, yd)
    with pytest.warns(RuntimeWarning, match="1 row"):
        assert plain.compute()["n_bad"] == 1


# ------------------------------------------------------------------------------------------- ClipMLP and the probes
def _clip_head(**kw):
    from test_supervised_gpu import _batch, _cuda, _head
    model = _head("classification", seed=11, **kw).cuda().eval()
    val = [_cuda(_batch(32, seed=200)), _cuda(_batch(11, seed=201)), _cuda(_batch(5, seed=202))]
    return model, val


def _validate(model, val):
    with torch.no_grad():
        model.on_validation_start()
        for i, b in enumerate(val):
            model.validation_step(b, i)
        model.on_validation_epoch_end()


def test_clip_mlp_logs_calibration_metrics_when_asked():
    K = _K()
    model, val = _clip_head(calibration_metrics=True)
    assert model.ranking is None
    seen, update = [], model.calibration.update
    model.calibration.update = lambda logits, target: (seen.append(logits.clone()), update(logits, target))[1]   # what the model fed
    _validate(model, val)
    assert [tuple(t.shape) for t in seen] == [(32, 5), (11, 5), (5, 5)]
    y = torch.cat([b[8] for b in val]).to(torch.int64)
    acc, tot = K.calibration_counts(K.softmax_rows(torch.cat(seen)), y)              # direct, on the concatenated logits
    assert torch.equal(model.calibration.acc, acc) and torch.equal(model.calibration.tot, tot)
    assert model.logged["ece_val"] == K.ece_from_counts(acc.cpu()) and model.logged["brier_val"] == K.brier_from_counts(tot.cpu())
    want = K.calibration_counts_reference(K.softmax_rows(torch.cat(seen)).cpu().numpy(), y.cpu().numpy())
    assert _equal((acc, tot), want) and int(tot[0]) == 48
    assert 0.0 < model.logged["ece_val"] < 1.0 and 0.0 < model.logged["brier_val"] < 2.0
    assert set(model.logged) == {"val_loss", "f1_val", "f1_micro_val", "acc_val", "ece_val", "brier_val"}
    first = dict(model.logged)
    model.on_validation_start()                                  # a second epoch starts from nothing
    with torch.no_grad():
        model.validation_step(val[0], 0)
        model.on_validation_epoch_end()
    assert int(model.calibration.tot[0]) == 32
    both, _ = _clip_head(calibration_metrics=True, ranking_metrics=True)
    _validate(both, val)
    assert set(both.logged) == {"val_loss", "f1_val", "f1_micro_val", "acc_val", "auroc_val", "ap_val", "top2_acc_val", "ece_val",
                                "brier_val"}
    assert both.logged["ece_val"] == first["ece_val"] and both.logged["brier_val"] == first["brier_val"]


def test_clip_mlp_logs_todays_keys_without_the_keyword():
    model, val = _clip_head()
    assert model.calibration is None
    _validate(model, val)
    assert set(model.logged) == {"val_loss", "f1_val", "f1_micro_val", "acc_val"}
    ranked, _ = _clip_head(ranking_metrics=True)
    _validate(ranked, val)
    assert set(ranked.logged) == {"val_loss", "f1_val", "f1_micro_val", "acc_val", "auroc_val", "ap_val", "top2_acc_val"}
    from multimodal_supernovae_amd.models_finetune import ClipMLP
    from test_supervised_gpu import _clip
    reg = ClipMLP(_clip(0), regression=True, calibration_metrics=True)               # classification only: nothing for regression
    assert reg.calibration is None


def test_probe_metrics_carry_the_calibration_keys_when_asked():
    from multimodal_supernovae_amd import probes, utils
    from test_probes_cpu import blobs
    K = _K()
    X, y, X2, y2 = (_dev(a) for a in blobs(500, 64, 5, 0.3, seed=500, fresh=True))
    new = {"ece", "mce", "brier"}
    plain = utils.linear_probe_metrics(X, y, X2, y2, task="classification")
    got = utils.linear_probe_metrics(X, y, X2, y2, task="classification", calibration=True)
    assert set(got) - set(plain) == new and {k: got[k] for k in plain} == plain
    scores = probes.LogisticRegressionProbe(n_classes=5).fit(X, y).decision_function(X2)
    acc, tot = K.calibration_counts_reference(K.softmax_rows(scores).cpu().numpy(), y2.cpu().numpy())
    assert got["ece"] == K.ece_from_counts(acc) and got["mce"] == K.ece_from_counts(acc, "max") and got["brier"] == K.brier_from_counts(tot)
    ranked = utils.linear_probe_metrics(X, y, X2, y2, task="classification", ranking=True)
    both = utils.linear_probe_metrics(X, y, X2, y2, task="classification", ranking=True, calibration=True)
    assert set(both) - set(ranked) == new and set(ranked) - set(plain) == {"auroc_macro", "ap_macro", "auroc_per_class", "ap_per_class"}
    plain = utils.knn_probe_metrics(X, y, X2, y2, k=7, task="classification")
    got = utils.knn_probe_metrics(X, y, X2, y2, k=7, task="classification", calibration=True)
    assert set(got) - set(plain) == new and {k: got[k] for k in plain} == plain
    proba = probes.KNeighborsClassifierProbe(n_neighbors=7, n_classes=5).fit(X, y).predict_proba(X2).cpu().numpy()
    acc, tot = K.calibration_counts_reference(proba, y2.cpu().numpy())
    assert got["ece"] == K.ece_from_counts(acc) and got["brier"] == K.brier_from_counts(tot) and tot[0] > 0
    Xr, Yr = torch.randn(200, 16, device="cuda"), torch.rand(200, device="cuda")
    assert set(utils.linear_probe_metrics(Xr, Yr, Xr, Yr, task="regression")) == {"L1", "L2", "R2", "OLF"}
    with pytest.raises(ValueError, match="classification"):
        utils.linear_probe_metrics(Xr, Yr, Xr, Yr, task="regression", calibration=True)
    with pytest.raises(ValueError, match="classification"):
        utils.knn_probe_metrics(Xr, Yr, Xr, Yr, task="regression", calibration=True)


def test_two_ranks_equal_the_single_process_result():
    """Two ranks sharing the GPU over gloo (tools/dist_check_calibration.py): shards of unequal sizes, one rank with an empty last
    batch; acc / tot after all_reduce are torch.equal to one process over all rows, the fitted temperature is identical on both
    ranks and within the bound of the one-process fit."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "dist_check_calibration.py")], capture_output=True, text=True,
                       timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "DIST CHECK OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
