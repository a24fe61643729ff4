"""Robust, Gaussian-NLL and quantile regression losses on the GPU (csrc/regression_loss.hip, models_finetune.py): the kernels
against the longdouble reference within derived bounds, ignored rows, bit-identity over runs, strides and alignments,
cross-checks between the kinds and with masked_mse, the validation statistics against exact numpy restatements, and
ClipMLP(regression=True, loss=...) eager, graph-replayed and on two ranks."""
import copy
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_supervised_gpu as S          # the tiny towers, their batches, and the gate of the cross-entropy tests

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GATE = S.GATE                  # 1e-6 against the reference
FLOOR = 2.0 ** -126
T = 256                        # the kernels' single-workgroup threshold: one row per lane of a 256-thread workgroup
# both sides of every switch: one workgroup / several + the finishing block (T, T + 1), rows that are no multiple of a block
# (4099), 274 partials for the finishing block's 256 threads (70001: some threads add two), and 2048 * 256 + 1, the first N at
# which a lane of the capped grid walks on to a second row
SIZES = [1, 2, T, T + 1, 4099, 70001, 2048 * 256 + 1]
LEVELS = {1: (0.5,), 2: (0.25, 0.75), 3: (0.16, 0.5, 0.84), 16: tuple((q + 1) / 17 for q in range(16))}
KINDS = [("mse", 1), ("l1", 1), ("huber", 1), ("log_cosh", 1), ("gaussian_nll", 2), ("pinball", 1), ("pinball", 2), ("pinball", 3),
         ("pinball", 16)]
DELTA = 0.05                   # half a standard deviation of the residuals: both branches of the Huber loss are taken
CASES = [(kind, K, N) for kind, K in KINDS for N in SIZES if N <= 70001 or (kind, K) in (("huber", 1), ("gaussian_nll", 2), ("pinball", 3))]


def _levels(kind, K):
    return LEVELS[K] if kind == "pinball" else None


@functools.lru_cache(maxsize=4)
def _case(N, K, gaussian=False, holes=True):
    """Redshift-like targets uniform in [0, 1.2), predictions = target + 0.1 normal (the second Gaussian column a normal log
    variance); with `holes` every fifth target is NaN and one is +inf."""
    g = torch.Generator().manual_seed(1000 * N + K)
    y = torch.rand(N, generator=g) * 1.2
    p = y[:, None] + 0.1 * torch.randn(N, K, generator=g)
    if gaussian:
        p[:, 1] = torch.randn(N, generator=g)
    if holes:
        y[4::5] = float("nan")
        if N > 2:
            y[2] = float("inf")
    return p, y


@functools.lru_cache(maxsize=4)
def _reference(kind, K, N):
    """(loss, dpred, sum of A_i / n_valid, n_valid) on _case's draw: computed once, shared, never modified."""
    from multimodal_supernovae_amd.models_finetune import regression_loss_reference
    p, y = _case(N, K, kind == "gaussian_nll")
    loss, dx = regression_loss_reference(p, y, kind, DELTA, _levels(kind, K))
    valid = np.isfinite(y.numpy())
    pv, yv = p.numpy()[valid].astype(np.float64), y.numpy()[valid].astype(np.float64)
    if kind == "gaussian_nll":                 # the parts of the row term can have either sign
        d, s = pv[:, 0] - yv, pv[:, 1]
        a_mean = float((0.5 * (np.abs(s) + d * d * np.exp(-s))).sum()) / valid.sum()
    else:                                      # every part is >= 0: the sum of their absolute values is the term
        a_mean = abs(loss)
    return loss, dx, a_mean, int(valid.sum())


def _run(p, y, kind, K, delta=DELTA, p_dev=None):
    """loss and dpred of the HIP path; p_dev: a prepared (row-strided / offset) device view of p."""
    from multimodal_supernovae_amd.models_finetune import regression_loss
    pd = (p.cuda() if p_dev is None else p_dev).detach().requires_grad_()
    loss = regression_loss(pd, y.cuda(), kind, delta=delta, quantiles=_levels(kind, K))
    loss.backward()
    return loss.detach().cpu(), pd.grad.cpu()


@pytest.mark.parametrize("kind,K,N", CASES)
def test_regression_loss_matches_the_reference(kind, K, N):
    """|loss - ref| <= GATE |ref| + (n + 8) 2^-53 sum_i A_i / n + FLOOR over the n valid rows, A_i the sum of the absolute values
    of the parts of row i's term (the order-independent bound of an fp64 sum plus a few ulps of the device's exp / log1p /
    tanh), and max|dpred - ref| <= GATE max|ref| + FLOOR.  Expected, since the rows are fp64: one fp32 rounding of the loss
    (6e-8: 0.06 of the bound) and two of a gradient entry -- its own and that of the fp32 count the backward divides by, which
    is exact up to 2^24 rows (0.06 of the bound, 0.12 beyond).  Measured on an MI355X over the 57 cases: the worst error / bound
    is 0.043 for the loss and 0.059 for the gradient (profiles/regression_loss_accuracy.txt)."""
    p, y = _case(N, K, kind == "gaussian_nll")
    rl, rdx, a_mean, n = _reference(kind, K, N)
    loss, dx = _run(p, y, kind, K)
    le, lb = abs(float(loss.double()) - rl), GATE * abs(rl) + (n + 8) * 2.0 ** -53 * a_mean + FLOOR
    ge, gb = float(np.abs(dx.double().numpy() - rdx).max()), GATE * float(np.abs(rdx).max()) + FLOOR
    print(f"{kind} K={K} N={N}: loss {float(loss):.9g} ref {rl:.9g} error / bound {le / lb:.3e}; max|dpred - ref| / bound {ge / gb:.3e}")
    assert dx.shape == (N, K)
    assert le <= lb, (kind, K, N, le, lb)
    assert ge <= gb, (kind, K, N, ge, gb)
    hole = torch.from_numpy(~np.isfinite(y.numpy()))
    assert int(hole.sum()) == N // 5 + (1 if N > 2 else 0)
    assert float(dx[hole].abs().sum()) == 0.0                   # exact zeros, not small numbers


@pytest.mark.parametrize("kind,K", KINDS)
def test_no_valid_row_gives_nan_and_a_zero_gradient(kind, K):
    for N in (3, T + 1):
        p, _ = _case(N, K, kind == "gaussian_nll")
        y = torch.full((N,), float("nan"))
        y[1] = float("-inf")
        loss, dx = _run(p, y, kind, K)
        assert torch.isnan(loss) and float(dx.abs().max()) == 0.0 and not bool(torch.isnan(dx).any())


@pytest.mark.parametrize("kind,K", KINDS)
def test_exact_ties_take_the_stated_subgradients(kind, K):
    """Predictions equal to their targets (d = 0, e_q = 0) and, for the Huber loss, |d| = delta exactly."""
    from multimodal_supernovae_amd.models_finetune import regression_loss_reference
    y = torch.tensor([0.5, 0.25, 1.0, 0.75])
    p = y[:, None].repeat(1, K).clone()
    p[1] += 0.5                                                # d = +0.5 = delta, exact in fp32
    p[2] -= 0.5
    if kind == "gaussian_nll":
        p[:, 1] = torch.tensor([0.0, 1.0, -1.0, 2.0])
    loss, dx = _run(p, y, kind, K, delta=0.5)
    rl, rdx = regression_loss_reference(p, y, kind, 0.5, _levels(kind, K))
    assert abs(float(loss) - rl) <= GATE * abs(rl) + FLOOR and float(np.abs(dx.double().numpy() - rdx).max()) <= GATE * float(np.abs(rdx).max()) + FLOOR
    if kind != "gaussian_nll":
        assert float(dx[0].abs().max()) == 0.0 and float(dx[3].abs().max()) == 0.0
    if kind == "huber":
        assert dx[:, 0].tolist() == [0.0, 0.125, -0.125, 0.0]                    # d / 4, not delta sign(d) / 4 rounded another way


@pytest.mark.parametrize("kind,K", KINDS)
def test_runs_strides_and_alignments_give_the_same_bits(kind, K):
    for N in (T, 4099):
        p, y = _case(N, K, kind == "gaussian_nll")
        dense = _run(p, y, kind, K)
        again = _run(p, y, kind, K)
        wide = torch.randn(N, K + 3).cuda()
        wide[:, :K] = p.cuda()
        strided = _run(p, y, kind, K, p_dev=wide[:, :K])                          # ld = K + 3
        flat = torch.zeros(N * K + 1).cuda()
        flat[1:] = p.cuda().reshape(-1)
        assert flat[1:].data_ptr() % 16 == 4
        offset = _run(p, y, kind, K, p_dev=flat[1:].view(N, K))                   # one float past a 16-byte boundary
        for other in (again, strided, offset):
            assert torch.equal(dense[0], other[0]) and torch.equal(dense[1], other[1]), (kind, K, N)


def test_non_finite_predictions_propagate():
    p, y = _case(300, 3)
    for kind, K, bad in (("huber", 1, float("nan")), ("l1", 1, float("inf")), ("gaussian_nll", 2, float("nan")), ("pinball", 3, float("nan"))):
        q = p[:, :K].clone()
        q[7, 0] = bad                                           # row 7 has a finite target
        loss, dx = _run(q, y, kind, K)
        assert not bool(torch.isfinite(loss)), kind
        assert bool(torch.isfinite(dx[:7]).all()) and bool(torch.isfinite(dx[8:]).all())
    q = p[:, :2].clone()
    q[7, 1] = -800.0                                            # exp(800) overflows fp64: it propagates
    assert not bool(torch.isfinite(_run(q, y, "gaussian_nll", 2)[0]))


@pytest.mark.parametrize("N", [T, 4099])
def test_cross_checks_between_the_kinds_and_with_masked_mse(N):
    from multimodal_supernovae_amd.models_pretraining import masked_mse
    p, y = _case(N, 1, False, False)                            # finite targets
    pd = p.cuda().requires_grad_()
    ref = masked_mse(pd.squeeze(1), y.cuda(), torch.ones(N, dtype=torch.uint8, device="cuda"))
    ref.backward()
    mse = _run(p, y, "mse", 1)
    assert abs(float(mse[0]) - float(ref.detach())) <= GATE * float(ref.detach())
    assert float((mse[1] - pd.grad.cpu()).abs().max()) <= GATE * float(pd.grad.abs().max())
    p, y = _case(N, 1)                                          # with ignored rows
    mse, l1 = _run(p, y, "mse", 1), _run(p, y, "l1", 1)
    hub = _run(p, y, "huber", 1, delta=1e30)
    assert abs(float(hub[0]) - 0.5 * float(mse[0])) <= GATE * 0.5 * float(mse[0])
    assert float((hub[1] - 0.5 * mse[1]).abs().max()) <= GATE * 0.5 * float(mse[1].abs().max())
    pin = _run(p, y, "pinball", 1)
    assert abs(float(pin[0]) - 0.5 * float(l1[0])) <= GATE * 0.5 * float(l1[0])
    assert float((pin[1] - 0.5 * l1[1]).abs().max()) <= GATE * 0.5 * float(l1[1].abs().max())


def test_the_callers_denominator_replaces_the_local_one():
    """The kernel's own interface: out = {numerator / denom_in, valid rows, numerator}."""
    from multimodal_supernovae_amd._lib import check, lib, ptr, stream_ptr
    from multimodal_supernovae_amd.models_finetune import regression_loss_reference
    for N in (100, 9000):
        p, y = _case(N, 1)
        rl = regression_loss_reference(p, y, "huber", DELTA)[0]
        n = int(np.isfinite(y.numpy()).sum())
        pd, yd = p.cuda(), y.cuda()
        nb = lib().msn_regression_loss_workspace_bytes(N, 1)
        ws = torch.empty(max(nb, 8), dtype=torch.uint8, device="cuda")
        for denom_in, den in ((None, float(n)), (torch.tensor([123.5], device="cuda"), 123.5)):
            out = torch.empty(3, device="cuda")
            check(lib().msn_regression_loss_fwd(ptr(pd), 1, ptr(yd), N, 1, 2, DELTA, ptr(None), ptr(denom_in), ptr(out), ptr(ws), nb,
                                                stream_ptr()), "msn_regression_loss_fwd")
            out = out.cpu().double()
            assert float(out[1]) == float(n)                                       # the count is an exact integer
            assert abs(float(out[2]) - rl * n) <= GATE * rl * n and abs(float(out[0]) - rl * n / den) <= GATE * rl * n / den


# ------------------------------------------------------------------------------------------------ validation statistics
def _six(p, y):
    """The six sums of msn_regression_stats in fp64 over the finite-target rows."""
    v = np.isfinite(y)
    d, yy = p[v].astype(np.float64) - y[v].astype(np.float64), y[v].astype(np.float64)
    return [float(v.sum()), np.abs(d).sum(), (d * d).sum(), yy.sum(), (yy * yy).sum(), float((np.abs(d) / (1 + yy) > 0.15).sum())]


def _close(got, want, rel=1e-12):
    return all(abs(a - b) <= rel * abs(b) for a, b in zip(got, want))


@pytest.mark.parametrize("N", [1, T, T + 1, 70001])
def test_point_mode_sums_agree_with_regression_metrics(N):
    from multimodal_supernovae_amd.models_finetune import IntervalMetrics, RegressionMetrics
    p, y = _case(N, 1, False, False)
    old, new = RegressionMetrics(), IntervalMetrics("point")
    for _ in range(2):
        old.update(p.cuda().squeeze(1), y.cuda())
        new.update(p.cuda(), y.cuda())
    a, b = old.sums.cpu().tolist(), new.acc.cpu().tolist()
    print(f"N={N}: relative differences of the six sums {[abs(u - v) / max(abs(u), 1e-300) for u, v in zip(a, b)]}")
    assert b[0] == a[0] == 2 * N and b[5] == a[5] and int(new.cnt[0]) == 2 * N
    assert _close(b[:6], a) and b[6:] == [0.0, 0.0] and new.cnt[1:].abs().sum().item() == 0
    if N > 1:                                                   # (one point has no variance: R2 is 0 / 0 either way)
        assert new.compute() == pytest.approx(old.compute(), rel=1e-9)
    p, y = _case(N, 1)                                       # rows without a finite target do not count
    new.reset()
    new.update(p.cuda().squeeze(1), y.cuda())                   # (N,) predictions are taken as (N, 1)
    want = _six(p.numpy()[:, 0], y.numpy())
    got = new.acc.cpu().tolist()
    assert got[0] == want[0] and got[5] == want[5] and int(new.cnt[0]) == int(want[0]) and _close(got[:6], want)


@pytest.mark.parametrize("N,K", [(N, K) for N in (T, T + 1, 70001) for K in (1, 2, 3, 16)] + [(2048 * 256 + 1, 3)])
def test_quantile_mode_counts_are_exact(N, K):
    """Every integer of the quantile mode against numpy in fp32 compares: no tolerance.  Rows with a crossed pair, a NaN
    prediction (below nothing) and predictions equal to the target are in the data.  (The capped grid is a property of N:
    one K at that size.)"""
    from multimodal_supernovae_amd.models_finetune import IntervalMetrics
    p, y = _case(N, K)
    p = torch.sort(p, dim=1).values.clone()
    p[1::7] = p[1::7].flip(1)                                   # crossed where K > 1
    p[3::11, 0] = float("nan")
    p[5::13, K - 1] = y[5::13]                                  # y <= pred_q with equality
    m = IntervalMetrics("quantile", LEVELS[K])
    m.update(p.cuda(), y.cuda())
    pn, yn = p.numpy(), y.numpy()
    v = np.isfinite(yn)
    with np.errstate(invalid="ignore"):
        below = [int((yn[v] <= pn[v, q]).sum()) for q in range(K)]
        inside = int(((pn[v, 0] <= yn[v]) & (yn[v] <= pn[v, K - 1])).sum())
        crossed = int((pn[v, :-1] > pn[v, 1:]).any(axis=1).sum()) if K > 1 else 0
    want = [int(v.sum()), inside, crossed] + below + [0] * (16 - K)
    assert m.cnt.cpu().tolist() == want
    assert K == 1 or (crossed > 0 and inside < want[0])
    ok = v & np.isfinite(pn).all(axis=1)                         # the fp64 sums on the rows without a NaN prediction
    m.reset()
    m.update(p[torch.from_numpy(ok)].cuda(), y[torch.from_numpy(ok)].cuda())
    pv, yv, tau = pn[ok].astype(np.float64), yn[ok].astype(np.float64), np.array(LEVELS[K])
    e = yv[:, None] - pv
    width = pv[:, K - 1] - pv[:, 0]                             # either sign where the row is crossed
    sums = _six(pn[ok][:, m.mid], yn[ok]) + [width.sum(), np.maximum(tau * e, (tau - 1) * e).mean(axis=1).sum()]
    scale = sums[:6] + [np.abs(width).sum(), sums[7]]           # an fp64 sum is known relative to the sum of its terms' magnitudes
    got = m.acc.cpu().tolist()
    assert got[0] == sums[0] and got[5] == sums[5]
    assert all(abs(a - b) <= 1e-12 * s for a, b, s in zip(got, sums, scale)), (got, sums)


@pytest.mark.parametrize("N", [T, T + 1, 70001])
def test_gaussian_mode_counts_are_exact_away_from_the_boundaries(N):
    from multimodal_supernovae_amd.models_finetune import IntervalMetrics
    p, y = _case(N, 2, True)
    p = p.clone()
    p[:, 1] += 2.0 * math.log(0.1)                              # sigma around the residuals' 0.1: every count differs
    m = IntervalMetrics("gaussian")
    m.update(p.cuda(), y.cuda())
    v = np.isfinite(y.numpy())
    ld = np.longdouble
    d = np.abs(p.numpy()[v, 0].astype(ld) - y.numpy()[v].astype(ld))
    sigma = np.exp(p.numpy()[v, 1].astype(ld) / 2)
    for k in (1, 2, 3):                                         # the reference's own assertion: no row sits on a boundary
        assert float(np.abs(d / (k * sigma) - 1).min()) >= 1e-9
    want = [int(v.sum())] + [int((d <= k * sigma).sum()) for k in (1, 2, 3)]
    assert m.cnt.cpu().tolist() == want + [0] * 15
    assert want[1] < want[2] < want[3] <= want[0]
    sums = _six(p.numpy()[:, 0], y.numpy()) + [float(sigma.sum()), float(((d / sigma) ** 2).sum())]
    got = m.acc.cpu().tolist()
    assert got[0] == sums[0] and got[5] == sums[5] and _close(got, sums)


@pytest.mark.parametrize("mode,K", [("gaussian", 2), ("quantile", 3)])
def test_cutting_an_epoch_into_batches_changes_no_count(mode, K):
    from multimodal_supernovae_amd.models_finetune import IntervalMetrics
    p, y = _case(4099, K, mode == "gaussian")
    q = LEVELS[K] if mode == "quantile" else None
    whole, cut = IntervalMetrics(mode, q), IntervalMetrics(mode, q)
    whole.update(p.cuda(), y.cuda())
    for a, b in ((0, 100), (100, 100 + T + 1), (100 + T + 1, 4099)):
        cut.update(p[a:b].cuda(), y[a:b].cuda())
    assert torch.equal(whole.cnt, cut.cnt) and int(whole.cnt[0]) > 0
    assert _close(cut.acc.cpu().tolist(), whole.acc.cpu().tolist())
    assert cut.compute() == pytest.approx(whole.compute(), rel=1e-12)


# ------------------------------------------------------------------------------------------------------- the module
LOSSES = {"huber": dict(loss="huber", loss_kwargs={"delta": 0.1}), "gaussian_nll": dict(loss="gaussian_nll"), "quantile": dict(loss="quantile")}
KEYS = {"huber": set(), "gaussian_nll": {"sigma_val", "z2_val", "cov1_val", "cov2_val"}, "quantile": {"coverage_val", "width_val", "crossing_val"}}
POINT_KEYS = {"val_loss", "L1_val", "L2_val", "R2_val", "OLF_val"}


def _torch_loss(h, y, name):
    """The loss of a head output in plain torch."""
    if name == "huber":
        return F.huber_loss(h.squeeze(1), y, delta=0.1)
    if name == "gaussian_nll":
        return F.gaussian_nll_loss(h[:, 0], y, var=torch.exp(h[:, 1]), full=False, eps=0.0)
    tau = torch.tensor([0.16, 0.5, 0.84])[None, :]
    e = y[:, None] - h
    return torch.maximum(tau * e, (tau - 1.0) * e).mean()


def _restated_loss(P, H, batch, name):
    """S._restated_loss with this file's losses: oracle towers -> concatenated embeddings -> plain-torch MLP -> torch loss."""
    from oracle import clip as oclip
    h = torch.cat(oclip.embeddings(P, S.CFG, batch, training=True), dim=1)
    idx = sorted({int(k.split(".")[1]) for k in H})
    for j, i in enumerate(idx):
        h = F.linear(h, H[f"layers.{i}.weight"], H[f"layers.{i}.bias"])
        if j < len(idx) - 1:
            h = F.relu(h)
    return _torch_loss(h, batch[7], name)


@pytest.mark.parametrize("name", sorted(LOSSES))
def test_module_step_matches_plain_torch_restatement(name):
    """An eager step against the restated head and loss at the tolerance of S.test_module_matches_plain_torch_restatement."""
    B = 7
    model = S._head("regression", seed=50, **LOSSES[name])
    P = {k: v.detach().clone().requires_grad_(v.is_floating_point()) for k, v in model.clip_model.state_dict().items()}
    H = {k: v.detach().clone().requires_grad_() for k, v in model.mlp.state_dict().items()}
    batch = S._batch(B, seed=B)
    ref = _restated_loss(P, H, batch, name)
    ref.backward()
    model.cuda().train()
    loss = model.training_step(S._cuda(batch), 0)
    err = abs(float(loss.detach()) - float(ref.detach()))
    print(f"{name}: loss {float(loss.detach()):.7g} restated {float(ref.detach()):.7g}")
    assert err <= 1e-5 + 1e-3 * abs(float(ref.detach()))
    assert float(model.logged["train_loss"]) == float(loss.detach())
    loss.backward()
    want_all = {"clip_model." + k: v for k, v in P.items() if v.requires_grad}
    want_all.update({"mlp." + k: v for k, v in H.items()})
    for k, p in model.named_parameters():
        if k in ("clip_model.logit_scale", "clip_model.logit_bias"):
            assert p.grad is None
            continue
        want = want_all[k].grad if want_all[k].grad is not None else torch.zeros_like(want_all[k])
        got = p.grad.cpu() if p.grad is not None else torch.zeros_like(want)
        scale = float(want.abs().max()) + 1e-6
        assert float((got - want).abs().max()) <= 2e-3 * scale + 1e-6, (k, float((got - want).abs().max()), scale)


@pytest.mark.parametrize("name", sorted(LOSSES))
def test_steps_lower_the_loss_and_validation_logs_the_listed_keys(name):
    from multimodal_supernovae_amd.models_finetune import IntervalMetrics, interval_metrics
    model = S._head("regression", seed=12, learning_rate=1e-2, **LOSSES[name]).cuda().train()
    batch = list(S._cuda(S._batch(32, seed=4)))
    batch[7] = batch[7].clone()
    batch[7][3], batch[7][20] = float("nan"), float("inf")              # two objects without a spectroscopic redshift
    opt = model.configure_optimizers()["optimizer"]
    losses = []
    for _ in range(20):
        opt.zero_grad(set_to_none=True)
        loss = model.training_step(tuple(batch), 0)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print(f"{name} over twenty steps:", [round(v, 5) for v in losses])
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
    model.eval()
    model.logged.clear()
    model.on_validation_start()
    with torch.no_grad():
        model.validation_step(tuple(batch), 0)
        model.validation_step(S._cuda(S._batch(11, seed=5)), 1)
    model.on_validation_epoch_end()
    assert set(model.logged) == POINT_KEYS | KEYS[name] and isinstance(model.metrics, IntervalMetrics)
    assert int(model.metrics.cnt[0]) == 30 + 11
    res = interval_metrics(model.metrics.cnt.cpu().tolist(), model.metrics.acc.cpu().tolist(), model.metrics.mode, model.metrics.quantiles)
    assert model.logged["L1_val"] == res["L1"] and all(math.isfinite(float(model.logged[k])) for k in model.logged)
    if name == "quantile":
        assert model.logged["coverage_val"] == res["coverage"] and 0.0 <= res["coverage"] <= 1.0


def test_the_default_regression_model_is_untouched():
    """loss=None: masked_mse and RegressionMetrics, the same logged keys, and the same bits as the explicit masked MSE."""
    from multimodal_supernovae_amd.models_finetune import RegressionMetrics
    from multimodal_supernovae_amd.models_pretraining import masked_mse
    model = S._head("regression", seed=6).cuda()
    batch = S._cuda(S._batch(16, seed=9))
    model.train()
    loss = model.training_step(batch, 0)
    with torch.no_grad():
        pred = model(*batch).squeeze(1)
    assert torch.equal(loss.detach(), masked_mse(pred, batch[7], torch.ones(16, dtype=torch.uint8, device="cuda")))
    explicit = S._head("regression", seed=6, loss="mse").cuda().train()
    other = float(explicit.training_step(batch, 0).detach())
    assert abs(other - float(loss.detach())) <= GATE * float(loss.detach())    # fp32 rounding apart, not bit for bit
    model.eval()
    model.logged.clear()
    model.on_validation_start()
    with torch.no_grad():
        model.validation_step(batch, 0)
    model.on_validation_epoch_end()
    assert set(model.logged) == POINT_KEYS and isinstance(model.metrics, RegressionMetrics)


def test_graphed_quantile_step_equals_eager_steps():
    from multimodal_supernovae_amd.trainer import GraphedTrainStep
    steps = 9                                           # crosses RAdam's rectification switch (rho_t > 5 from step 6)
    batches = [S._cuda(S._batch(8, seed=s)) for s in range(steps)]
    eager = S._head("regression", seed=7, learning_rate=3e-3, optimizer_kwargs={"weight_decay": 1e-3}, **LOSSES["quantile"]).cuda().train()
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
    assert losses_e[0] != losses_e[-1]


def test_two_rank_regression_step_equals_single_process_global_batch():
    """Two ranks sharing the GPU over gloo (tools/dist_check_regression.py): loss and gradients of the data-parallel Huber,
    Gaussian-NLL and quantile steps equal the single-process step at the doubled batch, with three NaN targets on one rank
    and one on the other; both ranks report the same train_loss."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "dist_check_regression.py")], capture_output=True, text=True,
                       timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "DIST CHECK OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
