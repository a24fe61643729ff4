"""Barlow Twins (loss.barlow_twins_loss, csrc/barlow.hip, LightCurveImageCLIP(loss="barlow")) without a GPU: the longdouble
restatements (loss.barlow_twins_reference, embedding_metrics.cross_correlation_reference) against torch.autograd in fp64 of the
paper's code form and against numpy.cov / numpy.corrcoef, the refusals, the C-ABI (declared, bound, resolved, the plan behind the
workspace sizes, every refusal with made-up addresses), the scratch report of the kernels, and the constructor of the model."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["msn_cross_cov_workspace_bytes", "msn_cross_cov", "msn_barlow_workspace_bytes", "msn_barlow_fwd", "msn_barlow_bwd"]

TK = dict(n_out=16, emb=16, heads=2, depth=1, dropout=0.0, time_norm=20583.37, agg="mean")
SK = dict(n_out=16, emb=16, heads=2, depth=1, dropout=0.0, time_norm=17945.14, agg="mean")


def cdiv(a, b):
    return -(-a // b)


def _rows(n, d, seed, base=None):
    """fp32 rows that are not unit-norm and not centred: normal values scaled column by column, plus an offset; with `base`,
    that set plus noise (partners are correlated, as two towers' embeddings of one object are)."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d)) * np.where(np.arange(d) % 2 == 0, 0.25, 4.0) + 0.5
    if base is not None:
        X = base.astype(np.float64) + 0.3 * X
    return X.astype(np.float32)


def _towers(n, d, towers, seed):
    first = _rows(n, d, seed)
    return [first] + [_rows(n, d, seed + k, base=first) for k in range(1, towers)]


def _off_diagonal(c):
    n = c.shape[0]
    return c.flatten()[:-1].view(n - 1, n + 1)[:, 1:].flatten() if n > 1 else c.new_zeros(0)


def _bn(x, eps):
    """BatchNorm1d(affine=False) in training mode, written out: the biased variance, eps inside the root."""
    return (x - x.mean(dim=0)) / torch.sqrt(x.var(dim=0, unbiased=False) + eps)


def _paper(embs, lambd, eps):
    """The published code form, pair by pair: c = bn(x).T @ bn(y) / N, on_diag + lambd * off_diag."""
    total = 0.0
    for i in range(len(embs)):
        for j in range(i + 1, len(embs)):
            x, y = embs[i], embs[j]
            c = (_bn(x, eps).T @ _bn(y, eps)) / x.shape[0]
            on_diag = torch.diagonal(c).add(-1).pow(2).sum()
            off_diag = _off_diagonal(c).pow(2).sum()
            total = total + on_diag + lambd * off_diag
    return total


def _against_autograd(X, lambd, eps, upstream=1.0):
    """The gradient within 1e-12 of the summed magnitudes of its terms, |Yc A^T| + |Xc diag(d)| (where c is close to +-1, as at
    (2, 1), the two nearly cancel and plain fp64 autograd itself is only good to 1.7e-11 of the net value)."""
    from multimodal_supernovae_amd.loss import barlow_twins_reference
    T = [torch.from_numpy(x.astype(np.float64)).requires_grad_(True) for x in X]
    want = _paper(T, lambd, eps)
    grads = torch.autograd.grad(want * upstream, T)
    loss, got, terms = barlow_twins_reference(X, lambd, eps, return_terms=True)
    want = float(want.detach())
    assert np.isfinite(want) and abs(float(loss) - want) <= 1e-12 * max(1.0, abs(want)), (float(loss), want)
    for g, w, mag in zip(got, grads, terms["magnitude"]):
        assert g.dtype == np.longdouble and g.shape == tuple(w.shape) and bool(torch.isfinite(w).all())
        scale = abs(upstream) * float(mag.max())
        assert scale > 0
        assert float(np.abs((upstream * g).astype(np.float64) - w.numpy()).max()) <= 1e-12 * scale


@pytest.mark.parametrize("towers", [2, 3])
@pytest.mark.parametrize("n,d", [(2, 1), (5, 3), (33, 12), (130, 70)])
def test_reference_equals_autograd_of_the_paper_form(n, d, towers):
    X = _towers(n, d, towers, 100 * n + 10 * d)
    for lambd in (0.0, 5e-3):
        _against_autograd(X, lambd, 1e-5)
    _against_autograd(X, 5e-3, 1e-2, upstream=-3.5)


@pytest.mark.parametrize("n,d", [(5, 3), (33, 12)])
def test_a_constant_column_stays_finite(n, d):
    """v = 0: the standardised column is 0 / sqrt(eps) = 0, its row and column of c are 0, the loss and the gradient finite."""
    from multimodal_supernovae_amd.loss import barlow_twins_reference
    X = _towers(n, d, 2, 7 * n + d)
    X[0][:, 1] = 0.75
    loss, grads, terms = barlow_twins_reference(X, 5e-3, 1e-5, return_terms=True)
    c = terms["corr"][(0, 1)]
    assert float(np.abs(c[1]).max()) == 0.0 and np.isfinite(float(loss)) and all(np.isfinite(g.astype(np.float64)).all() for g in grads)
    _against_autograd(X, 5e-3, 1e-5)
    _against_autograd(X, 0.0, 1e-5, upstream=0.25)


def test_one_column_has_no_off_diagonal_term():
    from multimodal_supernovae_amd.loss import barlow_twins_reference
    X = _towers(9, 1, 2, 3)
    a = barlow_twins_reference(X, 5e-3, 1e-5, return_terms=True)
    b = barlow_twins_reference(X, 7.0, 1e-5)
    assert a[2]["off"][(0, 1)] == 0 and a[2]["on"][(0, 1)] > 0
    assert a[0] == b[0] and all(np.array_equal(g, h) for g, h in zip(a[1], b[1]))


@pytest.mark.parametrize("n,d", [(2, 1), (3, 2), (40, 7), (129, 33)])
def test_cross_correlation_reference_equals_numpy(n, d):
    """As eps -> 0: the (X, Y) block of numpy.cov(ddof=0) and of numpy.corrcoef of the stacked columns."""
    from multimodal_supernovae_amd.embedding_metrics import cross_correlation_reference
    X, Y = _towers(n, d, 2, n + d)
    mx, my, vx, vy, cov, corr = cross_correlation_reference(X, Y, eps=1e-300)
    assert all(a.dtype == np.longdouble for a in (mx, my, vx, vy, cov, corr))
    assert mx.shape == my.shape == vx.shape == vy.shape == (d,) and cov.shape == corr.shape == (d, d)
    both = np.concatenate([X, Y], axis=1).astype(np.float64)
    full = np.cov(both, rowvar=False, ddof=0).reshape(2 * d, 2 * d)
    assert np.abs(cov.astype(np.float64) - full[:d, d:]).max() <= 1e-12 * np.abs(full).max()
    assert np.abs(vx.astype(np.float64) - np.diag(full)[:d]).max() <= 1e-12 * np.abs(full).max()
    assert np.abs(vy.astype(np.float64) - np.diag(full)[d:]).max() <= 1e-12 * np.abs(full).max()
    assert np.abs(mx.astype(np.float64) - X.astype(np.float64).mean(axis=0)).max() <= 1e-14 * np.abs(X).max()
    assert np.abs(my.astype(np.float64) - Y.astype(np.float64).mean(axis=0)).max() <= 1e-14 * np.abs(Y).max()
    if n > 2:                                                  # two rows: every correlation is +-1 and corrcoef's rounding decides
        want = np.corrcoef(both, rowvar=False).reshape(2 * d, 2 * d)[:d, d:]
        assert np.abs(corr.astype(np.float64) - want).max() <= 1e-12
    # eps enters inside the root
    with_eps = cross_correlation_reference(X, Y, eps=0.5)[5]
    want = cov / np.outer(np.sqrt(vx + np.longdouble(0.5)), np.sqrt(vy + np.longdouble(0.5)))
    assert np.abs((with_eps - want).astype(np.float64)).max() <= 1e-15
    with pytest.raises(ValueError):
        cross_correlation_reference(X[:1], Y[:1])
    with pytest.raises(ValueError):
        cross_correlation_reference(X, Y[:, :-1] if d > 1 else Y[:-1])


def test_refusals_come_before_the_gpu_is_asked_for(monkeypatch):
    from multimodal_supernovae_amd import _lib, embedding_metrics as E, loss as Lo
    X = torch.from_numpy(_rows(8, 4, 1))
    asked = []
    monkeypatch.setattr(_lib, "require_gpu", lambda: asked.append(1))
    for kw, word in ((dict(lambd=-1.0), "lambd"), (dict(lambd=float("nan")), "lambd"), (dict(lambd=float("inf")), "lambd"),
                     (dict(eps=0.0), "eps"), (dict(eps=float("nan")), "eps"), (dict(eps=-1e-4), "eps"), (dict(eps=float("inf")), "eps")):
        with pytest.raises(ValueError, match=word + " must be finite"):
            Lo.barlow_twins_loss(X, X, **kw)
    with pytest.raises(ValueError, match="at least two"):
        Lo.barlow_twins_loss_multimodal([X])
    with pytest.raises(ValueError, match="eps must be finite and positive"):
        E.cross_correlation(X, X, eps=0.0)
    assert asked == []                                       # as _vicreg_args: the values first, then the device
    # CPU tensors, then the shapes
    with pytest.raises(_lib.MsnHipError, match="must live on the GPU"):
        Lo.barlow_twins_loss(X, X)
    assert asked == [1]
    monkeypatch.setattr(Lo, "_device_f32", lambda *named: None)
    with pytest.raises(ValueError, match="one shape"):
        Lo.barlow_twins_loss(X, X[:7])
    with pytest.raises(_lib.MsnHipError, match="N must be at least 2"):
        Lo.barlow_twins_loss(X[:1], X[:1])
    with pytest.raises(_lib.MsnHipError, match=r"D must be in 1\.\.256"):
        Lo.barlow_twins_loss(torch.zeros(4, 257), torch.zeros(4, 257))
    with pytest.raises(_lib.MsnHipError, match=r"D must be in 1\.\.256"):
        Lo.barlow_twins_loss(torch.zeros(4, 0), torch.zeros(4, 0))
    # sharded: statistics over gathered rows are not built
    monkeypatch.setattr(Lo, "_is_sharded", lambda global_negatives, group: bool(global_negatives))
    with pytest.raises(NotImplementedError, match="global_negatives=False"):
        Lo.barlow_twins_loss(X, X)
    with pytest.raises(ValueError):
        Lo.barlow_twins_reference([X.numpy()])
    with pytest.raises(ValueError):
        Lo.barlow_twins_reference([X.numpy(), X.numpy()[:7]])
    monkeypatch.undo()
    with pytest.raises(_lib.MsnHipError):                     # no CPU path
        E.cross_correlation(X, X)


# ---------------------------------------------------------------------------------------------------------- the C-ABI
def xcov_plan(N, D):
    """The plan of include/msn_hip.h: (mrows, mslabs, pairs, per, slabs)."""
    mrows = max(64, cdiv(N, 64))
    T = cdiv(D, 64)
    pairs = T * T
    chunks = cdiv(N, 32)
    per = max(4, cdiv(chunks, cdiv(512, pairs)))
    return mrows, cdiv(N, mrows), pairs, per, cdiv(chunks, per)


def test_entry_points_declared_bound_and_resolved():
    from multimodal_supernovae_amd import _lib
    header = open(os.path.join(ROOT, "include", "msn_hip.h")).read()
    handle = _lib.lib()
    for name in ENTRY_POINTS:
        assert name in _lib.SIGNATURES, f"{name} is not bound in _lib.py"
        assert getattr(handle, name) is not None
        decl = re.search(r"\b" + name + r"\(([^;]*)\);", header)
        assert decl, f"{name} is not declared in include/msn_hip.h"
        assert len(_lib.SIGNATURES[name][1]) == decl.group(1).count(",") + 1, name
    cov, bt = handle.msn_cross_cov_workspace_bytes, handle.msn_barlow_workspace_bytes
    assert cov(1, 4) == 0 and cov(2 ** 31, 4) == 0 and cov(8, 0) == 0 and cov(8, 257) == 0
    assert bt(0) == 0 and bt(257) == 0 and bt(-1) == 0
    for n, d in [(2, 1), (65, 33), (130, 128), (200, 256), (1100, 4), (2100, 256), (4096, 128), (10 ** 6, 130)]:
        _, mslabs, pairs, _, slabs = xcov_plan(n, d)
        assert cov(n, d) == 8 * (2 * mslabs * d + 2 * slabs * d + 4096 * slabs * pairs), (n, d)
        assert bt(d) == 16 * min(cdiv(d * d, 256), 64), d


def test_every_refusal_returns_msn_err_shape_without_a_gpu():
    """The refusals come before any launch and never follow a pointer: made-up addresses do."""
    from multimodal_supernovae_amd import _lib
    L = _lib.lib()
    X, Y, MEAN, COV, WS, OUT, G = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000
    big = 1 << 40

    def cov(x=X, ldx=4, y=Y, ldy=4, n=8, d=4, mx=MEAN, my=MEAN + 64, vx=MEAN + 128, vy=MEAN + 192, c=COV, ws=WS, nb=big):
        return L.msn_cross_cov(x, ldx, y, ldy, n, d, mx, my, vx, vy, c, ws, nb, None)

    def fwd(vx=MEAN, vy=MEAN + 64, c=COV, n=8, d=4, lambd=5e-3, eps=1e-5, loss=OUT, comp=OUT + 8, corr=COV + 512, mx=COV + 1024,
            my=COV + 2048, dx=MEAN + 128, dy=MEAN + 192, ws=WS, nb=big):
        return L.msn_barlow_fwd(vx, vy, c, n, d, lambd, eps, loss, comp, corr, mx, my, dx, dy, ws, nb, None)

    def bwd(x=X, ldx=4, y=Y, ldy=4, n=8, d=4, mx=MEAN, my=MEAN + 64, Mx=COV, My=COV + 512, dx=MEAN + 128, dy=MEAN + 192, g=G, gx=OUT,
            lddx=4, gy=OUT + 4096, lddy=4):
        return L.msn_barlow_bwd(x, ldx, y, ldy, n, d, mx, my, Mx, My, dx, dy, g, gx, lddx, gy, lddy, None)

    nan, inf = float("nan"), float("inf")
    need = 8 * (2 * 4 + 2 * 4 + 4096)
    refused = {
        "cov D = 0": cov(d=0, ldx=1, ldy=1), "cov D = 257": cov(d=257, ldx=300, ldy=300), "cov N = 1": cov(n=1), "cov N = 2^31": cov(n=2 ** 31),
        "cov null X": cov(x=0), "cov null Y": cov(y=0), "cov null mean_x": cov(mx=0), "cov null mean_y": cov(my=0), "cov null var_x": cov(vx=0),
        "cov null var_y": cov(vy=0), "cov null cov": cov(c=0), "cov row stride x": cov(ldx=3), "cov row stride y": cov(ldy=3),
        "cov misaligned X": cov(x=X + 2), "cov misaligned Y": cov(y=Y + 1), "cov misaligned mean_x": cov(mx=MEAN + 4),
        "cov misaligned var_y": cov(vy=MEAN + 196), "cov misaligned cov": cov(c=COV + 4), "cov misaligned workspace": cov(ws=WS + 4),
        "cov null workspace": cov(ws=0, nb=0), "cov workspace too small": cov(nb=need - 1),
        "fwd D = 0": fwd(d=0), "fwd D = 257": fwd(d=257), "fwd N = 1": fwd(n=1), "fwd N = 2^31": fwd(n=2 ** 31),
        "fwd lambd < 0": fwd(lambd=-1.0), "fwd lambd nan": fwd(lambd=nan), "fwd lambd inf": fwd(lambd=inf), "fwd eps = 0": fwd(eps=0.0),
        "fwd eps < 0": fwd(eps=-1.0), "fwd eps nan": fwd(eps=nan), "fwd eps inf": fwd(eps=inf), "fwd null var_x": fwd(vx=0),
        "fwd null var_y": fwd(vy=0), "fwd null cov": fwd(c=0), "fwd null loss": fwd(loss=0), "fwd null comp": fwd(comp=0),
        "fwd null corr": fwd(corr=0), "fwd null M_x": fwd(mx=0), "fwd null M_y": fwd(my=0), "fwd null d_x": fwd(dx=0), "fwd null d_y": fwd(dy=0),
        "fwd misaligned comp": fwd(comp=OUT + 4), "fwd misaligned loss": fwd(loss=OUT + 2), "fwd misaligned corr": fwd(corr=COV + 516),
        "fwd null workspace": fwd(ws=0, nb=0), "fwd misaligned workspace": fwd(ws=WS + 4), "fwd workspace too small": fwd(nb=16 - 1),
        "bwd D = 0": bwd(d=0), "bwd D = 257": bwd(d=257, ldx=300, ldy=300, lddx=300, lddy=300), "bwd N = 1": bwd(n=1), "bwd N = 2^31": bwd(n=2 ** 31),
        "bwd null X": bwd(x=0), "bwd null Y": bwd(y=0), "bwd null mean_x": bwd(mx=0), "bwd null mean_y": bwd(my=0), "bwd null M_x": bwd(Mx=0),
        "bwd null M_y": bwd(My=0), "bwd null d_x": bwd(dx=0), "bwd null d_y": bwd(dy=0), "bwd null g": bwd(g=0), "bwd null dX": bwd(gx=0),
        "bwd null dY": bwd(gy=0), "bwd row stride x": bwd(ldx=3), "bwd row stride y": bwd(ldy=3), "bwd row stride dX": bwd(lddx=3),
        "bwd row stride dY": bwd(lddy=3), "bwd misaligned M_x": bwd(Mx=COV + 4), "bwd misaligned d_y": bwd(dy=MEAN + 196),
        "bwd misaligned dX": bwd(gx=OUT + 2), "bwd misaligned g": bwd(g=G + 1),
    }
    assert {k: v for k, v in refused.items() if v != 1} == {}
    assert L.msn_last_error()


def test_barlow_kernels_compile_for_gfx950_without_scratch(tmp_path):
    """hipcc's resource report for every kernel of barlow.hip through tools/check_scratch.py: 0 bytes of scratch (the fp64
    accumulators of the Gram and of the backward's product, and the rows fetched a step early, stay in registers)."""
    from multimodal_supernovae_amd import build as B
    src = os.path.join(B.CSRC, "barlow.hip")
    r = subprocess.run([B.HIPCC] + B.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "barlow.o")],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    remarks = tmp_path / "barlow.remarks"
    remarks.write_text(r.stderr)
    names = re.findall(r"remark: Function Name: (\S+)", r.stderr)
    assert len(names) == 3 + 2 + 1, names           # sums, Gram, finish; coefficients, finish; the backward
    for kind in ["xcov_sum", "xcov_gram", "xcov_finish", "barlow_coef", "barlow_finish", "barlow_bwd"]:
        assert any(kind in n for n in names), f"no kernel named {kind}* in barlow.hip"
    c = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_scratch.py"), str(remarks), "--", "xcov_", "barlow_"],
                       capture_output=True, text=True, timeout=60)
    print(c.stdout)
    assert c.returncode == 0 and f"scratch check: {len(names)} kernels -> OK" in c.stdout, c.stdout + c.stderr


# ---------------------------------------------------------------------------------------------------------- the model
def _clip(**kw):
    from multimodal_supernovae_amd.models_multimodal import LightCurveImageCLIP
    return LightCurveImageCLIP(enc_dim=32, nband=2, transformer_kwargs=TK, transformer_spectral_kwargs=SK,
                               combinations=["lightcurve", "spectral"], **kw)


def test_constructor_under_the_new_loss():
    model = _clip(loss="barlow", loss_kwargs={"lambd": 0.01, "eps": 1e-3})
    assert model.loss == "barlow"
    assert model.loss_kwargs == {"lambd": 0.01, "eps": 1e-3}
    assert _clip(loss="barlow").loss_kwargs == {}
    assert _clip(loss="barlow", loss_kwargs={"lambd": 0.5}).loss_kwargs == {"lambd": 0.5}
    assert not model.logit_scale.requires_grad and not model.logit_bias.requires_grad
    frozen = [k for k, p in model.named_parameters() if not p.requires_grad]
    assert frozen == ["logit_scale", "logit_bias"]
    other = _clip(loss="softmax")
    assert other.logit_scale.requires_grad and other.logit_bias.requires_grad
    assert list(other.state_dict()) == list(model.state_dict())
    with pytest.raises(ValueError, match="lambd and eps"):
        _clip(loss="barlow", loss_kwargs={"t": 2.0})
    with pytest.raises(ValueError, match="lambd and eps"):
        _clip(loss="barlow", loss_kwargs={"gamma": 1.0})
    # what the other objectives' constructors said, they still say
    with pytest.raises(ValueError, match="alpha, t and lam"):
        _clip(loss="align_uniform", loss_kwargs={"lambd": 1.0})
    with pytest.raises(ValueError, match="sim_coeff, std_coeff, cov_coeff, gamma and eps"):
        _clip(loss="vicreg", loss_kwargs={"lambd": 1.0})
    with pytest.raises(ValueError, match="align_uniform"):
        _clip(loss="softmax", loss_kwargs={"lambd": 1.0})
    assert _clip(loss="align_uniform").loss_kwargs == {}
    bad = _clip(loss="barlow_twins")                          # "unknown loss" comes from _loss, not from the constructor
    with pytest.raises(ValueError, match="unknown loss"):
        bad._loss([torch.zeros(2, 32), torch.zeros(2, 32)])
