"""VICReg (loss.vicreg_loss, csrc/vicreg.hip, LightCurveImageCLIP(loss="vicreg")) without a GPU: the longdouble restatements
(loss.vicreg_reference, embedding_metrics.column_covariance_reference) against torch.autograd in fp64 of the paper's code form
and against numpy.cov, the refusals, the C-ABI (declared, bound, resolved, the plan behind the workspace sizes, every refusal
with made-up addresses), the scratch report of the kernels, and the constructor of the model."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["msn_column_cov_workspace_bytes", "msn_column_cov", "msn_vicreg_workspace_bytes", "msn_vicreg_fwd", "msn_vicreg_bwd"]

TK = dict(n_out=16, emb=16, heads=2, depth=1, dropout=0.0, time_norm=20583.37, agg="mean")
SK = dict(n_out=16, emb=16, heads=2, depth=1, dropout=0.0, time_norm=17945.14, agg="mean")


def cdiv(a, b):
    return -(-a // b)


def _rows(n, d, seed):
    """fp32 rows whose columns have very different spreads: even columns scaled by 0.25, odd ones by 4 (one column keeps its
    normal values: unit norm would leave only +1 and -1)."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d))
    if d > 1:
        X /= np.linalg.norm(X, axis=1, keepdims=True)
    X *= np.where(np.arange(d) % 2 == 0, 0.25, 4.0)
    return X.astype(np.float32)


def _off_diagonal(c):
    n = c.shape[0]
    return c.flatten()[:-1].view(n - 1, n + 1)[:, 1:].flatten() if n > 1 else c.new_zeros(0)


def _paper(embs, sim, std, covc, gamma, eps):
    """The published code form, pair by pair."""
    total = 0.0
    for i in range(len(embs)):
        for j in range(i + 1, len(embs)):
            x, y = embs[i], embs[j]
            n, d = x.shape
            repr_loss = F.mse_loss(x, y)
            xc, yc = x - x.mean(dim=0), y - y.mean(dim=0)
            std_x, std_y = torch.sqrt(xc.var(dim=0) + eps), torch.sqrt(yc.var(dim=0) + eps)
            std_loss = torch.mean(F.relu(gamma - std_x)) + torch.mean(F.relu(gamma - std_y))
            cov_x, cov_y = (xc.T @ xc) / (n - 1), (yc.T @ yc) / (n - 1)
            cov_loss = _off_diagonal(cov_x).pow(2).sum().div(d) + _off_diagonal(cov_y).pow(2).sum().div(d)
            total = total + sim * repr_loss + std * std_loss + covc * cov_loss
    return total


def _against_autograd(X, coeffs, gamma, eps, upstream=1.0):
    from multimodal_supernovae_amd.loss import vicreg_reference
    T = [torch.from_numpy(x.astype(np.float64)).requires_grad_(True) for x in X]
    want = _paper(T, *coeffs, gamma, eps)
    grads = torch.autograd.grad(want * upstream, T)
    loss, got = vicreg_reference(X, *coeffs, gamma, eps)
    want = float(want.detach())
    assert abs(float(loss) - want) <= 1e-12 * max(1.0, abs(want)), (float(loss), want)
    scale = max(max(float(g.abs().max()) for g in grads), 1e-300)
    for g, w in zip(got, grads):
        assert g.dtype == np.longdouble and g.shape == tuple(w.shape)
        assert float(np.abs((upstream * g).astype(np.float64) - w.numpy()).max()) <= 1e-12 * scale


@pytest.mark.parametrize("towers", [2, 3])
@pytest.mark.parametrize("n,d", [(2, 1), (5, 3), (40, 7), (33, 32)])
def test_reference_equals_autograd_of_the_paper_form(n, d, towers):
    X = [_rows(n, d, 100 * n + 10 * d + k) for k in range(towers)]
    s = np.concatenate([np.sqrt(np.cov(x.astype(np.float64), rowvar=False).reshape(d, d).diagonal() + 1e-4) for x in X])
    # gamma below every s_c, between them (both branches of the hinge), above every s_c; the paper's coefficients and each one at 0
    gammas = [0.5 * s.min(), 0.5 * (np.sort(s)[len(s) // 2 - 1] + np.sort(s)[len(s) // 2]), 2.0 * s.max()]
    for gamma in gammas:
        assert np.abs(s - gamma).min() > 1e-6
        for coeffs in ((25.0, 25.0, 1.0), (0.0, 25.0, 1.0), (25.0, 0.0, 1.0), (25.0, 25.0, 0.0), (1.0, 2.0, 3.0)):
            _against_autograd(X, coeffs, float(gamma), 1e-4)
    _against_autograd(X, (25.0, 25.0, 1.0), float(gammas[1]), 1e-2, upstream=-3.5)


def test_one_column_has_no_covariance_term():
    from multimodal_supernovae_amd.loss import vicreg_reference
    X = [_rows(9, 1, 3), _rows(9, 1, 4)]
    _, _, terms = vicreg_reference(X, 25.0, 25.0, 1.0, 10.0, 1e-4, return_terms=True)
    assert terms["cov"] == [0, 0] and all(v > 0 for v in terms["var"])
    a = vicreg_reference(X, 25.0, 25.0, 1.0, 10.0, 1e-4)
    b = vicreg_reference(X, 25.0, 25.0, 7.0, 10.0, 1e-4)
    assert a[0] == b[0] and all(np.array_equal(g, h) for g, h in zip(a[1], b[1]))


def test_the_hinge_is_inactive_at_gamma():
    """s_c == gamma exactly: torch's relu has the subgradient 0 there, and so has the reference."""
    from multimodal_supernovae_amd.loss import vicreg_reference
    X = np.array([[1.0, 0.0], [-1.0, 0.5], [0.0, -0.5]], dtype=np.float32)         # var of column 0 is exactly 1
    gamma = float(np.sqrt(np.longdouble(1.0) + np.longdouble(0.5625)))              # = 1.25 exactly with eps = 0.5625
    _, grads = vicreg_reference([X, X], 0.0, 1.0, 0.0, gamma, 0.5625)
    assert float(np.abs(grads[0][:, 0]).max()) == 0.0 and float(np.abs(grads[0][:, 1]).max()) > 0.0


@pytest.mark.parametrize("n,d", [(2, 1), (3, 2), (40, 7), (129, 33)])
def test_covariance_reference_equals_numpy_cov(n, d):
    from multimodal_supernovae_amd.embedding_metrics import column_covariance_reference
    X = _rows(n, d, n + d)
    mean, cov = column_covariance_reference(X)
    assert mean.dtype == np.longdouble and mean.shape == (d,) and cov.shape == (d, d)
    want = np.cov(X.astype(np.float64), rowvar=False).reshape(d, d)
    assert np.abs(cov.astype(np.float64) - want).max() <= 1e-12 * np.abs(want).max()
    assert np.abs(mean.astype(np.float64) - X.astype(np.float64).mean(axis=0)).max() <= 1e-14 * np.abs(X).max()
    assert np.array_equal(cov, cov.T)
    with pytest.raises(ValueError):
        column_covariance_reference(X[:1])


def test_refusals_come_before_the_gpu_is_asked_for(monkeypatch):
    from multimodal_supernovae_amd import _lib, embedding_metrics as E, loss as Lo
    X = torch.from_numpy(_rows(8, 4, 1))
    asked = []
    monkeypatch.setattr(_lib, "require_gpu", lambda: asked.append(1))
    for kw, word in ((dict(sim_coeff=-1.0), "sim_coeff"), (dict(std_coeff=float("nan")), "std_coeff"),
                     (dict(cov_coeff=float("inf")), "cov_coeff"), (dict(gamma=-0.5), "gamma"), (dict(gamma=float("inf")), "gamma"),
                     (dict(eps=0.0), "eps"), (dict(eps=float("nan")), "eps"), (dict(eps=-1e-4), "eps")):
        with pytest.raises(ValueError, match=word):
            Lo.vicreg_loss(X, X, **kw)
    with pytest.raises(ValueError, match="at least two"):
        Lo.vicreg_loss_multimodal([X])
    assert asked == []                                       # as _align_uniform_args: the values first, then the device
    # CPU tensors, then the shapes
    with pytest.raises(_lib.MsnHipError, match="must live on the GPU"):
        Lo.vicreg_loss(X, X)
    assert asked == [1]
    monkeypatch.setattr(Lo, "_device_f32", lambda *named: None)
    with pytest.raises(ValueError, match="one shape"):
        Lo.vicreg_loss(X, X[:7])
    with pytest.raises(_lib.MsnHipError, match="N must be at least 2"):
        Lo.vicreg_loss(X[:1], X[:1])
    with pytest.raises(_lib.MsnHipError, match=r"D must be in 1\.\.256"):
        Lo.vicreg_loss(torch.zeros(4, 257), torch.zeros(4, 257))
    with pytest.raises(_lib.MsnHipError, match=r"D must be in 1\.\.256"):
        Lo.vicreg_loss(torch.zeros(4, 0), torch.zeros(4, 0))
    # sharded: statistics over gathered rows are not built
    monkeypatch.setattr(Lo, "_is_sharded", lambda global_negatives, group: bool(global_negatives))
    with pytest.raises(NotImplementedError, match="global_negatives=False"):
        Lo.vicreg_loss(X, X)
    with pytest.raises(ValueError):
        Lo.vicreg_reference([X.numpy()])
    with pytest.raises(ValueError):
        Lo.vicreg_reference([X.numpy(), X.numpy()[:7]])
    monkeypatch.undo()
    with pytest.raises(_lib.MsnHipError):                     # no CPU path
        E.column_covariance(X)


# ---------------------------------------------------------------------------------------------------------- the C-ABI
def cov_plan(N, D):
    """The plan of include/msn_hip.h: (mrows, mslabs, pairs, per, slabs)."""
    mrows = max(64, cdiv(N, 64))
    T = cdiv(D, 64)
    pairs = T * (T + 1) // 2
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
    cov, vic = handle.msn_column_cov_workspace_bytes, handle.msn_vicreg_workspace_bytes
    for q in (cov, vic):
        assert q(1, 4) == 0 and q(2 ** 31, 4) == 0 and q(8, 0) == 0 and q(8, 257) == 0
    for n, d in [(2, 1), (65, 33), (130, 128), (200, 256), (1100, 4), (2100, 256), (4096, 128), (10 ** 6, 130)]:
        _, mslabs, pairs, _, slabs = cov_plan(n, d)
        assert cov(n, d) == 8 * (mslabs * d + 4096 * slabs * pairs), (n, d)
        assert vic(n, d) == 8 * (min(cdiv(n, 256), 1024) + 4 * min(cdiv(d * d, 256), 64)), (n, d)


def test_every_refusal_returns_msn_err_shape_without_a_gpu():
    """The refusals come before any launch and never follow a pointer: made-up addresses do."""
    from multimodal_supernovae_amd import _lib
    L = _lib.lib()
    X, Y, MEAN, COV, WS, OUT, G = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000
    big = 1 << 40

    def cov(x=X, ld=4, n=8, d=4, mean=MEAN, c=COV, ws=WS, nb=big):
        return L.msn_column_cov(x, ld, n, d, mean, c, ws, nb, None)

    def fwd(x=X, ldx=4, y=Y, ldy=4, n=8, d=4, cx=COV, cy=COV, sim=25.0, std=25.0, covc=1.0, gamma=1.0, eps=1e-4, loss=OUT, comp=OUT + 8,
            mx=MEAN, my=MEAN, ws=WS, nb=big):
        return L.msn_vicreg_fwd(x, ldx, y, ldy, n, d, cx, cy, sim, std, covc, gamma, eps, loss, comp, mx, my, ws, nb, None)

    def bwd(x=X, ldx=4, y=Y, ldy=4, n=8, d=4, mx=MEAN, my=MEAN, Mx=COV, My=COV, g=G, sim=25.0, dx=OUT, lddx=4, dy=OUT, lddy=4):
        return L.msn_vicreg_bwd(x, ldx, y, ldy, n, d, mx, my, Mx, My, g, sim, dx, lddx, dy, lddy, None)

    nan, inf = float("nan"), float("inf")
    refused = {
        "cov D = 0": cov(d=0, ld=1), "cov D = 257": cov(d=257, ld=300), "cov N = 1": cov(n=1), "cov N = 2^31": cov(n=2 ** 31),
        "cov null X": cov(x=0), "cov null mean": cov(mean=0), "cov null cov": cov(c=0), "cov row stride below D": cov(ld=3),
        "cov misaligned X": cov(x=X + 2), "cov misaligned mean": cov(mean=MEAN + 4), "cov misaligned cov": cov(c=COV + 4),
        "cov misaligned workspace": cov(ws=WS + 4), "cov null workspace": cov(ws=0, nb=0),
        "cov workspace too small": cov(nb=8 * (4 + 4096) - 1),
        "fwd D = 0": fwd(d=0), "fwd D = 257": fwd(d=257, ldx=300, ldy=300), "fwd N = 1": fwd(n=1), "fwd N = 2^31": fwd(n=2 ** 31),
        "fwd sim < 0": fwd(sim=-1.0), "fwd sim nan": fwd(sim=nan), "fwd std < 0": fwd(std=-1.0), "fwd std inf": fwd(std=inf),
        "fwd cov < 0": fwd(covc=-1.0), "fwd cov nan": fwd(covc=nan), "fwd gamma < 0": fwd(gamma=-1.0), "fwd gamma inf": fwd(gamma=inf),
        "fwd gamma nan": fwd(gamma=nan), "fwd eps = 0": fwd(eps=0.0), "fwd eps < 0": fwd(eps=-1.0), "fwd eps nan": fwd(eps=nan),
        "fwd eps inf": fwd(eps=inf), "fwd null X": fwd(x=0), "fwd null Y": fwd(y=0), "fwd null cov_x": fwd(cx=0), "fwd null cov_y": fwd(cy=0),
        "fwd null loss": fwd(loss=0), "fwd null comp": fwd(comp=0), "fwd null M_x": fwd(mx=0), "fwd null M_y": fwd(my=0),
        "fwd row stride x": fwd(ldx=3), "fwd row stride y": fwd(ldy=3), "fwd misaligned comp": fwd(comp=OUT + 4),
        "fwd misaligned X": fwd(x=X + 1), "fwd null workspace": fwd(ws=0, nb=0), "fwd workspace too small": fwd(nb=8 * (1 + 4) - 1),
        "bwd D = 257": bwd(d=257, ldx=300, ldy=300, lddx=300, lddy=300), "bwd N = 1": bwd(n=1), "bwd sim < 0": bwd(sim=-1.0),
        "bwd sim nan": bwd(sim=nan), "bwd null X": bwd(x=0), "bwd null Y": bwd(y=0), "bwd null mean_x": bwd(mx=0), "bwd null mean_y": bwd(my=0),
        "bwd null M_x": bwd(Mx=0), "bwd null M_y": bwd(My=0), "bwd null g": bwd(g=0), "bwd null dX": bwd(dx=0), "bwd null dY": bwd(dy=0),
        "bwd row stride x": bwd(ldx=3), "bwd row stride dX": bwd(lddx=3), "bwd row stride dY": bwd(lddy=3), "bwd misaligned M_x": bwd(Mx=COV + 4),
        "bwd misaligned dX": bwd(dx=OUT + 2),
    }
    assert {k: v for k, v in refused.items() if v != 1} == {}
    assert L.msn_last_error()


def test_vicreg_kernels_compile_for_gfx950_without_scratch(tmp_path):
    """hipcc's resource report for every kernel of vicreg.hip through tools/check_scratch.py: 0 bytes of scratch (the fp64
    accumulators of the Gram and of the backward's product, and the rows fetched a step early, stay in registers)."""
    from multimodal_supernovae_amd import build as B
    src = os.path.join(B.CSRC, "vicreg.hip")
    r = subprocess.run([B.HIPCC] + B.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "vicreg.o")],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    remarks = tmp_path / "vicreg.remarks"
    remarks.write_text(r.stderr)
    names = re.findall(r"remark: Function Name: (\S+)", r.stderr)
    assert len(names) == 3 + 3 + 1, names           # means, Gram, finish; rows, coefficients, finish; the backward
    for kind in ["column_sum", "column_gram", "column_cov_finish", "vicreg_rows", "vicreg_coef", "vicreg_finish", "vicreg_bwd"]:
        assert any(kind in n for n in names), f"no kernel named {kind}* in vicreg.hip"
    c = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_scratch.py"), str(remarks), "--", "column_", "vicreg_"],
                       capture_output=True, text=True, timeout=60)
    print(c.stdout)
    assert c.returncode == 0 and f"scratch check: {len(names)} kernels -> OK" in c.stdout, c.stdout + c.stderr


# ---------------------------------------------------------------------------------------------------------- the model
def _clip(**kw):
    from multimodal_supernovae_amd.models_multimodal import LightCurveImageCLIP
    return LightCurveImageCLIP(enc_dim=32, nband=2, transformer_kwargs=TK, transformer_spectral_kwargs=SK,
                               combinations=["lightcurve", "spectral"], **kw)


def test_constructor_under_the_new_loss():
    model = _clip(loss="vicreg", loss_kwargs={"sim_coeff": 10.0, "eps": 1e-3})
    assert model.loss == "vicreg"
    assert model.loss_kwargs == {"sim_coeff": 10.0, "eps": 1e-3, "gamma": 1.0 / math.sqrt(32)}
    assert _clip(loss="vicreg").loss_kwargs == {"gamma": 1.0 / math.sqrt(32)}
    assert _clip(loss="vicreg", loss_kwargs={"gamma": 0.5}).loss_kwargs == {"gamma": 0.5}
    assert not model.logit_scale.requires_grad and not model.logit_bias.requires_grad
    frozen = [k for k, p in model.named_parameters() if not p.requires_grad]
    assert frozen == ["logit_scale", "logit_bias"]
    other = _clip(loss="softmax")
    assert other.logit_scale.requires_grad and other.logit_bias.requires_grad
    assert list(other.state_dict()) == list(model.state_dict())
    with pytest.raises(ValueError, match="sim_coeff, std_coeff, cov_coeff, gamma and eps"):
        _clip(loss="vicreg", loss_kwargs={"t": 2.0})
    # what the other objectives' constructors said, they still say
    with pytest.raises(ValueError, match="alpha, t and lam"):
        _clip(loss="align_uniform", loss_kwargs={"gamma": 1.0})
    with pytest.raises(ValueError, match="align_uniform"):
        _clip(loss="softmax", loss_kwargs={"gamma": 1.0})
    assert _clip(loss="align_uniform").loss_kwargs == {}
