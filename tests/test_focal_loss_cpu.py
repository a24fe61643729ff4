"""Focal loss and label smoothing (models_finetune.py, csrc/focal_loss.hip) without a GPU: the longdouble reference against
torch in fp64, the host pieces, the ClipMLP contract, and the build (C-ABI declared, bound and resolved; no scratch)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["msn_focal_loss_workspace_bytes", "msn_focal_loss_fwd", "msn_focal_loss_bwd"]
TK = dict(n_out=8, emb=16, heads=2, depth=1, dropout=0.0, time_norm=1000.0, agg="mean")
SHAPES = [(7, 5), (64, 17), (3, 2)]
TOL = 1e-12


def _case(N, C, seed, scale=4.0):
    """fp64 logits of scale <= 4, class weights, and ignored rows (-100 and out of range) where the shape has room."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, generator=g, dtype=torch.float64) * scale
    y = torch.randint(0, C, (N,), generator=g)
    w = torch.rand(C, generator=g, dtype=torch.float64) + 0.25
    if N > 3:
        y[1] = -100
        y[N - 1] = -100
    return x, y, w


def _autograd_form(x, y, w, gamma, eps):
    """The issue's formula on torch.autograd in fp64: log p from log_softmax, u = 1 - p = -expm1(log p)."""
    N, C = x.shape
    xr = x.clone().requires_grad_()
    lp = F.log_softmax(xr, dim=1)
    u = -torch.expm1(lp)
    valid = (y >= 0) & (y < C)
    ys = y.clamp(0, C - 1)
    q = torch.full((N, C), eps / C, dtype=torch.float64)
    q[torch.arange(N), ys] += 1.0 - eps
    ww = torch.ones(C, dtype=torch.float64) if w is None else w
    loss = (q * ww * u.pow(gamma) * (-lp))[valid].sum() / ww[ys][valid].sum()
    loss.backward()
    return float(loss.detach()), xr.grad.numpy()


@pytest.mark.parametrize("eps", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("N,C", SHAPES)
def test_reference_at_gamma_zero_is_torch_cross_entropy_with_label_smoothing(N, C, weighted, eps):
    from multimodal_supernovae_amd.models_finetune import focal_loss_reference
    x, y, w = _case(N, C, seed=100 * N + C)
    w = w if weighted else None
    xr = x.clone().requires_grad_()
    want = F.cross_entropy(xr, y, weight=w, label_smoothing=eps, reduction="mean")
    want.backward()
    loss, dx = focal_loss_reference(x, y, w, 0.0, eps)
    assert abs(loss - float(want.detach())) <= TOL
    assert float(np.abs(dx - xr.grad.numpy()).max()) <= TOL


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("gamma", [0.0, 0.5, 1.0, 2.0, 5.0])
@pytest.mark.parametrize("N,C", SHAPES)
def test_reference_matches_autograd_fp64(N, C, gamma, eps):
    from multimodal_supernovae_amd.models_finetune import focal_loss_reference
    x, y, w = _case(N, C, seed=100 * N + C + 7)
    for ww in (w, None):
        want_loss, want_dx = _autograd_form(x, y, ww, gamma, eps)
        loss, dx = focal_loss_reference(x, y, ww, gamma, eps)
        assert abs(loss - want_loss) <= TOL, (gamma, eps, loss, want_loss)
        assert float(np.abs(dx - want_dx).max()) <= TOL
        assert float(np.abs(dx[(y < 0).numpy()]).max(initial=0.0)) == 0.0


@pytest.mark.parametrize("gamma", [0.0, 0.5, 2.0, 5.0])
def test_reference_without_smoothing_is_the_multiclass_focal_loss(gamma):
    from multimodal_supernovae_amd.models_finetune import focal_loss_reference
    x, y, w = _case(64, 17, seed=3)
    valid = y >= 0
    p = torch.softmax(x, dim=1)[torch.arange(64), y.clamp(min=0)]
    rows = w[y.clamp(min=0)] * (1.0 - p) ** gamma * (-torch.log(p))
    want = float(rows[valid].sum() / w[y.clamp(min=0)][valid].sum())
    loss, _ = focal_loss_reference(x, y, w, gamma, 0.0)
    assert abs(loss - want) <= TOL


def test_reference_on_confident_rows():
    """A target that wins by 40: 1 - p_y = 2 exp(-40) is far below the spacing of the numbers next to 1, so a form that
    subtracts p_y from 1 returns zero here; the reference keeps loss and gradient.  Where u is exactly 0 (the others
    underflow) and gamma > 0, loss and gradient are exactly zero, not nan."""
    from multimodal_supernovae_amd.models_finetune import focal_loss_reference
    x = torch.tensor([[40.0, 0.0, 0.0]], dtype=torch.float64)
    y = torch.tensor([0])
    u = 2.0 * np.exp(-40.0)
    for gamma in (0.0, 2.0):
        loss, dx = focal_loss_reference(x, y, None, gamma, 0.0)
        assert np.isfinite(loss) and np.isfinite(dx).all()
        assert loss == pytest.approx(u ** (gamma + 1.0), rel=1e-10)           # u^gamma * -log(1 - u), -log(1 - u) = u (1 + u / 2 + ...)
        assert dx[0, 0] == pytest.approx(-(gamma + 1.0) * u ** (gamma + 1.0), rel=1e-10) and dx[0, 0] < 0.0
        assert dx[0, 1] == pytest.approx(-dx[0, 0] / 2.0, rel=1e-10)
    x = torch.tensor([[20000.0, 0.0, -5.0], [0.0, 1.0, 2.0]], dtype=torch.float64)
    loss, dx = focal_loss_reference(x, torch.tensor([0, -100]), None, 2.0, 0.0)
    assert loss == 0.0 and float(np.abs(dx).max()) == 0.0
    loss, dx = focal_loss_reference(x, torch.tensor([0, 1]), None, 0.5, 0.0)
    assert np.isfinite(loss) and np.isfinite(dx).all() and float(np.abs(dx[0]).max()) == 0.0 and dx[1, 1] < 0.0


def test_class_balanced_weights_on_a_hand_computed_example():
    from multimodal_supernovae_amd.models_finetune import class_balanced_weights
    w = class_balanced_weights([2, 1, 0], beta=0.5)
    # (1 - 0.5) / (1 - 0.25) = 2 / 3 and (1 - 0.5) / (1 - 0.5) = 1, no weight for the empty class, scaled to sum to 3
    assert w.dtype == torch.float64
    assert w.tolist() == pytest.approx([3 * (2 / 3) / (5 / 3), 3 * 1 / (5 / 3), 0.0], abs=1e-15)
    assert float(w.sum()) == pytest.approx(3.0, abs=1e-15)
    assert class_balanced_weights([10, 3, 700, 1], beta=0.0).tolist() == [1.0, 1.0, 1.0, 1.0]
    rare = class_balanced_weights([1000, 10], beta=0.999)
    assert rare[1] > rare[0] and float(rare.sum()) == pytest.approx(2.0, abs=1e-15)
    assert float(rare[1] / rare[0]) == pytest.approx((1 - 0.999 ** 1000) / (1 - 0.999 ** 10), rel=1e-12)
    for bad in ([0, 0], [-1, 2]):
        with pytest.raises(ValueError):
            class_balanced_weights(bad)
    with pytest.raises(ValueError):
        class_balanced_weights([1, 2], beta=1.0)


def _clip():
    from multimodal_supernovae_amd.models_multimodal import LightCurveImageCLIP
    return LightCurveImageCLIP(enc_dim=16, nband=2, transformer_kwargs=TK, transformer_spectral_kwargs=TK,
                               conv_kwargs=dict(dim=8, depth=1, channels=3, kernel_size=5, patch_size=8, n_out=8,
                                                dropout_prob=0.0),
                               meta_kwargs=dict(input_dim=8, hidden_dim=8, num_layers=1),
                               combinations=["lightcurve", "spectral"], loss="softmax")


def test_clipmlp_loss_contract():
    from multimodal_supernovae_amd.models_finetune import ClipMLP
    kw = dict(classification=True, n_classes=5, hidden_dim=12, class_weights=[1.0, 2.0, 0.5, 1.0, 1.0])
    default = ClipMLP(_clip(), **kw)
    focal = ClipMLP(_clip(), loss="focal", loss_kwargs={"gamma": 1.5, "label_smoothing": 0.1}, **kw)
    smooth = ClipMLP(_clip(), loss="cross_entropy", loss_kwargs={"label_smoothing": 0.1}, **kw)
    keys = sorted(default.state_dict().keys())
    assert sorted(focal.state_dict().keys()) == keys and sorted(smooth.state_dict().keys()) == keys
    assert [n for n, _ in focal.named_parameters()] == [n for n, _ in default.named_parameters()]
    assert (default.loss_name, default.loss_gamma, default.label_smoothing) == ("cross_entropy", 0.0, 0.0)
    assert (focal.loss_name, focal.loss_gamma, focal.label_smoothing) == ("focal", 1.5, 0.1)
    assert ClipMLP(_clip(), loss="focal", **kw).loss_gamma == 2.0
    for bad in (dict(loss="cross_entropy", loss_kwargs={"gamma": 2.0}), dict(loss="focal", loss_kwargs={"alpha": 0.25}),
                dict(loss="hinge"), dict(loss="focal", loss_kwargs={"gamma": -1.0}),
                dict(loss="focal", loss_kwargs={"gamma": float("inf")}), dict(loss_kwargs={"label_smoothing": 1.5})):
        with pytest.raises(ValueError):
            ClipMLP(_clip(), **kw, **bad)
    for bad in (dict(loss="focal"), dict(loss_kwargs={"label_smoothing": 0.1}), dict(loss="cross_entropy")):
        with pytest.raises(ValueError):
            ClipMLP(_clip(), regression=True, **bad)


def test_focal_loss_and_smoothed_cross_entropy_have_no_cpu_path():
    from multimodal_supernovae_amd import _lib
    from multimodal_supernovae_amd.models_finetune import cross_entropy, focal_loss
    x, y = torch.randn(4, 5), torch.zeros(4, dtype=torch.int64)
    with pytest.raises(_lib.MsnHipError):
        focal_loss(x, y)
    with pytest.raises(_lib.MsnHipError):
        cross_entropy(x, y, label_smoothing=0.1)


def test_entry_points_declared_bound_and_resolved():
    from multimodal_supernovae_amd import _lib
    header = open(os.path.join(ROOT, "include", "msn_hip.h")).read()
    handle = _lib.lib()
    for name in ENTRY_POINTS:
        assert re.search(r"\b" + name + r"\(", header), f"{name} is not declared in include/msn_hip.h"
        assert name in _lib.SIGNATURES, f"{name} is not bound in _lib.py"
        assert getattr(handle, name) is not None
        decl = re.search(r"\b" + name + r"\(([^;]*)\);", header).group(1)
        assert len(_lib.SIGNATURES[name][1]) == decl.count(",") + 1, name
    query = handle.msn_focal_loss_workspace_bytes
    assert query.restype is ctypes.c_size_t
    assert query(10, 1) == 0 and query(10, 1025) == 0 and query(0, 5) == 0 and query(2 ** 31, 5) == 0
    assert query(256, 5) == 0 and query(256, 16) == 0 and query(4, 17) == 0 and query(4, 1024) == 0      # one workgroup: no partials
    assert query(100000, 5) > 0 and query(257, 16) == 2 * 2 * 8 and query(5, 17) == 2 * 2 * 8 and query(4096, 5) == 16 * 2 * 8


def test_focal_kernels_compile_for_gfx950_without_scratch(tmp_path):
    """hipcc's resource report for every kernel of focal_loss.hip: 0 bytes of scratch -- the fp64 pow and a row's registers
    fit (the check of test_supervised_cpu.py, pointed at this file)."""
    from multimodal_supernovae_amd import build as B
    src = os.path.join(B.CSRC, "focal_loss.hip")
    r = subprocess.run([B.HIPCC] + B.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "focal_loss.o")],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    names = re.findall(r"remark: Function Name: (\S+)", r.stderr)
    scratch = [int(v) for v in re.findall(r"remark:\s+ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(names) == len(scratch) and len(names) == 9, (names, scratch)
    for kind in ("focal_fwd_lane", "focal_fwd_wave", "focal_bwd_lane", "focal_bwd_wave", "focal_finish"):
        assert any(kind in n for n in names), f"no kernel named {kind}* in focal_loss.hip"
    assert all(s == 0 for s in scratch), dict(zip(names, scratch))
