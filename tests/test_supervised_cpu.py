"""Supervised heads (models_finetune.py, csrc/supervised.hip) without a GPU: the C-ABI is declared, bound and resolves; the
kernels of supervised.hip compile for gfx950 without scratch; the host part of the metrics on hand-written inputs; the
constructor contract of ClipMLP."""
import ctypes
import math
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["msn_cross_entropy_workspace_bytes", "msn_cross_entropy_fwd", "msn_cross_entropy_bwd", "msn_confusion_matrix",
                "msn_regression_stats_workspace_bytes", "msn_regression_stats"]
TK = dict(n_out=8, emb=16, heads=2, depth=1, dropout=0.0, time_norm=1000.0, agg="mean")


def _clip(combos=("lightcurve", "spectral")):
    from multimodal_supernovae_amd.models_multimodal import LightCurveImageCLIP
    return LightCurveImageCLIP(enc_dim=16, nband=2, transformer_kwargs=TK, transformer_spectral_kwargs=TK,
                               conv_kwargs=dict(dim=8, depth=1, channels=3, kernel_size=5, patch_size=8, n_out=8,
                                                dropout_prob=0.0),
                               meta_kwargs=dict(input_dim=8, hidden_dim=8, num_layers=1), combinations=list(combos),
                               loss="softmax")


def test_entry_points_declared_bound_and_resolved():
    from multimodal_supernovae_amd import _lib
    header = open(os.path.join(ROOT, "include", "msn_hip.h")).read()
    handle = _lib.lib()
    for name in ENTRY_POINTS:
        assert re.search(r"\b" + name + r"\(", header), f"{name} is not declared in include/msn_hip.h"
        assert name in _lib.SIGNATURES, f"{name} is not bound in _lib.py"
        assert getattr(handle, name) is not None
    # argument counts of the bindings follow the declarations
    for name in ENTRY_POINTS:
        decl = re.search(r"\b" + name + r"\(([^;]*)\);", header).group(1)
        n_args = 0 if decl.strip() in ("", "void") else decl.count(",") + 1
        assert len(_lib.SIGNATURES[name][1]) == n_args, name
    # workspace queries are host-side decisions (no launch): one workgroup takes the shapes of training
    handle.msn_cross_entropy_workspace_bytes.restype = ctypes.c_size_t
    assert handle.msn_cross_entropy_workspace_bytes(4096, 5) == 0
    assert handle.msn_cross_entropy_workspace_bytes(100000, 5) > 0
    assert handle.msn_cross_entropy_workspace_bytes(10, 1) == 0 and handle.msn_cross_entropy_workspace_bytes(10, 1025) == 0
    assert handle.msn_regression_stats_workspace_bytes(1000) == 0 and handle.msn_regression_stats_workspace_bytes(100000) > 0


def test_supervised_kernels_compile_for_gfx950_without_scratch(tmp_path):
    """hipcc's resource report for every kernel of supervised.hip: 0 bytes of scratch (the property tools/check_scratch.py
    keeps for the GEMM and attention families)."""
    from multimodal_supernovae_amd import build as B
    src = os.path.join(B.CSRC, "supervised.hip")
    r = subprocess.run([B.HIPCC] + B.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "supervised.o")],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    names = re.findall(r"remark: Function Name: (\S+)", r.stderr)
    scratch = [int(v) for v in re.findall(r"remark:\s+ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(names) == len(scratch) and len(names) >= 6, (names, scratch)
    for kind in ("ce_fwd_lane", "ce_fwd_wave", "ce_bwd_lane", "ce_bwd_wave", "sup_finish", "confusion", "regression_stats"):
        assert any(kind in n for n in names), f"no kernel named {kind}* in supervised.hip"
    assert all(s == 0 for s in scratch), dict(zip(names, scratch))


def test_classification_metrics_on_hand_written_matrices():
    from multimodal_supernovae_amd.models_finetune import classification_metrics
    # class 2 neither occurs nor is predicted: macro averages over three classes
    cm = torch.tensor([[3, 1, 0, 0],
                       [2, 4, 0, 1],
                       [0, 0, 0, 0],
                       [1, 0, 0, 5]])
    m = classification_metrics(cm)
    f0 = 2 * 3 / (2 * 3 + 3 + 1)        # tp 3, fp 2 + 1, fn 1
    f1 = 2 * 4 / (2 * 4 + 1 + 3)        # tp 4, fp 1,     fn 2 + 1
    f3 = 2 * 5 / (2 * 5 + 1 + 1)        # tp 5, fp 1,     fn 1
    assert m["acc"] == pytest.approx(12 / 17, abs=1e-15)
    assert m["f1_per_class"] == pytest.approx([f0, f1, 0.0, f3], abs=1e-15)
    assert m["f1_macro"] == pytest.approx((f0 + f1 + f3) / 3, abs=1e-15)
    assert m["f1_micro"] == pytest.approx(2 * 12 / (2 * 12 + 5 + 5), abs=1e-15)
    perfect = classification_metrics(torch.diag(torch.tensor([4, 1, 7])))
    assert perfect["acc"] == 1.0 and perfect["f1_macro"] == 1.0 and perfect["f1_micro"] == 1.0
    assert perfect["f1_per_class"] == [1.0, 1.0, 1.0]
    wrong = classification_metrics(torch.tensor([[0, 2, 1], [3, 0, 0], [1, 4, 0]]))
    assert wrong["acc"] == 0.0 and wrong["f1_macro"] == 0.0 and wrong["f1_micro"] == 0.0


def test_regression_metrics_on_a_five_point_example():
    from multimodal_supernovae_amd.models_finetune import regression_metrics
    y = torch.tensor([0.10, 0.25, 0.40, 0.80, 1.50], dtype=torch.float64)
    p = torch.tensor([0.12, 0.20, 0.75, 0.79, 1.00], dtype=torch.float64)
    d = p - y
    out = (d.abs() / (1 + y) > 0.15).sum()
    sums = [5.0, float(d.abs().sum()), float((d * d).sum()), float(y.sum()), float((y * y).sum()), float(out)]
    m = regression_metrics(sums)
    assert int(out) == 2
    assert m["L1"] == pytest.approx(float(d.abs().mean()), rel=1e-14)
    assert m["L2"] == pytest.approx(float((d * d).mean()), rel=1e-14)
    assert m["R2"] == pytest.approx(float(1 - (d * d).sum() / ((y - y.mean()) ** 2).sum()), rel=1e-12)
    assert m["OLF"] == pytest.approx(0.4, rel=1e-14)
    assert all(math.isnan(v) for v in regression_metrics([0.0] * 6).values())


def test_clipmlp_constructor_contract():
    from multimodal_supernovae_amd.models_finetune import ClipMLP
    from multimodal_supernovae_amd.models_multimodal import LightCurveImageCLIP
    from multimodal_supernovae_amd.optim import RAdam
    with pytest.raises(NotImplementedError, match="ClipMLP"):
        LightCurveImageCLIP(regression=True)
    with pytest.raises(NotImplementedError):
        LightCurveImageCLIP(classification=True)
    with pytest.raises(ValueError):
        ClipMLP(_clip())
    with pytest.raises(ValueError):
        ClipMLP(_clip(), regression=True, classification=True)
    with pytest.raises(ValueError, match="meta"):
        ClipMLP(_clip(("lightcurve", "meta")), classification=True)
    m = ClipMLP(_clip(), classification=True, n_classes=5, hidden_dim=12, num_layers=2, class_weights=[1.0, 2.0, 0.5, 1.0, 1.0])
    keys = list(m.state_dict().keys())
    clip_keys = ["clip_model." + k for k in _clip().state_dict().keys()]
    head_keys = [f"mlp.layers.{i}.{w}" for i in (0, 3, 6) for w in ("weight", "bias")]
    assert sorted(keys) == sorted(clip_keys + head_keys + ["class_weights"])
    assert m.mlp.layers[0].in_features == 2 * 16 and m.mlp.layers[6].out_features == 5
    r = ClipMLP(_clip(("host_galaxy", "lightcurve", "spectral")), regression=True, num_layers=1)
    assert "class_weights" not in r.state_dict() and r.mlp.layers[0].in_features == 3 * 16 and r.mlp.layers[3].out_features == 1
    assert sorted(k for k in r.state_dict() if k.startswith("mlp.")) == [f"mlp.layers.{i}.{w}" for i in (0, 3) for w in ("bias", "weight")]

    def stepped(model):
        opt = model.configure_optimizers()["optimizer"]
        assert isinstance(opt, RAdam)
        ids = {id(p) for g in opt.param_groups for p in g["params"]}
        return {k for k, p in model.named_parameters() if id(p) in ids}, opt

    names, opt = stepped(m)
    every = {k for k, _ in m.named_parameters()}
    assert names == every - {"clip_model.logit_scale", "clip_model.logit_bias"}
    assert opt.param_groups[0]["lr"] == 1e-3
    frozen = ClipMLP(_clip(), classification=True, freeze_backbone=True, learning_rate=3e-4, optimizer_kwargs={"weight_decay": 0.01})
    names, opt = stepped(frozen)
    assert names == {k for k in every if k.startswith("mlp.")}
    assert opt.param_groups[0]["lr"] == 3e-4 and opt.param_groups[0]["weight_decay"] == 0.01
    assert not any(p.requires_grad for p in frozen.clip_model.parameters()) and all(p.requires_grad for p in frozen.mlp.parameters())
    frozen.train()
    assert frozen.training and frozen.mlp.training and not any(mod.training for mod in frozen.clip_model.modules())
    m.train()
    assert all(mod.training for mod in m.clip_model.modules())


def test_cross_entropy_has_no_cpu_path():
    from multimodal_supernovae_amd import _lib
    from multimodal_supernovae_amd.models_finetune import cross_entropy
    with pytest.raises(_lib.MsnHipError):
        cross_entropy(torch.randn(4, 5), torch.zeros(4, dtype=torch.int64))
