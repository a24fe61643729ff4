"""Gradient clipping without a GPU: the C-ABI of csrc/grad_clip.hip refuses bad arguments before any launch, the Trainer /
GraphedTrainStep refuse bad clipping arguments at construction, and the kernels keep every value in registers."""
import ctypes
import math
import os
import shutil
import subprocess
import sys

import pytest
import torch

from conftest import ROOT

FAKE = ctypes.c_void_p(4096)          # never dereferenced: validation rejects the call before any launch


def _lib():
    import __graft_entry__ as entry
    entry.build()
    from multimodal_supernovae_amd import _lib
    return _lib.lib()


def test_grad_norm_refuses_bad_arguments():
    lib = _lib()
    need = lib.msn_grad_norm_workspace_bytes(3, 5000)
    assert need == 3 * 2 * 8                       # 2 blocks of 4096 elements per tensor, one fp64 partial each
    assert lib.msn_grad_norm_workspace_bytes(0, 10) == 0 and lib.msn_grad_norm_workspace_bytes(65536, 10) == 0
    cases = [
        ((None, 3, 5000, 2.0, 1.0, FAKE, FAKE, FAKE, need, None), b"null"),
        ((FAKE, 3, 5000, 2.0, 1.0, None, FAKE, FAKE, need, None), b"null"),
        ((FAKE, 3, 5000, 2.0, 1.0, FAKE, None, FAKE, need, None), b"null"),
        ((FAKE, 0, 5000, 2.0, 1.0, FAKE, FAKE, FAKE, need, None), b"1..65535"),
        ((FAKE, 65536, 5000, 2.0, 1.0, FAKE, FAKE, FAKE, need, None), b"1..65535"),
        ((FAKE, 3, -1, 2.0, 1.0, FAKE, FAKE, FAKE, need, None), b"max_numel"),
        ((FAKE, 3, 5000, 3.0, 1.0, FAKE, FAKE, FAKE, need, None), b"norm_type"),
        ((FAKE, 3, 5000, 0.0, 1.0, FAKE, FAKE, FAKE, need, None), b"norm_type"),
        ((FAKE, 3, 5000, 2.0, -1.0, FAKE, FAKE, FAKE, need, None), b"max_norm"),
        ((FAKE, 3, 5000, 2.0, math.nan, FAKE, FAKE, FAKE, need, None), b"max_norm"),
        ((FAKE, 3, 5000, 2.0, 1.0, FAKE, FAKE, FAKE, need - 1, None), b"workspace"),
        ((FAKE, 3, 5000, 2.0, 1.0, FAKE, FAKE, None, need, None), b"workspace"),
    ]
    for args, msg in cases:
        rc = lib.msn_grad_norm(*args)
        assert rc == 1 and msg in lib.msn_last_error(), (args, lib.msn_last_error())


def test_multi_tensor_geometry_through_the_workspace_sizes():
    """mt_grid_x of csrc/multi_tensor.h, as the two entry points that size caller-owned scratch from it expose it: one fp64 partial
    per block for the gradient norm, two for the layer-wise steps, whose size is an envelope that never shrinks with n or m."""
    lib = _lib()

    def gx(n, m):
        return max(1, min(-(-m // 4096), min(1024, max(32, 8192 // n))))

    points = {(3, 5000): 48, (8, 0): 64, (40, 200_000): 15_680, (301, 300_001): 77_056, (1, 10**9): 8_192,
              (65_535, 10**7): 16_776_960}
    for (n, m), want in points.items():
        assert n * gx(n, m) * 8 == want
        assert lib.msn_grad_norm_workspace_bytes(n, m) == want, (n, m)
        assert lib.msn_layerwise_workspace_bytes(n, m) == 2 * want, (n, m)
    assert 100 * gx(100, 10**6) * 16 == 129_600 and lib.msn_layerwise_workspace_bytes(100, 10**6) == 131_072    # the envelope
    assert lib.msn_grad_norm_workspace_bytes(100, 10**6) == 64_800


def test_grad_scale_and_clamp_refuse_bad_arguments():
    lib = _lib()
    for args, msg in [((None, 2, 10, FAKE, None), b"null"), ((FAKE, 2, 10, None, None), b"null"),
                      ((FAKE, 0, 10, FAKE, None), b"1..65535"), ((FAKE, 65536, 10, FAKE, None), b"1..65535"),
                      ((FAKE, 2, -5, FAKE, None), b"max_numel")]:
        assert lib.msn_grad_scale(*args) == 1 and msg in lib.msn_last_error(), args
    for args, msg in [((None, 2, 10, 1.0, None), b"null"), ((FAKE, 0, 10, 1.0, None), b"1..65535"),
                      ((FAKE, 65536, 10, 1.0, None), b"1..65535"), ((FAKE, 2, -5, 1.0, None), b"max_numel"),
                      ((FAKE, 2, 10, -0.5, None), b"clip_value"), ((FAKE, 2, 10, math.nan, None), b"clip_value")]:
        assert lib.msn_grad_clamp(*args) == 1 and msg in lib.msn_last_error(), args


def test_python_api_refuses_bad_arguments_and_cpu_gradients():
    from multimodal_supernovae_amd import _lib as L
    from multimodal_supernovae_amd import optim
    p = torch.zeros(4, requires_grad=True)
    p.grad = torch.ones(4)
    with pytest.raises(ValueError, match="1, 2, inf"):
        optim.clip_grad_norm_([p], 1.0, norm_type=3)
    with pytest.raises(ValueError):
        optim.clip_grad_value_([p], -1.0)
    with pytest.raises(L.MsnHipError):           # no CPU path
        optim.clip_grad_norm_([p], 1.0)
    with pytest.raises(L.MsnHipError):
        optim.clip_grad_value_([p], 1.0)
    q = torch.zeros(3, requires_grad=True)       # no gradient anywhere: total norm 0, nothing launched
    assert float(optim.clip_grad_norm_([q], 1.0)) == 0.0 and float(optim.clip_grad_norm_([], 1.0)) == 0.0
    assert optim.clip_grad_value_([q], 1.0) is None


def test_trainer_and_graphed_step_reject_bad_clipping_arguments():
    from multimodal_supernovae_amd.trainer import GraphedTrainStep, Trainer
    dev = torch.device("cpu")
    for kw in (dict(gradient_clip_val=-1.0), dict(gradient_clip_val=1.0, gradient_clip_algorithm="l2"),
               dict(gradient_clip_algorithm="bogus")):
        with pytest.raises(ValueError):
            Trainer(device=dev, **kw)
        with pytest.raises(ValueError):
            GraphedTrainStep(torch.nn.Linear(2, 2), None, **kw)
    assert Trainer(device=dev).clip is None
    assert Trainer(device=dev, gradient_clip_val=0).clip is None                      # 0 = no clipping, as Lightning
    assert Trainer(device=dev, gradient_clip_val=0.5).clip == ("norm", 0.5)            # algorithm None = "norm"
    assert Trainer(device=dev, gradient_clip_val=2, gradient_clip_algorithm="value").clip == ("value", 2.0)
    assert GraphedTrainStep(torch.nn.Linear(2, 2), None, gradient_clip_val=1.0).clip == ("norm", 1.0)


def test_grad_clip_kernels_have_no_scratch(tmp_path):
    from multimodal_supernovae_amd.build import HIPCC
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "multimodal_supernovae_amd", "csrc", "grad_clip.hip")
    asm, err = tmp_path / "grad_clip.s", tmp_path / "grad_clip.err"
    with open(err, "w") as fe:
        r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-ffp-contract=fast",
                            "-Rpass-analysis=kernel-resource-usage", "-S", "--cuda-device-only", src, "-o", str(asm)],
                           stderr=fe, timeout=600)
    assert r.returncode == 0 and asm.stat().st_size > 0, err.read_text()[-3000:]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_scratch.py"), str(err), "--", "grad_"],
                       capture_output=True, text=True, timeout=60)
    last = r.stdout.strip().splitlines()[-1]
    # norm partial + finish for p = 1, 2, inf; scale; clamp
    assert last == "scratch check: 8 kernels -> OK", r.stdout[-3000:]
    assert r.returncode == 0
