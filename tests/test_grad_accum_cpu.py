"""Gradient accumulation without a GPU: the C-ABI of csrc/grad_accum.hip refuses bad arguments before any launch, the Trainer /
GraphedTrainStep refuse bad accumulate_grad_batches values at construction, and the kernel keeps every value in registers."""
import ctypes
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


def test_grad_accumulate_refuses_bad_arguments():
    lib = _lib()
    cases = [
        ((None, 3, 5000, 1, None, None), b"null"),
        ((FAKE, 0, 5000, 1, None, None), b"1..65535"),
        ((FAKE, -2, 5000, 0, None, None), b"1..65535"),
        ((FAKE, 65536, 5000, 1, None, None), b"1..65535"),
        ((FAKE, 3, -1, 1, None, None), b"max_numel"),
        ((FAKE, 3, 5000, 2, None, None), b"add must be"),
        ((FAKE, 3, 5000, -1, FAKE, None), b"add must be"),
    ]
    for args, msg in cases:
        rc = lib.msn_grad_accumulate(*args)
        assert rc == 1 and msg in lib.msn_last_error(), (args, lib.msn_last_error())


def test_python_api_refuses_cpu_and_mismatched_tensors():
    from multimodal_supernovae_amd import _lib as L
    from multimodal_supernovae_amd import optim
    a, g = torch.zeros(4), torch.ones(4)
    with pytest.raises(L.MsnHipError):           # no CPU path
        optim.grad_accumulate_([a], [a], [g])
    with pytest.raises(ValueError):
        optim.grad_accumulate_([a], [a, a], [g])
    assert optim.grad_accumulate_([], [], []) is None               # nothing to do, nothing launched
    p = torch.zeros(4, requires_grad=True)
    p.grad = torch.ones(4)
    acc = optim.GradAccumulator([p, torch.zeros(2)])                # only what requires a gradient is kept
    assert acc.params == [p] and not acc.window_open
    acc.accumulate(True)                                            # a window of one: nothing launched, even on the CPU
    with pytest.raises(L.MsnHipError):
        acc.accumulate(False)


@pytest.mark.parametrize("bad", [0, -1, 2.5, True, {0: 2}])
def test_trainer_and_graphed_step_refuse_bad_accumulate_grad_batches(bad):
    from multimodal_supernovae_amd.trainer import GraphedTrainStep, Trainer
    with pytest.raises(ValueError, match="out of scope" if isinstance(bad, dict) else "int >= 1"):
        Trainer(device=torch.device("cpu"), accumulate_grad_batches=bad)
    with pytest.raises(ValueError, match="out of scope" if isinstance(bad, dict) else "int >= 1"):
        GraphedTrainStep(torch.nn.Linear(2, 2), None, accumulate_grad_batches=bad)


def test_trainer_and_graphed_step_accept_one_and_four():
    from multimodal_supernovae_amd.trainer import GraphedTrainStep, Trainer
    assert Trainer(device=torch.device("cpu")).accumulate_grad_batches == 1
    for k in (1, 4):
        assert Trainer(device=torch.device("cpu"), accumulate_grad_batches=k).accumulate_grad_batches == k
        assert GraphedTrainStep(torch.nn.Linear(2, 2), None, accumulate_grad_batches=k).k == k


def test_with_last_looks_one_batch_ahead_without_len():
    from multimodal_supernovae_amd.trainer import _with_last
    assert list(_with_last(iter(()))) == []
    assert list(_with_last(x for x in "a")) == [(0, "a", True)]
    assert list(_with_last(x for x in "abc")) == [(0, "a", False), (1, "b", False), (2, "c", True)]


def test_grad_accum_kernel_has_no_scratch(tmp_path):
    from multimodal_supernovae_amd.build import HIPCC
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "multimodal_supernovae_amd", "csrc", "grad_accum.hip")
    asm, err = tmp_path / "grad_accum.s", tmp_path / "grad_accum.err"
    with open(err, "w") as fe:
        r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-ffp-contract=fast",
                            "-Rpass-analysis=kernel-resource-usage", "-S", "--cuda-device-only", src, "-o", str(asm)],
                           stderr=fe, timeout=600)
    assert r.returncode == 0 and asm.stat().st_size > 0, err.read_text()[-3000:]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_scratch.py"), str(err), "--", "grad_accum"],
                       capture_output=True, text=True, timeout=60)
    last = r.stdout.strip().splitlines()[-1]
    assert last == "scratch check: 1 kernels -> OK", r.stdout[-3000:]
    assert r.returncode == 0
