"""Weight averaging without a GPU: the update rule of checkpoint.WeightAveraging, the argument checks of optim.AveragedWeights,
the callback and the C-ABI of csrc/weight_avg.hip (refused before any launch), the callback's state in a checkpoint, the new
no-op hooks of checkpoint.Callback, and the kernel's registers."""
import ctypes
import os
import shutil
import subprocess
import sys

import pytest
import torch

from conftest import ROOT

FAKE = ctypes.c_void_p(4096)          # never dereferenced: validation rejects the call before any launch
HOOKS = ["on_fit_start", "on_optimizer_step", "on_train_epoch_end", "on_validation_start", "on_validation_end", "on_fit_end"]


def test_update_rule_over_a_table():
    from multimodal_supernovae_amd.checkpoint import WeightAveraging, averaging_due
    table = [  # (global_step, start_step, every_n_steps) -> updated after that step?
        ((1, 0, 1), True), ((2, 0, 1), True), ((1, 1, 1), False), ((2, 1, 1), True), ((1, 0, 2), False), ((2, 0, 2), True),
        ((3, 0, 2), False), ((4, 0, 2), True), ((2, 2, 2), False), ((3, 2, 2), False), ((4, 2, 2), True), ((5, 2, 2), False),
        ((6, 2, 2), True), ((7, 2, 2), False), ((0, 0, 1), False), ((5, 10, 1), False), ((10, 10, 1), False), ((11, 10, 1), True),
        ((13, 10, 3), True), ((14, 10, 3), False), ((16, 10, 3), True),
    ]
    for args, want in table:
        assert averaging_due(*args) is want, args
    assert [s for s in range(1, 8) if averaging_due(s, 2, 2)] == [4, 6]
    cb = WeightAveraging(start_step=2, every_n_steps=2)
    assert [s for s in range(1, 8) if cb.due(s)] == [4, 6]
    assert all(WeightAveraging().due(s) for s in range(1, 50))


def test_averaged_weights_refuses_bad_arguments():
    from multimodal_supernovae_amd import _lib as L
    from multimodal_supernovae_amd import optim
    lin = torch.nn.Linear(3, 2)
    with pytest.raises(ValueError, match="'ema' or 'swa'"):
        optim.AveragedWeights(lin, avg="mean")
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match=r"decay must lie in \[0, 1\]"):
            optim.AveragedWeights(lin, decay=bad)
    with pytest.raises(ValueError, match="needs a module"):
        optim.AveragedWeights(list(lin.parameters()), use_buffers=True)
    frozen = torch.nn.Linear(3, 2).requires_grad_(False)
    with pytest.raises(ValueError, match="nothing to average"):
        optim.AveragedWeights(frozen)
    with pytest.raises(L.MsnHipError):            # no CPU path
        optim.AveragedWeights(lin)


def test_weight_averaging_refuses_bad_arguments():
    from multimodal_supernovae_amd.checkpoint import EarlyStopping, WeightAveraging
    from multimodal_supernovae_amd.trainer import Trainer
    with pytest.raises(ValueError, match="'ema' or 'swa'"):
        WeightAveraging(avg="lerp")
    for bad in (-1e-3, 1.0001, float("nan")):
        with pytest.raises(ValueError, match="decay"):
            WeightAveraging(decay=bad)
    with pytest.raises(ValueError, match="update_on"):
        WeightAveraging(update_on="batch")
    for bad in (0, -3, 1.5, True):
        with pytest.raises(ValueError, match="every_n_steps"):
            WeightAveraging(every_n_steps=bad)
    with pytest.raises(ValueError, match="start_step"):
        WeightAveraging(start_step=-1)
    with pytest.raises(ValueError, match="start_epoch"):
        WeightAveraging(start_epoch=-1)
    for decay in (0.0, 1.0, 0.9999):
        assert WeightAveraging(decay=decay).decay == decay
    with pytest.raises(ValueError, match="2 WeightAveraging"):
        Trainer(device=torch.device("cpu"), callbacks=[WeightAveraging(), EarlyStopping("val_loss"), WeightAveraging("swa")])
    one = WeightAveraging("swa", update_on="epoch")
    tr = Trainer(device=torch.device("cpu"), callbacks=[one, EarlyStopping("val_loss")])
    assert tr.weight_averaging is one and Trainer(device=torch.device("cpu")).weight_averaging is None


def test_callback_state_is_plain_and_round_trips(tmp_path):
    from multimodal_supernovae_amd import checkpoint as C
    inner = {"avg": "ema", "decay": 0.9, "use_buffers": False, "n_averaged": 5, "swapped": False,
             "averages": {"w": torch.arange(6.0).view(2, 3), "b": torch.tensor([float("nan"), -0.0])}}
    cb = C.WeightAveraging("ema", 0.9, start_step=2, every_n_steps=3)
    assert cb.state_dict()["average"] is None                  # nothing averaged yet: still a plain state
    cb.load_state_dict({"avg": "ema", "average": inner})       # before fit: kept until the average exists
    state = cb.state_dict()
    plain = C._plain({cb.state_key: state}, "callbacks")
    path = tmp_path / "cb.pt"
    torch.save(plain, path)
    back = torch.load(path, weights_only=True)[cb.state_key]
    assert back["avg"] == "ema" and back["decay"] == 0.9 and back["start_step"] == 2 and back["every_n_steps"] == 3
    got = back["average"]
    assert got["n_averaged"] == 5 and got["swapped"] is False and set(got["averages"]) == {"w", "b"}
    assert torch.equal(got["averages"]["w"], inner["averages"]["w"])
    assert torch.equal(got["averages"]["b"].view(torch.int32), inner["averages"]["b"].view(torch.int32))
    with pytest.raises(ValueError, match="avg='swa'"):
        C.WeightAveraging("ema").load_state_dict({"avg": "swa", "average": inner})
    with pytest.raises(ValueError, match="no weight average"):
        C.WeightAveraging.load_average(torch.nn.Linear(2, 2), {"callbacks": {}, "state_dict": {}})


def test_existing_callbacks_inherit_the_new_hooks_as_no_ops(tmp_path):
    from multimodal_supernovae_amd import checkpoint as C
    for cb in (C.Callback(), C.ModelCheckpoint(str(tmp_path)), C.EarlyStopping("val_loss")):
        before = dict(cb.state_dict())
        for name in HOOKS:
            assert getattr(type(cb), name) is getattr(C.Callback, name), (type(cb).__name__, name)
            assert getattr(cb, name)(None) is None              # never touches the trainer
        assert cb.state_dict() == before
    for name in HOOKS:
        if name != "on_optimizer_step":                         # (decided by update_on / the graphed step inside the hook)
            assert getattr(C.WeightAveraging, name) is not getattr(C.Callback, name), name


def _lib():
    import __graft_entry__ as entry
    entry.build()
    from multimodal_supernovae_amd import _lib
    return _lib.lib()


def test_weight_average_refuses_bad_arguments():
    lib = _lib()
    EMA, SWA, SWAP = 0, 1, 2
    cases = [
        ((None, 3, 5000, EMA, 0.1, FAKE, None), b"null table"),
        ((FAKE, 0, 5000, EMA, 0.1, FAKE, None), b"1..65535"),
        ((FAKE, -2, 5000, SWA, 0.1, FAKE, None), b"1..65535"),
        ((FAKE, 65536, 5000, SWAP, 0.1, None, None), b"1..65535"),
        ((FAKE, 3, -1, EMA, 0.1, FAKE, None), b"max_numel"),
        ((FAKE, 3, 5000, 3, 0.1, FAKE, None), b"mode must be"),
        ((FAKE, 3, 5000, -1, 0.1, FAKE, None), b"mode must be"),
        ((FAKE, 3, 5000, EMA, -0.001, FAKE, None), b"[0, 1]"),
        ((FAKE, 3, 5000, EMA, 1.001, FAKE, None), b"[0, 1]"),
        ((FAKE, 3, 5000, EMA, float("nan"), FAKE, None), b"[0, 1]"),
        ((FAKE, 3, 5000, EMA, 0.1, None, None), b"null state"),
        ((FAKE, 3, 5000, SWA, 0.1, None, None), b"null state"),
    ]
    for args, msg in cases:
        rc = lib.msn_weight_average(*args)
        assert rc == 1 and msg in lib.msn_last_error(), (args, lib.msn_last_error())


def test_weight_avg_kernel_has_no_scratch(tmp_path):
    from multimodal_supernovae_amd.build import HIPCC
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "multimodal_supernovae_amd", "csrc", "weight_avg.hip")
    asm, err = tmp_path / "weight_avg.s", tmp_path / "weight_avg.err"
    with open(err, "w") as fe:
        r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-ffp-contract=fast",
                            "-Rpass-analysis=kernel-resource-usage", "-S", "--cuda-device-only", src, "-o", str(asm)],
                           stderr=fe, timeout=600)
    assert r.returncode == 0 and asm.stat().st_size > 0, err.read_text()[-3000:]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_scratch.py"), str(err), "--", "weight_avg"],
                       capture_output=True, text=True, timeout=60)
    last = r.stdout.strip().splitlines()[-1]
    assert last == "scratch check: 2 kernels -> OK", r.stdout[-3000:]
    assert r.returncode == 0
