"""The wide-head attention kernels (csrc/attention_wide.hip) compiled to ISA with the flags of tools/lint_kernels.sh (no GPU
needed): every instantiation of the three kernels must keep all its values in registers -- no scratch (tools/check_scratch.py).
They count no LDS waits by hand, so tools/check_fragment_waits.py has nothing to check in them."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from multimodal_supernovae_amd.build import HIPCC  # noqa: E402  (the compiler the library is built with)


def test_wide_attention_kernels_have_no_scratch(tmp_path):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "multimodal_supernovae_amd", "csrc", "attention_wide.hip")
    asm, err = tmp_path / "attention_wide.s", tmp_path / "attention_wide.err"
    with open(err, "w") as fe:
        r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17",
                            "-ffp-contract=fast", "-Rpass-analysis=kernel-resource-usage", "-S", "--cuda-device-only", src,
                            "-o", str(asm)], stderr=fe, timeout=900)
    assert r.returncode == 0 and asm.stat().st_size > 0, err.read_text()[-3000:]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_scratch.py"), str(err), "--", "wattn_"],
                       capture_output=True, text=True, timeout=60)
    last = r.stdout.strip().splitlines()[-1]
    # 3 kernels (forward, dQ, dK / dV) x 6 padded widths (192, 256, ..., 512)
    assert last == "scratch check: 18 kernels -> OK", r.stdout[-3000:]
    assert r.returncode == 0
