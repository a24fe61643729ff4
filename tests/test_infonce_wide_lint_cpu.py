"""The wide contrastive-loss kernels (csrc/infonce_wide.hip) compiled to ISA with the flags of tools/lint_kernels.sh (no GPU
needed): every instantiation of the three kernels (forward, backward, retrieval rank) must keep all its values in registers -- no
scratch (tools/check_scratch.py)."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from multimodal_supernovae_amd.build import HIPCC  # noqa: E402  (the compiler the library is built with)


def test_wide_infonce_kernels_have_no_scratch(tmp_path):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "multimodal_supernovae_amd", "csrc", "infonce_wide.hip")
    asm, err = tmp_path / "infonce_wide.s", tmp_path / "infonce_wide.err"
    with open(err, "w") as fe:
        r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17",
                            "-ffp-contract=fast", "-Rpass-analysis=kernel-resource-usage", "-S", "--cuda-device-only", src,
                            "-o", str(asm)], stderr=fe, timeout=900)
    assert r.returncode == 0 and asm.stat().st_size > 0, err.read_text()[-3000:]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_scratch.py"), str(err), "--", "nce_wide_"],
                       capture_output=True, text=True, timeout=60)
    last = r.stdout.strip().splitlines()[-1]
    # 3 kernels (forward, backward, rank) x 6 columns per wave (96, 128, ..., 256)
    assert last == "scratch check: 18 kernels -> OK", r.stdout[-3000:]
    assert r.returncode == 0
