"""The label-aware contrastive loss under data parallel with global negatives: two ranks (sharing the one GPU of the test box,
gloo transport with CUDA tensors, as tests/test_distributed_gpu.py runs tools/dist_check.py) against the single-process step at
twice the batch -- the loss, the gradients of the embeddings and the parameters after one step."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_two_rank_supcon_step_equals_single_process_global_batch():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "dist_check_supcon.py")], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and "DIST CHECK OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
