#!/usr/bin/env python3
"""Contrastive-loss forward / backward and retrieval rank across embedding widths (D = 128 / 256: csrc/infonce.hip; 512 / 1024:
csrc/infonce_wide.hip), single process, straight through the C-ABI with preallocated workspace: HIP events around `reps`
back-to-back calls, after a warm-up.  Each call is its main kernel plus the finish kernel.  TFLOP/s counts the fp32 MFMA work:
forward 2 directions x 2 N^2 D, backward 2 directions x (score recompute + dQ) 4 N^2 D, rank 2 N^2 D.

    python tools/bench_infonce_wide.py [--reps 100]
"""
import argparse
import ctypes
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multimodal_supernovae_amd._lib import check, lib, require_gpu, stream_ptr  # noqa: E402


def unit(n, d, seed):
    x = torch.randn(n, d, generator=torch.Generator().manual_seed(seed))
    return (x / x.norm(dim=-1, keepdim=True)).cuda()


def timed(fn, reps):
    for _ in range(5):
        fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps * 1e3          # microseconds per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    args = ap.parse_args()
    require_gpu()
    L = lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    for n in (1024, 4096):
        for d in (128, 256, 512, 1024):
            e1, e2 = unit(n, d, 1), unit(n, d, 2)
            nb = L.msn_infonce_workspace_bytes(n, n, n, n, d)
            ws = torch.empty(nb // 4 + 1, dtype=torch.float32, device="cuda")
            ls, lb, one = (torch.tensor(v, device="cuda") for v in (math.log(19.5), -10.0, 1.0))
            lr, lc, loss = torch.empty(n, device="cuda"), torch.empty(n, device="cuda"), torch.empty((), device="cuda")
            g1, g2, dsb = torch.empty(n, d, device="cuda"), torch.empty(n, d, device="cuda"), torch.empty(2, device="cuda")
            rank = torch.empty(n, dtype=torch.int32, device="cuda")
            st = stream_ptr()

            def fwd():
                check(L.msn_infonce_fwd(p(e1), d, n, p(e2), d, n, p(e1), d, n, p(e2), d, n, d, 0, p(ls), p(lb), p(lr), p(lc),
                                        p(loss), p(ws), nb, st), "msn_infonce_fwd")

            def bwd():
                check(L.msn_infonce_bwd(p(e1), d, n, p(e2), d, n, p(e1), d, n, p(e2), d, n, d, 0, p(ls), p(lb), p(lr), p(lc),
                                        p(one), p(g1), d, p(g2), d, p(dsb), p(ws), nb, st), "msn_infonce_bwd")

            def rnk():
                check(L.msn_retrieval_rank(p(e1), d, p(e2), d, n, d, p(rank), p(ws), nb, st), "msn_retrieval_rank")

            fwd()
            tf, tb, tr = timed(fwd, args.reps), timed(bwd, args.reps), timed(rnk, args.reps)
            nn = float(n) * n * d
            row = {"N": n, "D": d, "workspace_MB": round(nb / 1e6, 1),
                   "fwd_us": round(tf, 1), "bwd_us": round(tb, 1), "rank_us": round(tr, 1),
                   "fwd_tflops": round(4 * nn / tf / 1e6, 1), "bwd_tflops": round(8 * nn / tb / 1e6, 1),
                   "rank_tflops": round(2 * nn / tr / 1e6, 1),
                   "fwd_plus_bwd_us_per_128_columns": round((tf + tb) * 128 / d, 1)}
            print(json.dumps(row), flush=True)
            del ws


if __name__ == "__main__":
    main()
