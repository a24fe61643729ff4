#!/usr/bin/env python3
"""The exact kNN search (csrc/knn.hip, probes.knn_search) on one GPU, next to torch.cdist(...).topk on the same tensors in the
same process.  Median (min .. max) of 5 alternated rounds, device events around `--iters` calls each; nothing here gates.

    search     (Nq, Nx, D, k) = (4096, 16384, 128, 5), (4096, 65536, 128, 5), (2048, 16384, 1024, 5), (4096, 16384, 128, 64):
               us per call and fp64 TFLOP/s over the 2 Nq Nx D flops of the dot products, beside torch.cdist in fp64 + topk
               (the equal-precision alternative: the casts, the Nq x Nx matrix and the selection all timed) and, for
               information, beside torch.cdist in fp32 + topk, where near-ties resolve by rounding
    probe      a whole utils.knn_probe_metrics call (fit, search, predict, metrics, the copy of the sums) at
               (4096, 16384, 128, 5) in wall time, and the share of the search's two launches in it

Run it as one `timeout`-wrapped process; --out appends the report to a file (profiles/knn_bench.txt)."""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SEARCH_SHAPES = [(4096, 16384, 128, 5), (4096, 65536, 128, 5), (2048, 16384, 1024, 5), (4096, 16384, 128, 64)]
PROBE_SHAPE = (4096, 16384, 128, 5)
ROUNDS = 5


def _fmt(v, unit="us"):
    v = sorted(v)
    return f"{v[len(v) // 2]:10.1f} {unit} ({v[0]:.1f} .. {v[-1]:.1f})"


def _alternate(fns, iters):
    """{name: [us per call per round]}: ROUNDS rounds, the forms in turns inside every round."""
    for fn in fns.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    res = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            e1.synchronize()
            res[name].append(e0.elapsed_time(e1) / iters * 1e3)
    return res


def search(iters, say):
    from multimodal_supernovae_amd import probes
    for Nq, Nx, D, k in SEARCH_SHAPES:
        g = torch.Generator().manual_seed(Nx + D + k)
        X = torch.randn(Nx, D, generator=g).cuda()
        Q = torch.randn(Nq, D, generator=g).cuda()

        def hip():
            return probes.knn_search(Q, X, k, return_squared=True)

        def aten64():
            return torch.cdist(Q.double(), X.double()).topk(k, dim=1, largest=False)

        def aten32():
            return torch.cdist(Q, X).topk(k, dim=1, largest=False)

        idx, _ = hip()
        same = float((idx.long().sort(dim=1).values == aten64().indices.sort(dim=1).values).float().mean())
        res = _alternate({"hip": hip, "aten64": aten64, "aten32": aten32}, iters)
        med = {n: sorted(v)[len(v) // 2] for n, v in res.items()}
        flops = 2.0 * Nq * Nx * D
        say(f"  search ({Nq}, {Nx}, {D}, {k})   msn_knn_search {_fmt(res['hip'])}  {flops / med['hip'] / 1e6:6.2f} fp64 TFLOP/s over the dot "
            f"products;  neighbours equal to the fp64 yardstick's: {100 * same:.3f} %")
        say(f"  {'':30s} torch fp64 cdist + topk {_fmt(res['aten64'])};  hip / torch fp64 = {med['hip'] / med['aten64']:.3f}")
        say(f"  {'':30s} torch fp32 cdist + topk {_fmt(res['aten32'])}  (for information);  hip / torch fp32 = "
            f"{med['hip'] / med['aten32']:.3f}")


def probe(iters, say):
    from multimodal_supernovae_amd import probes, utils
    Nq, Nx, D, k = PROBE_SHAPE
    g = torch.Generator().manual_seed(Nx)
    X = torch.randn(Nx, D, generator=g).cuda()
    Xv = torch.randn(Nq, D, generator=g).cuda()
    Y = torch.randn(Nx, generator=g).cuda()
    Yv = torch.randn(Nq, generator=g).cuda()
    utils.knn_probe_metrics(X, Y, Xv, Yv, k=k)                               # warm-up
    whole, alone = [], []
    for _ in range(ROUNDS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            utils.knn_probe_metrics(X, Y, Xv, Yv, k=k)
        whole.append((time.perf_counter() - t0) / iters * 1e6)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            probes.knn_search(Xv, X, k, return_squared=True)
        torch.cuda.synchronize()
        alone.append((time.perf_counter() - t0) / iters * 1e6)
    mw, ma = sorted(whole)[ROUNDS // 2], sorted(alone)[ROUNDS // 2]
    say(f"  probe ({Nq}, {Nx}, {D}, {k})   utils.knn_probe_metrics (regression), wall {_fmt(whole)};  the search alone "
        f"{_fmt(alone)} = {100 * ma / mw:.1f} % of the call")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_knn.py measures on the GPU; none is visible")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"tools/bench_knn.py on {torch.cuda.get_device_name(0)}; median (min .. max) of {ROUNDS} alternated rounds, "
        f"{a.iters} calls per round")
    search(a.iters, say)
    probe(a.iters, say)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
