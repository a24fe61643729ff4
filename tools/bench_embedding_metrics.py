#!/usr/bin/env python3
"""The all-pairs Gaussian potential (csrc/embedding_metrics.hip, embedding_metrics.pair_potential) on one GPU, next to a torch
fp64 form on the same tensors in the same process.  Median (min .. max) of 5 alternated rounds, device events around `--iters`
calls each; nothing here gates.

    potential  "within" at (N, D) = (4096, 128), (16384, 128), (65536, 128), (16384, 1024) and "offdiag" at (16384, 128): us per
               call and fp64 TFLOP/s over the 2 * 64 * 64 * D flops of every tile computed (within: T (T + 1) / 2 tiles of the
               T^2), beside torch in fp64: casts, the matrix |x|^2 + |y|^2 - 2 X Y^T by mm, clamp, exp and the masked sums, all
               timed.  Above 16384 rows the torch form runs in chunks of 8192 rows (the matrix of 65536^2 doubles is 34 GB, and
               the form keeps three of them alive); the kernel never chunks.
    compute    a whole EmbeddingMetrics.compute() at (16384, 128) in wall time, and its parts timed alone

Run it as one `timeout`-wrapped process; --out appends the report to a file (profiles/embedding_metrics_bench.txt)."""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CASES = [("within", 4096, 128), ("within", 16384, 128), ("within", 65536, 128), ("within", 16384, 1024), ("offdiag", 16384, 128)]
COMPUTE_SHAPE = (16384, 128)
TORCH_CHUNK = 8192
ROUNDS = 5
T = 2.0


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


def torch_potential(X, Y, t, pairs):
    """(sum exp(-t d2), sum d2) in fp64 by the expansion with mm, in row chunks above 16384 rows."""
    Xd = X.double()
    Yd = Xd if Y is None else Y.double()
    nx, ny = (Xd * Xd).sum(dim=1), (Yd * Yd).sum(dim=1)
    cols = torch.arange(Yd.shape[0], device=X.device)
    step = Xd.shape[0] if Xd.shape[0] <= 16384 else TORCH_CHUNK
    se = torch.zeros((), dtype=torch.float64, device=X.device)
    sd = torch.zeros((), dtype=torch.float64, device=X.device)
    for r0 in range(0, Xd.shape[0], step):
        rows = torch.arange(r0, min(r0 + step, Xd.shape[0]), device=X.device)
        d2 = (nx[rows][:, None] + ny[None, :] - 2.0 * (Xd[rows] @ Yd.T)).clamp_min_(0.0)
        keep = cols[None, :] > rows[:, None] if pairs == "within" else cols[None, :] != rows[:, None]
        se += torch.where(keep, torch.exp(-t * d2), 0.0).sum()
        sd += torch.where(keep, d2, 0.0).sum()
    return torch.stack([se, sd])


def potential(iters, say):
    from multimodal_supernovae_amd import embedding_metrics as E
    slower = []
    for pairs, N, D in CASES:
        g = torch.Generator().manual_seed(N + D)
        X = torch.nn.functional.normalize(torch.randn(N, D, generator=g), dim=1).cuda()
        Y = None if pairs == "within" else torch.nn.functional.normalize(torch.randn(N, D, generator=g), dim=1).cuda()

        def hip():
            return E.pair_potential(X, Y, T, pairs)

        def aten64():
            return torch_potential(X, Y, T, pairs)

        a, b = hip().cpu(), aten64().cpu()
        rel = float(((a - b).abs() / b.abs()).max())
        res = _alternate({"hip": hip, "aten64": aten64}, iters)
        med = {n: sorted(v)[len(v) // 2] for n, v in res.items()}
        tiles = -(-N // 64)
        tiles = tiles * (tiles + 1) // 2 if pairs == "within" else tiles * tiles
        flops = 2.0 * 64 * 64 * D * tiles
        mark = "  ** slower than the yardstick **" if med["hip"] > med["aten64"] else ""
        if mark:
            slower.append((pairs, N, D))
        say(f"  potential {pairs:8s}({N}, {D})   msn_pair_potential {_fmt(res['hip'])}  {flops / med['hip'] / 1e6:6.2f} fp64 TFLOP/s over "
            f"{tiles} tiles;  largest relative difference to the yardstick {rel:.1e}")
        chunks = "one matrix" if N <= 16384 else f"chunks of {TORCH_CHUNK} rows"
        say(f"  {'':33s} torch fp64 mm + clamp + exp + masked sums ({chunks}) {_fmt(res['aten64'])};  hip / torch fp64 = "
            f"{med['hip'] / med['aten64']:.3f}{mark}")
    say(f"  cases slower than the yardstick: {slower if slower else 'none'}")


def _wall(fn, iters):
    out = []
    for _ in range(ROUNDS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / iters * 1e6)
    return out


def compute(iters, say):
    from multimodal_supernovae_amd import embedding_metrics as E
    from multimodal_supernovae_amd.utils import retrieval_ranks
    N, D = COMPUTE_SHAPE
    g = torch.Generator().manual_seed(N)
    A = torch.randn(N, D, generator=g).cuda()
    B = (A + 0.5 * torch.randn(N, D, generator=g).cuda())
    acc = E.EmbeddingMetrics().update(A, B)
    acc.compute()                                                               # warm-up
    Au, Bu = acc._a[0], acc._b[0]
    Gh = acc.gram_a.cpu().numpy()
    parts = {
        "update (two normalisations, two Gram calls)": lambda: E.EmbeddingMetrics().update(A, B),
        "compute()": acc.compute,
        "  pair_alignment": lambda: E.pair_alignment(Au, Bu),
        "  pair_potential within, twice": lambda: (E.pair_potential(Au, None, T), E.pair_potential(Bu, None, T)),
        "  pair_potential offdiag": lambda: E.pair_potential(Au, Bu, T, "offdiag"),
        "  retrieval_ranks, both directions": lambda: (retrieval_ranks(Au, Bu), retrieval_ranks(Bu, Au)),
        "  host: two spectra and entropies": lambda: [E.effective_rank(E.covariance_spectrum(Gh, D)) for _ in range(2)],
    }
    for fn in parts.values():
        fn()
    res = {name: _wall(fn, iters) for name, fn in parts.items()}
    whole = sorted(res["compute()"])[ROUNDS // 2]
    say(f"  EmbeddingMetrics at ({N}, {D}), wall time, median (min .. max) of {ROUNDS} rounds:")
    for name, v in res.items():
        share = f" = {100 * sorted(v)[ROUNDS // 2] / whole:5.1f} % of compute()" if name.startswith("  ") else ""
        say(f"    {name:46s} {_fmt(v)}{share}")
    say(f"    (what is left of compute() is the concatenation, the copies into the one buffer and its {8 * (8 + 2 * (D + 1) ** 2 + 2 * N)} "
        f"bytes to the host)")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_embedding_metrics.py measures on the GPU; none is visible")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"tools/bench_embedding_metrics.py on {torch.cuda.get_device_name(0)}; median (min .. max) of {ROUNDS} alternated rounds, "
        f"{a.iters} calls per round, t = {T}")
    potential(a.iters, say)
    compute(a.iters, say)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
