#!/usr/bin/env python3
"""The linear-probe kernels (csrc/probes.hip, probes.py) on one GPU, next to torch's fp64 on the same device in the same
process.  Median (min .. max) of 5 alternated rounds, device events around `--iters` calls each; nothing here gates.

    Gram       (N, D, K) = (65536, 128, 1) and (65536, 1024, 1): us per call and fp64 TFLOP/s counted over the 64 x 64 tiles of
               the upper triangle actually computed, beside Z.double().T @ Z.double() with the cast, the concatenation and the
               product all timed
    logistic   one loss-and-gradient evaluation at (N, D, C) = (65536, 128, 5) and (8192, 1024, 16) beside torch's fp64
               F.linear + F.cross_entropy(reduction="sum") + backward
    fit        a whole LogisticRegressionProbe.fit at (65536, 128, 5): wall time, iterations, evaluations; with scikit-learn
               importable also LogisticRegression().fit on the host with the copy of the embeddings included

Run it as one `timeout`-wrapped process; --out appends the report to a file (profiles/probes_bench.txt)."""
import argparse
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GRAM_SHAPES = [(65536, 128, 1), (65536, 1024, 1)]
LOGISTIC_SHAPES = [(65536, 128, 5), (8192, 1024, 16)]
FIT_SHAPE = (65536, 128, 5, 0.15)
ROUNDS = 5


def _fmt(v, unit="us"):
    v = sorted(v)
    return f"{v[len(v) // 2]:9.1f} {unit} ({v[0]:.1f} .. {v[-1]:.1f})"


def _alternate(fns, iters):
    """{name: [us per call per round]}: ROUNDS rounds, the forms in turns inside every round."""
    for fn in fns.values():
        for _ in range(3):
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


def gram(iters, say):
    from multimodal_supernovae_amd import probes
    for N, D, K in GRAM_SHAPES:
        g = torch.Generator().manual_seed(N + D)
        X = torch.randn(N, D, generator=g).cuda()
        Y = torch.randn(N, K, generator=g).cuda()
        M = D + 1 + K
        G = torch.empty((M, M), dtype=torch.float64, device="cuda")
        ones = torch.ones(N, 1, device="cuda")

        def hip():
            probes.probe_gram(X, Y, out=G)

        def aten():
            Z = torch.cat([X, ones, Y], dim=1).double()
            return Z.T @ Z

        res = _alternate({"hip": hip, "aten": aten}, iters)
        T = -(-M // 64)
        flops_tri = 2.0 * N * (T * (T + 1) // 2) * 64 * 64
        flops_full = 2.0 * N * M * M
        med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
        say(f"  Gram ({N}, {D}, {K})   msn_probe_gram {_fmt(res['hip'])}  {flops_tri / med['hip'] / 1e6:6.2f} fp64 TFLOP/s over the "
            f"{T * (T + 1) // 2} upper tiles")
        say(f"  {'':22s} torch cat+double+matmul {_fmt(res['aten'])}  {flops_full / med['aten'] / 1e6:6.2f} fp64 TFLOP/s over the full "
            f"{M} x {M};  hip / torch = {med['hip'] / med['aten']:.3f}")


def logistic(iters, say):
    from multimodal_supernovae_amd import probes
    for N, D, C in LOGISTIC_SHAPES:
        g = torch.Generator().manual_seed(N + D + C)
        X = torch.randn(N, D, generator=g).cuda()
        y = torch.randint(0, C, (N,), generator=g).cuda()
        W = (torch.randn(C, D + 1, generator=g, dtype=torch.float64) * 0.1).cuda()
        out = torch.empty(1 + C * (D + 1), dtype=torch.float64, device="cuda")
        Xd = X.double()                                   # torch's side gets its fp64 copy of X for free
        Wt = W[:, :D].clone().requires_grad_()
        bt = W[:, D].clone().requires_grad_()

        def hip():
            probes.logreg_loss_grad(X, y, W, out=out)

        def aten():
            Wt.grad = bt.grad = None
            F.cross_entropy(F.linear(Xd, Wt, bt), y, reduction="sum").backward()

        res = _alternate({"hip": hip, "aten": aten}, iters)
        med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
        say(f"  logistic ({N}, {D}, {C})   msn_logreg_loss_grad {_fmt(res['hip'])}   torch fp64 linear + cross_entropy + backward "
            f"(X already fp64) {_fmt(res['aten'])};  hip / torch = {med['hip'] / med['aten']:.3f}")


def fit(say):
    from multimodal_supernovae_amd import probes
    N, D, C, spread = FIT_SHAPE
    rng = np.random.default_rng(N)
    mu = rng.standard_normal((C, D)) * spread
    yh = rng.integers(0, C, N)
    Xh = (mu[yh] + rng.standard_normal((N, D))).astype(np.float32)
    X, y = torch.from_numpy(Xh).cuda(), torch.from_numpy(yh).cuda()
    probes.LogisticRegressionProbe(n_classes=C, max_iter=3).fit(X, y)        # warm-up
    times = []
    for _ in range(ROUNDS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        p = probes.LogisticRegressionProbe(n_classes=C).fit(X, y)
        times.append((time.perf_counter() - t0) * 1e3)
    say(f"  fit ({N}, {D}, {C})   LogisticRegressionProbe.fit {_fmt(times, 'ms')}: {p.n_iter_} iterations, {p.n_evals_} evaluations, "
        f"objective {p.objective_:.10g}")
    try:
        from sklearn.linear_model import LogisticRegression
    except ImportError:
        say("  scikit-learn is not importable here: no host fit beside it")
        return
    times = []
    for _ in range(ROUNDS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m = LogisticRegression().fit(X.cpu().numpy(), y.cpu().numpy())
        times.append((time.perf_counter() - t0) * 1e3)
    Ws = np.concatenate([m.coef_, m.intercept_[:, None]], axis=1)
    say(f"  {'':20s} scikit-learn LogisticRegression().fit on the host, copy included {_fmt(times, 'ms')}: {int(m.n_iter_[0])} "
        f"iterations, objective {probes.logistic_objective(Xh, yh, Ws)[0]:.10g}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_probes.py measures on the GPU; none is visible")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"tools/bench_probes.py on {torch.cuda.get_device_name(0)}; median (min .. max) of {ROUNDS} alternated rounds, "
        f"{a.iters} calls per round")
    gram(a.iters, say)
    logistic(a.iters, say)
    fit(say)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
