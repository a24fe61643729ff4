#!/usr/bin/env python3
"""Centred kernel alignment (embedding_metrics.hsic_sums / cka on csrc/cka.hip) on one GPU, as a replayed graph and through
Python, next to two torch forms that materialise the N x N kernel matrices on the device, one in fp64 and one in fp32, on the
same tensors in the same process; and the headline training step of bench.py, which runs no code of this change, in this tree
and in a checkout of the parent commit in turns.  Median (min .. max) of 5 alternated rounds; nothing here gates.

    sums   hsic_sums (the launches alone) and cka (with its one host copy) at (N, Dx, Dy) = (1024, 128, 128), (4096, 128, 128),
           (4096, 1024, 256), (8192, 256, 256), linear and RBF (derived bandwidth): us per call, and the fp64 TFLOP/s over the
           tiles computed: 2 * 64 * 64 * (32 ceil(Dx / 32) + 32 ceil(Dy / 32)) flops per tile pair, ceil(N / 64)^2 of them (the
           full square; row sums need no transposed contributions that way).
    torch  biased CKA from the centred N x N matrices, K - row means - column means + mean, in fp64 and in fp32, with the same
           derived bandwidth; the fp32 form's CKA error is taken against the fp64 form (a longdouble restatement of 8192^2
           entries is out of reach; tests/test_cka_gpu.py pins the kernel to longdouble at sizes where it is not).  A case slower
           than a yardstick is marked.
    step   `python bench.py --gpus 1 --steps K --warmup W` as fresh processes, this tree and --parent-tree in turns, the order
           swapped every round: ms per step of each and the ratio.  Expected: unchanged within the parent's own spread.

Run it as one `timeout`-wrapped process; --out appends the report to a file (profiles/cka_bench.txt)."""
import argparse
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CASES = [(1024, 128, 128), (4096, 128, 128), (4096, 1024, 256), (8192, 256, 256)]
ROUNDS = 5


def _fmt(v, unit="us", digits=1):
    v = sorted(v)
    return f"{v[len(v) // 2]:10.{digits}f} {unit} ({v[0]:.{digits}f} .. {v[-1]:.{digits}f})"


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


def _torch_kernel(Z, kernel):
    zc = Z - Z.mean(dim=0)
    g = zc @ zc.T
    if kernel == "linear":
        return g
    n = torch.diagonal(g)
    d2 = (n[:, None] + n[None, :] - 2 * g).clamp_min_(0)
    N = Z.shape[0]
    s2 = d2.sum() / (N * (N - 1))
    return torch.exp(d2 / (-2 * s2))


def _centre(K):
    return K - K.mean(dim=0, keepdim=True) - K.mean(dim=1, keepdim=True) + K.mean()


def torch_cka(X, Y, kernel, dtype):
    """Biased CKA with both N x N matrices written: <HKH, HLH> / (|HKH|_F |HLH|_F), a device scalar."""
    Kc, Lc = _centre(_torch_kernel(X.to(dtype), kernel)), _centre(_torch_kernel(Y.to(dtype), kernel))
    return (Kc * Lc).sum() / torch.sqrt((Kc * Kc).sum() * (Lc * Lc).sum())


def sums(iters, say):
    from multimodal_supernovae_amd.embedding_metrics import cka, hsic_sums
    slower = []
    for N, Dx, Dy in CASES:
        g = torch.Generator().manual_seed(N + Dx + Dy)
        X = torch.nn.functional.normalize(torch.randn(N, Dx, generator=g), dim=1).cuda()
        Y = torch.randn(N, Dy, generator=g).cuda() * 0.3
        k = min(Dx, Dy)
        Y[:, :k] += X[:, :k]
        T = -(-N // 64)
        flops = 2.0 * 64 * 64 * (32 * -(-Dx // 32) + 32 * -(-Dy // 32)) * T * T
        for kernel in ("linear", "rbf"):
            first = hsic_sums(X, Y, kernel)
            value = cka(X, Y, kernel)
            v64, v32 = float(torch_cka(X, Y, kernel, torch.float64)), float(torch_cka(X, Y, kernel, torch.float32))
            # the launches recorded once and replayed: what a graphed evaluation pays
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(3):
                    hsic_sums(X, Y, kernel)
            torch.cuda.current_stream().wait_stream(side)
            out = torch.empty((2, 8), dtype=torch.float64, device="cuda")
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                hsic_sums(X, Y, kernel, out=out)
            graph.replay()
            torch.cuda.synchronize()
            same = bool(torch.equal(out, first))
            n_it = max(1, iters // 2) if N >= 8192 else iters
            res = _alternate({"graph": graph.replay, "hip": lambda: hsic_sums(X, Y, kernel), "cka": lambda: cka(X, Y, kernel),
                              "aten64": lambda: torch_cka(X, Y, kernel, torch.float64),
                              "aten32": lambda: torch_cka(X, Y, kernel, torch.float32)}, n_it)
            med = {n: sorted(v)[len(v) // 2] for n, v in res.items()}
            marks = {y: "  **slower than this yardstick**" if med["hip"] > med[y] else "" for y in ("aten64", "aten32")}
            if any(marks.values()):
                slower.append((N, Dx, Dy, kernel))
            head = f"  ({N}, {Dx}, {Dy}) {kernel:6s}"
            say(f"{head} hsic_sums, replayed graph      {_fmt(res['graph'])}  {flops / med['graph'] / 1e6:6.2f} fp64 TFLOP/s over the tiles "
                f"computed;  the sums equal to the eager call's bit for bit: {same}")
            say(f"  {'':{len(head) - 2}s} hsic_sums through Python      {_fmt(res['hip'])}  {flops / med['hip'] / 1e6:6.2f} fp64 TFLOP/s")
            say(f"  {'':{len(head) - 2}s} cka (one host copy)           {_fmt(res['cka'])};  cka {value:.12f}, torch fp64 form {v64:.12f}, "
                f"difference {abs(value - v64):.1e}")
            say(f"  {'':{len(head) - 2}s} torch fp64, N x N written     {_fmt(res['aten64'])};  hip / torch fp64 = {med['hip'] / med['aten64']:.3f}, "
                f"graph / torch fp64 = {med['graph'] / med['aten64']:.3f}{marks['aten64']}")
            say(f"  {'':{len(head) - 2}s} torch fp32, N x N written     {_fmt(res['aten32'])};  hip / torch fp32 = {med['hip'] / med['aten32']:.3f}, "
                f"graph / torch fp32 = {med['graph'] / med['aten32']:.3f}{marks['aten32']};  CKA error of the fp32 form {abs(v32 - v64):.1e}")
            del graph
    say(f"  cases whose hsic_sums is slower through Python than a yardstick: {slower if slower else 'none'}")


def _bench_once(tree, steps, warmup, limit):
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)], cwd=tree,
                       capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        raise SystemExit(f"bench.py in {tree} ended with {r.returncode}:\n{r.stderr[-2000:]}")
    for line in reversed(r.stdout.splitlines()):
        if line.startswith("{"):
            return json.loads(line)["ms_per_step"]
    raise SystemExit(f"bench.py in {tree} printed no result line")


def step(parent, rounds, steps, warmup, limit, say):
    trees = {"parent": os.path.abspath(parent), "this change": ROOT}
    res = {k: [] for k in trees}
    for r in range(rounds):
        order = list(trees) if r % 2 == 0 else list(trees)[::-1]
        for name in order:
            res[name].append(_bench_once(trees[name], steps, warmup, limit))
    med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
    say(f"  headline step, bench.py --gpus 1 --steps {steps} --warmup {warmup}, fresh processes in turns, the order swapped every round, "
        f"{rounds} rounds:")
    for k, v in res.items():
        say(f"    {k:12s} {_fmt(v, 'ms per step', 3)}   rounds: {', '.join(f'{x:.3f}' for x in v)}")
    lo, hi = min(res["parent"]), max(res["parent"])
    inside = lo <= med["this change"] <= hi
    say(f"    this change / parent = {med['this change'] / med['parent']:.4f};  the median of this change lies "
        f"{'inside' if inside else '** outside **'} the parent's own spread ({lo:.2f} .. {hi:.2f} ms)")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit; without it the step is not timed")
    ap.add_argument("--step-rounds", type=int, default=ROUNDS)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step-timeout", type=float, default=180.0, help="seconds allowed to one bench.py process")
    ap.add_argument("--skip-sums", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cka.py measures on the GPU; none is visible")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"tools/bench_cka.py on {torch.cuda.get_device_name(0)}; median (min .. max) of {ROUNDS} alternated rounds, "
        f"{a.iters} calls per round ({max(1, a.iters // 2)} at N = 8192), unit-norm X, Y sharing its first columns with X")
    if not a.skip_sums:
        sums(a.iters, say)
    if a.parent_tree:
        # the children open the GPU themselves: this process holds it too, and is idle while they run
        step(a.parent_tree, a.step_rounds, a.steps, a.warmup, a.step_timeout, say)
    else:
        say("  headline step: not timed (no --parent-tree given)")
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
