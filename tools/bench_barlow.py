#!/usr/bin/env python3
"""The Barlow Twins loss (loss.barlow_twins_loss on csrc/barlow.hip) on one GPU, forward + backward, as a replayed graph and
through Python, next to a torch fp32 form and a torch fp64 autograd form of the same formula on the same tensors in the same
process; the cross correlation alone next to torch on the fp64 cast; and the headline training step of bench.py, which runs no
code of the loss, in this tree and in a checkout of the parent commit in turns.  Median (min .. max) of 5 alternated rounds;
nothing here gates.

    loss   forward + backward at (N, D) = (256, 128), (1024, 128), (4096, 128), (1024, 256): us per call.  The yardsticks are
           for information; a case slower than one of them is marked.
    corr   embedding_metrics.cross_correlation alone (five launches) beside the same statistics by torch on the fp64 cast, with
           the fp64 TFLOP/s over the tiles computed: 2 * 64 * 64 * N flops per tile pair, T^2 of them.
    step   `python bench.py --gpus 1 --steps K --warmup W` as fresh processes, this tree and --parent-tree in turns, the order
           swapped every round: ms per step of each and the ratio.  Expected: unchanged within the parent's own spread.

Run it as one `timeout`-wrapped process; --out appends the report to a file (profiles/barlow_bench.txt)."""
import argparse
import json
import os
import subprocess
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CASES = [(256, 128), (1024, 128), (4096, 128), (1024, 256)]
ROUNDS = 5
LAMBD, EPS = 5e-3, 1e-5


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


def _statistics(x, y):
    """BatchNorm's statistics and the cross correlation in the dtype of x, y."""
    n = x.shape[0]
    xc, yc = x - x.mean(dim=0), y - y.mean(dim=0)
    vx, vy = (xc * xc).mean(dim=0), (yc * yc).mean(dim=0)
    cov = xc.T @ yc / n
    return vx, vy, cov, cov / torch.outer(torch.sqrt(vx + EPS), torch.sqrt(vy + EPS))


def torch_loss(e1, e2, dtype):
    """The paper's code form in `dtype`: bn(x).T @ bn(y) / N, the diagonal against 1, the off-diagonal squared."""
    c = _statistics(e1.to(dtype), e2.to(dtype))[3]
    d = c.shape[0]
    off = ~torch.eye(d, dtype=torch.bool, device=c.device)
    return torch.diagonal(c).add(-1).pow(2).sum() + LAMBD * c[off].pow(2).sum()


def loss(iters, say):
    from multimodal_supernovae_amd.loss import barlow_twins_loss
    slower = []
    for N, D in CASES:
        g = torch.Generator().manual_seed(N + D)
        a = F.normalize(torch.randn(N, D, generator=g), dim=1)
        b = F.normalize(a + 0.3 * F.normalize(torch.randn(N, D, generator=g), dim=1), dim=1)
        e1, e2 = a.cuda().requires_grad_(True), b.cuda().requires_grad_(True)

        def run(fn):
            e1.grad = e2.grad = None
            out = fn()
            out.backward()
            return out

        def hip():
            return run(lambda: barlow_twins_loss(e1, e2, LAMBD, EPS))

        def aten32():
            return run(lambda: torch_loss(e1, e2, torch.float32))

        def aten64():
            return run(lambda: torch_loss(e1, e2, torch.float64))

        la = float(hip().detach())
        ga = e1.grad.clone()
        lb = float(aten64().detach())
        rel = float((ga - e1.grad).abs().max() / e1.grad.abs().max())
        # forward + backward recorded once and replayed: what a graphed training step pays
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                hip()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        e1.grad = e2.grad = None
        with torch.cuda.graph(graph):
            barlow_twins_loss(e1, e2, LAMBD, EPS).backward()
        graph.replay()
        torch.cuda.synchronize()
        same = bool(torch.equal(e1.grad, ga))
        res = _alternate({"graph": graph.replay, "hip": hip, "aten32": aten32, "aten64": aten64}, iters)
        med = {n: sorted(v)[len(v) // 2] for n, v in res.items()}
        marks = {k: "  ** slower than this yardstick **" if med["hip"] > med[k] else "" for k in ("aten32", "aten64")}
        if any(marks.values()):
            slower.append((N, D))
        say(f"  loss fwd + bwd ({N}, {D})   barlow_twins_loss, replayed graph   {_fmt(res['graph'])};  gradients equal to the eager call's bit for bit: {same}")
        say(f"  {'':29s} barlow_twins_loss through Python      {_fmt(res['hip'])};  loss {la:.6f} against {lb:.6f}, largest gradient "
            f"difference / largest gradient {rel:.1e}")
        say(f"  {'':29s} torch fp32 form + autograd            {_fmt(res['aten32'])};  hip / torch fp32 = {med['hip'] / med['aten32']:.3f}, "
            f"graph / torch fp32 = {med['graph'] / med['aten32']:.3f}{marks['aten32']}")
        say(f"  {'':29s} torch fp64 form + autograd            {_fmt(res['aten64'])};  hip / torch fp64 = {med['hip'] / med['aten64']:.3f}, "
            f"graph / torch fp64 = {med['graph'] / med['aten64']:.3f}{marks['aten64']}")
        del graph
    say(f"  cases slower through Python than a yardstick: {slower if slower else 'none'}")


def corr(iters, say):
    """The cross correlation alone: what the forward's time is made of once the host keeps up."""
    from multimodal_supernovae_amd.embedding_metrics import cross_correlation
    for N, D in CASES:
        g = torch.Generator().manual_seed(N + D)
        X = F.normalize(torch.randn(N, D, generator=g), dim=1).cuda()
        Y = F.normalize(X + 0.3 * F.normalize(torch.randn(N, D, generator=g), dim=1).cuda(), dim=1)
        res = _alternate({"hip": lambda: cross_correlation(X, Y, EPS), "aten64": lambda: _statistics(X.double(), Y.double())}, 4 * iters)
        med = {n: sorted(v)[len(v) // 2] for n, v in res.items()}
        T = -(-D // 64)
        flops = 2.0 * 64 * 64 * N * T * T
        mark = "  ** slower than the yardstick **" if med["hip"] > med["aten64"] else ""
        say(f"  cross_correlation ({N}, {D})   {_fmt(res['hip'])}  {flops / med['hip'] / 1e6:6.3f} fp64 TFLOP/s over the tiles computed;  "
            f"torch on the fp64 cast {_fmt(res['aten64'])};  hip / torch = {med['hip'] / med['aten64']:.3f}{mark}")


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
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit; without it the step is not timed")
    ap.add_argument("--step-rounds", type=int, default=ROUNDS)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step-timeout", type=float, default=180.0, help="seconds allowed to one bench.py process")
    ap.add_argument("--skip-loss", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_barlow.py measures on the GPU; none is visible")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"tools/bench_barlow.py on {torch.cuda.get_device_name(0)}; median (min .. max) of {ROUNDS} alternated rounds, "
        f"{a.iters} calls per round, lambd = {LAMBD}, eps = {EPS}, unit-norm rows")
    if not a.skip_loss:
        loss(a.iters, say)
        corr(a.iters, say)
    if a.parent_tree:
        # the children open the GPU themselves: this process holds it too, and is idle while they run
        step(a.parent_tree, a.step_rounds, a.steps, a.warmup, a.step_timeout, say)
    else:
        say("  headline step: not timed (no --parent-tree given)")
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
