#!/usr/bin/env python3
"""The alignment + uniformity loss (loss.align_uniform_loss on csrc/uniformity_loss.hip) on one GPU, forward + backward, next to
a torch fp64 autograd form of the same formula on the same tensors in the same process; and the headline training step of
bench.py, which runs no code of the loss, in this tree and in a checkout of the parent commit in turns.  Median (min .. max)
of 5 alternated rounds; nothing here gates.

    loss   forward + backward at (N, D) = (1024, 128), (4096, 128), (1024, 256): us per call, and the fp64 TFLOP/s of the two
           row fields over their 2 * 2 * 2 * 64 * 64 * D flops per tile pair (scores and W.Y, both towers), beside torch in fp64:
           casts, |x|^2 + |y|^2 - 2 X X^T by mm, clamp, exp, the masked sum, log, and autograd's backward through all of it.
           The yardstick is for information; a case slower than it is marked.
    field  embedding_metrics.pair_field of one tower alone at the same shapes: the two launches without the autograd node
    step   `python bench.py --gpus 1 --steps K --warmup W` as fresh processes, this tree and --parent-tree in turns, the order
           swapped every round: ms per step of each and the ratio.  Expected: unchanged within the parent's own spread.

Run it as one `timeout`-wrapped process; --out appends the report to a file (profiles/align_uniform_bench.txt)."""
import argparse
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CASES = [(1024, 128), (4096, 128), (1024, 256)]
ROUNDS = 5
ALPHA, T, LAM = 2, 2.0, 1.0


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


def torch_loss(e1, e2, alpha, t, lam):
    """The same formula in fp64 by the expansion with mm: differentiable, the N x N matrices written out."""
    x, y = e1.double(), e2.double()
    n = x.shape[0]
    off = ~torch.eye(n, dtype=torch.bool, device=x.device)

    def uniform(z):
        sq = (z * z).sum(dim=1)
        d2 = (sq[:, None] + sq[None, :] - 2.0 * (z @ z.T)).clamp_min(0.0)
        return (torch.where(off, torch.exp(-t * d2), 0.0).sum() / (n * (n - 1))).log()

    d2 = ((x - y) ** 2).sum(dim=1)
    align = d2.mean() if alpha == 2 else d2.sqrt().mean()
    return align + lam / 2 * (uniform(x) + uniform(y))


def loss(iters, say):
    from multimodal_supernovae_amd.loss import align_uniform_loss
    slower = []
    for N, D in CASES:
        g = torch.Generator().manual_seed(N + D)
        a = torch.nn.functional.normalize(torch.randn(N, D, generator=g), dim=1)
        b = torch.nn.functional.normalize(0.8 * a + 0.6 * torch.nn.functional.normalize(torch.randn(N, D, generator=g), dim=1), dim=1)
        e1, e2 = a.cuda().requires_grad_(True), b.cuda().requires_grad_(True)

        def run(fn):
            e1.grad = e2.grad = None
            out = fn(e1, e2, ALPHA, T, LAM)
            out.backward()
            return out

        def hip():
            return run(align_uniform_loss)

        def aten64():
            return run(torch_loss)

        la = float(hip().detach())
        ga = e1.grad.clone()
        lb = float(aten64().detach())
        rel = float((ga - e1.grad).abs().max() / e1.grad.abs().max())
        res = _alternate({"hip": hip, "aten64": aten64}, iters)
        med = {n: sorted(v)[len(v) // 2] for n, v in res.items()}
        tiles = (-(-N // 64)) ** 2
        flops = 2 * 2 * 2.0 * 64 * 64 * D * tiles
        mark = "  ** slower than the yardstick **" if med["hip"] > med["aten64"] else ""
        if mark:
            slower.append((N, D))
        say(f"  loss fwd + bwd ({N}, {D})   align_uniform_loss {_fmt(res['hip'])}  {flops / med['hip'] / 1e6:6.2f} fp64 TFLOP/s of the two "
            f"fields over the whole call;  loss {la:.6f} against {lb:.6f}, largest gradient difference / largest gradient {rel:.1e}")
        say(f"  {'':29s} torch fp64 mm + exp + log + autograd    {_fmt(res['aten64'])};  hip / torch fp64 = "
            f"{med['hip'] / med['aten64']:.3f}{mark}")
    say(f"  cases slower than the yardstick: {slower if slower else 'none'}")


def field(iters, say):
    """The row field of one tower alone (two launches): what the loss's time is made of once the host keeps up."""
    from multimodal_supernovae_amd.embedding_metrics import pair_field
    for N, D in CASES:
        g = torch.Generator().manual_seed(N + D)
        X = torch.nn.functional.normalize(torch.randn(N, D, generator=g), dim=1).cuda()
        res = _alternate({"field": lambda: pair_field(X, None, T)}, 4 * iters)["field"]
        med = sorted(res)[len(res) // 2]
        say(f"  pair_field ({N}, {D}), one tower   {_fmt(res)}  {2 * 2.0 * 64 * 64 * D * (-(-N // 64)) ** 2 / med / 1e6:6.2f} fp64 TFLOP/s "
            f"over the two products of every tile")


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
        raise SystemExit("bench_align_uniform.py measures on the GPU; none is visible")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"tools/bench_align_uniform.py on {torch.cuda.get_device_name(0)}; median (min .. max) of {ROUNDS} alternated rounds, "
        f"{a.iters} calls per round, alpha = {ALPHA}, t = {T}, lam = {LAM}")
    if not a.skip_loss:
        loss(a.iters, say)
        field(a.iters, say)
    if a.parent_tree:
        # the children open the GPU themselves: this process holds it too, and is idle while they run
        step(a.parent_tree, a.step_rounds, a.steps, a.warmup, a.step_timeout, say)
    else:
        say("  headline step: not timed (no --parent-tree given)")
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
