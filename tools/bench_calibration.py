#!/usr/bin/env python3
"""The calibration metrics (csrc/calibration.hip, calibration.py) on one GPU, next to the torch forms a caller has without
them.  Median (min .. max) of 5 alternated rounds in one run; nothing here gates -- calibration is not on the training path.

    counts     softmax_rows + calibration_counts of (N, C) logits at (4096, 5), (65536, 5), (16384, 64), 15 bins, with and
               without classwise, by device events, beside a torch form on the device (softmax, max, bucketize, bincount /
               index_add; fp32 probabilities, fp64 sums) -- the yardstick, for information: its sums are floating point and
               depend on the order of the atomics
    objective  one temperature_nll evaluation (value, gradient and curvature in beta) beside torch fp64 cross_entropy of
               (beta x) + backward with respect to beta (value and gradient only)
    fit        a whole TemperatureScaling.fit, wall time, host copies included
    step       with --parent-tree DIR (a checkout of the parent commit with its library built): bench.py --gpus 1 of both trees
               as child processes, in alternated rounds; the headline step runs no code of this change

Run it as one `timeout`-wrapped process; --out appends the report to a file (profiles/calibration_bench.txt)."""
import argparse
import json
import os
import subprocess
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = [(4096, 5), (65536, 5), (16384, 64)]
BINS = 15
ROUNDS = 5


def _fmt(v, unit="us"):
    v = sorted(v)
    d = 3 if unit == "ms" else 1
    return f"{v[len(v) // 2]:10.{d}f} {unit} ({v[0]:.{d}f} .. {v[-1]:.{d}f})"


def _med(v):
    return sorted(v)[len(v) // 2]


def _alternate(fns, iters, wall):
    """{name: [us per call per round]}: ROUNDS rounds, the forms in turns inside every round.  wall: host clock around calls
    that end in a host copy; else device events."""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    res = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for name, fn in fns.items():
            if wall:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(iters):
                    fn()
                torch.cuda.synchronize()
                res[name].append((time.perf_counter() - t0) / iters * 1e6)
            else:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(iters):
                    fn()
                e1.record()
                e1.synchronize()
                res[name].append(e0.elapsed_time(e1) / iters * 1e3)
    return res


def _case(N, C):
    """An over-confident head: logits 2.5 z with labels drawn from softmax(z), z ~ 2 normal; a few targets -100."""
    g = torch.Generator().manual_seed(N + C)
    z = 2.0 * torch.randn(N, C, generator=g)
    y = torch.multinomial(torch.softmax(z, 1), 1, generator=g).squeeze(1)
    y[::97] = -100
    return (2.5 * z).cuda(), y.cuda()


def _torch_counts(x, y, classwise):
    """(count, hits, confidence sums per bin [, the same per class], Brier sum) on the device."""
    N, C = x.shape
    P = torch.softmax(x, 1)
    valid = (y >= 0) & (y < C)
    Pv, yv = P[valid], y[valid]
    edges = torch.linspace(0, 1, BINS + 1, device=x.device)[1:-1]
    conf, a = Pv.max(1)
    b = torch.bucketize(conf, edges, right=True)
    out = [torch.bincount(b, minlength=BINS), torch.bincount(b, (a == yv).double(), minlength=BINS),
           torch.zeros(BINS, dtype=torch.float64, device=x.device).index_add_(0, b, conf.double())]
    onehot = F.one_hot(yv, C)
    if classwise:
        cell = (torch.bucketize(Pv, edges, right=True) + BINS * torch.arange(C, device=x.device)[None, :]).reshape(-1)
        out += [torch.bincount(cell, minlength=C * BINS), torch.bincount(cell, onehot.reshape(-1).double(), minlength=C * BINS),
                torch.zeros(C * BINS, dtype=torch.float64, device=x.device).index_add_(0, cell, Pv.reshape(-1).double())]
    out.append(((Pv.double() - onehot) ** 2).sum())
    return out


def counts(iters, say):
    from multimodal_supernovae_amd import calibration as K
    slower = []
    for N, C in SHAPES:
        x, y = _case(N, C)
        for classwise in (False, True):
            res = _alternate({"hip": lambda: K.calibration_counts(K.softmax_rows(x), y, BINS, classwise),
                              "torch": lambda: _torch_counts(x, y, classwise)}, iters, wall=False)
            acc, tot = (t.cpu() for t in K.calibration_counts(K.softmax_rows(x), y, BINS, classwise))
            t = _torch_counts(x, y, classwise)
            ece_t = float((t[2] - t[1]).abs().sum() / t[0].sum())
            ratio = _med(res["hip"]) / _med(res["torch"])
            mark = "**" if ratio > 1 else ""
            say(f"  counts ({N}, {C}){' classwise' if classwise else ''}   softmax_rows + calibration_counts {_fmt(res['hip'])};  torch form "
                f"{_fmt(res['torch'])};  {mark}hip / torch = {ratio:.3f}{mark};  ece {K.ece_from_counts(acc):.6f} (torch form {ece_t:.6f}) "
                f"brier {K.brier_from_counts(tot):.6f} (torch form {float(t[-1] / t[0].sum()):.6f})")
            if ratio > 1:
                slower.append(f"counts ({N}, {C}){' classwise' if classwise else ''}: {ratio:.2f} x")
    return slower


def objective(iters, say):
    from multimodal_supernovae_amd import calibration as K
    slower = []
    for N, C in SHAPES:
        x, y = _case(N, C)

        def torch_form():
            beta = torch.tensor(0.4, dtype=torch.float64, device=x.device, requires_grad=True)
            loss = F.cross_entropy(x.double() * beta, y, ignore_index=-100, reduction="sum")
            loss.backward()
            return loss.detach(), beta.grad

        res = _alternate({"hip": lambda: K.temperature_nll(x, y, beta=0.4), "torch": torch_form}, iters, wall=False)
        got, want = K.temperature_nll(x, y, beta=0.4).cpu().tolist(), [float(v) for v in torch_form()]
        ratio = _med(res["hip"]) / _med(res["torch"])
        mark = "**" if ratio > 1 else ""
        say(f"  objective ({N}, {C})   temperature_nll (value, gradient, curvature) {_fmt(res['hip'])};  torch fp64 cross_entropy + backward "
            f"(value, gradient) {_fmt(res['torch'])};  {mark}hip / torch = {ratio:.3f}{mark};  relative difference value "
            f"{abs(got[1] - want[0]) / want[0]:.1e} gradient {abs(got[2] - want[1]) / abs(want[1]):.1e}")
        if ratio > 1:
            slower.append(f"objective ({N}, {C}): {ratio:.2f} x")
        fit = K.TemperatureScaling()
        wall = _alternate({"fit": lambda: fit.fit(x, y)}, max(1, iters // 4), wall=True)["fit"]
        say(f"  fit ({N}, {C})   TemperatureScaling.fit {_fmt(wall)} wall;  T = {fit.temperature_:.6f} in {fit.n_iter_} evaluations, "
            f"mean nll {fit.nll_before_:.6f} -> {fit.nll_after_:.6f}")
    return slower


def _bench_step(tree, steps, warmup):
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--no-alt", "--no-cpu-baseline",
           "--no-weak", "--no-three-tower"]
    env = {k: v for k, v in os.environ.items() if k != "MSN_HIP_LIB"}
    r = subprocess.run(cmd, cwd=tree, env=env, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(f"bench.py failed in {tree} (code {r.returncode}): {r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])["ms_per_step"]


def step(parent, rounds, steps, warmup, say):
    """bench.py of both trees, each run a fresh child process; the order is swapped every round."""
    ms = {"parent": [], "this change": []}
    trees = {"parent": parent, "this change": ROOT}
    for r in range(rounds):
        for name in (("parent", "this change") if r % 2 == 0 else ("this change", "parent")):
            ms[name].append(_bench_step(trees[name], steps, warmup))
    say(f"  headline step (bench.py --gpus 1 --steps {steps} --warmup {warmup}), {rounds} rounds, the order swapped every round, ms per step")
    for name, v in ms.items():
        say(f"    {name:12s} {_fmt(v, 'ms')}   rounds " + " ".join(f"{t:.3f}" for t in v))
    d = _med(ms["this change"]) - _med(ms["parent"])
    spread = max(ms["parent"]) - min(ms["parent"])
    inside = abs(d) <= spread
    mark = "" if inside or d < 0 else "**"
    say(f"    {mark}medians {d:+.3f} ms ({100 * d / _med(ms['parent']):+.2f} %) apart; the parent's own rounds span {spread:.3f} ms: "
        f"{'inside' if inside else 'OUTSIDE'} the spread{mark}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--step-rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_calibration.py needs the GPU: there is nothing to measure without it")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"tools/bench_calibration.py on {torch.cuda.get_device_name(0)}; median (min .. max) of {ROUNDS} alternated rounds, {a.iters} calls "
        f"per round; ** marks a case slower than its yardstick")
    slower = counts(a.iters, say) + objective(a.iters, say)
    say("  slower than its yardstick: " + ("; ".join(f"**{s}**" for s in slower) if slower else "no case"))
    if a.parent_tree:
        step(os.path.abspath(a.parent_tree), a.step_rounds, a.steps, a.warmup, say)
    else:
        say("  headline step against the parent commit: not measured (no --parent-tree)")
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
