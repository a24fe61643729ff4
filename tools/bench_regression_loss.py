#!/usr/bin/env python3
"""The regression losses (models_finetune.regression_loss on csrc/regression_loss.hip) on one GPU next to a torch fp32 form of
the same formula on the same tensors in the same process: forward + backward through Python and as a replayed graph; the
single-workgroup threshold from either side; the kernels' own times from a kernel trace; and the headline training step of
bench.py, which runs no code of these losses, in this tree and in a checkout of the parent commit in turns.  Median
(min .. max) of 5 alternated rounds; nothing here gates.

    loss       forward + backward at (N, K) = (256, 1), (4096, 1), (4096, 3), (65536, 3), us per call, for huber (K = 1),
               gaussian_nll (K = 2 in place of 3) and quantile, each through Python and as a replayed graph, beside the torch
               form (F.huber_loss / the Gaussian-NLL and pinball formulas) on the rows with a finite target.  A shape at
               which regression_loss is slower than the torch form is marked.
    threshold  replayed graphs of forward + backward at N = 128, 256 (one workgroup, one launch each way), 257, 512 and 1024
               (256-thread workgroups + the finishing block), for mse (no transcendental) and log_cosh (fp64 sinh / log1p /
               tanh): what the threshold of 256 rows separates
    kernels    `--kernels N`: N calls of every form per shape and nothing else, to be run under
               `rocprofv3 --kernel-trace -d DIR --output-format csv -- python tools/bench_regression_loss.py --kernels N`;
               `--trace DIR` then reads that one trace: median kernel time per kernel, workgroup and grid size
    step       bench_focal_loss.py's: `python bench.py --gpus 1 --steps K --warmup W` as fresh processes, this tree and
               --parent-tree in turns, the order swapped every round.  Expected: unchanged within the parent's own spread.

Run each mode as one `timeout`-wrapped process; --out appends the report to a file (profiles/regression_loss_bench.txt)."""
import argparse
import collections
import csv
import glob
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_focal_loss import _fmt, _median, step  # noqa: E402

CASES = [(256, 1), (4096, 1), (4096, 3), (65536, 3)]
THRESHOLD_SIZES = [128, 256, 257, 512, 1024]
ROUNDS = 5
DELTA = 0.05
LEVELS = (0.16, 0.5, 0.84)
TAU = None                      # the levels on the device, for the torch form


def torch_form(p, y, kind):
    """The formula in torch on the device, fp32 throughout, over the rows with a finite target: the rows are selected by a
    mask, not by a boolean index (whose size is read on the host), so that a graph records this form too."""
    v = torch.isfinite(y)
    y = torch.where(v, y, torch.zeros_like(y))
    if kind == "mse":
        rows = F.mse_loss(p[:, 0], y, reduction="none")
    elif kind == "huber":
        rows = F.huber_loss(p[:, 0], y, delta=DELTA, reduction="none")
    elif kind == "log_cosh":
        d = p[:, 0] - y
        rows = torch.logaddexp(d, -d) - 0.6931471805599453
    elif kind == "gaussian_nll":
        d = p[:, 0] - y                 # (F.gaussian_nll_loss reads `any(var < 0)` on the host: no graph records it)
        rows = 0.5 * (p[:, 1] + d * d * torch.exp(-p[:, 1]))
    else:
        e = y[:, None] - p
        rows = torch.maximum(TAU[:, :p.shape[1]] * e, (TAU[:, :p.shape[1]] - 1.0) * e).mean(dim=1)
    return (rows * v).sum() / v.sum()


def _inputs(N, K, kind):
    g = torch.Generator().manual_seed(N + K)
    y = torch.rand(N, generator=g) * 1.2
    p = y[:, None] + 0.1 * torch.randn(N, K, generator=g)
    if kind == "gaussian_nll":
        p[:, 1] = torch.randn(N, generator=g)
    y[4::5] = float("nan")
    return p.cuda().requires_grad_(), y.cuda()


def _width(kind, K):
    return 2 if kind == "gaussian_nll" else K if kind == "quantile" else 1


def _pair(N, K, kind):
    """{name: callable} for one shape and loss: regression_loss and the torch form, forward + backward."""
    from multimodal_supernovae_amd.models_finetune import regression_loss
    from multimodal_supernovae_amd.trainer import _backward_seed
    global TAU
    if TAU is None:
        TAU = torch.tensor(LEVELS, device="cuda")[None, :]
    p, y = _inputs(N, _width(kind, K), kind)
    name ="pinball" if kind == "quantile" else kind
    kw = dict(quantiles=LEVELS[:p.shape[1]]) if kind == "quantile" else dict(delta=DELTA)

    def run(fn):
        def one():
            p.grad = None
            l = fn()
            l.backward(_backward_seed(l))
            return l
        return one

    return {f"regression_loss {kind}": run(lambda: regression_loss(p, y, name, **kw)), f"torch fp32 form {kind}": run(lambda: torch_form(p, y, kind))}


def _graphed(fn):
    """fn recorded once and replayed: the launches without Python."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return graph.replay


def _time(forms, iters):
    for fn in forms.values():
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    res = {k: [] for k in forms}
    for _ in range(ROUNDS):
        for name, fn in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            e1.synchronize()
            res[name].append(e0.elapsed_time(e1) / iters * 1e3)
    return res


def loss(iters, say):
    slower = []
    for N, K in CASES:
        say(f"  forward + backward at N = {N}, K = {K} (gaussian_nll: 2 columns; huber: 1), {iters} calls per round")
        for kind in ("huber", "gaussian_nll", "quantile"):
            forms = _pair(N, K, kind)
            ours, theirs = list(forms)
            agree = abs(float(forms[ours]().detach()) - float(forms[theirs]().detach()))
            both = dict(forms)
            both.update({f"{name}, replayed graph": _graphed(fn) for name, fn in forms.items()})
            res = _time(both, iters)
            med = {k: _median(v) for k, v in res.items()}
            for name in both:
                graph = name.endswith("graph")
                base = med[theirs + ", replayed graph" if graph else theirs]
                mark = ""
                if name.startswith("regression_loss") and med[name] > base:
                    mark = "  ** slower than the torch form **"
                    slower.append((N, K, kind, "graph" if graph else "python"))
                say(f"    {name:48s} {_fmt(res[name])}   / torch form = {med[name] / base:.3f}{mark}")
            say(f"    ({kind}: regression_loss and the torch form differ by {agree:.1e})")
    say(f"  regression_loss slower than the torch form: {slower if slower else 'nowhere'}")


def threshold(iters, say):
    say(f"  the single-workgroup threshold (256 rows): replayed graphs of forward + backward, {iters} replays per round")
    for kind in ("mse", "log_cosh"):
        forms = {f"{kind} N = {N}": _graphed(_pair(N, 1, kind)[f"regression_loss {kind}"]) for N in THRESHOLD_SIZES}
        res = _time(forms, iters)
        for name in forms:
            say(f"    {name:48s} {_fmt(res[name])}")


def kernels(n):
    for N, K in CASES:
        for kind in ("huber", "gaussian_nll", "quantile"):
            for fn in _pair(N, K, kind).values():
                for _ in range(n):
                    fn()
    torch.cuda.synchronize()
    print(json.dumps({"calls_per_form_and_shape": n, "shapes": CASES}))


def trace(path, say):
    files = glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {path}")
    rows = collections.defaultdict(list)
    for r in csv.DictReader(open(files[0])):
        name = r["Kernel_Name"].split("(")[0].replace("void ", "")
        if "reg_loss" in name or "reg_interval" in name:
            rows[(name, int(r["Workgroup_Size_X"]), int(r["Grid_Size_X"]))].append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    say(f"  kernel times from one kernel trace ({os.path.basename(files[0])}): median (min .. max) over the calls, by kernel, workgroup and grid "
        f"size in threads")
    for (name, wg, grid), v in sorted(rows.items()):
        say(f"    {name:60s} workgroup {wg:5d} grid {grid:8d} {len(v):6d} calls {_fmt([d / 1e3 for d in v], 'us', 2)}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--kernels", type=int, default=0, help="only run every form this many times per shape (for a kernel trace)")
    ap.add_argument("--trace", default=None, help="only summarise the kernel trace under this directory")
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit; without it the step is not timed")
    ap.add_argument("--step-rounds", type=int, default=ROUNDS)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step-timeout", type=float, default=180.0, help="seconds allowed to one bench.py process")
    ap.add_argument("--skip-loss", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    if a.trace:
        trace(a.trace, say)
    else:
        if not torch.cuda.is_available():
            raise SystemExit("bench_regression_loss.py measures on the GPU; none is visible")
        if a.kernels:
            kernels(a.kernels)
        else:
            say(f"tools/bench_regression_loss.py on {torch.cuda.get_device_name(0)}; median (min .. max) of {ROUNDS} alternated rounds")
            if not a.skip_loss:
                loss(a.iters, say)
                threshold(a.iters, say)
            if a.parent_tree:
                # the children open the GPU themselves: this process holds it too, and is idle while they run
                step(a.parent_tree, a.step_rounds, a.steps, a.warmup, a.step_timeout, say)
            else:
                say("  headline step: not timed (no --parent-tree given)")
    if a.out and lines:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
