#!/usr/bin/env python3
"""The focal loss with label smoothing (models_finetune.focal_loss on csrc/focal_loss.hip) on one GPU, forward + backward
through Python, next to this package's cross_entropy and to a torch fp32 form of the same formula on the same tensors in the
same process; the kernels' own times from a kernel trace; and the headline training step of bench.py, which runs no code of
the loss, in this tree and in a checkout of the parent commit in turns.  Median (min .. max) of 5 alternated rounds; nothing
here gates.

    loss     forward + backward at (N, C) = (256, 5), (4096, 5), (4096, 1000), us per call: focal_loss at gamma = 2 with
             label_smoothing 0.1 (a pow for every column) and 0 (one pow per row), cross_entropy(label_smoothing=0.1) (the
             same kernel at gamma = 0: no pow), cross_entropy (csrc/supervised.hip), and the formula in torch fp32:
             log_softmax, exp, pow, one_hot, the sums, and autograd's backward through all of it.  A shape at which
             focal_loss is slower than the torch form is marked.
    kernels  `--kernels N`: N calls of every form per shape and nothing else, to be run under
             `rocprofv3 --kernel-trace -d DIR --output-format csv -- python tools/bench_focal_loss.py --kernels N`;
             `--trace DIR` then reads that one trace: median kernel time per kernel, workgroup and grid size (the three shapes take
             different grids, so the rows tell them apart)
    step     `python bench.py --gpus 1 --steps K --warmup W` as fresh processes, this tree and --parent-tree in turns, the order
             swapped every round: ms per step of each and the ratio.  Expected: unchanged within the parent's own spread.

Run each mode as one `timeout`-wrapped process; --out appends the report to a file (profiles/focal_loss_bench.txt)."""
import argparse
import collections
import csv
import glob
import json
import os
import subprocess
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CASES = [(256, 5), (4096, 5), (4096, 1000)]
ROUNDS = 5
GAMMA, EPS = 2.0, 0.1


def _fmt(v, unit="us", digits=1):
    v = sorted(v)
    return f"{v[len(v) // 2]:10.{digits}f} {unit} ({v[0]:.{digits}f} .. {v[-1]:.{digits}f})"


def _median(v):
    return sorted(v)[len(v) // 2]


def torch_form(x, y, w, gamma, eps):
    """The formula in torch on the device, fp32 throughout."""
    C = x.shape[1]
    lp = F.log_softmax(x, dim=1)
    q = F.one_hot(y, C).to(x.dtype) * (1.0 - eps) + eps / C
    return (q * w * (1.0 - lp.exp()).pow(gamma) * (-lp)).sum() / w[y].sum()


def _forms(x, y, w):
    from multimodal_supernovae_amd.models_finetune import cross_entropy, focal_loss
    from multimodal_supernovae_amd.trainer import _backward_seed

    def run(fn):
        def one():
            x.grad = None
            l = fn()
            l.backward(_backward_seed(l))
            return l
        return one

    return {
        f"focal_loss gamma {GAMMA:g} smoothing {EPS:g}": run(lambda: focal_loss(x, y, w, GAMMA, EPS)),
        f"focal_loss gamma {GAMMA:g} smoothing 0": run(lambda: focal_loss(x, y, w, GAMMA, 0.0)),
        f"cross_entropy smoothing {EPS:g}": run(lambda: cross_entropy(x, y, w, label_smoothing=EPS)),
        "cross_entropy": run(lambda: cross_entropy(x, y, w)),
        f"torch fp32 form gamma {GAMMA:g} smoothing {EPS:g}": run(lambda: torch_form(x, y, w, GAMMA, EPS)),
    }


def _inputs(N, C):
    g = torch.Generator().manual_seed(N + C)
    x = torch.randn(N, C, generator=g).cuda().requires_grad_()
    y = torch.randint(0, C, (N,), generator=g).cuda()
    w = (torch.rand(C, generator=g) + 0.25).cuda()
    return x, y, w


def loss(iters, say):
    slower = []
    for N, C in CASES:
        forms = _forms(*_inputs(N, C))
        for fn in forms.values():
            for _ in range(20):
                fn()
        torch.cuda.synchronize()
        names = list(forms)
        agree = abs(float(forms[names[0]]().detach()) - float(forms[names[-1]]().detach()))
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
        med = {k: _median(v) for k, v in res.items()}
        say(f"  forward + backward ({N}, {C}), {iters} calls per round; focal_loss and the torch form differ by {agree:.1e}")
        for name in names:
            mark = ""
            if name.startswith("focal_loss") and med[name] > med[names[-1]]:
                mark = "  ** slower than the torch form **"
                slower.append((N, C, name))
            say(f"    {name:44s} {_fmt(res[name])}   / cross_entropy = {med[name] / med['cross_entropy']:.3f}   / torch form = "
                f"{med[name] / med[names[-1]]:.3f}{mark}")
    say(f"  focal_loss slower than the torch form: {slower if slower else 'nowhere'}")


def kernels(n):
    for N, C in CASES:
        forms = _forms(*_inputs(N, C))
        for fn in forms.values():
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
        if "focal_" in name or "ce_fwd" in name or "ce_bwd" in name:
            rows[(name, int(r["Workgroup_Size_X"]), int(r["Grid_Size_X"]))].append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    say(f"  kernel times from one kernel trace ({os.path.basename(files[0])}): median (min .. max) over the calls, by kernel, workgroup and grid "
        f"size in threads; the calls of a row mix the forms that share its kernel (gamma, smoothing)")
    for (name, wg, grid), v in sorted(rows.items()):
        say(f"    {name:44s} workgroup {wg:5d} grid {grid:8d} {len(v):6d} calls {_fmt([d / 1e3 for d in v], 'us', 2)}")


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
    med = {k: _median(v) for k, v in res.items()}
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
            raise SystemExit("bench_focal_loss.py measures on the GPU; none is visible")
        if a.kernels:
            kernels(a.kernels)
        else:
            say(f"tools/bench_focal_loss.py on {torch.cuda.get_device_name(0)}; median (min .. max) of {ROUNDS} alternated rounds")
            if not a.skip_loss:
                loss(a.iters, say)
            if a.parent_tree:
                # the children open the GPU themselves: this process holds it too, and is idle while they run
                step(a.parent_tree, a.step_rounds, a.steps, a.warmup, a.step_timeout, say)
            else:
                say("  headline step: not timed (no --parent-tree given)")
    if a.out and lines:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
