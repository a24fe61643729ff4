#!/usr/bin/env python3
"""The label-aware contrastive loss (loss.supcon_loss on csrc/supcon.hip) on one GPU next to its two yardsticks on the same
tensors in the same process; and the headline training step of bench.py, which runs no code of the loss, in this tree and in a
checkout of the parent commit in turns.  Median (min .. max) of 5 alternated rounds; nothing here gates.

    loss     forward + backward through Python at (N, D) = (1024, 128), (4096, 128), (1024, 256), five classes drawn uniformly:
             supcon_loss, clip_loss (the InfoNCE kernels: per score the new kernels add a compare, a select and an add; also
             through clip_loss_multimodal, the autograd node supcon_loss is built like), and a plain
             torch fp32 autograd form of the same formula that writes the N x N matrix.  A slowdown over clip_loss beyond the
             run's own spread, and a case slower than the torch form, are marked.
    kernels  msn_supcon_fwd + msn_supcon_bwd alone (loss.HipSupConKernels, no autograd node) beside msn_infonce_fwd + _bwd
    step     `python bench.py --gpus 1 --steps K --warmup W` as fresh processes, this tree and --parent-tree in turns, the order
             swapped every round: ms per step of each and the ratio.  Expected: unchanged within the parent's own spread.

Run it as one `timeout`-wrapped process; --out appends the report to a file (profiles/supcon_bench.txt)."""
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
LOG_SCALE, BIAS = 2.5, -1.0


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


def torch_loss(e1, e2, mask_w, ls, lb):
    """The same formula in fp32 from log_softmax and the (N, N) weights P / c: differentiable, the N x N matrices written out."""
    S = torch.exp(ls) * (e2 @ e1.T) + lb
    rows = -(mask_w * torch.log_softmax(S, dim=1)).sum()
    cols = -(mask_w * torch.log_softmax(S.T, dim=1)).sum()
    return (rows + cols) / (2 * e1.shape[0])


def loss(iters, say):
    from multimodal_supernovae_amd.loss import HipPairKernels, HipSupConKernels, clip_loss, clip_loss_multimodal, supcon_loss
    findings = []
    for N, D in CASES:
        g = torch.Generator().manual_seed(N + D)
        a = torch.nn.functional.normalize(torch.randn(N, D, generator=g), dim=1)
        b = torch.nn.functional.normalize(0.8 * a + 0.6 * torch.nn.functional.normalize(torch.randn(N, D, generator=g), dim=1), dim=1)
        y = torch.randint(0, 5, (N,), generator=g).cuda()
        e1, e2 = a.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
        ls = torch.tensor(LOG_SCALE, device="cuda", requires_grad=True)
        lb = torch.tensor(BIAS, device="cuda", requires_grad=True)
        P = (y[:, None] == y[None, :])
        mask_w = P.float() / P.sum(1, keepdim=True)

        def run(fn):
            e1.grad = e2.grad = ls.grad = lb.grad = None
            out = fn()
            out.backward()
            return out

        forms = {"supcon": lambda: run(lambda: supcon_loss(e1, e2, y, ls, lb)),
                 "clip": lambda: run(lambda: clip_loss(e1, e2, ls, lb)),
                 "clip_mm": lambda: run(lambda: clip_loss_multimodal([e1, e2], ls, lb)),
                 "aten32": lambda: run(lambda: torch_loss(e1, e2, mask_w, ls, lb))}
        la = float(forms["supcon"]().detach())
        ga = e1.grad.clone()
        lt = float(forms["aten32"]().detach())
        rel = float((ga - e1.grad).abs().max() / e1.grad.abs().max())
        res = _alternate(forms, iters)
        med = {n: sorted(v)[len(v) // 2] for n, v in res.items()}
        say(f"  loss fwd + bwd ({N}, {D}), five classes   supcon_loss {_fmt(res['supcon'])};  loss {la:.6f} against torch fp32 {lt:.6f}, "
            f"largest gradient difference / largest gradient {rel:.1e}")
        spread = max(res["clip"]) - min(res["clip"])
        over = med["supcon"] - med["clip"]
        mark = f"  **{over / med['clip'] * 100:+.1f} % over clip_loss, beyond the run's spread of {spread:.1f} us**" if over > spread else ""
        say(f"  {'':39s} clip_loss   {_fmt(res['clip'])};  supcon / clip = {med['supcon'] / med['clip']:.3f}{mark}")
        say(f"  {'':39s} clip_loss_multimodal (the node supcon_loss is built like) {_fmt(res['clip_mm'])};  supcon / it = "
            f"{med['supcon'] / med['clip_mm']:.3f}")
        slow = "  **slower than the torch form**" if med["supcon"] > med["aten32"] else ""
        say(f"  {'':39s} torch fp32 N x N + autograd {_fmt(res['aten32'])};  supcon / torch = {med['supcon'] / med['aten32']:.3f}{slow}")
        if mark:
            findings.append(f"({N}, {D}) over clip_loss")
        if slow:
            findings.append(f"({N}, {D}) slower than torch")
        # the kernels alone
        with torch.no_grad():
            d1, d2, sc, bi = e1.detach(), e2.detach(), ls.detach(), lb.detach()
            y32 = y.to(torch.int32)
            one = torch.ones((), device="cuda")

            def sup():
                lr, lc, cnt, _ = HipSupConKernels.forward(d1, d2, d1, d2, y32, 0, sc, bi)
                return HipSupConKernels.backward(d1, d2, d1, d2, y32, 0, sc, bi, lr, lc, cnt, one)

            def nce():
                lr, lc, _ = HipPairKernels.forward(d1, d2, d1, d2, 0, sc, bi)
                return HipPairKernels.backward(d1, d2, d1, d2, 0, sc, bi, lr, lc, one)

            kres = _alternate({"supcon": sup, "infonce": nce}, 4 * iters)
        km = {n: sorted(v)[len(v) // 2] for n, v in kres.items()}
        kspread = max(kres["infonce"]) - min(kres["infonce"])
        kover = km["supcon"] - km["infonce"]
        kmark = f"  **{kover / km['infonce'] * 100:+.1f} % over the InfoNCE kernels, beyond the run's spread of {kspread:.1f} us**" if kover > kspread else ""
        say(f"  kernels alone, fwd + bwd ({N}, {D})       msn_supcon_*  {_fmt(kres['supcon'])}")
        say(f"  {'':39s} msn_infonce_* {_fmt(kres['infonce'])};  supcon / infonce = {km['supcon'] / km['infonce']:.3f}{kmark}")
    say(f"  findings: {findings if findings else 'none'}")


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
            print(f"    round {r + 1} {name}: {res[name][-1]:.3f} ms per step", flush=True)
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
        raise SystemExit("bench_supcon.py measures on the GPU; none is visible")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"tools/bench_supcon.py on {torch.cuda.get_device_name(0)}; median (min .. max) of {ROUNDS} alternated rounds, "
        f"{a.iters} calls per round, logit_scale = {LOG_SCALE}, logit_bias = {BIAS}")
    if not a.skip_loss:
        loss(a.iters, say)
    if a.parent_tree:
        # the children open the GPU themselves: this process holds it too, and is idle while they run
        step(a.parent_tree, a.step_rounds, a.steps, a.warmup, a.step_timeout, say)
    else:
        say("  headline step: not timed (no --parent-tree given)")
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
