#!/usr/bin/env python3
"""The threshold-free classification metrics (csrc/rank_metrics.hip, metrics.py) on one GPU, next to the routes a caller has
without them.  Median (min .. max) of 5 alternated rounds in one run; nothing here gates.

    exact      macro AUROC + average precision of (N, C) scores at (4096, 5), (16384, 5), (65536, 5), (16384, 64), wall time
               of the whole call (pair count, finishing launch, the one host copy, the host arithmetic), beside
                 scikit-learn on the host with the copy (roc_auc_score + average_precision_score per class) -- the yardstick
                 a sort-based torch implementation on the device with its copy (argsort per column, cumulative sums; it gives
                 tied scores no special treatment) -- for information
               and the pair count's two launches alone by device events, in pairs per second
    scan       hip against the sort at C = 5 up to N = 262144: where O(N^2) loses to O(N log N)
    launches   msn_threshold_counts (T = 100) and msn_topk_ranks at (65536, 5) by device events, beside torch forms

Run it as one `timeout`-wrapped process; --out appends the report to a file (profiles/rank_metrics_bench.txt)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
EXACT_SHAPES = [(4096, 5), (16384, 5), (65536, 5), (16384, 64)]
SCAN_N = [4096, 16384, 65536, 262144]
LAUNCH_SHAPE = (65536, 5, 100)
ROUNDS = 5


def _fmt(v, unit="us"):
    v = sorted(v)
    return f"{v[len(v) // 2]:10.1f} {unit} ({v[0]:.1f} .. {v[-1]:.1f})"


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
    """Imbalanced classes (the first holds most rows), logits that know something about the class."""
    g = torch.Generator().manual_seed(N + C)
    p = torch.tensor([0.6] + [0.4 / (C - 1)] * (C - 1))
    y = torch.multinomial(p, N, replacement=True, generator=g)
    S = torch.randn(N, C, generator=g)
    S[torch.arange(N), y] += 1.0
    return S.cuda(), y.cuda()


def _sort_based(S, y):
    """(macro AUROC, macro AP) by one argsort per column on the device; tied scores get no special treatment."""
    N, C = S.shape
    order = S.argsort(dim=0, descending=True)
    pos = (y[order] == torch.arange(C, device=S.device)[None, :]).double()
    P = pos.sum(0)
    place = torch.arange(1, N + 1, device=S.device, dtype=torch.float64)[:, None]
    ap = (pos.cumsum(0) / place * pos).sum(0) / P
    above = (place - pos.cumsum(0)) * pos                     # negatives placed before each positive
    au = 1.0 - above.sum(0) / (P * (N - P))
    return torch.stack([au.mean(), ap.mean()]).cpu()


def exact(iters, say):
    from multimodal_supernovae_amd import metrics as M
    try:
        from sklearn.metrics import average_precision_score, roc_auc_score
    except ImportError:
        roc_auc_score = None
    slower = []
    for N, C in EXACT_SHAPES:
        S, y = _case(N, C)

        def hip():
            _, istats, ap_sum = M.rank_counts(S, y)
            istats, ap_sum = istats.cpu(), ap_sum.cpu()
            return M.auroc_from_stats(istats), M.average_precision_from_stats(istats, ap_sum)

        def sk():
            Sh, yh = S.cpu().numpy(), y.cpu().numpy()
            return (float(np.mean([roc_auc_score(yh == c, Sh[:, c]) for c in range(C)])),
                    float(np.mean([average_precision_score(yh == c, Sh[:, c]) for c in range(C)])))

        fns = {"hip": hip, "sort": lambda: _sort_based(S, y)}
        if roc_auc_score is not None:
            fns["sklearn"] = sk
        res = _alternate(fns, iters, wall=True)
        launches = _alternate({"hip": lambda: M.rank_counts(S, y)}, iters, wall=False)["hip"]
        got, srt = hip(), _sort_based(S, y).tolist()
        say(f"  exact ({N}, {C})   metrics.rank_counts + copy + host {_fmt(res['hip'])};  the two launches alone {_fmt(launches)} = "
            f"{N * N / _med(launches) / 1e3:7.1f} G pairs/s;  auroc_macro {got[0]:.6f} ap_macro {got[1]:.6f}")
        if "sklearn" in res:
            want = sk()
            ratio = _med(res["hip"]) / _med(res["sklearn"])
            mark = "**" if ratio > 1 else ""
            say(f"  {'':20s} scikit-learn on the host with the copy {_fmt(res['sklearn'])};  {mark}hip / scikit-learn = {ratio:.3f}{mark};  "
                f"|difference| auroc {abs(got[0] - want[0]):.1e} ap {abs(got[1] - want[1]):.1e}")
            if ratio > 1:
                slower.append(f"({N}, {C}) against scikit-learn: {ratio:.2f} x")
        else:
            say(f"  {'':20s} scikit-learn is not installed here: not measured")
        ratio = _med(res["hip"]) / _med(res["sort"])
        mark = "**" if ratio > 1 else ""
        say(f"  {'':20s} torch argsort form on the device with its copy {_fmt(res['sort'])}  (for information);  {mark}hip / sort = "
            f"{ratio:.3f}{mark};  |difference| auroc {abs(got[0] - srt[0]):.1e} ap {abs(got[1] - srt[1]):.1e}")
        if ratio > 1:
            slower.append(f"({N}, {C}) against the torch argsort form: {ratio:.2f} x")
    return slower


def scan(iters, say):
    from multimodal_supernovae_amd import metrics as M
    rows = []
    for N in SCAN_N:
        S, y = _case(N, 5)

        def hip():
            _, istats, ap_sum = M.rank_counts(S, y)
            return istats.cpu(), ap_sum.cpu()

        res = _alternate({"hip": hip, "sort": lambda: _sort_based(S, y)}, iters if N <= 65536 else 1, wall=True)
        ratio = _med(res["hip"]) / _med(res["sort"])
        rows.append((N, ratio))
        mark = "**" if ratio > 1 else ""
        say(f"  scan ({N}, 5)   pair count + copy {_fmt(res['hip'])};  argsort form + copy {_fmt(res['sort'])};  {mark}hip / sort = {ratio:.3f}{mark}")
    below = [n for n, r in rows if r <= 1]
    above = [n for n, r in rows if r > 1]
    if below and above:
        say(f"  crossover at C = 5: the pair count is ahead up to N = {max(below)} and behind from N = {min(above)} on")
    elif above:
        say(f"  crossover at C = 5: below N = {min(above)}: the pair count is behind at every size measured")
    else:
        say(f"  crossover at C = 5: above N = {max(below)}: the pair count is ahead at every size measured")


def launches(iters, say):
    from multimodal_supernovae_amd import metrics as M
    N, C, T = LAUNCH_SHAPE
    S, y = _case(N, C)
    P = torch.softmax(S, dim=1).contiguous()
    thr = torch.linspace(0, 1, T, device="cuda")
    acc = torch.zeros((C, T, 2), dtype=torch.int64, device="cuda")
    tot = torch.zeros((C, 2), dtype=torch.int64, device="cuda")
    hist = torch.zeros(C, dtype=torch.int64, device="cuda")
    onehot = torch.nn.functional.one_hot(y, C).bool()

    def aten_binned():
        ge = P.t()[:, :, None] >= thr[None, None, :]                       # (C, N, T)
        pos = onehot.t()[:, :, None]
        return torch.stack([(ge & pos).sum(1), (ge & ~pos).sum(1)], dim=2)

    def aten_topk():
        s = S.gather(1, y[:, None])
        lower = torch.arange(C, device="cuda")[None, :] < y[:, None]
        return torch.bincount(((S > s) | ((S == s) & lower)).sum(1), minlength=C)

    res = _alternate({"binned": lambda: M.threshold_counts(P, y, thr, acc=acc, tot=tot), "aten_binned": aten_binned,
                      "topk": lambda: M.topk_ranks(S, y, hist=hist, return_ranks=False), "aten_topk": aten_topk}, iters, wall=False)
    for name, other, label in (("binned", "aten_binned", f"msn_threshold_counts ({N}, {C}, T = {T})"), ("topk", "aten_topk", f"msn_topk_ranks ({N}, {C})")):
        ratio = _med(res[name]) / _med(res[other])
        mark = "**" if ratio > 1 else ""
        say(f"  launch {label} {_fmt(res[name])};  torch form (compare, mask, sum) {_fmt(res[other])};  {mark}hip / torch = {ratio:.3f}{mark}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rank_metrics.py measures on the GPU; none is visible")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"tools/bench_rank_metrics.py on {torch.cuda.get_device_name(0)}; median (min .. max) of {ROUNDS} alternated rounds, "
        f"{a.iters} calls per round; ** marks a case slower than its yardstick")
    slower = exact(a.iters, say)
    scan(a.iters, say)
    launches(a.iters, say)
    say("  slower than its yardstick: " + ("; ".join(slower) if slower else "no exact case"))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
