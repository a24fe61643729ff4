#!/usr/bin/env python3
"""Two ranks sharing ONE GPU (gloo transport, CUDA tensors): metrics.RankingMetrics under data parallel vs the single process
on all rows.  The shards have unequal sizes (rank 0: 37 rows, rank 1: 22) and rank 1's last batch is empty.  Exact mode: every
rank gathers all rows (a shard padded to the largest with rows of target -100) and counts the pairs itself; binned mode: the
int64 accumulators are SUM-all-reduced.  istats, the accumulators, the top-k histogram and every reported metric of both ranks
must equal the single-process result bit for bit (counts are integers; the exact mode's ap_sum is compared through the
reported average precision, which the padding rows leave within the summation bound).  A third case has rank 1 see no row at
all.  (tools/dist_check_supervised.py is the same kind of check for the supervised step.)"""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
C, T = 5, 11
SHARDS = [[(0, 20), (20, 37)], [(37, 59), (59, 59)]]           # row ranges of the batches per rank; the last one is empty
N = 59
CASES = ["exact", "binned", "exact_empty_rank"]


def make_rows():
    g = torch.Generator().manual_seed(7)
    grid = torch.linspace(0, 1, T)
    S = grid[torch.randint(0, T, (N, C), generator=g)]          # on the thresholds, ties everywhere
    y = torch.randint(0, C, (N,), generator=g)
    y[y == 3] = 4                                               # class 3 has no positive
    y[::8] = -100
    return S, y


def run(metric, S, y, batches):
    for a, b in batches:
        metric.update(S[a:b].cuda(), y[a:b].cuda())


def state(metric, res):
    """Everything a rank reports, as plain Python numbers (integers and floats compare exactly)."""
    out = {k: v.tolist() if isinstance(v, np.ndarray) else v for k, v in res.items()}
    out["hist"] = metric.hist.tolist()
    if metric.binned:
        out["acc"], out["tot"] = metric.acc.tolist(), metric.tot.tolist()
    else:
        out["istats"] = metric.istats.tolist()
    return out


def make_metric(case):
    from multimodal_supernovae_amd.metrics import RankingMetrics
    return RankingMetrics(C, thresholds=T if case == "binned" else None, top_k=(1, 2))


def worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    from multimodal_supernovae_amd import distributed as D
    D.init_from_env(backend="gloo")
    S, y = make_rows()
    for case in CASES:
        m = make_metric(case)
        if case == "exact_empty_rank":
            run(m, S, y, [(0, N)] if rank == 0 else [])
        else:
            run(m, S, y, SHARDS[rank])
        m.all_reduce()
        out[f"{case}_r{rank}"] = state(m, m.compute())
    dist.barrier()
    dist.destroy_process_group()
    if rank == 0:                                               # single process on all rows
        for case in CASES:
            m = make_metric(case)
            run(m, S, y, [(0, 31), (31, N)])
            out[f"{case}_single"] = state(m, m.compute())


def same(a, b, slack=False):
    """Equal, nan == nan; slack: floats within the bound of a sum of at most N terms in another order."""
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(x, y, slack) for x, y in zip(a, b))
    if isinstance(a, dict):
        # the exact mode's one fp64 sum (ap_sum) meets the gathered rows at other positions than the single process does
        return set(a) == set(b) and all(same(a[k], b[k], slack and k.startswith("ap_")) for k in a)
    if isinstance(a, float):
        return a == b or (a != a and b != b) or (slack and abs(a - b) <= N * 2.0 ** -52 * abs(b))
    return a == b


if __name__ == "__main__":
    ctx = mp.get_context("spawn")
    out = ctx.Manager().dict()
    procs = [ctx.Process(target=worker, args=(r, 2, 29637, out)) for r in range(2)]
    [p.start() for p in procs]
    [p.join(300) for p in procs]
    [p.terminate() for p in procs if p.is_alive()]
    res = dict(out)
    ok = all(p.exitcode == 0 for p in procs)
    print([p.exitcode for p in procs], sorted(res))
    for case in CASES:
        if not ok or any(f"{case}_{w}" not in res for w in ("r0", "r1", "single")):
            ok = False
            break
        single = res[f"{case}_single"]
        print(case, {k: v for k, v in single.items() if isinstance(v, float)})
        ok = ok and same(res[f"{case}_r0"], res[f"{case}_r1"])                   # the ranks agree to the bit
        for r in range(2):
            good = same(res[f"{case}_r{r}"], single, slack=case != "binned")
            print(f"  rank {r}: {'equal' if good else 'DIFFERENT'}")
            ok = ok and good
        ok = ok and single["auroc_macro"] == single["auroc_macro"]              # the case is a check only if the metric is defined
    print("DIST CHECK", "OK" if ok else "FAILED")
    sys.exit(0 if ok else 1)
