#!/usr/bin/env python3
"""Two ranks sharing ONE GPU (gloo transport, CUDA tensors), a fresh child process per rank: calibration.CalibrationMetrics and
calibration.TemperatureScaling under data parallel vs the single process on all rows.  The shards have unequal sizes (rank 0:
1500 rows, rank 1: 2596) and rank 1's last batch is empty; a second metrics case has rank 1 see no row at all.
  * acc / tot after all_reduce are integers: on both ranks they must equal the single-process accumulators exactly, and so must
    every reported number.
  * TemperatureScaling.fit(group=...) SUM-all-reduces the five doubles of every evaluation, so both ranks take identical steps:
    temperature_ and n_iter_ must be identical on the two ranks, and beta within 2 tol n / h of the one-process fit (both stop at
    |g| / n <= tol; h is the curvature at the single-process beta).
(tools/dist_check_rank_metrics.py is the same kind of check for the ranking metrics.)"""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N, C = 4096, 5
SHARDS = [[(0, 900), (900, 1500)], [(1500, 4096), (4096, 4096)]]       # row ranges of the batches per rank; the last one is empty
CASES = ["metrics", "metrics_empty_rank"]


def make_rows():
    """Over-confident logits 2.5 z with labels drawn from softmax(z), some targets -100, one row with a NaN."""
    rng = np.random.default_rng(20240)
    z = 2.0 * rng.standard_normal((N, C))
    p = np.exp(z - z.max(axis=1, keepdims=True))
    p /= p.sum(axis=1, keepdims=True)
    y = (rng.random(N)[:, None] > np.cumsum(p, axis=1)).sum(axis=1).clip(0, C - 1)
    y[::50] = -100
    x = (2.5 * z).astype(np.float32)
    x[7, 2] = np.nan
    return torch.from_numpy(x), torch.from_numpy(y.astype(np.int64))


def make_metric():
    from multimodal_supernovae_amd.calibration import CalibrationMetrics
    return CalibrationMetrics(C, classwise=True, normalize="softmax")


def run(metric, S, y, batches):
    for a, b in batches:
        metric.update(S[a:b].cuda(), y[a:b].cuda())


def state(metric):
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)           # the NaN row is a bad row on purpose
        res = metric.compute()
    out = {k: v.tolist() if isinstance(v, np.ndarray) else v for k, v in res.items()}
    out["acc"], out["tot"] = metric.acc.tolist(), metric.tot.tolist()
    return out


def fit_state(ts):
    return {"temperature": ts.temperature_, "beta": ts.beta_, "n_iter": ts.n_iter_, "nll_before": ts.nll_before_,
            "nll_after": ts.nll_after_, "n": ts.n_, "n_bad": ts.n_bad_, "converged": ts.converged_, "tol": ts.tol}


def worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    from multimodal_supernovae_amd import distributed as D
    from multimodal_supernovae_amd.calibration import TemperatureScaling, temperature_nll
    D.init_from_env(backend="gloo")
    S, y = make_rows()
    for case in CASES:
        m = make_metric()
        if case == "metrics_empty_rank":
            run(m, S, y, [(0, N)] if rank == 0 else [])
        else:
            run(m, S, y, SHARDS[rank])
        m.all_reduce()
        out[f"{case}_r{rank}"] = state(m)
    a, b = SHARDS[rank][0][0], SHARDS[rank][-1][1]
    out[f"fit_r{rank}"] = fit_state(TemperatureScaling().fit(S[a:b].cuda(), y[a:b].cuda(), group=None))
    dist.barrier()
    dist.destroy_process_group()
    if rank == 0:                                               # single process on all rows
        for case in CASES:
            m = make_metric()
            run(m, S, y, [(0, 2000), (2000, N)])
            out[f"{case}_single"] = state(m)
        ts = TemperatureScaling().fit(S.cuda(), y.cuda())
        out["fit_single"] = dict(fit_state(ts), h=float(temperature_nll(S.cuda(), y.cuda(), beta=ts.beta_)[3]))


def same(a, b):
    """Equal, nan == nan."""
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, dict):
        return set(a) == set(b) and all(same(a[k], b[k]) for k in a)
    if isinstance(a, float):
        return a == b or (a != a and b != b)
    return a == b


if __name__ == "__main__":
    ctx = mp.get_context("spawn")
    out = ctx.Manager().dict()
    procs = [ctx.Process(target=worker, args=(r, 2, 29641, out)) for r in range(2)]
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
        print(case, {k: v for k, v in single.items() if isinstance(v, (float, int))})
        for r in range(2):
            good = same(res[f"{case}_r{r}"], single)
            print(f"  rank {r}: {'equal' if good else 'DIFFERENT'}")
            ok = ok and good
        ok = ok and single["ece"] == single["ece"] and single["n_bad"] == 1      # the case is a check only if the metric is defined
    if ok and all(f"fit_{w}" in res for w in ("r0", "r1", "single")):
        r0, r1, single = res["fit_r0"], res["fit_r1"], res["fit_single"]
        bound = 2 * single["tol"] * single["n"] / single["h"]
        print("fit", {k: single[k] for k in ("temperature", "n_iter", "n", "n_bad")}, "ranks", r0["temperature"], r1["temperature"],
              f"|beta - beta_single| = {abs(r0['beta'] - single['beta']):.2e} (bound {bound:.2e})")
        ok = ok and same(r0, r1) and r0["converged"] and r0["n"] == single["n"] and r0["n_bad"] == single["n_bad"] == 1
        ok = ok and abs(r0["beta"] - single["beta"]) <= bound
    else:
        ok = False
    print("DIST CHECK", "OK" if ok else "FAILED")
    sys.exit(0 if ok else 1)
