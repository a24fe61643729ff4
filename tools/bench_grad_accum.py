#!/usr/bin/env python3
"""Gradient accumulation (Trainer(accumulate_grad_batches=k), csrc/grad_accum.hip) on one MI355X.  Two modes:

    --kernel R     the accumulate launch in add mode (12 B per element: two reads, one write) on the headline model's
                   parameter set (ViT-S/8 + light-curve transformer, bench.build_model -- the set tools/bench_grad_clip.py
                   builds) beside torch._foreach_add_ on the same tensors.  Each is recorded N times into a HIP graph, so the
                   device events around a replay time the launches and not the host that issues them; R alternated rounds,
                   median (min .. max) of the rounds, us per launch and TB/s beside the 8 TB/s HBM spec
    --micro R      what a micro-batch costs: maven_lc_sp at 64 rows, eager and graph-replayed, k = 4 against the k = 1 step of
                   the same run (device-synchronised host clock), R alternated rounds, median (min .. max) ms per micro-batch

The k = 1 path against the parent commit is measured with tools/ab_step.sh (bench.py of both trees, interleaved).
Memory: 4 bytes per trainable parameter (the accumulators), with or without data parallel -- the reducer's bucket buffer
receives the window's last add but is not the accumulator."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_SPEC = 8.0e12


def _spread(xs):
    s = sorted(xs)
    return {"median": round(s[len(s) // 2], 3), "min": round(s[0], 3), "max": round(s[-1], 3)}


def kernel(rounds, per_graph):
    import bench
    from multimodal_supernovae_amd import optim
    model = bench.build_model(torch.device("cuda"))
    params = list(model.parameters())
    gen = torch.Generator(device="cuda").manual_seed(0)
    grads = [torch.randn(p.shape, device="cuda", generator=gen) * 1e-3 for p in params]
    accs = [torch.zeros_like(g) for g in grads]
    P = sum(g.numel() for g in grads)

    def ours():
        optim.grad_accumulate_(accs, accs, grads, add=True)

    def stock():
        torch._foreach_add_(accs, grads)

    graphs = {}
    for name, fn in (("msn_grad_accumulate", ours), ("torch._foreach_add_", stock)):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                fn()
        torch.cuda.current_stream().wait_stream(side)
        if fn is ours:
            for _ in range(per_graph):                 # one pinned descriptor table per launch recorded
                optim.accum_graph_prepare(params)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(per_graph):
                fn()
        g.replay()
        graphs[name] = g
    torch.cuda.synchronize()
    res = {name: [] for name in graphs}
    for _ in range(rounds):
        for name, g in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            e1.synchronize()
            res[name].append(e0.elapsed_time(e1) * 1e3 / per_graph)
    out = {"parameters": P, "tensors": len(params), "bytes_per_launch": 12 * P, "launches_per_replay": per_graph, "rounds": rounds,
           "hbm_spec_TBps": HBM_SPEC / 1e12}
    for name, us in res.items():
        s = _spread(us)
        tb = {k: round(12 * P / (v * 1e-6) / 1e12, 3) for k, v in s.items()}
        out[name] = {"us_per_launch": s, "TBps_at_median": tb["median"], "share_of_hbm_spec_at_median": round(tb["median"] * 1e12 / HBM_SPEC, 3),
                     "TBps_range": [tb["max"], tb["min"]]}
    print(json.dumps(out))


def micro(rounds, per_round):
    import bench
    from multimodal_supernovae_amd.trainer import GraphedTrainStep, _accumulate_seed, _backward_seed
    from multimodal_supernovae_amd import optim
    dev = torch.device("cuda")

    def eager_runner(k):
        model, batch = bench.build_workload("maven_lc_sp", 64, 0, dev)
        opt = model.configure_optimizers()["optimizer"]
        acc = optim.GradAccumulator([p for group in opt.param_groups for p in group["params"]]) if k > 1 else None
        state = {"i": 0}

        def one():
            opt.zero_grad(set_to_none=True)
            loss = model.training_step(batch, 0)
            if k == 1:
                loss.backward(_backward_seed(loss))
                opt.step()
                return
            boundary = (state["i"] + 1) % k == 0
            state["i"] += 1
            loss.backward(_accumulate_seed(loss, k))
            acc.accumulate(boundary)
            if boundary:
                opt.step()
        return one

    def graphed_runner(k):
        model, batch = bench.build_workload("maven_lc_sp", 64, 0, dev)
        step = GraphedTrainStep(model, model.configure_optimizers()["optimizer"], warmup=3, accumulate_grad_batches=k)
        return lambda: step(batch)

    out = {"workload": "maven_lc_sp", "rows": 64, "k": 4, "rounds": rounds, "micro_batches_per_round": per_round}
    for form, make in (("eager", eager_runner), ("graphed", graphed_runner)):
        runners = {1: make(1), 4: make(4)}
        for fn in runners.values():
            for _ in range(12):
                fn()
        res = {1: [], 4: []}
        for _ in range(rounds):
            for k, fn in runners.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(per_round):
                    fn()
                torch.cuda.synchronize()
                res[k].append((time.perf_counter() - t0) / per_round * 1e3)
        out[form] = {"ms_per_step_k1": _spread(res[1]), "ms_per_micro_batch_k4": _spread(res[4])}
    print(json.dumps(out))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", type=int, default=0, help="rounds")
    ap.add_argument("--launches", type=int, default=50, help="launches recorded per graph (--kernel)")
    ap.add_argument("--micro", type=int, default=0, help="rounds")
    ap.add_argument("--per-round", type=int, default=40, help="micro-batches per round (--micro; a multiple of 4)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_grad_accum.py measures on the GPU; none is visible")
    if a.kernel:
        kernel(a.kernel, a.launches)
    if a.micro:
        micro(a.micro, a.per_round)
