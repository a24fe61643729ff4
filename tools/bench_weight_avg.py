#!/usr/bin/env python3
"""Weight averaging (checkpoint.WeightAveraging, optim.AveragedWeights, csrc/weight_avg.hip) on one MI355X, at the headline
parameter set (ViT-S/8 + light-curve transformer, bench.build_model).  Median (min .. max) of R alternated rounds each:

  launch   the update launch (12 B per element: two reads, one write) beside torch._foreach_lerp_ on the same tensors, and the
           swap (16 B per element).  Each is recorded N times into a HIP graph, so the device events around a replay time the
           launches and not the host that issues them; us per launch and TB/s beside the 8 TB/s HBM spec
  step     the headline step at 1024 pairs without and with an EMA update after every optimizer step, eager and graph-replayed
           (GraphedTrainStep(weight_averaging=...)): device-synchronised host clock, ms per step
  save     Trainer.save_checkpoint of the headline model without and with the callback's average in the file

Text on stdout and in --out.  The step WITHOUT the callback against the parent commit is not this tool's: bench.py of both
trees is run in turns (tools/ab_step.sh's way) and the rounds are appended to profiles/weight_avg_bench.txt by hand."""
import argparse
import os
import shutil
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_SPEC = 8.0e12


def _mid(xs):
    return sorted(xs)[len(xs) // 2]


def _fmt(xs, unit, digits=1):
    s = sorted(xs)
    return f"{_mid(s):9.{digits}f} {unit} ({s[0]:.{digits}f} .. {s[-1]:.{digits}f})"


def launches(rounds, per_graph):
    import bench
    from multimodal_supernovae_amd import optim
    model = bench.build_model(torch.device("cuda"))
    aw = optim.AveragedWeights(model, "ema", 0.999)
    aw.update()                                               # the first update is the copy: time the averaging form
    params = aw.tensors
    stock_avg = [torch.zeros_like(p) for p in params]
    w = 1.0 - 0.999
    fns = {"msn_weight_average (EMA)": aw.update, "torch._foreach_lerp_": lambda: torch._foreach_lerp_(stock_avg, params, w),
           "msn_weight_average (swap)": aw.swap}
    graphs = {}
    for name, fn in fns.items():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(4):
                fn()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        if fn == aw.swap:                                     # swap() refuses a capture (it is not part of a step): time its launch
            fn = lambda: aw._launch(optim._AVG_SWAP, None)    # noqa: E731
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
    P = aw.numel
    lines = [f"launch: {P / 1e6:.1f} M averaged elements in {len(params)} tensors, {per_graph} launches per replay, {rounds} alternated rounds"]
    for name, us in res.items():
        nbytes = (16 if "swap" in name else 12) * P
        tb = nbytes / (_mid(us) * 1e-6) / 1e12
        lines.append(f"  {name:28s} {_fmt(us, 'us')}   {tb:.2f} TB/s of {nbytes // P} B per element = {tb * 1e12 / HBM_SPEC:.2f} of the HBM spec")
    return lines


def steps(rounds, per_round, batch):
    import bench
    from multimodal_supernovae_amd import optim
    from multimodal_supernovae_amd.trainer import GraphedTrainStep, _backward_seed
    dev = torch.device("cuda")
    data = bench.synthetic_batch(batch, 0, dev)

    def eager(averaged):
        model = bench.build_model(dev)
        opt = model.configure_optimizers()["optimizer"]
        aw = optim.AveragedWeights(model, "ema", 0.999) if averaged else None

        def one():
            opt.zero_grad(set_to_none=True)
            loss = model.training_step(data, 0)
            loss.backward(_backward_seed(loss))
            opt.step()
            if aw is not None:
                aw.update()
        return one

    def graphed(averaged):
        model = bench.build_model(dev)
        aw = optim.AveragedWeights(model, "ema", 0.999) if averaged else None
        step = GraphedTrainStep(model, model.configure_optimizers()["optimizer"], warmup=3, weight_averaging=aw)
        return lambda: step(data)

    lines = [f"step: headline workload at {batch} pairs, {per_round} steps per round, {rounds} alternated rounds, ms per step"]
    for form, make in (("eager", eager), ("graph-replayed", graphed)):
        runners = {"without": make(False), "with EMA": make(True)}
        for fn in runners.values():
            for _ in range(8):
                fn()
        res = {k: [] for k in runners}
        for _ in range(rounds):
            for k, fn in runners.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(per_round):
                    fn()
                torch.cuda.synchronize()
                res[k].append((time.perf_counter() - t0) / per_round * 1e3)
        for k, ms in res.items():
            lines.append(f"  {form:15s} {k:9s} {_fmt(ms, 'ms', 3)}")
        lines.append(f"  {form:15s} difference of the medians {(_mid(res['with EMA']) - _mid(res['without'])) * 1e3:+.0f} us")
        del runners
        torch.cuda.empty_cache()
    return lines


def saves(rounds):
    import bench
    from multimodal_supernovae_amd import checkpoint as C
    from multimodal_supernovae_amd.trainer import Trainer
    dev = torch.device("cuda")
    folder = tempfile.mkdtemp(prefix="msn_wavg_bench_")
    try:
        data = [bench.synthetic_batch(64, 0, dev)] * 2
        trainers = {}
        for name, cbs in (("without", []), ("with the average", [C.WeightAveraging("ema", 0.999, apply_at_end=False)])):
            trainers[name] = Trainer(max_epochs=1, callbacks=cbs).fit(bench.build_model(dev), data)
        res, size = {k: [] for k in trainers}, {}
        for r in range(rounds + 1):                           # the first round is warm-up
            for name, tr in trainers.items():
                path = os.path.join(folder, name.replace(" ", "_") + ".ckpt")
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                tr.save_checkpoint(path)
                if r:
                    res[name].append((time.perf_counter() - t0) * 1e3)
                size[name] = os.path.getsize(path)
        lines = [f"save: Trainer.save_checkpoint of the headline model (parameters + 2 RAdam moments), {rounds} alternated rounds"]
        for name, ms in res.items():
            lines.append(f"  {name:17s} {_fmt(ms, 'ms')}   file {size[name] / 1e6:.1f} MB")
        lines.append(f"  the average adds {_mid(res['with the average']) - _mid(res['without']):+.1f} ms (difference of the medians) and "
                     f"{(size['with the average'] - size['without']) / 1e6:.1f} MB")
        return lines
    finally:
        shutil.rmtree(folder, ignore_errors=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=50, help="launches recorded per graph (an even count: the swaps undo each other)")
    ap.add_argument("--per-round", type=int, default=10, help="steps per round")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--only", default="launch,step,save")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "weight_avg_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_weight_avg.py measures on the GPU; none is visible")
    text = [f"tools/bench_weight_avg.py on {torch.cuda.get_device_name(0)}; median (min .. max)"]
    parts = a.only.split(",")
    if "launch" in parts:
        text += launches(a.rounds, a.launches)
    if "step" in parts:
        text += steps(a.rounds, a.per_round, a.batch)
    if "save" in parts:
        text += saves(a.rounds)
    text = "\n".join(text)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
