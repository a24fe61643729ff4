#!/usr/bin/env python3
"""The fused optimizer steps (optim.AdamW / Adam / SGD, csrc/optim_steps.hip) on one MI355X, at the headline parameter set
(ViT-S/8 + light-curve transformer, bench.build_model).  Median (min .. max) of R alternated rounds each:

  launch     the eager entry points msn_adam_step (AdamW, Adam: 28 B per element), msn_sgd_step (with momentum 20 B, plain 12 B)
             and, to report against, msn_radam_step (28 B), over one device table of all parameters; beside each update rule
             torch.optim's foreach=True form and, where this torch build has one, its fused=True form on tensors of the same
             shapes (Adam / AdamW with capturable=True, without which torch's step cannot be recorded).  Each is recorded N
             times into a HIP graph, so the device events around a replay time the launches and not the host that issues them;
             us per step and TB/s beside the 8 TB/s HBM spec
  scheduler  the maven_lc_sp step at batch 256, graph-replayed, with a constant lr and with a step-interval scheduler that
             changes lr in front of every replay (one copy of the 64-byte hyper-parameter block per replay), for RAdam and AdamW:
             device-synchronised host clock, ms per step

Text on stdout and in --out.  The headline step with RAdam against the parent commit is not this tool's: bench.py of both
trees is run in turns and the rounds are appended to profiles/optim_bench.txt by hand."""
import argparse
import os
import sys
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


def _table(rows, dev):
    words = []
    for row in rows:
        words += [0 if t is None else t.data_ptr() for t in row[:-1]] + [row[-1]]
    return torch.tensor(words, dtype=torch.int64).to(dev)


def launches(rounds, per_graph):
    import bench
    from multimodal_supernovae_amd._lib import check, lib, ptr, stream_ptr
    dev = torch.device("cuda")
    model = bench.build_model(dev)
    params = [p.detach() for p in model.parameters() if p.requires_grad]
    gen = torch.Generator(device=dev).manual_seed(3)
    grads = [torch.randn(p.shape, device=dev, generator=gen) * 1e-3 for p in params]
    n_t, max_n, P = len(params), max(p.numel() for p in params), sum(p.numel() for p in params)

    def fresh():
        return [p.clone() for p in params]

    def ours_adam(decoupled):
        ps, ms, vs = fresh(), [torch.zeros_like(p) for p in params], [torch.zeros_like(p) for p in params]
        table = _table([(p, g, m, v, p.numel()) for p, g, m, v in zip(ps, grads, ms, vs)], dev)
        keep = (ps, ms, vs, table)
        return lambda: (keep, check(lib().msn_adam_step(ptr(table), n_t, max_n, 1e-4, 0.9, 0.999, 1e-8, 1e-2, decoupled, 10, stream_ptr()),
                                    "msn_adam_step"))

    def ours_radam():
        ps, ms, vs = fresh(), [torch.zeros_like(p) for p in params], [torch.zeros_like(p) for p in params]
        table = _table([(p, g, m, v, p.numel()) for p, g, m, v in zip(ps, grads, ms, vs)], dev)
        keep = (ps, ms, vs, table)
        return lambda: (keep, check(lib().msn_radam_step(ptr(table), n_t, max_n, 1e-4, 0.9, 0.999, 1e-8, 1e-2, 10, stream_ptr()),
                                    "msn_radam_step"))

    def ours_sgd(momentum):
        ps = fresh()
        bufs = [torch.zeros_like(p) if momentum else None for p in params]
        table = _table([(p, g, b, p.numel()) for p, g, b in zip(ps, grads, bufs)], dev)
        keep = (ps, bufs, table)
        return lambda: (keep, check(lib().msn_sgd_step(ptr(table), n_t, max_n, 1e-4, momentum, 0.0, 1e-4, 0, 0, stream_ptr()), "msn_sgd_step"))

    def stock(cls, **kw):
        ps = [torch.nn.Parameter(p.clone()) for p in params]
        for p, g in zip(ps, grads):
            p.grad = g.clone()
        opt = cls(ps, lr=1e-4, **kw)
        return opt.step

    adam_kw = dict(weight_decay=1e-2, capturable=True)
    forms = [   # (name, bytes per element, maker)
        ("msn_radam_step (RAdam)", 28, ours_radam),
        ("msn_adam_step (AdamW)", 28, lambda: ours_adam(1)),
        ("torch AdamW foreach", 28, lambda: stock(torch.optim.AdamW, foreach=True, **adam_kw)),
        ("torch AdamW fused", 28, lambda: stock(torch.optim.AdamW, fused=True, **adam_kw)),
        ("msn_adam_step (Adam)", 28, lambda: ours_adam(0)),
        ("torch Adam foreach", 28, lambda: stock(torch.optim.Adam, foreach=True, **adam_kw)),
        ("torch Adam fused", 28, lambda: stock(torch.optim.Adam, fused=True, **adam_kw)),
        ("msn_sgd_step (momentum)", 20, lambda: ours_sgd(0.9)),
        ("torch SGD momentum foreach", 20, lambda: stock(torch.optim.SGD, momentum=0.9, weight_decay=1e-4, foreach=True)),
        ("torch SGD momentum fused", 20, lambda: stock(torch.optim.SGD, momentum=0.9, weight_decay=1e-4, fused=True)),
        ("msn_sgd_step (plain)", 12, lambda: ours_sgd(0.0)),
        ("torch SGD plain foreach", 12, lambda: stock(torch.optim.SGD, weight_decay=1e-4, foreach=True)),
        ("torch SGD plain fused", 12, lambda: stock(torch.optim.SGD, weight_decay=1e-4, fused=True)),
    ]
    graphs, absent = {}, {}
    for name, nbytes, make in forms:
        try:
            fn = make()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(3):
                    fn()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for _ in range(per_graph):
                    fn()
            g.replay()
            torch.cuda.synchronize()
            graphs[name] = (g, nbytes, fn)
        except (RuntimeError, ValueError, TypeError) as exc:      # this torch build has no such form
            if name.startswith("msn_"):
                raise
            absent[name] = str(exc).splitlines()[0][:100]
    res = {name: [] for name in graphs}
    for _ in range(rounds):
        for name, (g, _, _) in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            e1.synchronize()
            res[name].append(e0.elapsed_time(e1) * 1e3 / per_graph)
    lines = [f"launch: {P / 1e6:.1f} M elements in {n_t} tensors, {per_graph} steps per replay, {rounds} alternated rounds"]
    for name, _, _ in forms:
        if name in res:
            nbytes = graphs[name][1] * P
            tb = nbytes / (_mid(res[name]) * 1e-6) / 1e12
            lines.append(f"  {name:28s} {_fmt(res[name], 'us')}   {tb:.2f} TB/s of {nbytes // P} B per element = "
                         f"{tb * 1e12 / HBM_SPEC:.2f} of the HBM spec")
        else:
            lines.append(f"  {name:28s} not in this torch build: {absent[name]}")
    return lines


def scheduler_cost(rounds, per_round, batch):
    import bench
    from multimodal_supernovae_amd.trainer import GraphedTrainStep
    dev = torch.device("cuda")
    lines = [f"scheduler: maven_lc_sp at {batch} rows, graph-replayed, {per_round} steps per round, {rounds} alternated rounds, ms per step"]
    for name in ("radam", "adamw"):
        runners = {}
        for form in ("constant lr", "lr changed every step"):
            model, data = bench.build_workload("maven_lc_sp", batch, 0, dev)
            model.optimizer = name
            opt = model.configure_optimizers()["optimizer"]
            step = GraphedTrainStep(model, opt, warmup=3)
            sch = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: 1.0 / (1.0 + 1e-3 * s)) if form != "constant lr" else None

            def one(step=step, sch=sch, data=data):
                step(data)
                if sch is not None:
                    sch.step()
            runners[form] = one
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
            lines.append(f"  {name:6s} {k:22s} {_fmt(ms, 'ms', 3)}")
        lines.append(f"  {name:6s} difference of the medians {(_mid(res['lr changed every step']) - _mid(res['constant lr'])) * 1e3:+.0f} us "
                     "(scheduler.step() on the host + one copy of the hyper-parameter block per replay)")
        del runners
        torch.cuda.empty_cache()
    return lines


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20, help="steps recorded per graph")
    ap.add_argument("--per-round", type=int, default=20, help="training steps per round")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--only", default="launch,scheduler")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim.py measures on the GPU; none is visible")
    text = [f"tools/bench_optim.py on {torch.cuda.get_device_name(0)}; median (min .. max)"]
    parts = a.only.split(",")
    if "launch" in parts:
        text += launches(a.rounds, a.launches)
    if "scheduler" in parts:
        text += scheduler_cost(a.rounds, a.per_round, a.batch)
    text = "\n".join(text)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
