#!/usr/bin/env python3
"""The layer-wise optimizer steps (optim.LAMB / LARS, csrc/optim_layerwise.hip) on one MI355X, at the headline parameter set
(ViT-S/8 + light-curve transformer, bench.build_model), in the form of tools/bench_optim.py.  Median (min .. max) of R
alternated rounds each, all in one run:

  launch   msn_lamb_step (three launches, 40 B per element) beside msn_adam_step (AdamW, one launch, 28 B), and msn_lars_step with
           momentum (three launches, 28 B) beside msn_sgd_step with momentum (one launch, 20 B), each over one device table of
           all parameters.  Each is recorded N times into a HIP graph, so the device events around a replay time the launches
           and not the host that issues them; us per step, TB/s beside the 8 TB/s HBM spec, and the time against the byte ratio
  finish   the share of the finishing launch (one block per tensor) in the device time of a step, from the kernel times
           torch.profiler reports for a few eager steps

Text on stdout and in --out.  The headline step against the parent commit is not this tool's: bench.py of both trees is run in
turns and the rounds are appended to profiles/layerwise_optim_bench.txt by hand."""
import argparse
import os
import sys

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
    ws = torch.empty(int(lib().msn_layerwise_workspace_bytes(n_t, max_n)), dtype=torch.uint8, device=dev)
    ratio = torch.empty(n_t, dtype=torch.float32, device=dev)

    def moments():
        ps, ms, vs = [p.clone() for p in params], [torch.zeros_like(p) for p in params], [torch.zeros_like(p) for p in params]
        return (ps, ms, vs), _table([(p, g, m, v, p.numel()) for p, g, m, v in zip(ps, grads, ms, vs)], dev)

    def buffers():
        ps, bufs = [p.clone() for p in params], [torch.zeros_like(p) for p in params]
        return (ps, bufs), _table([(p, g, b, p.numel()) for p, g, b in zip(ps, grads, bufs)], dev)

    def adamw():
        keep, table = moments()
        return lambda: (keep, check(lib().msn_adam_step(ptr(table), n_t, max_n, 1e-4, 0.9, 0.999, 1e-8, 1e-2, 1, 10, stream_ptr()),
                                    "msn_adam_step"))

    def lamb():
        keep, table = moments()
        return lambda: (keep, check(lib().msn_lamb_step(ptr(table), n_t, max_n, 1e-4, 0.9, 0.999, 1e-6, 1e-2, 1, 0, 0, 10, ptr(ws),
                                                        ws.numel(), ptr(ratio), stream_ptr()), "msn_lamb_step"))

    def sgd():
        keep, table = buffers()
        return lambda: (keep, check(lib().msn_sgd_step(ptr(table), n_t, max_n, 1e-4, 0.9, 0.0, 1e-4, 0, 0, stream_ptr()), "msn_sgd_step"))

    def lars():
        keep, table = buffers()
        return lambda: (keep, check(lib().msn_lars_step(ptr(table), n_t, max_n, 1e-4, 0.9, 0.0, 1e-4, 0, 1e-3, 1e-8, 0, ptr(ws),
                                                        ws.numel(), ptr(ratio), stream_ptr()), "msn_lars_step"))

    forms = [("msn_adam_step (AdamW)", 28, adamw), ("msn_lamb_step (LAMB)", 40, lamb), ("msn_sgd_step (momentum)", 20, sgd),
             ("msn_lars_step (momentum)", 28, lars)]
    graphs = {}
    for name, nbytes, make in forms:
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
    for name, nbytes, _ in forms:
        tb = nbytes * P / (_mid(res[name]) * 1e-6) / 1e12
        lines.append(f"  {name:26s} {_fmt(res[name], 'us')}   {tb:.2f} TB/s of {nbytes} B per element = "
                     f"{tb * 1e12 / HBM_SPEC:.2f} of the HBM spec")
    for ours, base, by_bytes in (("msn_lamb_step (LAMB)", "msn_adam_step (AdamW)", 40 / 28), ("msn_lars_step (momentum)", "msn_sgd_step (momentum)", 28 / 20)):
        lines.append(f"  {ours} / {base}: {_mid(res[ours]) / _mid(res[base]):.2f}x the time for {by_bytes:.2f}x the bytes")
    return lines, {name: fn for name, (_, _, fn) in graphs.items()}


def finish_share(fns, steps=10):
    """Device time per kernel of `steps` eager steps, from torch.profiler: the finishing launch's share of the step."""
    lines = [f"finish: device time per step by launch, {steps} eager steps under torch.profiler"]
    for name in ("msn_lamb_step (LAMB)", "msn_lars_step (momentum)"):
        fn = fns[name]
        fn()
        torch.cuda.synchronize()
        try:
            with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA, torch.profiler.ProfilerActivity.CPU]) as prof:
                for _ in range(steps):
                    fn()
                torch.cuda.synchronize()
            times = {}
            for ev in prof.key_averages():
                us = getattr(ev, "device_time_total", None)
                if us is None:
                    us = getattr(ev, "cuda_time_total", 0.0)
                if us and "_kernel" in ev.key and ("lamb_" in ev.key or "lars_" in ev.key):
                    short = ev.key.split("(")[0].split("::")[-1]
                    times[short] = times.get(short, 0.0) + us / steps
        except Exception as exc:      # noqa: BLE001 -- a profiler that does not work here is reported, not fatal
            lines.append(f"  {name}: torch.profiler failed: {str(exc).splitlines()[0][:100]}")
            continue
        total = sum(times.values())
        if not total:
            lines.append(f"  {name}: torch.profiler reported no kernel times")
            continue
        for k, us in sorted(times.items(), key=lambda kv: -kv[1]):
            lines.append(f"  {name:26s} {k:24s} {us:8.1f} us  {100.0 * us / total:5.1f} %")
    return lines


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20, help="steps recorded per graph")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "layerwise_optim_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim_layerwise.py measures on the GPU; none is visible")
    text = [f"tools/bench_optim_layerwise.py on {torch.cuda.get_device_name(0)}; median (min .. max)"]
    lines, fns = launches(a.rounds, a.launches)
    text += lines + finish_share(fns)
    text = "\n".join(text)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
