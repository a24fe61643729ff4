#!/usr/bin/env python3
"""Masked-light-curve pretraining with the masks drawn on the device (csrc/pretrain_masks.hip) on one MI355X, at the
reference's pretraining light-curve shape: T = 200 in 2 bands, the light-curve transformer of maven_pretrain_config.yaml
(emb 64, 8 heads, depth 5), batches of 64 and 256.  Two modes:

    --step R       ms per training step (zero_grad, training_step, backward, RAdam), device-synchronised host clock, R
                   alternated rounds, median (min .. max) of the rounds, for
                     eager, mask_generator="reference"   (host draws: one random.randint per sample and band)
                     eager, mask_generator="device"      (one msn_pretrain_masks launch)
                     graph-replayed (GraphedTrainStep), mask_generator="device"
    --kernel R     the mask launch alone (masks + x_masked), both modes: N launches recorded into a HIP graph, device events
                   around a replay, R alternated rounds, us per launch

The headline step against the parent commit is measured with tools/ab_step.sh's method (bench.py of both trees, alternated)."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
T, NBAND = 200, 2
LC = dict(n_out=1, emb=64, heads=8, depth=5, dropout=0.0, time_norm=20583.369161312577)      # bench.py's LC (maven_pretrain_config.yaml)
BATCHES = (64, 256)


def _spread(xs):
    s = sorted(xs)
    return {"median": round(s[len(s) // 2], 3), "min": round(s[0], 3), "max": round(s[-1], 3)}


def _batch(rows, device):
    """(t, x, padding_mask): every band holds 30 .. 100 observed points packed at its start, as the simulated light curves do."""
    g = torch.Generator().manual_seed(rows)
    band = T // NBAND
    counts = torch.randint(30, band + 1, (rows, NBAND), generator=g)
    pad = (torch.arange(band)[None, None, :] < counts[:, :, None]).reshape(rows, T)
    return tuple(v.to(device) for v in (torch.rand(rows, T, generator=g) * 100, torch.randn(rows, T, generator=g), pad))


def _model(generator, device):
    from multimodal_supernovae_amd.models_pretraining import MaskedLightCurveEncoder
    torch.manual_seed(0)
    return MaskedLightCurveEncoder(nband=NBAND, transformer_kwargs=LC, mask_generator=generator).to(device).train()


def step(rounds, per_round):
    from multimodal_supernovae_amd.trainer import GraphedTrainStep
    dev = torch.device("cuda")

    def eager_runner(generator, batch):
        model = _model(generator, dev)
        opt = model.configure_optimizers()["optimizer"]

        def one():
            opt.zero_grad(set_to_none=True)
            model.training_step(batch, 0).backward()
            opt.step()
        return one

    def graphed_runner(batch):
        model = _model("device", dev)
        graphed = GraphedTrainStep(model, model.configure_optimizers()["optimizer"], warmup=3)
        return lambda: graphed(batch)

    for rows in BATCHES:
        batch = _batch(rows, dev)
        runners = {"eager_reference_masks": eager_runner("reference", batch), "eager_device_masks": eager_runner("device", batch),
                   "graphed_device_masks": graphed_runner(batch)}
        for fn in runners.values():
            for _ in range(12):
                fn()
        res = {name: [] for name in runners}
        for _ in range(rounds):
            for name, fn in runners.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(per_round):
                    fn()
                torch.cuda.synchronize()
                res[name].append((time.perf_counter() - t0) / per_round * 1e3)
        out = {"rows": rows, "T": T, "nband": NBAND, "transformer": LC, "rounds": rounds, "steps_per_round": per_round,
               "ms_per_step": {name: _spread(v) for name, v in res.items()}}
        print(json.dumps(out), flush=True)


def kernel(rounds, per_graph):
    from multimodal_supernovae_amd.models_pretraining import device_masks
    dev = torch.device("cuda")
    for rows in BATCHES:
        _, x, pad = _batch(rows, dev)
        graphs = {}
        for mode in ("continuous", "random"):
            def fn(mode=mode):
                device_masks(pad, NBAND, 0.2, x=x, mask_type=mode, seed=7)
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
            graphs[mode] = g
        torch.cuda.synchronize()
        res = {mode: [] for mode in graphs}
        for _ in range(rounds):
            for mode, g in graphs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                g.replay()
                e1.record()
                e1.synchronize()
                res[mode].append(e0.elapsed_time(e1) * 1e3 / per_graph)
        print(json.dumps({"rows": rows, "T": T, "nband": NBAND, "launches_per_replay": per_graph, "rounds": rounds,
                          "us_per_launch": {mode: _spread(v) for mode, v in res.items()}}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", type=int, default=0, help="rounds")
    ap.add_argument("--per-round", type=int, default=30, help="steps per round (--step)")
    ap.add_argument("--kernel", type=int, default=0, help="rounds")
    ap.add_argument("--launches", type=int, default=50, help="launches recorded per graph (--kernel)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pretrain_masks.py measures on the GPU; none is visible")
    if a.step:
        step(a.step, a.per_round)
    if a.kernel:
        kernel(a.kernel, a.launches)
