#!/usr/bin/env python3
"""The supervised heads (models_finetune.py, csrc/supervised.hip) on one GPU.  Three modes:

    --loss R       cross-entropy forward + backward at (256, 5), (1024, 5), (4096, 5), (4096, 1000) next to
                   torch.nn.functional.cross_entropy (ATen) on the same device in the same process: R alternating rounds
                   (>= 5), device events around `--iters` calls each, median and spread (min .. max) of the rounds in us per
                   call; at C = 1000 also the achieved bytes/s against the 12 B per element forward + backward need
                   (two reads and one write of the logits)
    --step R       one training step of the maven_lc_sp towers at batch 256: contrastive (the reference), supervised
                   classification unfrozen and frozen, each eager and graph-replayed, R alternating rounds of
                   `--steps-per-round` steps (device-synchronised host clock), ms per step
    --kernels N    the loss and metric kernels N times each at the training shape (256, 5) and at (100000, 5), and the loss
                   at (4096, 1000) (the only shape on the wave-per-row kernels `ce_*_wave_kernel<16>`, so their rows of the
                   table are that shape's kernel times) -- run under `rocprofv3 --kernel-trace --stats` for the launch
                   counts and the kernel times
Every shape is warmed up before the timed window."""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LOSS_SHAPES = [(256, 5), (1024, 5), (4096, 5), (4096, 1000)]


def _median(v):
    return sorted(v)[len(v) // 2]


def loss(rounds, iters):
    from multimodal_supernovae_amd.models_finetune import cross_entropy
    from multimodal_supernovae_amd.trainer import _backward_seed
    rounds = max(rounds, 5)
    out = {"iters_per_round": iters, "rounds": rounds, "unit": "us per forward + backward", "shapes": {}}
    for N, C in LOSS_SHAPES:
        g = torch.Generator().manual_seed(N + C)
        x = torch.randn(N, C, generator=g).cuda().requires_grad_()
        y = torch.randint(0, C, (N,), generator=g).cuda()

        def hip():
            x.grad = None
            l = cross_entropy(x, y)
            l.backward(_backward_seed(l))

        def aten():
            x.grad = None
            l = F.cross_entropy(x, y)
            l.backward(_backward_seed(l))

        res = {"hip": [], "aten": []}
        for fn in (hip, aten):
            for _ in range(20):
                fn()
        torch.cuda.synchronize()
        for _ in range(rounds):
            for name, fn in (("hip", hip), ("aten", aten)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(iters):
                    fn()
                e1.record()
                e1.synchronize()
                res[name].append(e0.elapsed_time(e1) / iters * 1e3)
        entry = {}
        for name, v in res.items():
            entry[name] = {"median": round(_median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
        entry["hip_over_aten"] = round(entry["hip"]["median"] / entry["aten"]["median"], 3)
        if C >= 64:
            nbytes = 12 * N * C
            entry["bytes_needed"] = nbytes
            entry["hip_achieved_TBps"] = round(nbytes / (entry["hip"]["median"] * 1e-6) / 1e12, 3)
            entry["aten_achieved_TBps"] = round(nbytes / (entry["aten"]["median"] * 1e-6) / 1e12, 3)
        out["shapes"][f"({N}, {C})"] = entry
    print(json.dumps(out, indent=1))


def step(rounds, per_round, b):
    import copy

    import bench
    from multimodal_supernovae_amd.models_finetune import ClipMLP
    from multimodal_supernovae_amd.trainer import GraphedTrainStep, _backward_seed
    dev = torch.device("cuda")
    clip, batch = bench.build_workload("maven_lc_sp", b, 0, dev)
    g = torch.Generator().manual_seed(7)
    batch = batch[:7] + (torch.rand(b, generator=g).to(dev), torch.randint(0, 5, (b,), generator=g).to(dev))

    def eager(model):
        opt = model.configure_optimizers()["optimizer"]

        def one():
            opt.zero_grad(set_to_none=True)
            l = model.training_step(batch, 0)
            l.backward(_backward_seed(l))
            opt.step()
        return one

    def graphed(model):
        st = GraphedTrainStep(model, model.configure_optimizers()["optimizer"], warmup=3)
        return lambda: st(batch, 0)

    def head(frozen):
        return ClipMLP(copy.deepcopy(clip), classification=True, n_classes=5, freeze_backbone=frozen,
                       learning_rate=bench.LR).to(dev).train()

    forms = {
        "contrastive eager": eager(copy.deepcopy(clip)),
        "contrastive graphed": graphed(copy.deepcopy(clip)),
        "classification eager": eager(head(False)),
        "classification graphed": graphed(head(False)),
        "classification frozen eager": eager(head(True)),
        "classification frozen graphed": graphed(head(True)),
    }
    for fn in forms.values():                       # warm-up of every form (the graphed ones record here)
        for _ in range(6):
            fn()
    torch.cuda.synchronize()
    res = {k: [] for k in forms}
    for _ in range(rounds):
        for name, fn in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(per_round):
                fn()
            torch.cuda.synchronize()
            res[name].append((time.perf_counter() - t0) / per_round * 1e3)
    out = {"workload": "maven_lc_sp", "batch": b, "rounds": rounds, "steps_per_round": per_round, "unit": "ms per step", "forms": {}}
    for name, v in res.items():
        out["forms"][name] = {"median": round(_median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
    print(json.dumps(out, indent=1))


def kernels(n):
    from multimodal_supernovae_amd.models_finetune import ClassificationMetrics, RegressionMetrics, _cross_entropy
    shapes = [(256, 5), (100000, 5), (4096, 1000)]
    for N, C in shapes:
        g = torch.Generator().manual_seed(N)
        x = torch.randn(N, C, generator=g).cuda().requires_grad_()
        y = torch.randint(0, C, (N,), generator=g).cuda()
        z = torch.rand(N, generator=g).cuda()
        cm, rm = ClassificationMetrics(C), RegressionMetrics()
        seed = torch.ones((), device="cuda")
        for _ in range(n):
            x.grad = None
            l, pred = _cross_entropy(x, y)
            l.backward(seed)
            if C == 5:
                cm.update(pred, y)
                rm.update(z, z)
    torch.cuda.synchronize()
    print(json.dumps({"calls_each_per_shape": n, "loss_shapes": shapes, "metric_shapes": shapes[:2]}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--loss", type=int, default=0)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--step", type=int, default=0)
    ap.add_argument("--steps-per-round", type=int, default=10)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--kernels", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_supervised.py measures on the GPU; none is visible")
    if a.loss:
        loss(a.loss, a.iters)
    if a.step:
        step(a.step, a.steps_per_round, a.batch)
    if a.kernels:
        kernels(a.kernels)
