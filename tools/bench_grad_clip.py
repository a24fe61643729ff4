#!/usr/bin/env python3
"""Gradient clipping on the headline model's parameter set (ViT-S/8 + light-curve transformer, bench.build_model), seeded
gradients.  Three modes:

    --kernels N          msn_grad_norm (norm 2), msn_grad_scale, msn_grad_clamp and the RAdam step on the same tensors, N times
                         each -- run under `rocprofv3 --kernel-trace --stats` for the kernel times
    --report STATS.csv   per-kernel mean time from that stats table -> us, achieved bytes/s and share of the 8 TB/s HBM spec
                         (bytes from shapes: norm reads 4 P, scale and clamp read and write 8 P, RAdam 28 P)
    --step R             the headline step at 1024 pairs without and with Trainer(gradient_clip_val=1.0)'s clip, alternated
                         over R rounds in one process (device-synchronised host clock), ms per step of each
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_SPEC = 8.0e12
KERNELS = {   # kernel-name substring -> (label, bytes per parameter)
    "grad_norm_partial_kernel<2>": ("msn_grad_norm (partials, p = 2)", 4),
    "grad_norm_finish_kernel<2>": ("msn_grad_norm (finishing block)", 0),
    "grad_scale_kernel": ("msn_grad_scale", 8),
    "grad_clamp_kernel": ("msn_grad_clamp", 8),
    "radam_kernel": ("RAdam step (msn_radam_step)", 28),
}


def _setup():
    import bench
    model = bench.build_model(torch.device("cuda"))
    params = list(model.parameters())
    g = torch.Generator(device="cuda").manual_seed(0)
    for p in params:
        p.grad = torch.randn(p.shape, device="cuda", generator=g) * 1e-3
    return model, params


def kernels(n):
    from multimodal_supernovae_amd import optim
    model, params = _setup()
    opt = model.configure_optimizers()["optimizer"]
    P = sum(p.numel() for p in params)
    for _ in range(n):
        optim.clip_grad_norm_(params, 1e9)           # coef 1: the gradients keep their values from call to call
    for _ in range(n):
        optim.clip_grad_value_(params, 1.0)
    for _ in range(n):
        opt.step()
    torch.cuda.synchronize()
    print(json.dumps({"parameters": P, "tensors": len(params), "calls_each": n}))


def report(path, P):
    import csv
    rows = list(csv.DictReader(open(path)))
    out = {"parameters": P, "hbm_spec_TBps": HBM_SPEC / 1e12, "kernels": {}}
    for key, (label, bpp) in KERNELS.items():
        hit = [r for r in rows if key in r["Name"]]
        if not hit:
            out["kernels"][label] = "not measured"
            continue
        calls = sum(int(r["Calls"]) for r in hit)
        us = sum(float(r["TotalDurationNs"]) for r in hit) / calls / 1e3
        e = {"us": round(us, 2), "calls": calls}
        if bpp:
            bps = bpp * P / (us * 1e-6)
            e.update(bytes=bpp * P, achieved_TBps=round(bps / 1e12, 3), share_of_hbm_spec=round(bps / HBM_SPEC, 3))
        out["kernels"][label] = e
    print(json.dumps(out, indent=1))


def step(rounds, per_round):
    import bench
    from multimodal_supernovae_amd import optim
    from multimodal_supernovae_amd.trainer import _backward_seed
    model = bench.build_model(torch.device("cuda"))
    batch = bench.synthetic_batch(1024, 0, torch.device("cuda"))
    opt = model.configure_optimizers()["optimizer"]
    params = [p for group in opt.param_groups for p in group["params"]]

    def one(clip):
        opt.zero_grad(set_to_none=True)
        loss = model.training_step(batch, 0)
        loss.backward(_backward_seed(loss))
        if clip:
            optim.clip_grad_norm_(params, 1.0)
        opt.step()

    for clip in (False, True, False, True):          # warm-up of both forms
        one(clip)
    res = {False: [], True: []}
    for _ in range(rounds):
        for clip in (False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(per_round):
                one(clip)
            torch.cuda.synchronize()
            res[clip].append((time.perf_counter() - t0) / per_round * 1e3)
    out = {"global_batch": 1024, "rounds": rounds, "steps_per_round": per_round,
           "ms_per_step_plain": [round(x, 3) for x in res[False]], "ms_per_step_clip_norm": [round(x, 3) for x in res[True]],
           "median_plain": sorted(res[False])[rounds // 2], "median_clip_norm": sorted(res[True])[rounds // 2]}
    out["median_overhead_ms"] = out["median_clip_norm"] - out["median_plain"]
    print(json.dumps(out))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", type=int, default=0)
    ap.add_argument("--report", default=None)
    ap.add_argument("--parameters", type=int, default=0, help="P of the --kernels run (its first output line)")
    ap.add_argument("--step", type=int, default=0)
    ap.add_argument("--steps-per-round", type=int, default=8)
    a = ap.parse_args()
    if a.kernels:
        kernels(a.kernels)
    if a.report:
        report(a.report, a.parameters)
    if a.step:
        step(a.step, a.steps_per_round)
