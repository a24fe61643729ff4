#!/usr/bin/env python3
"""Two ranks sharing ONE GPU (gloo transport, CUDA tensors): the classification step of models_finetune.ClipMLP on the focal
loss with label smoothing (csrc/focal_loss.hip) under data parallel vs the single-process step at the doubled batch --
without class weights, with class weights and targets chosen so that the two ranks' weight sums differ, and the smoothed
cross-entropy (gamma = 0) with those weights.  Every rank's loss is its numerator over the GLOBAL denominator and gradients
are SUM-all-reduced, so loss and gradients must agree with the global batch, and both ranks must report the same
train_loss.  (tools/dist_check_supervised.py is the same check for the plain cross-entropy and the regression loss.)"""
import os
import sys

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dist_check_supervised as base  # noqa: E402  (the towers and their batch: rank 0 holds classes 0-1, rank 1 classes 2-4)

B, WEIGHTS, make_batch = base.B, base.WEIGHTS, base.make_batch
FOCAL = dict(loss="focal", loss_kwargs={"gamma": 2.0, "label_smoothing": 0.1})
CASES = [(None, FOCAL), (WEIGHTS, FOCAL), (WEIGHTS, dict(loss="cross_entropy", loss_kwargs={"label_smoothing": 0.1}))]


def make_model(weights, loss):
    from multimodal_supernovae_amd.models_finetune import ClipMLP
    from multimodal_supernovae_amd.models_multimodal import LightCurveImageCLIP
    torch.manual_seed(0)
    clip = LightCurveImageCLIP(enc_dim=16, nband=2, transformer_kwargs=base.TK, transformer_spectral_kwargs=base.SK,
                               combinations=["lightcurve", "spectral"], loss="softmax")
    return ClipMLP(clip, classification=True, n_classes=5, hidden_dim=16, class_weights=weights, **loss).cuda().train()


def worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    from multimodal_supernovae_amd import distributed as D
    D.init_from_env(backend="gloo")
    full = make_batch(world * B)
    local = tuple(t[rank * B:(rank + 1) * B].cuda() if t is not None else None for t in full)
    got = []
    for ci, (weights, loss_cfg) in enumerate(CASES):
        model = make_model(weights, loss_cfg)
        D.broadcast_module(model)
        reducer = D.GradientReducer(model.parameters(), bucket_bytes=64 << 10)   # several buckets, launched under backward
        loss = model.training_step(local, 0)
        loss.backward()
        reducer.finish()
        torch.cuda.synchronize()
        reducer.remove()
        out[f"train_loss_{ci}_r{rank}"] = float(model.logged["train_loss"])
        got.append((float(loss.detach()), {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}))
    dist.barrier()
    dist.destroy_process_group()
    if rank != 0:
        return
    batch = tuple(t.cuda() if t is not None else None for t in full)                # single process at the global batch
    for ci, (weights, loss_cfg) in enumerate(CASES):
        ref = make_model(weights, loss_cfg)
        rl = ref.training_step(batch, 0)
        rl.backward()
        worst = 0.0
        for k, q in ref.named_parameters():
            if q.grad is None:
                continue
            worst = max(worst, float((got[ci][1][k] - q.grad).abs().max()) / (float(q.grad.abs().max()) + 1e-12))
        if weights is not None:
            w = torch.tensor(weights)
            out[f"weight_sums_{ci}"] = [float(w[full[8][r * B:(r + 1) * B]].sum()) for r in range(world)]
        out[f"loss_{ci}"] = (got[ci][0], float(rl.detach()))
        out[f"worst_rel_grad_err_{ci}"] = worst


if __name__ == "__main__":
    ctx = mp.get_context("spawn")
    out = ctx.Manager().dict()
    procs = [ctx.Process(target=worker, args=(r, 2, 29623, out)) for r in range(2)]
    [p.start() for p in procs]
    [p.join(300) for p in procs]
    [p.terminate() for p in procs if p.is_alive()]
    res = dict(out)
    print(res, [p.exitcode for p in procs])
    ok = all(p.exitcode == 0 for p in procs)
    for ci, (weights, _) in enumerate(CASES):
        ok = ok and f"loss_{ci}" in res
        if not ok:
            break
        dp, single = res[f"loss_{ci}"]
        # dist_check_supervised.py's gate for the cross-entropy: loss 1e-4 relative, gradients 1e-3 of their largest entry
        ok = ok and abs(dp - single) < 1e-4 * abs(single) and res[f"worst_rel_grad_err_{ci}"] < 1e-3
        ok = ok and res[f"train_loss_{ci}_r0"] == res[f"train_loss_{ci}_r1"]
        if weights is not None:
            s = res[f"weight_sums_{ci}"]
            ok = ok and abs(s[0] - s[1]) > 0.5                 # the case is only a check if the ranks' denominators differ
    print("DIST CHECK", "OK" if ok else "FAILED")
    sys.exit(0 if ok else 1)
