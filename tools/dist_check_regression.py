#!/usr/bin/env python3
"""Two ranks sharing ONE GPU (gloo transport, CUDA tensors): the regression step of models_finetune.ClipMLP on the Huber,
Gaussian-NLL and quantile losses (csrc/regression_loss.hip) under data parallel vs the single-process step at the doubled
batch, with targets that are NaN -- objects without a spectroscopic redshift -- spread unevenly over the ranks (three on
rank 0, one on rank 1), so that the ranks' counts of valid rows differ.  Every rank's loss is its numerator over the GLOBAL
count and gradients are SUM-all-reduced, so loss and gradients must agree with the global batch, and both ranks must report
the same train_loss.  The validation statistics follow: each rank updates an IntervalMetrics on its shard, the two SUM
all-reduces give the counts of the whole batch exactly.  (tools/dist_check_supervised.py is the same check for the
cross-entropy and the MSE, tools/dist_check_focal.py for the focal loss.)"""
import os
import sys

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dist_check_supervised as base  # noqa: E402  (the towers and their batch)

B = base.B
CASES = [dict(loss="huber", loss_kwargs={"delta": 0.1}), dict(loss="gaussian_nll"), dict(loss="quantile")]
MISSING = (0, 3, 5, B + 2)                 # rows of the global batch without a redshift: three on rank 0, one on rank 1


def make_batch(n):
    batch = list(base.make_batch(n))
    batch[7] = batch[7].clone()
    batch[7][list(MISSING)] = float("nan")
    return tuple(batch)


def make_model(loss):
    from multimodal_supernovae_amd.models_finetune import ClipMLP
    from multimodal_supernovae_amd.models_multimodal import LightCurveImageCLIP
    torch.manual_seed(0)
    clip = LightCurveImageCLIP(enc_dim=16, nband=2, transformer_kwargs=base.TK, transformer_spectral_kwargs=base.SK,
                               combinations=["lightcurve", "spectral"], loss="softmax")
    return ClipMLP(clip, regression=True, hidden_dim=16, **loss).cuda().train()


def worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    from multimodal_supernovae_amd import distributed as D
    D.init_from_env(backend="gloo")
    full = make_batch(world * B)
    local = tuple(t[rank * B:(rank + 1) * B].cuda() if t is not None else None for t in full)
    got = []
    for ci, loss_cfg in enumerate(CASES):
        model = make_model(loss_cfg)
        D.broadcast_module(model)
        reducer = D.GradientReducer(model.parameters(), bucket_bytes=64 << 10)   # several buckets, launched under backward
        loss = model.training_step(local, 0)
        loss.backward()
        reducer.finish()
        torch.cuda.synchronize()
        reducer.remove()
        out[f"train_loss_{ci}_r{rank}"] = float(model.logged["train_loss"])
        with torch.no_grad():
            model.metrics.update(model(*local), local[7])
        model.metrics.all_reduce()
        torch.cuda.synchronize()
        got.append((float(loss.detach()), {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None},
                    model.metrics.cnt.cpu().tolist()))
    dist.barrier()
    dist.destroy_process_group()
    if rank != 0:
        return
    batch = tuple(t.cuda() if t is not None else None for t in full)                # single process at the global batch
    for ci, loss_cfg in enumerate(CASES):
        ref = make_model(loss_cfg)
        rl = ref.training_step(batch, 0)
        rl.backward()
        worst = 0.0
        for k, q in ref.named_parameters():
            if q.grad is None:
                continue
            worst = max(worst, float((got[ci][1][k] - q.grad).abs().max()) / (float(q.grad.abs().max()) + 1e-12))
        with torch.no_grad():
            ref.metrics.update(ref(*batch), batch[7])
        out[f"loss_{ci}"] = (got[ci][0], float(rl.detach()))
        out[f"worst_rel_grad_err_{ci}"] = worst
        out[f"counts_{ci}"] = (got[ci][2], ref.metrics.cnt.cpu().tolist())
    out["valid_rows"] = [int(torch.isfinite(full[7][r * B:(r + 1) * B]).sum()) for r in range(world)]


if __name__ == "__main__":
    ctx = mp.get_context("spawn")
    out = ctx.Manager().dict()
    procs = [ctx.Process(target=worker, args=(r, 2, 29625, out)) for r in range(2)]
    [p.start() for p in procs]
    [p.join(300) for p in procs]
    [p.terminate() for p in procs if p.is_alive()]
    res = dict(out)
    print(res, [p.exitcode for p in procs])
    ok = all(p.exitcode == 0 for p in procs)
    for ci in range(len(CASES)):
        ok = ok and f"loss_{ci}" in res
        if not ok:
            break
        dp, single = res[f"loss_{ci}"]
        # dist_check_supervised.py's gate: loss 1e-4 relative, gradients 1e-3 of their largest entry
        ok = ok and abs(dp - single) < 1e-4 * abs(single) and res[f"worst_rel_grad_err_{ci}"] < 1e-3
        ok = ok and res[f"train_loss_{ci}_r0"] == res[f"train_loss_{ci}_r1"]
        counts_dp, counts_single = res[f"counts_{ci}"]
        ok = ok and counts_dp[0] == 2 * B - len(MISSING)
        # the towers' forward is not bit-identical between batch 8 and batch 16, so a compare may flip: the row count is exact
        ok = ok and all(abs(a - b) <= 1 for a, b in zip(counts_dp, counts_single))
    ok = ok and res.get("valid_rows") == [B - 3, B - 1]             # the case is only a check if the ranks' counts differ
    print("DIST CHECK", "OK" if ok else "FAILED")
    sys.exit(0 if ok else 1)
