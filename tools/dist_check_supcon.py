#!/usr/bin/env python3
"""Two ranks sharing ONE GPU (gloo transport, CUDA tensors): one training step under loss="supcon" with global negatives against
the single-process step at twice the batch -- the loss, the gradients of the embeddings (each rank's rows of the global ones) and
the parameters after one optimizer step, at the tolerances tools/dist_check.py applies to the softmax loss (loss 1e-4 relative,
gradients and updates 1e-3 of their largest entry).  The labels are five classes in turn with two unknown rows, so the positives
of a row live on both ranks."""
import os
import sys

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TK = dict(n_out=8, emb=16, heads=4, depth=2, dropout=0.0, time_norm=20583.37, agg="mean")
SK = dict(n_out=8, emb=8, heads=2, depth=2, dropout=0.0, time_norm=17945.14, agg="mean")
B = 8


def make_model():
    from multimodal_supernovae_amd.models_multimodal import LightCurveImageCLIP
    torch.manual_seed(0)
    return LightCurveImageCLIP(enc_dim=16, nband=2, transformer_kwargs=TK, transformer_spectral_kwargs=SK,
                               combinations=["lightcurve", "spectral"], loss="supcon", lr=1e-2).cuda().train()


def make_batch(n):
    g = torch.Generator().manual_seed(1)
    mask = torch.ones(n, 12, dtype=torch.bool)
    mask[:, 9:] = False
    labels = torch.arange(n) % 5
    labels[3], labels[n - 2] = -1, -1
    return (None, torch.randn(n, 12, generator=g), torch.rand(n, 12, generator=g) * 100, mask,
            torch.randn(n, 10, generator=g), torch.rand(n, 10, generator=g) * 6000 + 3000,
            torch.ones(n, 10, dtype=torch.bool), None, labels)


def step(model, batch, reducer):
    """-> (loss, [dloss/dembedding per tower], parameters after the step)"""
    opt = model.configure_optimizers()["optimizer"]
    embs = model(*batch)
    for e in embs:
        e.retain_grad()
    loss = model._loss(embs, batch[8])
    loss.backward()
    if reducer is not None:
        reducer.finish()
    opt.step()
    torch.cuda.synchronize()
    return float(loss.detach()), [e.grad.detach().clone() for e in embs], [p.detach().clone() for p in model.parameters()]


def worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    from multimodal_supernovae_amd import distributed as D
    D.init_from_env(backend="gloo")
    full = make_batch(world * B)
    both = lambda r: {int(v) for v in full[8][r * B:(r + 1) * B] if int(v) >= 0}
    assert both(0) & both(1), "the labels must put positives of a row on both ranks"
    local = tuple(t[rank * B:(rank + 1) * B].cuda() if t is not None else None for t in full)
    model = make_model()
    D.broadcast_module(model)
    p0 = [p.detach().clone() for p in model.parameters()]
    reducer = D.GradientReducer(model.parameters(), bucket_bytes=64 << 10)
    loss, dembs, params = step(model, local, reducer)
    reducer.remove()
    dist.barrier()
    dist.destroy_process_group()
    ref = make_model()                     # single process at the global batch
    rl, rdembs, rparams = step(ref, tuple(t.cuda() if t is not None else None for t in full), None)
    emb_err = max(float((a - c[rank * B:(rank + 1) * B]).abs().max()) / (float(c.abs().max()) + 1e-12) for a, c in zip(dembs, rdembs))
    upd_err = 0.0
    for (k, _), a, c, q0 in zip(ref.named_parameters(), params, rparams, p0):
        du = c - q0
        if k == "logit_bias" or float(du.abs().max()) == 0.0:      # analytically zero gradient: rounding noise only
            continue
        upd_err = max(upd_err, float(((a - q0) - du).abs().max()) / float(du.abs().max()))
    out[f"r{rank}"] = (loss, rl, emb_err, upd_err)


if __name__ == "__main__":
    ctx = mp.get_context("spawn")
    out = ctx.Manager().dict()
    procs = [ctx.Process(target=worker, args=(r, 2, 29619, out)) for r in range(2)]
    [p.start() for p in procs]
    [p.join(300) for p in procs]
    print(dict(out), [p.exitcode for p in procs])
    ok = all(p.exitcode == 0 for p in procs) and len(out) == 2
    for loss, rl, emb_err, upd_err in out.values():
        ok = ok and abs(loss - rl) < 1e-4 * abs(rl) and emb_err < 1e-3 and upd_err < 1e-3
    print("DIST CHECK", "OK" if ok else "FAILED")
    sys.exit(0 if ok else 1)
