#!/usr/bin/env python3
"""Two ranks sharing ONE GPU (gloo transport, CUDA tensors): Trainer(accumulate_grad_batches=2) under data parallel against
ONE process at twice the batch with the same accumulation.  Two fresh child processes, joined with a timeout; the first one
that fails ends the other.

  * 4 batches of 8 rows per rank and epoch, 2 epochs, k = 2: 4 optimizer steps, in the eager form (hook-driven reducer: the
    boundary micro-batch starts each bucket's all-reduce under backward, the bucket's gather being the window's last add)
    and in the graph-replayed form (deferred reducer, the step recorded once);
  * against the single process at 16-row batches, same k: losses within 1e-4 relative, parameter updates within 1e-3 of
    their largest entry -- the bounds tools/dist_check.py uses for 2 ranks against twice the batch;
  * distributed.COMM_LOG: (optimizer steps) x (buckets) gradient all-reduces in all, none of them between the exchanges
    of a micro-batch that does not close a window -- whose loss exchanges still run -- and `buckets` in each one that does.

Time limits: both forms and the single-process reference run inside one child per rank under ONE deadline (300 s, the way
tools/dist_check_checkpoint.py joins its children), not one per GPU step; the rendezvous port (29641) is fixed, so two
copies of the tool cannot run on one host at the same time."""
import os
import sys
import time

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B, BATCHES, EPOCHS, K = 8, 4, 2, 2
TK = dict(n_out=8, emb=16, heads=4, depth=2, dropout=0.0, time_norm=20583.37, agg="mean")
SK = dict(n_out=8, emb=8, heads=2, depth=2, dropout=0.0, time_norm=17945.14, agg="mean")


def make_model():
    from multimodal_supernovae_amd.models_multimodal import LightCurveImageCLIP
    torch.manual_seed(0)
    return LightCurveImageCLIP(enc_dim=16, nband=2, transformer_kwargs=TK, transformer_spectral_kwargs=SK,
                               combinations=["lightcurve", "spectral"], loss="softmax", lr=3e-3,
                               optimizer_kwargs={"weight_decay": 1e-3}).cuda().train()


def make_batches(world):
    """[batch i of rank r] and [batch i of the single process = the rows of rank 0, then of rank 1]."""
    g = torch.Generator().manual_seed(5)
    n = BATCHES * world * B
    mask = torch.ones(n, 12, dtype=torch.bool)
    mask[:, 9:] = torch.rand(n, 3, generator=g) > 0.5
    full = (None, torch.randn(n, 12, generator=g), torch.rand(n, 12, generator=g) * 100, mask,
            torch.randn(n, 10, generator=g), torch.rand(n, 10, generator=g) * 6000 + 3000,
            torch.ones(n, 10, dtype=torch.bool), None, None)
    cut = lambda lo, rows: tuple(t[lo:lo + rows] if t is not None else None for t in full)
    local = [[cut((i * world + r) * B, B) for i in range(BATCHES)] for r in range(world)]
    return local, [cut(i * world * B, world * B) for i in range(BATCHES)]


def run(batches, graphed):
    """One fit; returns (losses, parameters, global_step, log split per micro-batch, buckets, replayed)."""
    from multimodal_supernovae_amd import distributed as D
    from multimodal_supernovae_amd import trainer as T
    model = make_model()
    real = T._to_device

    def marked(batch, device):                   # once per micro-batch, in front of its exchanges, eager or replayed
        if D.COMM_LOG is not None:
            D.COMM_LOG.append(("micro_batch", 0, None, None))
        return real(batch, device)

    T._to_device, D.COMM_LOG = marked, []
    try:
        tr = T.Trainer(max_epochs=EPOCHS, graphed_steps=graphed, accumulate_grad_batches=K).fit(model, batches)
        torch.cuda.synchronize()
        kinds = [e[0] for e in D.COMM_LOG]
    finally:
        T._to_device, D.COMM_LOG = real, None
    spans = []
    for kind in kinds:
        if kind == "micro_batch":
            spans.append([])
        else:
            spans[-1].append(kind)
    replayed = tr.graphed_step is not None and tr.graphed_step.graph is not None
    return ([float(x) for x in tr.step_losses], [p.detach().clone() for p in model.parameters()], tr.global_step, spans,
            len(tr.reducer.buckets), replayed)


def worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    from multimodal_supernovae_amd import distributed as D
    D.init_from_env(backend="gloo")

    class SmallBuckets(D.GradientReducer):       # several buckets on the tiny model, as tools/dist_check.py builds them
        def __init__(self, params, **kw):
            kw["bucket_bytes"] = 16 << 10
            super().__init__(params, **kw)

    real_reducer, D.GradientReducer = D.GradientReducer, SmallBuckets
    local, whole = make_batches(world)
    res = {}
    for form, graphed in (("eager", False), ("graphed", True)):
        losses, params, steps, spans, buckets, replayed = run(local[rank], graphed)
        boundary = [(i % BATCHES + 1) % K == 0 or i % BATCHES == BATCHES - 1 for i in range(len(spans))]
        res[form] = dict(
            losses=losses, params=params, steps=steps, buckets=buckets, replayed=replayed, micro_batches=len(spans),
            grad_all_reduces=sum(s.count("grad_all_reduce") for s in spans),
            quiet=all(s.count("grad_all_reduce") == 0 and len(s) > 0 for s, b in zip(spans, boundary) if not b),
            reduced=all(s.count("grad_all_reduce") == buckets and len(s) > buckets for s, b in zip(spans, boundary) if b))
    D.GradientReducer = real_reducer
    dist.barrier()
    dist.destroy_process_group()
    if rank == 0:                                # the single process at the global batch, same k
        p0 = [p.detach().clone() for p in make_model().parameters()]
        names = [k for k, _ in make_model().named_parameters()]
        rl, rp, rsteps, _, _, _ = run(whole, False)
        for form in res:
            r = res[form]
            r["steps_ref"] = rsteps
            r["loss_err"] = max(abs(x - y) / abs(y) for x, y in zip(r["losses"], rl)) if len(r["losses"]) == len(rl) else 1.0
            worst = 0.0
            for k, a, c, q0 in zip(names, r["params"], rp, p0):
                if k == "logit_bias":            # analytically zero gradient: rounding noise only
                    continue
                du = c - q0
                worst = max(worst, float(((a - q0) - du).abs().max()) / (float(du.abs().max()) + 1e-12))
            r["update_err"] = worst
    for r in res.values():
        del r["params"]
    out[f"r{rank}"] = res


if __name__ == "__main__":
    ctx = mp.get_context("spawn")
    out = ctx.Manager().dict()
    procs = [ctx.Process(target=worker, args=(r, 2, 29641, out)) for r in range(2)]
    [p.start() for p in procs]
    deadline = time.time() + 300
    while any(p.is_alive() for p in procs) and time.time() < deadline:
        if any(p.exitcode not in (None, 0) for p in procs):
            break                                # a rank failed: the other would wait in a collective
        [p.join(0.2) for p in procs]
    [p.terminate() for p in procs if p.is_alive()]
    res = dict(out)
    print(res, [p.exitcode for p in procs])
    ok = all(p.exitcode == 0 for p in procs) and len(res) == 2
    steps = EPOCHS * BATCHES // K
    for rank in range(2):
        for form in ("eager", "graphed"):
            r = (res.get(f"r{rank}") or {}).get(form)
            if not ok or r is None:
                ok = False
                break
            ok = ok and r["steps"] == steps and r["micro_batches"] == EPOCHS * BATCHES and r["buckets"] > 1
            ok = ok and r["grad_all_reduces"] == steps * r["buckets"] and r["quiet"] and r["reduced"]
            ok = ok and r["replayed"] == (form == "graphed")
            if rank == 0:
                ok = ok and r["steps_ref"] == steps and r["loss_err"] < 1e-4 and r["update_err"] < 1e-3
    print("DIST CHECK", "OK" if ok else "FAILED")
    sys.exit(0 if ok else 1)
