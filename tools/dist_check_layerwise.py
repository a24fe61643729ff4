#!/usr/bin/env python3
"""Two ranks sharing ONE GPU (gloo transport, CUDA tensors): optim.LAMB and optim.LARS under data parallel.  There is no
collective in the trust ratios: the gradients are all-reduced before the step, so every rank forms the same norms from the same
values in the same order, and the parameters AND the ratios must be identical BIT FOR BIT on both ranks.  Two fresh child
processes, joined under one deadline; the first one that fails ends the other.

  * LAMB (the class handed to `optimizer=`) with eager steps, LARS (by name) with graph-replayed steps and a step-interval
    warm-up: 2 epochs of 3 batches of 8 rows per rank, every rank its own rows;
  * per form the parent compares the two ranks' parameters and last trust ratios with torch.equal, and checks that the ratios
    are finite and not all 1 (the layer-wise rate was at work).

Time limit: everything runs inside one child per rank under ONE deadline (200 s, the way tools/dist_check_weight_avg.py joins
its children); the rendezvous port (29661) is fixed, so two copies of the tool cannot run on one host at the same time."""
import os
import sys
import time

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B, BATCHES, EPOCHS = 8, 3, 2


def make_model(seed, optimizer, lr):
    from multimodal_supernovae_amd.models_multimodal import LightCurveImageCLIP
    tk = dict(n_out=8, emb=16, heads=4, depth=2, dropout=0.0, time_norm=20583.37, agg="mean")
    sk = dict(n_out=8, emb=8, heads=2, depth=2, dropout=0.0, time_norm=17945.14, agg="mean")
    torch.manual_seed(seed)
    return LightCurveImageCLIP(enc_dim=16, nband=2, transformer_kwargs=tk, transformer_spectral_kwargs=sk,
                               combinations=["lightcurve", "spectral"], loss="softmax", lr=lr, optimizer=optimizer,
                               optimizer_kwargs={"weight_decay": 1e-2}).cuda().train()


def make_batches(rank, world):
    g = torch.Generator().manual_seed(5)
    n = BATCHES * world * B
    mask = torch.ones(n, 12, dtype=torch.bool)
    mask[:, 9:] = torch.rand(n, 3, generator=g) > 0.5
    full = (None, torch.randn(n, 12, generator=g), torch.rand(n, 12, generator=g) * 100, mask,
            torch.randn(n, 10, generator=g), torch.rand(n, 10, generator=g) * 6000 + 3000,
            torch.ones(n, 10, dtype=torch.bool), None, None)
    return [tuple(t[(i * world + rank) * B:(i * world + rank + 1) * B] if t is not None else None for t in full)
            for i in range(BATCHES)]


def warmup(step):
    return min(1.0, (step + 1) / 4.0)


def worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    from multimodal_supernovae_amd import distributed as D
    from multimodal_supernovae_amd import optim
    from multimodal_supernovae_amd.trainer import Trainer
    D.init_from_env(backend="gloo")
    train = make_batches(rank, world)
    res = {}
    for form, optimizer, lr, graphed in (("lamb_eager", optim.LAMB, 3e-3, False), ("lars_graphed", "lars", 0.1, True)):
        model = make_model(0, optimizer, lr)
        plain = model.configure_optimizers

        def configure(plain=plain):
            cfg = plain()
            cfg["lr_scheduler"] = {"scheduler": torch.optim.lr_scheduler.LambdaLR(cfg["optimizer"], warmup), "interval": "step"}
            return cfg
        model.configure_optimizers = configure
        tr = Trainer(max_epochs=EPOCHS, graphed_steps=graphed).fit(model, train)
        torch.cuda.synchronize()
        res[form] = {"params": torch.cat([p.detach().reshape(-1) for p in model.parameters()]).cpu(),
                     "ratios": torch.cat(tr.optimizer.trust_ratios()).cpu(), "steps": tr.global_step,
                     "kind": type(tr.optimizer).__name__,
                     "replayed": tr.graphed_step is not None and tr.graphed_step.graph is not None}
    out[f"r{rank}"] = res
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    ctx = mp.get_context("spawn")
    out = ctx.Manager().dict()
    procs = [ctx.Process(target=worker, args=(r, 2, 29661, out)) for r in range(2)]
    [p.start() for p in procs]
    deadline = time.time() + 200
    while any(p.is_alive() for p in procs) and time.time() < deadline:
        if any(p.exitcode not in (None, 0) for p in procs):
            break                            # a rank failed: the other would wait in a collective
        [p.join(0.2) for p in procs]
    [p.terminate() for p in procs if p.is_alive()]
    res = dict(out)
    ok = all(p.exitcode == 0 for p in procs) and len(res) == 2
    report = {}
    if ok:
        r0, r1 = res["r0"], res["r1"]
        for key, kind, graphed in (("lamb_eager", "LAMB", False), ("lars_graphed", "LARS", True)):
            a, b = r0[key], r1[key]
            report[key] = {"params_equal": torch.equal(a["params"], b["params"]), "ratios_equal": torch.equal(a["ratios"], b["ratios"]),
                           "ratios": (int(a["ratios"].numel()), float(a["ratios"].min()), float(a["ratios"].max())),
                           "steps": (a["steps"], b["steps"]), "kind": (a["kind"], b["kind"]), "replayed": (a["replayed"], b["replayed"])}
            ok = ok and report[key]["params_equal"] and report[key]["ratios_equal"]
            ok = ok and a["steps"] == b["steps"] == EPOCHS * BATCHES and a["kind"] == b["kind"] == kind
            ok = ok and a["replayed"] == b["replayed"] == graphed
            ok = ok and a["ratios"].numel() > 0 and bool(torch.isfinite(a["ratios"]).all()) and not bool((a["ratios"] == 1.0).all())
            ok = ok and bool(torch.isfinite(a["params"]).all())
    print(report, [p.exitcode for p in procs])
    print("DIST CHECK", "OK" if ok else "FAILED")
    sys.exit(0 if ok else 1)
