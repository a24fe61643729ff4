#!/usr/bin/env python3
"""Two ranks sharing ONE GPU (gloo transport, CUDA tensors): checkpoint.WeightAveraging under data parallel.  There is no
collective in the averaging: after the gradient all-reduce every rank steps to identical parameters, so the averages must be
identical BIT FOR BIT.  Two fresh child processes, joined under one deadline; the first one that fails ends the other.

  * eager form and graph-replayed form, EMA 0.9 with start_step=1, every_n_steps=2 (so the graphed form exercises the device
    word `active`): 3 epochs of 4 batches of 8 rows per rank -> 12 steps, updates after steps 3, 5, 7, 9, 11;
  * per form the two ranks' averages and parameters are compared bitwise by the parent, n_averaged on host and device is 5;
  * one checkpoint of the first epoch, written by rank 0 alone, is resumed by BOTH ranks into models of other seeds: the
    resumed ranks agree bitwise with each other, and in the eager form with the uninterrupted run (the graphed form resumes to
    the closeness checkpoint.py states, so there only the ranks are compared).

Time limit: everything runs inside one child per rank under ONE deadline (300 s, the way tools/dist_check_accumulate.py joins
its children); the rendezvous port (29651) is fixed, so two copies of the tool cannot run on one host at the same time."""
import os
import shutil
import sys
import tempfile
import time

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B, BATCHES, EPOCHS = 8, 4, 3
UPDATES = 5                               # steps 3, 5, 7, 9, 11 of 12


def make_model(seed):
    from multimodal_supernovae_amd.models_multimodal import LightCurveImageCLIP
    tk = dict(n_out=8, emb=16, heads=4, depth=2, dropout=0.0, time_norm=20583.37, agg="mean")
    sk = dict(n_out=8, emb=8, heads=2, depth=2, dropout=0.0, time_norm=17945.14, agg="mean")
    torch.manual_seed(seed)
    return LightCurveImageCLIP(enc_dim=16, nband=2, transformer_kwargs=tk, transformer_spectral_kwargs=sk,
                               combinations=["lightcurve", "spectral"], loss="softmax", lr=3e-3,
                               optimizer_kwargs={"weight_decay": 1e-3}).cuda().train()


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


def worker(rank, world, port, out, folder):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    from multimodal_supernovae_amd import checkpoint as C
    from multimodal_supernovae_amd import distributed as D
    from multimodal_supernovae_amd.trainer import Trainer
    D.init_from_env(backend="gloo")
    writes = []
    real_save = C.atomic_save
    C.atomic_save = lambda obj, path: (writes.append(os.path.basename(path)), real_save(obj, path))[1]
    train = make_batches(rank, world)

    def callback():
        return C.WeightAveraging("ema", 0.9, start_step=1, every_n_steps=2, apply_at_end=False)

    def result(model, tr, cb):
        torch.cuda.synchronize()
        aw = cb.averager
        return {"averages": torch.cat([a.reshape(-1) for a in aw.averages]).cpu(),
                "params": torch.cat([p.detach().reshape(-1) for p in model.parameters()]).cpu(),
                "n": (aw.n_averaged, aw.device_n_averaged()), "steps": tr.global_step,
                "replayed": tr.graphed_step is not None and tr.graphed_step.graph is not None}

    res = {}
    for form, graphed in (("eager", False), ("graphed", True)):
        model, cb = make_model(0), callback()
        tr = Trainer(max_epochs=EPOCHS, graphed_steps=graphed, callbacks=[cb]).fit(model, train)
        res[form] = result(model, tr, cb)
        first, cb1 = make_model(0), callback()
        mc = C.ModelCheckpoint(os.path.join(folder, form))
        Trainer(max_epochs=1, graphed_steps=graphed, callbacks=[cb1, mc]).fit(first, train)
        other, cb2 = make_model(7 + rank), callback()          # after the callback's barrier the file stands for every rank
        tr2 = Trainer(max_epochs=EPOCHS, graphed_steps=graphed, callbacks=[cb2]).fit(other, train, ckpt_path=mc.best_model_path)
        res[form + "_resumed"] = result(other, tr2, cb2)
        res[form + "_files"] = sorted(os.listdir(os.path.join(folder, form)))
    res["writes"] = list(writes)
    out[f"r{rank}"] = res
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    ctx = mp.get_context("spawn")
    out = ctx.Manager().dict()
    folder = tempfile.mkdtemp(prefix="msn_wavg_")
    try:
        procs = [ctx.Process(target=worker, args=(r, 2, 29651, out, folder)) for r in range(2)]
        [p.start() for p in procs]
        deadline = time.time() + 300
        while any(p.is_alive() for p in procs) and time.time() < deadline:
            if any(p.exitcode not in (None, 0) for p in procs):
                break                            # a rank failed: the other would wait in a collective
            [p.join(0.2) for p in procs]
        [p.terminate() for p in procs if p.is_alive()]
    finally:
        shutil.rmtree(folder, ignore_errors=True)
    res = dict(out)
    ok = all(p.exitcode == 0 for p in procs) and len(res) == 2
    report = {}
    one = f"epoch=0-step={BATCHES}.ckpt"
    if ok:
        r0, r1 = res["r0"], res["r1"]
        for key in ("eager", "graphed", "eager_resumed", "graphed_resumed"):
            a, b = r0[key], r1[key]
            report[key] = {"averages_equal": torch.equal(a["averages"], b["averages"]), "params_equal": torch.equal(a["params"], b["params"]),
                           "n": (a["n"], b["n"]), "steps": (a["steps"], b["steps"]), "replayed": (a["replayed"], b["replayed"])}
            ok = ok and report[key]["averages_equal"] and report[key]["params_equal"]
            ok = ok and a["n"] == b["n"] == (UPDATES, UPDATES) and a["steps"] == b["steps"] == EPOCHS * BATCHES
            ok = ok and a["replayed"] == b["replayed"] == key.startswith("graphed")
            ok = ok and bool(a["averages"].abs().sum() > 0)
        report["eager_resume_is_uninterrupted"] = (torch.equal(r0["eager"]["averages"], r0["eager_resumed"]["averages"])
                                                   and torch.equal(r0["eager"]["params"], r0["eager_resumed"]["params"]))
        ok = ok and report["eager_resume_is_uninterrupted"]
        report["files"] = (r0["eager_files"], r0["graphed_files"], r0["writes"], r1["writes"])
        ok = ok and r0["eager_files"] == r1["eager_files"] == [one] and r0["graphed_files"] == r1["graphed_files"] == [one]
        ok = ok and r0["writes"] == [one, one] and r1["writes"] == []       # rank 0 alone writes
    print(report, [p.exitcode for p in procs])
    print("DIST CHECK", "OK" if ok else "FAILED")
    sys.exit(0 if ok else 1)
