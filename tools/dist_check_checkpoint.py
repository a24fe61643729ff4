#!/usr/bin/env python3
"""Two ranks sharing ONE GPU (gloo transport, CUDA tensors): save, resume and early-stop through trainer.Trainer under data
parallel (checkpoint.py).  Two fresh child processes, joined with a timeout.

  * eager form (dropout 0.1) and graph-replayed form (dropout 0): one epoch saved through ModelCheckpoint, then
    fit(ckpt_path=...) into a model of another seed with a fresh optimizer, a fresh Trainer and other RNG streams, against the
    UNINTERRUPTED 2-rank run of three epochs: bitwise for the eager form (state_dict, RAdam moments and step ints, history;
    the uninterrupted run twice is bitwise equal first); within rtol 1e-5 / atol 1e-7 of the EAGER uninterrupted run for the
    graphed form (tests/test_grad_clip_gpu.py's bound for graphed against eager steps);
  * one set of files, written by rank 0 alone (the other rank's write count stays 0);
  * EarlyStopping on a value that is constant on rank 0 and improves for ever on rank 1: both ranks stop in the epoch rank 0's
    value says (a rank deciding on its own value would train on alone and wait in a collective)."""
import copy
import os
import random
import shutil
import sys
import tempfile

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B, STEPS = 8, 4                           # rows per rank and batch, batches per epoch


def make_model(seed, dropout, lr=3e-3):
    from multimodal_supernovae_amd.models_multimodal import LightCurveImageCLIP
    tk = dict(n_out=8, emb=16, heads=4, depth=2, dropout=dropout, time_norm=20583.37, agg="mean")
    sk = dict(n_out=8, emb=8, heads=2, depth=2, dropout=dropout, time_norm=17945.14, agg="mean")
    torch.manual_seed(seed)
    return LightCurveImageCLIP(enc_dim=16, nband=2, transformer_kwargs=tk, transformer_spectral_kwargs=sk,
                               combinations=["lightcurve", "spectral"], loss="softmax", lr=lr,
                               optimizer_kwargs={"weight_decay": 1e-3}).cuda().train()


def make_batches(rank, world, steps, seed):
    g = torch.Generator().manual_seed(seed)
    n = steps * world * B
    mask = torch.ones(n, 12, dtype=torch.bool)
    mask[:, 9:] = torch.rand(n, 3, generator=g) > 0.5
    full = (None, torch.randn(n, 12, generator=g), torch.rand(n, 12, generator=g) * 100, mask,
            torch.randn(n, 10, generator=g), torch.rand(n, 10, generator=g) * 6000 + 3000,
            torch.ones(n, 10, dtype=torch.bool), None, None)
    return [tuple(t[(i * world + rank) * B:(i * world + rank + 1) * B] if t is not None else None for t in full)
            for i in range(steps)]


def seed_all(seed):
    torch.manual_seed(seed)
    torch.cuda.manual_seed(seed + 1)
    random.seed(seed + 2)
    np.random.seed(seed + 3)


def snap(model, tr):
    torch.cuda.synchronize()
    opt = tr.optimizer
    states = [(opt.state[p]["step"], opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone())
              for group in opt.param_groups for p in group["params"] if len(opt.state.get(p, {}))]
    return {"state": {k: v.detach().clone() for k, v in model.state_dict().items()}, "opt": states,
            "history": copy.deepcopy(tr.history), "global_step": tr.global_step}


def bitwise(a, b):
    """None, or what differs first."""
    for k in a["state"]:
        if not torch.equal(a["state"][k], b["state"][k]):
            return f"{k}: max |difference| {float((a['state'][k].double() - b['state'][k].double()).abs().max()):.3e}"
    if len(a["opt"]) != len(b["opt"]) or not a["opt"]:
        return "optimizer state entries"
    for i, ((s1, m1, v1), (s2, m2, v2)) in enumerate(zip(a["opt"], b["opt"])):
        if type(s1) is not int or type(s2) is not int or s1 != s2:
            return f"step {i}: {s1!r} / {s2!r}"
        if not (torch.equal(m1, m2) and torch.equal(v1, v2)):
            return f"moments {i}"
    if a["history"] != b["history"] or a["global_step"] != b["global_step"]:
        return f"history {a['history']} / {b['history']}, global_step {a['global_step']} / {b['global_step']}"
    return None


def close(a, b):
    """None, or the first parameter beyond rtol 1e-5 / atol 1e-7."""
    for k in a["state"]:
        x, y = a["state"][k], b["state"][k]
        if x.is_floating_point() and not torch.allclose(y, x, rtol=1e-5, atol=1e-7):
            return f"{k}: max |difference| {float((x - y).abs().max()):.3e}"
    return None


def worker(rank, world, port, out, folder):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    from multimodal_supernovae_amd import checkpoint as C
    from multimodal_supernovae_amd import distributed as D
    from multimodal_supernovae_amd.trainer import Trainer
    D.init_from_env(backend="gloo")
    writes = []
    real_save = C.atomic_save
    C.atomic_save = lambda obj, path: (writes.append(os.path.basename(path)), real_save(obj, path))[1]
    train = make_batches(rank, world, STEPS, seed=5)

    def whole(dropout, graphed=False):
        model = make_model(0, dropout)
        seed_all(100 + rank)
        tr = Trainer(max_epochs=3, graphed_steps=graphed).fit(model, train)
        return snap(model, tr)

    def interrupted(dropout, graphed, name):
        model = make_model(0, dropout)
        seed_all(100 + rank)
        cb = C.ModelCheckpoint(os.path.join(folder, name))
        Trainer(max_epochs=1, graphed_steps=graphed, callbacks=[cb]).fit(model, train)
        files = sorted(os.listdir(os.path.join(folder, name)))     # after the callback's barrier: the file stands for every rank
        other = make_model(7 + rank, dropout)
        seed_all(999 + rank)
        tr = Trainer(max_epochs=3, graphed_steps=graphed).fit(other, train, ckpt_path=cb.best_model_path)
        replayed = tr.graphed_step is not None and tr.graphed_step.graph is not None and tr.graphed_step.calls == 2 * STEPS
        return snap(other, tr), files, replayed

    res = {}
    a = whole(0.1)
    res["eager_twice"] = bitwise(a, whole(0.1))
    b, res["eager_files"], _ = interrupted(0.1, False, "eager")
    res["eager_resumed"] = bitwise(a, b)
    ref = whole(0.0)                                                 # the eager uninterrupted run: the graphed form's reference
    res["eager0_twice"] = bitwise(ref, whole(0.0))
    g, res["graphed_files"], res["graphed_replayed"] = interrupted(0.0, True, "graphed")
    res["graphed_resumed"] = close(ref, g)
    res["graphed_steps"] = ([s for s, _, _ in g["opt"]] == [3 * STEPS] * len(ref["opt"]) and all(type(s) is int for s, _, _ in g["opt"])
                            and g["global_step"] == 3 * STEPS)
    res["graphed_history"] = max(abs(x - y) / abs(x) for x, y in zip(ref["history"]["train_loss"], g["history"]["train_loss"]))

    # early stopping: rank 0's value is constant, rank 1's own value improves at every epoch
    model = make_model(0, 0.0, lr=0.0)
    stop = C.EarlyStopping(monitor="probe", patience=2)
    epochs = []

    def log(epoch, metrics):
        epochs.append(epoch)
        model.logged["probe"] = 1.0 if rank == 0 else 1.0 / (epoch + 2)

    tr = Trainer(max_epochs=6, callbacks=[stop, C.ModelCheckpoint(os.path.join(folder, "stop"))], log_fn=log).fit(model, train[:2])
    res["stop"] = (tr.should_stop, tr.current_epoch, epochs, stop.wait_count, sorted(os.listdir(os.path.join(folder, "stop"))))
    res["writes"] = list(writes)
    out[f"r{rank}"] = res
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    ctx = mp.get_context("spawn")
    out = ctx.Manager().dict()
    folder = tempfile.mkdtemp(prefix="msn_ckpt_")
    try:
        procs = [ctx.Process(target=worker, args=(r, 2, 29631, out, folder)) for r in range(2)]
        [p.start() for p in procs]
        [p.join(400) for p in procs]
        [p.terminate() for p in procs if p.is_alive()]
    finally:
        shutil.rmtree(folder, ignore_errors=True)
    res = dict(out)
    print(res, [p.exitcode for p in procs])
    ok = all(p.exitcode == 0 for p in procs) and len(res) == 2
    one = f"epoch=0-step={STEPS}.ckpt"
    for rank in range(2):
        r = res.get(f"r{rank}")
        if not ok or r is None:
            ok = False
            break
        ok = ok and r["eager_twice"] is None and r["eager_resumed"] is None and r["eager0_twice"] is None
        ok = ok and r["graphed_resumed"] is None and r["graphed_replayed"] and r["graphed_steps"] and r["graphed_history"] <= 1e-5
        ok = ok and r["eager_files"] == [one] and r["graphed_files"] == [one]
        # rank 0 wrote every file (one per form, then one per epoch of the early-stopping run), the other rank none
        ok = ok and (r["writes"] == [one, one] + [f"epoch={e}-step={2 * (e + 1)}.ckpt" for e in range(3)] if rank == 0 else r["writes"] == [])
        ok = ok and r["stop"] == (True, 2, [0, 1, 2], 2, ["epoch=2-step=6.ckpt"])
    print("DIST CHECK", "OK" if ok else "FAILED")
    sys.exit(0 if ok else 1)
