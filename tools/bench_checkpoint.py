#!/usr/bin/env python3
"""How long one checkpoint holds the training loop, at the headline parameter set (ViT-S/8 + light-curve transformer,
bench.build_model: 21.7 M parameters plus two RAdam moments each).

One Trainer.fit of 2 + 2 R epochs whose ModelCheckpoint (default arguments: the latest file only) runs at every second epoch,
so epochs without and with a save alternate in one process (R rounds, the first pair is warm-up).  The number is the GAP: the
host clock from the end of an epoch's last step (device synchronised) to the moment the next epoch asks for its first batch
(device synchronised again) -- epoch mean, hooks, scheduler, callbacks; with a save it holds the device-to-host copies, the
serialisation, the write + fsync and the rename.  Beside it, R timings each of

    torch.save(model.state_dict(), file)                  the yardstick: a third of the bytes (no moments)
    checkpoint._plain(...)                                the device-to-host copies of a checkpoint alone
    checkpoint.atomic_save(that dict)                     serialisation + write + fsync + rename alone

Median (min .. max) of each, as text on stdout and in --out."""
import argparse
import os
import shutil
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _stats(xs):
    xs = sorted(xs)
    return f"{xs[len(xs) // 2] * 1e3:8.1f} ms ({xs[0] * 1e3:.1f} .. {xs[-1] * 1e3:.1f})"


class _TimedEpochs:
    """The same batches every epoch; notes when an epoch's last step has finished and when the next epoch begins."""

    def __init__(self, batch, steps):
        self.batch, self.steps = batch, steps
        self.ended, self.gaps = None, []

    def __len__(self):
        return self.steps

    def __iter__(self):
        torch.cuda.synchronize()
        if self.ended is not None:
            self.gaps.append(time.perf_counter() - self.ended)
        for _ in range(self.steps):
            yield self.batch
        torch.cuda.synchronize()                  # the loop has come back for more: the last step is enqueued; wait for it
        self.ended = time.perf_counter()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--steps-per-epoch", type=int, default=2)
    ap.add_argument("--dir", default=None, help="where the checkpoints are written (default: a temporary directory)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "checkpoint_bench.txt"))
    a = ap.parse_args()
    import bench
    from multimodal_supernovae_amd import _lib
    from multimodal_supernovae_amd import checkpoint as C
    from multimodal_supernovae_amd.trainer import Trainer
    _lib.require_gpu()
    device = torch.device("cuda")
    folder = a.dir or tempfile.mkdtemp(prefix="msn_ckpt_bench_")
    os.makedirs(folder, exist_ok=True)
    try:
        model = bench.build_model(device)
        data = _TimedEpochs(bench.synthetic_batch(a.batch, 0, device), a.steps_per_epoch)
        epochs = 2 + 2 * a.rounds
        cb = C.ModelCheckpoint(os.path.join(folder, "fit"), every_n_epochs=2)
        tr = Trainer(max_epochs=epochs + 1, callbacks=[cb]).fit(model, data)      # the last epoch only closes the last gap
        gaps = data.gaps[2:]                                                        # gap e follows epoch e; epochs 0, 1: warm-up
        plain, saving = gaps[0::2], gaps[1::2]
        assert len(plain) == len(saving) == a.rounds and os.path.exists(cb.best_model_path)
        ckpt_bytes = os.path.getsize(cb.best_model_path)
        params = sum(p.numel() for p in model.parameters())
        bare, copies, writes = [], [], []
        bare_path, full_path = os.path.join(folder, "bare.pt"), os.path.join(folder, "full.ckpt")
        for _ in range(a.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            torch.save(model.state_dict(), bare_path)
            t1 = time.perf_counter()
            state = {"state_dict": C._plain(dict(model.state_dict())), "optimizer_states": [C._plain(tr.optimizer.state_dict())]}
            t2 = time.perf_counter()
            C.atomic_save(state, full_path)
            t3 = time.perf_counter()
            bare.append(t1 - t0)
            copies.append(t2 - t1)
            writes.append(t3 - t2)
        bare_bytes = os.path.getsize(bare_path)
        mid = lambda xs: sorted(xs)[len(xs) // 2]
        held = mid(saving) - mid(plain)
        lines = [
            f"tools/bench_checkpoint.py: headline parameter set, {params / 1e6:.1f} M parameters (+ 2 RAdam moments each), "
            f"{torch.cuda.get_device_name(0)}, batch {a.batch}, {a.steps_per_epoch} steps per epoch, {a.rounds} alternated rounds",
            f"checkpoint file {ckpt_bytes / 1e6:.1f} MB; bare state_dict file {bare_bytes / 1e6:.1f} MB (ratio {ckpt_bytes / bare_bytes:.2f})",
            "median (min .. max):",
            f"  gap between epochs, no callback run        {_stats(plain)}",
            f"  gap between epochs, ModelCheckpoint saves  {_stats(saving)}",
            f"  -> one save holds the loop for             {held * 1e3:8.1f} ms (difference of the medians)",
            f"  torch.save(model.state_dict())             {_stats(bare)}   = {bare_bytes / mid(bare) / 1e9:.2f} GB/s",
            f"  checkpoint: device-to-host copies          {_stats(copies)}",
            f"  checkpoint: serialise + write + fsync      {_stats(writes)}   = {ckpt_bytes / mid(writes) / 1e9:.2f} GB/s",
            f"  bare torch.save x byte ratio               {mid(bare) * ckpt_bytes / bare_bytes * 1e3:8.1f} ms (what the optimizer's share of the bytes would explain)",
        ]
        text = "\n".join(lines)
        print(text)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(text + "\n")
    finally:
        if a.dir is None:
            shutil.rmtree(folder, ignore_errors=True)


if __name__ == "__main__":
    main()
