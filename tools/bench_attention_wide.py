#!/usr/bin/env python3
"""msn_attention_fwd / bwd for heads wider than 128 (attention_wide.hip) beside the 128-wide matrix-core kernels: µs per call and
algorithmic TFLOP/s (4 B H Tq Tk s forward, 10 B H Tq Tk s backward with the recomputation).  Self-attention on a packed
(B, T, 3 emb) q | k | v buffer (ld = 3 emb, as the blocks call it), a random key mask, scale 1 / sqrt(emb).
    python tools/bench_attention_wide.py [--iters 20] [--json out.json]"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from multimodal_supernovae_amd import _lib, ops  # noqa: E402

# (B, T, emb, heads): the last one runs the 128-wide kernels, the per-flop baseline
SHAPES = [(256, 200, 512, 2), (256, 220, 256, 1), (64, 1024, 512, 2), (256, 200, 256, 2)]


def timeit(fn, iters, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    _lib.require_gpu()
    rows = []
    for B, T, E, H in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(B + T + E + H)
        qkv = torch.randn(B, T, 3 * E, device="cuda", generator=g)
        q, k, v = qkv[..., :E], qkv[..., E:2 * E], qkv[..., 2 * E:]
        mask = (torch.rand(B, T, device="cuda", generator=g) > 0.2).to(torch.uint8)
        mask[:, 0] = 1
        dout = torch.randn(B, T, E, device="cuda", generator=g)
        dqkv = torch.empty_like(qkv)
        scale = 1 / math.sqrt(E)
        out, lse = ops.attention_fwd(q, k, v, mask, H, scale)
        tf = timeit(lambda: ops.attention_fwd(q, k, v, mask, H, scale), args.iters)
        tb = timeit(lambda: ops.attention_bwd(q, k, v, mask, H, scale, out, lse, dout, dqkv[..., :E], dqkv[..., E:2 * E],
                                              dqkv[..., 2 * E:]), args.iters)
        s = E // H
        ff, fb = 4.0 * B * H * T * T * s, 10.0 * B * H * T * T * s
        row = dict(B=B, T=T, emb=E, heads=H, head_dim=s, kernels="wide" if s > 128 else "mfma<=128", fwd_us=round(tf, 1),
                   bwd_us=round(tb, 1), fwd_tflops=round(ff / tf / 1e6, 2), bwd_tflops=round(fb / tb / 1e6, 2))
        rows.append(row)
        print(f"B {B:4d} T {T:5d} emb {E:4d} heads {H}  (hd {s:3d}, {row['kernels']:9s}): fwd {tf:9.1f} us {row['fwd_tflops']:6.2f} TF/s"
              f"   bwd {tb:9.1f} us {row['bwd_tflops']:6.2f} TF/s", flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
