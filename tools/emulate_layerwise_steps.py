"""Where the margins of tests/test_layerwise_optim_gpu.py come from: the operation order of csrc/optim_layerwise.hip emulated in
numpy float32 on the CPU (no GPU, no library), judged the way the test judges the kernels -- by the test's own judge(), against
the test's own restatement in float64 (reference) and float32 (yardstick), over the test's own draws, shape sets and
hyper-parameter sets.

    python tools/emulate_layerwise_steps.py [--steps 40] [--shapes mixed one capped]

Every multiply, add, divide and square root is one numpy float32 operation (correctly rounded, as the device's are); a fused
multiply-add is formed in float64 -- the product of two float32 values is exact there -- and rounded to float32 once.  The scalars
are derived as the library derives them: in double from the exact hyper-parameters, each rounded to float32 once; the norms are
fp64 sums of the squared fp32 values (the order of a sum moves a norm by a few 1e-16 of itself, nothing a float sees), the ratio
is formed in double and rounded to float32 once.  Per case the script prints the largest (emulated_err - floor) / yardstick_err
over the checkpoints per quantity, and at the end the worst per quantity: the figures the docstring of the test cites."""
import argparse
import math
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import test_layerwise_optim_gpu as T  # noqa: E402

F = np.float32


def fma(a, b, c):
    """fmaf on float32 arrays / scalars: exact product and one sum in float64, rounded to float32."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F)


def tensor(a):
    """A float32 CPU tensor of an emulated quantity (numpy hands back scalars for 0-dim arrays)."""
    return torch.from_numpy(np.asarray(a, F).copy())


def norm64(x):
    return math.sqrt(float((np.asarray(x, np.float64) ** 2).sum()))


class EmulatedLAMB:
    def __init__(self, ps, lr, betas, eps, weight_decay, bias_correction, always_adapt, trust_clip):
        self.p = [p.astype(F) for p in ps]
        self.m, self.v, self.t = [np.zeros_like(p) for p in self.p], [np.zeros_like(p) for p in self.p], 0
        self.lr, (self.b1, self.b2), self.eps, self.wd = lr, betas, eps, weight_decay
        self.bc, self.aa, self.tc = bias_correction, always_adapt, trust_clip
        self.ratios = []

    def step(self, grads):
        self.t += 1
        b2, omb1, omb2, eps, lr, wd = F(self.b2), F(1.0 - self.b1), F(1.0 - self.b2), F(self.eps), F(self.lr), F(self.wd)
        c1, c2 = (1.0 - self.b1 ** self.t, 1.0 - self.b2 ** self.t) if self.bc else (1.0, 1.0)
        inv_c1, bc2_sqrt = F(1.0 / c1), F(math.sqrt(c2))
        self.ratios = []
        for i, g in enumerate(grads):
            g, p = g.astype(F), self.p[i]
            d = g - self.m[i]
            self.m[i] = fma(omb1, d, self.m[i]) if omb1 < 0.5 else fma(-(F(1.0) - omb1), d, g)
            self.v[i] = fma(b2, self.v[i], (omb2 * g) * g)
            u = (self.m[i] * inv_c1) / (np.sqrt(self.v[i]) / bc2_sqrt + eps)
            if wd != 0:
                u = fma(wd, p, u)
            pn, un = norm64(p), norm64(u)
            r = F(pn / un) if (self.wd != 0 or self.aa) and pn > 0 and un > 0 else F(1.0)
            if self.tc and r > 1:
                r = F(1.0)
            self.p[i] = fma(-(lr * r), u, p)
            self.ratios.append(float(r))

    def state(self, i):
        return {"step": self.t, "exp_avg": tensor(self.m[i]), "exp_avg_sq": tensor(self.v[i])}


class EmulatedLARS:
    def __init__(self, ps, lr, momentum, dampening, weight_decay, nesterov, trust_coefficient, eps):
        self.p, self.buf = [p.astype(F) for p in ps], [None] * len(ps)
        self.lr, self.mom, self.damp, self.wd, self.nesterov, self.tc, self.eps = (lr, momentum, dampening, weight_decay, nesterov,
                                                                                   trust_coefficient, eps)
        self.ratios = []

    def step(self, grads):
        lr, mom, omd, wd = F(self.lr), F(self.mom), F(1.0 - self.damp), F(self.wd)
        self.ratios = []
        for i, g in enumerate(grads):
            g, p = g.astype(F), self.p[i]
            pn, gn = norm64(p), norm64(g)
            q = F(self.tc * pn / (gn + self.wd * pn + self.eps)) if self.wd != 0 and pn > 0 and gn > 0 else F(1.0)
            if wd != 0:
                g = fma(wd, p, g)
            g = q * g
            if self.mom != 0:
                self.buf[i] = np.array(g, F) if self.buf[i] is None else fma(mom, self.buf[i], omd * g)
                g = fma(mom, self.buf[i], g) if self.nesterov else self.buf[i]
            self.p[i] = fma(-lr, g, p)
            self.ratios.append(float(q))

    def state(self, i):
        return {} if self.buf[i] is None else {"momentum_buffer": tensor(self.buf[i])}


def run(kind, hyper, shapes, spread, steps):
    w0 = T._set_weights(shapes)
    groups = [(range(len(w0)), hyper)]
    y, r = T.Restated(kind, [w.clone() for w in w0], groups), T.Restated(kind, [w.double() for w in w0], groups)
    full = dict(T.DEFAULTS[kind], **hyper)
    emu = (EmulatedLAMB if kind == "lamb" else EmulatedLARS)([w.numpy().copy() for w in w0], **full)
    worst, fails = {}, []
    for step, grads in enumerate(T._grads(shapes, spread)[:steps], start=1):
        emu.step([g.numpy() for g in grads])
        y.step(grads)
        r.step(grads)
        if step in T.CHECK_STEPS:
            k = [tensor(p) for p in emu.p]
            holder = types.SimpleNamespace(state={k[i]: emu.state(i) for i in range(len(k))})
            T.judge(kind, f"step{step}", k, holder, torch.tensor(emu.ratios, dtype=torch.float32), y, r, worst, fails)
    return {key: v[0] for key, v in worst.items()}, fails, (min(r.ratios), max(r.ratios))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--shapes", nargs="+", default=list(T.SHAPE_SETS))
    args = ap.parse_args()
    overall, missed = {}, 0
    for kind, hname in T.ACCURACY_CASES:
        for shapes in args.shapes:
            for spread in ("unit", "wide"):
                worst, fails, (lo, hi) = run(kind, T.HYPERS[kind][hname], shapes, spread, args.steps)
                missed += len(fails)
                print(f"EMULATED {kind}-{hname}-{shapes}-{spread}: " + " ".join(f"{k}={v:.2f}" for k, v in worst.items())
                      + f"  ratios {lo:.3g} .. {hi:.3g}" + (f"  MISSED {len(fails)}" if fails else ""))
                for k, v in worst.items():
                    overall[(k, spread)] = max(overall.get((k, spread), 0.0), v)
    for spread in ("unit", "wide"):
        print(f"WORST {spread}: " + " ".join(f"{k}={v:.2f}" for (k, s), v in sorted(overall.items()) if s == spread))
    print(f"bounds of the test missed by the emulation: {missed}")


if __name__ == "__main__":
    main()
