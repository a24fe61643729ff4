"""Where the margins of tests/test_optim_steps_gpu.py come from: the operation order of csrc/optim_steps.hip emulated in numpy
float32 on the CPU (no GPU, no library), judged the way the test judges the kernels.

    python tools/emulate_optim_steps.py [--elements 200003] [--steps 40]

Every multiply, add, divide and square root is one numpy float32 operation (correctly rounded, as the device's are); a fused
multiply-add is formed in float64 -- the product of two float32 values is exact there -- and rounded to float32 once.  The scalars
are derived as the library derives them: in double from the exact hyper-parameters, each rounded to float32 once.  Reference:
the torch.optim class (foreach=False) in float64; yardstick: the same class in float32.  Per quantity the script prints the
largest ratio (emulated_err - floor) / yardstick_err over the checkpoints and cases, floor = one fp32 ulp of the largest
reference magnitude (2^-23 for the relative error of exp_avg_sq): the figures the docstring of the test cites.  The weights
and gradients are the seeded draws the test itself uses for its 200 003-element case.

The first moment is torch's lerp, m + (1 - beta1) (g - m).  --exp-avg product emulates m = fma(beta1, m, (1 - beta1) g) instead,
the form the RAdam kernel has: under the wide gradients it is up to 6.72x torch's max error (an entry that one large gradient of
k steps ago dominates decays by (float)beta1 each step and ends k * 2.6e-8 off), which is why the kernels do not use it."""
import argparse
import math

import numpy as np
import torch

F = np.float32
CHECK_STEPS = (1, 2, 5, 12, 40)
ADAM_HYPERS = {
    "default": dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0),
    "default_wd": dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-3),
    "fast_betas": dict(lr=1e-2, betas=(0.8, 0.9), eps=1e-6, weight_decay=1e-2),
    "large_eps": dict(lr=3e-3, betas=(0.95, 0.99), eps=1e-3, weight_decay=0.1),
    "never_rectified": dict(lr=1e-2, betas=(0.0, 0.5), eps=1e-8, weight_decay=0.0),
}
SGD_HYPERS = {
    "plain": dict(lr=1e-2, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False),
    "momentum": dict(lr=1e-2, momentum=0.9, dampening=0.0, weight_decay=0.0, nesterov=False),
    "nesterov_wd": dict(lr=1e-2, momentum=0.9, dampening=0.0, weight_decay=1e-3, nesterov=True),
    "dampening_wd": dict(lr=1e-2, momentum=0.8, dampening=0.3, weight_decay=1e-2, nesterov=False),
}


def fma(a, b, c):
    """fmaf on float32 arrays / scalars: exact product and one sum in float64, rounded to float32."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F)


class EmulatedAdam:
    product_form = False

    def __init__(self, p, lr, betas, eps, weight_decay, decoupled):
        self.p, self.m, self.v, self.t = p.astype(F), np.zeros_like(p, F), np.zeros_like(p, F), 0
        self.lr, (self.b1, self.b2), self.eps, self.wd, self.decoupled = lr, betas, eps, weight_decay, decoupled

    def step(self, g):
        self.t += 1
        b2 = F(self.b2)
        omb1, omb2, eps = F(1.0 - self.b1), F(1.0 - self.b2), F(self.eps)
        step_size = F(self.lr / (1.0 - self.b1 ** self.t))
        bc2_sqrt = F(math.sqrt(1.0 - self.b2 ** self.t))
        g = g.astype(F)
        if self.decoupled:
            self.p = self.p * F(1.0 - self.lr * self.wd)
        elif self.wd != 0:
            g = fma(F(self.wd), self.p, g)
        if self.product_form:
            self.m = fma(F(self.b1), self.m, omb1 * g)
        else:
            d = g - self.m                              # torch's lerp_, both branches, the product fused
            self.m = fma(omb1, d, self.m) if omb1 < 0.5 else fma(-(F(1.0) - omb1), d, g)
        self.v = fma(b2, self.v, (omb2 * g) * g)
        denom = np.sqrt(self.v) / bc2_sqrt + eps
        self.p = fma(-step_size, self.m / denom, self.p)

    def state(self):
        return {"p": self.p, "m": self.m, "v": self.v}


class EmulatedSGD:
    def __init__(self, p, lr, momentum, dampening, weight_decay, nesterov):
        self.p, self.buf = p.astype(F), None
        self.lr, self.mom, self.damp, self.wd, self.nesterov = lr, momentum, dampening, weight_decay, nesterov

    def step(self, g):
        g = g.astype(F)
        if self.wd != 0:
            g = fma(F(self.wd), self.p, g)
        if self.mom != 0:
            self.buf = g.copy() if self.buf is None else fma(F(self.mom), self.buf, F(1.0 - self.damp) * g)
            g = fma(F(self.mom), self.buf, g) if self.nesterov else self.buf
        self.p = fma(-F(self.lr), g, self.p)

    def state(self):
        return {"p": self.p} if self.buf is None else {"p": self.p, "b": self.buf}


def ulp32(x):
    x = abs(float(x))
    return 2.0 ** (max(math.floor(math.log2(x)), -126) - 23) if x > 0.0 else 2.0 ** -149


def judge(name, k, y, r, worst, relative=False):
    ek, ey = np.abs(k.astype(np.float64) - r), np.abs(y.astype(np.float64) - r)
    floor = ulp32(np.abs(r).max())
    checks = [("rms", math.sqrt((ek ** 2).mean()), math.sqrt((ey ** 2).mean()), floor), ("max", ek.max(), ey.max(), floor)]
    if relative:
        nz = r != 0
        checks.append(("rel", (ek[nz] / np.abs(r[nz])).max(), (ey[nz] / np.abs(r[nz])).max(), 2.0 ** -23))
    for what, a, b, fl in checks:
        over = max(a - fl, 0.0)
        ratio = over / b if b > 0 else (0.0 if over == 0 else math.inf)
        worst[f"{name}.{what}"] = max(worst.get(f"{name}.{what}", 0.0), ratio)


def run(kind, hyper, w0, grads):
    cls = {"adam": torch.optim.Adam, "adamw": torch.optim.AdamW, "sgd": torch.optim.SGD}[kind]
    y, r = torch.from_numpy(w0.copy()), torch.from_numpy(w0.astype(np.float64))
    oy, orf = cls([y], foreach=False, **hyper), cls([r], foreach=False, **hyper)
    emu = EmulatedSGD(w0, **hyper) if kind == "sgd" else EmulatedAdam(w0, decoupled=kind == "adamw", **hyper)
    keys = {"m": "exp_avg", "v": "exp_avg_sq", "b": "momentum_buffer"}
    worst = {}
    for step, g in enumerate(grads, start=1):
        emu.step(g)
        for p, opt in ((y, oy), (r, orf)):
            p.grad = torch.from_numpy(g).to(p.dtype)
            opt.step()
        if step in CHECK_STEPS:
            for name, k in emu.state().items():
                ty = y if name == "p" else oy.state[y][keys[name]]
                tr = r if name == "p" else orf.state[r][keys[name]]
                judge(name, k, ty.detach().numpy(), tr.detach().numpy(), worst, relative=(name == "v"))
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--elements", type=int, default=200003)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--exp-avg", choices=["lerp", "product"], default="lerp")
    args = ap.parse_args()
    EmulatedAdam.product_form = args.exp_avg == "product"
    # the draws of tests/test_optim_steps_gpu.py for its shape set "one" (_weights, _grads): the same inputs the kernels get
    w0 = (torch.randn((args.elements,), generator=torch.Generator().manual_seed(7)) * 0.1).numpy()
    draws = {}
    for spread, seed in (("unit", 1235), ("wide", 1335)):
        g = torch.Generator().manual_seed(seed)
        rows = []
        for _ in range(args.steps):
            u = torch.randn((args.elements,), generator=g)
            if spread == "wide":
                u = u * torch.exp(3.0 * torch.randn(u.shape, generator=g))
            rows.append(u.numpy())
        draws[spread] = rows
    unit, wide = draws["unit"], draws["wide"]
    overall = {}
    cases = [(k, h, hp) for k in ("adam", "adamw") for h, hp in ADAM_HYPERS.items()] + [("sgd", h, hp) for h, hp in SGD_HYPERS.items()]
    for kind, hname, hyper in cases:
        for gname, grads in (("unit", unit), ("wide", wide)):
            worst = run(kind, hyper, w0, grads)
            print(f"EMULATED {kind}-{hname}-{gname}: " + " ".join(f"{k}={v:.2f}" for k, v in worst.items()))
            for k, v in worst.items():
                key = (k, gname)
                overall[key] = max(overall.get(key, 0.0), v)
    for gname in ("unit", "wide"):
        print(f"WORST {gname}: " + " ".join(f"{k}={v:.2f}" for (k, g), v in sorted(overall.items()) if g == gname))


if __name__ == "__main__":
    main()
