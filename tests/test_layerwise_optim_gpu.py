"""The layer-wise adaptive optimizers (csrc/optim_layerwise.hip through optim.LAMB / LARS) against their definitions in float64, in
the form of tests/test_optim_steps_gpu.py.

Reference: `Restated`, a plain-torch restatement of the update rules written in this file (it never calls the code under test),
on float64 CPU copies of the same weights, fed the same gradients.  Yardstick: the same restatement on float32 CPU copies, with
the norms taken in float64 from the fp32 values, as the kernels take them.  Every accuracy assertion has the form

    kernel_err <= margin * yardstick_err + floor          (both errors against the float64 reference)

with floor = one fp32 ulp of the largest reference magnitude (for the relative error of exp_avg_sq: one fp32 ulp relative, 2^-23).
Judged: p, every state tensor and the trust ratios (as one vector per step, in table order).  The margins come from
tools/emulate_layerwise_steps.py, a numpy fp32 emulation of exactly the kernels' operation order (fused multiply-adds emulated
through float64, the ratio formed in double and rounded to float once) run on the CPU over the very draws, shape sets and
hyper-parameter sets below: 1.5 on RMS errors and 2.5 on max errors, the margins of tests/test_optim_steps_gpu.py, wherever the
emulation's worst figure stays within two thirds of them, and 1.5 times the emulation's worst figure elsewhere.  The emulation's
worst figures after the floor, unit / wide gradients:
    p    rms 0.00 / 0.00   max 1.00 / 1.82  -> max margin 2.73 (the worst case is LARS with Nesterov momentum on the mixed set, where
                                               the max runs over a few elements of tiny tensors whose buffers hold one large gradient)
    m    rms 0.00 / 0.00   max 0.45 / 0.22
    v    rms 0.39 / 0.00   max 0.83 / 0.80   rel 0.74 / 0.89
    b    rms 0.00 / 0.00   max 1.00 / 1.09
    r    rms 1.68 / 2.31   max 1.68 / 2.31  -> both margins 3.47.  The ratio of a step is ONE number per tensor, so its errors are
         not averaged: 1 / c1 and sqrt(c2) rounded to float move every element of u, and so ||u||, by up to an fp32 ulp in one
         direction -- as c1 and c2 rounded to float move the yardstick's, in another.  The scale of u cancels in ratio * u: p
         does not see it.
The headroom covers the device's own sqrtf and division.  No number in this file was taken from the kernels' own output.
Gradients are pre-generated from a seeded generator and do not depend on the weights.  profiles/layerwise_optim_accuracy.txt holds
the ratios measured on an MI355X.

Every accuracy case prints one line `OPTIM-ACC <case>: <quantity>=<bounded>/<raw> ...` BEFORE it asserts, the largest values over
the case's checkpoints of: bounded = (kernel_err - floor) / yardstick_err, the figure the margin bounds, and raw = kernel_err /
yardstick_err (p, m, v, b, r = parameter, exp_avg, exp_avg_sq, momentum_buffer, trust ratio; rms / max / rel).

Shapes: the smallest that reach every path of the launches -- one block covers 4096 elements per pass, a lane four consecutive
ones, and the blocks per tensor are capped at min(1024, max(32, 8192 / tensors)).  "mixed": a scalar, a tensor initialised to
zero (ratio 1 by the ||p|| > 0 rule; it must still move), a sub-vector one, two just past one block with a tail, one of several
blocks.  "one": 200 003 elements.  "capped": 256 tensors, so the cap is 32 blocks, and the first is three elements larger than 32
blocks cover in a single pass."""
import copy
import functools
import gc
import io
import math
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
RMS_MARGIN, MAX_MARGIN = 1.5, 2.5
MARGINS = {"p": (RMS_MARGIN, 2.73), "r": (3.47, 3.47)}          # (RMS, max) where the emulation leaves less headroom: see above
CHECK_STEPS = (1, 2, 5, 12, 40)
SENTINEL = 12345.0

DEFAULTS = {"lamb": dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.0, bias_correction=True, always_adapt=False,
                         trust_clip=False),
            "lars": dict(momentum=0.9, dampening=0.0, weight_decay=0.0, nesterov=False, trust_coefficient=1e-3, eps=1e-8)}
LAMB_HYPERS = {
    "wd": dict(weight_decay=1e-2),
    "no_wd": dict(weight_decay=0.0),                               # ratio exactly 1
    "always_adapt": dict(weight_decay=0.0, always_adapt=True),
    "no_bias_correction": dict(weight_decay=1e-2, bias_correction=False),
    "trust_clip": dict(weight_decay=1e-2, trust_clip=True),
    "fast_betas": dict(weight_decay=1e-2, betas=(0.8, 0.9)),
}
LARS_HYPERS = {
    "momentum": dict(lr=0.1, momentum=0.9, weight_decay=1e-4),
    "nesterov": dict(lr=0.1, momentum=0.9, weight_decay=1e-4, nesterov=True),
    "dampening": dict(lr=0.1, momentum=0.9, weight_decay=1e-4, dampening=0.3),
    "no_momentum": dict(lr=0.1, momentum=0.0, weight_decay=1e-4),
    "no_wd": dict(lr=0.1, momentum=0.9, weight_decay=0.0),          # plain SGD: test_lars_without_weight_decay_is_sgd_bit_for_bit
}
HYPERS = {"lamb": LAMB_HYPERS, "lars": LARS_HYPERS}
# (letter, state key, judged by relative error as well)
STATE = {"lamb": (("m", "exp_avg", False), ("v", "exp_avg_sq", True)), "lars": (("b", "momentum_buffer", False),)}
CAP_BLOCKS, BLOCK_ELEMS = 32, 4096                     # 256 tensors: max(32, 8192 / 256) blocks of 4096 elements per pass
SHAPE_SETS = {"mixed": [(), (5,), (7, 3), (129, 33), (4099,), (64, 384)], "one": [(200003,)],
              "capped": [(CAP_BLOCKS * BLOCK_ELEMS + 3,)] + [(3,)] * 255}
ZEROED = {"mixed": (1,)}                               # tensors of a set that start at zero
ACCURACY_CASES = [(kind, hyper) for kind in HYPERS for hyper in HYPERS[kind]]
PLUMBING = [("lamb", "wd"), ("lars", "nesterov")]      # one representative per optimizer where the arithmetic is not the point


@pytest.fixture(autouse=True)
def _leave_no_garbage():
    """Whatever cycle a test of this file leaves (optimizers, CUDA graphs, pinned tables) is collected when the test ends, outside
    any capture, and not by a collection that happens to start inside the capture of a later test."""
    yield
    gc.collect()


def _kernel(kind, groups):
    from multimodal_supernovae_amd import optim
    if kind == "lars":                                  # lr has no default: every group brings its own
        return optim.LARS(groups, lr=groups[0]["lr"])
    return optim.LAMB(groups)


def _norm64(t):
    """The 2-norm of the whole tensor in float64 from the values it holds."""
    return float(t.detach().double().pow(2).sum().sqrt())


class Restated:
    """LAMB / LARS as the issue states them, in plain torch on CPU tensors of one dtype.  groups: a list of (indices, hyper).
    state[i] holds the kernels' keys; ratios: the trust ratios of the last step in the order of the groups (Python floats)."""

    def __init__(self, kind, ps, groups):
        self.kind, self.ps = kind, ps
        self.groups = [dict(DEFAULTS[kind], idx=list(idx), **h) for idx, h in groups]
        self.state = {i: {} for G in self.groups for i in G["idx"]}
        self.ratios = []

    def step(self, grads):
        self.ratios = []
        for G in self.groups:
            for i in G["idx"]:
                if grads[i] is not None:
                    rule = self._lamb if self.kind == "lamb" else self._lars
                    self.ratios.append(rule(G, self.ps[i], grads[i].to(self.ps[i].dtype), self.state[i]))

    @staticmethod
    def _lamb(G, p, g, st):
        if not st:
            st.update(step=0, exp_avg=torch.zeros_like(p), exp_avg_sq=torch.zeros_like(p))
        st["step"] += 1
        (b1, b2), t, wd = G["betas"], st["step"], G["weight_decay"]
        c1, c2 = (1.0 - b1 ** t, 1.0 - b2 ** t) if G["bias_correction"] else (1.0, 1.0)
        m, v = st["exp_avg"], st["exp_avg_sq"]
        m.copy_(m + (1.0 - b1) * (g - m))
        v.copy_(b2 * v + (1.0 - b2) * g * g)
        u = (m / c1) / ((v / c2).sqrt() + G["eps"]) + wd * p
        pn, un = _norm64(p), _norm64(u)
        phi = pn / un if (wd != 0 or G["always_adapt"]) and pn > 0 and un > 0 else 1.0
        if G["trust_clip"]:
            phi = min(phi, 1.0)
        p.copy_(p - (G["lr"] * phi) * u)
        return phi

    @staticmethod
    def _lars(G, p, g, st):
        wd, mom = G["weight_decay"], G["momentum"]
        pn, gn = _norm64(p), _norm64(g)
        q = G["trust_coefficient"] * pn / (gn + wd * pn + G["eps"]) if wd != 0 and pn > 0 and gn > 0 else 1.0
        d = q * (g + wd * p)
        if mom != 0:
            if "momentum_buffer" not in st:
                st["momentum_buffer"] = d.clone()
            else:
                st["momentum_buffer"].copy_(mom * st["momentum_buffer"] + (1.0 - G["dampening"]) * d)
            buf = st["momentum_buffer"]
            d = d + mom * buf if G["nesterov"] else buf
        p.copy_(p - G["lr"] * d)
        return q


def _ulp32(x):
    """One fp32 ulp at magnitude x."""
    x = abs(float(x))
    return 2.0 ** (max(math.floor(math.log2(x)), -126) - 23) if x > 0.0 else 2.0 ** -149


def _flat64(ts):
    return torch.cat([t.detach().reshape(-1).cpu().double() for t in ts])


def _compare(tag, kern, yard, ref, worst, fails, relative=False):
    """kern / yard / ref: lists of tensors of one quantity (kernel fp32, yardstick fp32, reference fp64), judged as one vector."""
    k, y, r = _flat64(kern), _flat64(yard), _flat64(ref)
    assert k.shape == r.shape == y.shape and bool(torch.isfinite(k).all()) and bool(torch.isfinite(r).all()), tag
    ek, ey = (k - r).abs(), (y - r).abs()
    floor = _ulp32(r.abs().max())
    rms_margin, max_margin = MARGINS.get(tag.split("@")[0], (RMS_MARGIN, MAX_MARGIN))
    checks = [("rms", float(ek.pow(2).mean().sqrt()), float(ey.pow(2).mean().sqrt()), rms_margin, floor),
              ("max", float(ek.max()), float(ey.max()), max_margin, floor)]
    if relative:
        nz = r != 0
        if bool(nz.any()):
            checks.append(("rel", float((ek[nz] / r[nz].abs()).max()), float((ey[nz] / r[nz].abs()).max()), max_margin, 2.0 ** -23))
    for name, a, b, margin, fl in checks:
        over = max(a - fl, 0.0)
        ratio = over / b if b > 0.0 else (0.0 if over == 0.0 else math.inf)
        raw = a / b if b > 0.0 else (0.0 if a == 0.0 else math.inf)
        key = tag.split("@")[0] + "." + name
        was = worst.get(key, (0.0, 0.0))
        worst[key] = (max(was[0], ratio), max(was[1], raw))
        if not a <= margin * b + fl:
            fails.append(f"{tag} {name}: kernel {a:.3e} > {margin} * yardstick {b:.3e} + floor {fl:.1e}  (ratio {ratio:.2f})")


def _finish(case, worst, fails):
    print(f"OPTIM-ACC {case}: " + " ".join(f"{k}={v[0]:.2f}/{v[1]:.2f}" for k, v in worst.items()))
    assert not fails, f"{case}: {len(fails)} accuracy bound(s) missed\n" + "\n".join(fails[:20])


def _has(opt, p, key):
    return opt.state.get(p, {}).get(key) is not None


def _ratios(opt):
    """The trust ratios of the last step as one device vector, in launch and table order."""
    return torch.cat(opt.trust_ratios()) if opt.trust_ratios() else torch.zeros(0, device=DEV)


def judge(kind, tag, k, ok, kr, y, r, worst, fails):
    """k, ok, kr: the subject's parameters, optimizer-like state holder and ratios (the kernels: tensors on the GPU, the optimizer,
    a device vector; the emulation: the same on the CPU).  y, r: the yardstick and reference `Restated`."""
    _compare(f"p@{tag}", k, y.ps, r.ps, worst, fails)
    for i in range(len(k)):
        if len(r.state[i]) == 0:
            assert len(ok.state.get(k[i], {})) == 0, f"{tag}: parameter {i} gained state the reference does not hold"
        elif "step" in r.state[i]:
            ks = ok.state[k[i]]["step"]
            assert type(ks) is int and ks == r.state[i]["step"], (tag, i)
    for letter, key, relative in STATE[kind]:
        seen = [i for i in range(len(k)) if key in r.state[i]]
        assert [i for i in range(len(k)) if _has(ok, k[i], key)] == seen, f"{tag}: {key} held for other parameters"
        if seen:
            _compare(f"{letter}@{tag}", [ok.state[k[i]][key] for i in seen], [y.state[i][key] for i in seen],
                     [r.state[i][key] for i in seen], worst, fails, relative=relative)
    assert len(kr) == len(y.ratios) == len(r.ratios), f"{tag}: {len(kr)} trust ratios for {len(r.ratios)} tensors"
    if len(kr):
        _compare(f"r@{tag}", [kr], [torch.tensor(y.ratios, dtype=torch.float64)], [torch.tensor(r.ratios, dtype=torch.float64)],
                 worst, fails)


class Trio:
    """The kernel optimizer on the GPU, the fp32 yardstick and the fp64 reference on copies of the same weights.
    groups: None (one group with `hyper`) or a list of (indices, hyper)."""

    def __init__(self, kind, w0, hyper=None, groups=None):
        self.kind = kind
        groups = [(range(len(w0)), hyper)] if groups is None else groups
        self.k = [w.clone().to(DEV) for w in w0]
        self.ok = _kernel(kind, [dict(params=[self.k[i] for i in idx], **h) for idx, h in groups])
        self.y = Restated(kind, [w.clone() for w in w0], groups)
        self.r = Restated(kind, [w.double() for w in w0], groups)

    def step(self, grads):
        for p, g in zip(self.k, grads):
            p.grad = None if g is None else g.to(DEV, copy=True)
        self.ok.step()
        self.y.step(grads)
        self.r.step(grads)

    def edit(self, group=0, **kv):
        self.ok.param_groups[group].update(kv)
        self.y.groups[group].update(kv)
        self.r.groups[group].update(kv)

    def judge(self, tag, worst, fails):
        judge(self.kind, tag, self.k, self.ok, _ratios(self.ok), self.y, self.r, worst, fails)


@functools.lru_cache(maxsize=None)
def _grads(kind, spread, steps=40):
    """steps x tensors of gradients that depend on no weight: N(0, 1) draws ("unit"), or the same times exp(3 N(0, 1)) ("wide":
    magnitudes over some six decades inside one tensor)."""
    g = torch.Generator().manual_seed(1234 + len(SHAPE_SETS[kind]) + (100 if spread == "wide" else 0))
    out = []
    for _ in range(steps):
        row = [torch.randn(s, generator=g) for s in SHAPE_SETS[kind]]
        if spread == "wide":
            row = [u * torch.exp(3.0 * torch.randn(u.shape, generator=g)) for u in row]
        out.append(row)
    return out


def _weights(shapes, scale=0.1, seed=7, zeroed=()):
    g = torch.Generator().manual_seed(seed)
    ws = [torch.randn(s, generator=g) * scale for s in shapes]
    for i in zeroed:
        ws[i].zero_()
    return ws


def _set_weights(shapes):
    return _weights(SHAPE_SETS[shapes], zeroed=ZEROED.get(shapes, ()))


def _random_grads(shapes, steps, seed):
    g = torch.Generator().manual_seed(seed)
    return [[torch.randn(s, generator=g) for s in shapes] for _ in range(steps)]


# ---- 1. accuracy trajectories -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spread", ["unit", "wide"])
@pytest.mark.parametrize("shapes", list(SHAPE_SETS))
@pytest.mark.parametrize("kind,hyper", ACCURACY_CASES)
def test_trajectory_matches_fp64_reference(kind, hyper, shapes, spread):
    """40 steps judged after steps 1, 2, 5, 12 and 40: p, every state tensor and the trust ratios under the bound, step counts
    equal as ints.  The tensor that starts at zero has ratio 1 at step 1 and has moved after it."""
    w0 = _set_weights(shapes)
    trio = Trio(kind, w0, HYPERS[kind][hyper])
    worst, fails = {}, []
    for step, grads in enumerate(_grads(shapes, spread), start=1):
        trio.step(grads)
        if step in CHECK_STEPS:
            trio.judge(f"step{step}", worst, fails)
        if step == 1:
            for i in ZEROED.get(shapes, ()):
                assert float(_ratios(trio.ok)[i]) == 1.0 and trio.r.ratios[i] == 1.0 and bool((trio.k[i] != 0).all())
    if HYPERS[kind][hyper]["weight_decay"] == 0 and not HYPERS[kind][hyper].get("always_adapt"):
        assert bool((_ratios(trio.ok) == 1.0).all()), "weight_decay = 0 is not adapted"
    _finish(f"trajectory[{kind}-{hyper}-{shapes}-{spread}]", worst, fails)


@pytest.mark.parametrize("nesterov", [False, True])
def test_lars_without_weight_decay_is_sgd_bit_for_bit(nesterov):
    from multimodal_supernovae_amd import optim
    shapes = SHAPE_SETS["mixed"]
    w0 = _set_weights("mixed")
    a, b = [w.clone().to(DEV) for w in w0], [w.clone().to(DEV) for w in w0]
    hp = dict(lr=0.1, momentum=0.9, weight_decay=0.0, nesterov=nesterov)
    oa, ob = optim.LARS(a, **hp), optim.SGD(b, **hp)
    for gs in _random_grads(shapes, 4, seed=31):
        for p, q, g in zip(a, b, gs):
            p.grad, q.grad = g.to(DEV), g.to(DEV)
        oa.step()
        ob.step()
        for p, q in zip(a, b):
            assert torch.equal(p, q) and torch.equal(oa.state[p]["momentum_buffer"], ob.state[q]["momentum_buffer"])
        assert bool((_ratios(oa) == 1.0).all())


# ---- 2. alignment changes no bit ----------------------------------------------------------------------------------------------
SIZES = (1, 3, 4, 5, 1023, 1025, 4103, 9001)  # tail only; one quad; quads and a tail; past one block; several blocks


def _shifted(t):
    """The values of `t` in a view that starts 4 bytes into a larger 16-byte aligned buffer."""
    whole = torch.full((t.numel() + 8,), SENTINEL, dtype=torch.float32, device=DEV)
    view = whole[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4
    return view


@pytest.mark.parametrize("kind,hyper", PLUMBING)
def test_alignment_changes_no_bit(kind, hyper):
    """The same values in 16-byte aligned tensors (float4 loads) and with the parameter, the gradient or the state 4 bytes off a
    16-byte boundary (scalar loads): 5 steps, torch.equal on p, on every state tensor and on the trust ratios -- the fp64 sums
    keep their order."""
    hp = HYPERS[kind][hyper]
    shapes = [(n,) for n in SIZES]
    w0 = _weights(shapes, seed=11)
    grads = _random_grads(shapes, 5, seed=12)
    keys = [key for _, key, _ in STATE[kind]]
    runs, ratios = {}, {}
    for which in ("aligned", "p", "g", "state"):
        ps = [_shifted(w.to(DEV)) if which == "p" else w.clone().to(DEV) for w in w0]
        assert all(p.data_ptr() % 16 == (4 if which == "p" else 0) for p in ps)
        runs[which] = (ps, _kernel(kind, [dict(params=ps, **hp)]))
    for step, gs in enumerate(grads, start=1):
        for which, (ps, opt) in runs.items():
            for p, g in zip(ps, gs):
                p.grad = _shifted(g.to(DEV)) if which == "g" else g.clone().to(DEV)
            opt.step()
            ratios.setdefault(which, []).append(_ratios(opt))
            if which == "state" and step == 1:
                for p in ps:                                 # from the second step on the state lives 4 bytes off
                    for key in keys:
                        opt.state[p][key] = _shifted(opt.state[p][key])
    ref_ps, ref_opt = runs["aligned"]
    assert not bool((torch.stack(ratios["aligned"]) == 1.0).any())
    for which in ("p", "g", "state"):
        ps, opt = runs[which]
        assert torch.equal(torch.stack(ratios[which]), torch.stack(ratios["aligned"])), f"{which} misaligned: trust ratios differ"
        for i, n in enumerate(SIZES):
            assert torch.equal(ps[i], ref_ps[i]), f"{which} misaligned, {n} elements: p differs"
            for key in keys:
                assert torch.equal(opt.state[ps[i]][key], ref_opt.state[ref_ps[i]][key]), f"{which} misaligned, {n} elements: {key}"


# ---- 3. nothing else is written -----------------------------------------------------------------------------------------------
def _pack(values, lead, gap):
    """`values` copied into ONE flat device buffer at element offsets lead, lead + n0 + gap, ...; everything around and between
    them holds SENTINEL.  Returns (flat, views, mask of the sentinel positions)."""
    total = lead + sum(v.numel() + gap for v in values) + 5
    flat = torch.full((total,), SENTINEL, dtype=torch.float32, device=DEV)
    mask = torch.ones(total, dtype=torch.bool, device=DEV)
    views, off = [], lead
    for v in values:
        n = v.numel()
        view = flat[off:off + n].view(v.shape)
        view.copy_(v)
        mask[off:off + n] = False
        views.append(view)
        off += n + gap
    return flat, views, mask


@pytest.mark.parametrize("kind,hyper", PLUMBING)
def test_nothing_else_is_written(kind, hyper):
    """Parameters and gradients as slices of sentinel-filled buffers (aligned and not): the gaps hold the sentinel after every
    step and the gradients keep their bits; a parameter whose grad is None and a frozen one keep their bits and gain no state;
    the padding between the state slices stays zero."""
    hp = HYPERS[kind][hyper]
    shapes = [(5,), (7, 3), (4099,), (129, 33), (), (64,), (33,)]
    w0 = _weights(shapes, seed=21)
    grads = _random_grads(shapes, 3, seed=22)
    pflat, ps, pmask = _pack(w0, lead=4, gap=2)
    gflat, gs, gmask = _pack([torch.zeros(s) for s in shapes], lead=1, gap=0)
    assert {p.storage_offset() % 4 for p in ps} == {0, 1, 2, 3}
    ps = [p.requires_grad_(i != 6) for i, p in enumerate(ps)]                  # 6 is frozen, 5 never gets a gradient
    opt = _kernel(kind, [dict(params=ps, **hp)])
    twin = [w.clone().to(DEV) for w in w0]                                     # the same steps on plain tensors
    otwin = _kernel(kind, [dict(params=twin[:5], **hp)])
    for row in grads:
        for i in range(5):
            gs[i].copy_(row[i])
            ps[i].grad = gs[i]
            twin[i].grad = row[i].to(DEV)
        opt.step()
        otwin.step()
        assert bool((pflat[pmask] == SENTINEL).all()), "a write outside the parameters"
        assert bool((gflat[gmask] == SENTINEL).all()), "a write outside the gradients"
        assert _ratios(opt).numel() == 5 and torch.equal(_ratios(opt), _ratios(otwin))
        for i in range(5):
            assert ps[i].grad is gs[i] and torch.equal(gs[i], row[i].to(DEV)), f"gradient {i} was written"
            assert torch.equal(ps[i], twin[i]), f"parameter {i} differs from the run on plain tensors"
    for i in (5, 6):
        assert torch.equal(ps[i], w0[i].to(DEV)) and len(opt.state.get(ps[i], {})) == 0, f"parameter {i} was touched"
    flats = {opt.state[p][key]._base for p in ps[:5] for _, key, _ in STATE[kind]}
    assert len(flats) == 1
    for flat in flats:
        used = torch.zeros(flat.numel(), dtype=torch.bool, device=DEV)
        for p in ps[:5]:
            for _, key, _ in STATE[kind]:
                s = opt.state[p][key]
                used[s.storage_offset():s.storage_offset() + s.numel()] = True
        assert bool((flat[~used] == 0).all()), "a write into the padding of the state buffer"


# ---- 4. param groups ----------------------------------------------------------------------------------------------------------
SMALL = [(33,), (129, 33), (4099,), (7, 3)]
SECOND_GROUP = {"lamb": dict(lr=2e-3, betas=(0.8, 0.95), eps=1e-5, weight_decay=0.0),
                "lars": dict(lr=3e-2, momentum=0.5, weight_decay=0.0)}


@pytest.mark.parametrize("kind,hyper", PLUMBING)
def test_two_param_groups_and_an_lr_edited_between_steps(kind, hyper):
    """Two groups, the second with weight_decay = 0 (never adapted: its ratios are exactly 1); lr of the first group is halved
    before step 4 and lr of the second changes before step 7, on all three sides.  Judged after every step."""
    first = dict(HYPERS[kind][hyper], lr=1e-2) if kind == "lamb" else HYPERS[kind][hyper]
    trio = Trio(kind, _weights(SMALL, seed=41), groups=[([0, 2], first), ([1, 3], SECOND_GROUP[kind])])
    worst, fails = {}, []
    for step, gs in enumerate(_random_grads(SMALL, 10, seed=42), start=1):
        if step == 4:
            trio.edit(0, lr=0.5 * first["lr"])
        if step == 7:
            trio.edit(1, lr=1.25e-3)
        trio.step(gs)
        trio.judge(f"step{step}", worst, fails)
        per_launch = trio.ok.trust_ratios()
        assert [t.numel() for t in per_launch] == [2, 2] and bool((per_launch[1] == 1.0).all()) and not bool((per_launch[0] == 1.0).any())
    _finish(f"two_param_groups[{kind}]", worst, fails)


# ---- 5. state dict, reproducibility -------------------------------------------------------------------------------------------
def _steps(ps, opt, rows):
    out = []
    for gs in rows:
        for p, g in zip(ps, gs):
            p.grad = g.to(DEV)
        opt.step()
        out.append(_ratios(opt))
    return out


@pytest.mark.parametrize("kind,hyper", PLUMBING)
def test_own_state_dict_survives_save_and_load_and_aliases_nothing(kind, hyper):
    """3 steps, state_dict() through torch.save / torch.load(weights_only=True) into a fresh instance over copies of the weights:
    both continue for 3 steps with torch.equal (ratios included).  Loaded directly, the state aliases no tensor of the source."""
    hp = HYPERS[kind][hyper]
    w0 = _weights(SMALL, seed=91)
    grads = _random_grads(SMALL, 6, seed=92)
    keys = [key for _, key, _ in STATE[kind]]
    a = [w.clone().to(DEV) for w in w0]
    oa = _kernel(kind, [dict(params=a, **hp)])
    _steps(a, oa, grads[:3])
    buf = io.BytesIO()
    torch.save(oa.state_dict(), buf)
    buf.seek(0)
    b = [p.detach().clone() for p in a]
    ob = _kernel(kind, [dict(params=b, **hp)])
    ob.load_state_dict(torch.load(buf, weights_only=True))
    c = [p.detach().clone() for p in a]
    oc = _kernel(kind, [dict(params=c, **hp)])
    oc.load_state_dict(oa.state_dict())
    theirs = {oa.state[p][key].data_ptr() for p in a for key in keys}
    mine = {oc.state[p][key].data_ptr() for p in c for key in keys}
    assert len(mine) == len(theirs) and not (mine & theirs), "the loaded state shares storage with its source"
    ra, rb, rc = _steps(a, oa, grads[3:]), _steps(b, ob, grads[3:]), _steps(c, oc, grads[3:])
    assert torch.equal(torch.stack(ra), torch.stack(rb)) and torch.equal(torch.stack(ra), torch.stack(rc))
    for ps, opt in ((b, ob), (c, oc)):
        for p, q in zip(a, ps):
            assert torch.equal(p, q)
            for key in keys:
                assert torch.equal(oa.state[p][key], opt.state[q][key]), key
            if kind == "lamb":
                assert type(opt.state[q]["step"]) is int and opt.state[q]["step"] == oa.state[p]["step"] == 6


@pytest.mark.parametrize("kind,hyper", PLUMBING)
def test_two_runs_from_the_same_state_agree_bit_for_bit(kind, hyper):
    """No float atomics: the partial sums are added in a fixed order."""
    shapes = SHAPE_SETS["mixed"] + [(200003,)]
    w0 = _weights(shapes, seed=51)
    grads = _random_grads(shapes, 3, seed=52)
    runs = []
    for _ in range(2):
        ps = [w.clone().to(DEV) for w in w0]
        runs.append((ps, _steps(ps, _kernel(kind, [dict(params=ps, **HYPERS[kind][hyper])]), grads)))
    (pa, ra), (pb, rb) = runs
    assert all(torch.equal(p, q) for p, q in zip(pa, pb)) and torch.equal(torch.stack(ra), torch.stack(rb))
    assert bool(torch.isfinite(torch.stack(ra)).all()) and not bool((torch.stack(ra) == 1.0).any())


# ---- 6. the step recorded in a HIP graph --------------------------------------------------------------------------------------
def _capture(opt):
    """opt.step() recorded on a side stream, the way tests/test_optim_steps_gpu.py records.  A single chain of nodes.
    The garbage collector is run BEFORE the capture and held off during it, as torch.cuda.graph and trainer.GraphedTrainStep do:
    a refused capture leaves a cycle (exception -> traceback -> frame -> exception) that holds a CUDAGraph, an optimizer and its
    pinned and device buffers, and a collection that starts inside a later capture runs their destructors on a thread whose
    stream is capturing -- an allocator or runtime call that is illegal there throws out of a destructor and ends the process."""
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    tick = graph.tick = torch.zeros(1, device=DEV)     # lives as long as the graph that writes it
    side.wait_stream(torch.cuda.current_stream())
    failure = None
    gc.collect()
    was_enabled = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.stream(side):
            graph.capture_begin(capture_error_mode="thread_local")
            tick.add_(1.0)                              # a step that is refused records nothing: the graph is never empty
            try:
                opt.step()                              # recorded, not run
            except Exception as exc:                    # noqa: BLE001 -- the stream must leave capture mode before the test goes on
                failure = exc
            graph.capture_end()
    finally:
        if was_enabled:
            gc.enable()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    if failure is not None:
        try:
            raise failure
        finally:
            failure = None                              # no cycle through this frame: what the capture held dies with the test
    return graph


def _same(tag, kind, a, oa, b, ob):
    for i, (p, q) in enumerate(zip(a, b)):
        assert torch.equal(p, q), f"{tag}: p[{i}] differs by {float((p - q).abs().max()):.3e}"
        for _, key, _ in STATE[kind]:
            assert _has(oa, p, key) == _has(ob, q, key), (tag, key)
            if _has(oa, p, key):
                assert torch.equal(oa.state[p][key], ob.state[q][key]), f"{tag}: {key}[{i}]"
        if kind == "lamb":
            assert type(oa.state[p]["step"]) is int and oa.state[p]["step"] == ob.state[q]["step"], tag


@pytest.mark.parametrize("kind,hyper", PLUMBING + [("lamb", "trust_clip"), ("lars", "dampening")])
def test_recorded_step_equals_eager_steps(kind, hyper):
    """One eager step, graph_prepare(), the step captured, then 6 replays with graph_pre_replay() against 6 eager steps of a twin fed
    the same gradients: torch.equal on p, the state and the trust ratios after every replay, host step counts equal.  lr and
    weight_decay change between replays 3 and 4 on both sides; after replay 5 one eager step runs on both."""
    hp = HYPERS[kind][hyper]
    lr = hp.get("lr", 1e-3)
    shapes = [(129, 33), (4099,), (7, 3), (64, 384)]
    w0 = _weights(shapes, seed=111)
    grads = _random_grads(shapes, 8, seed=112)
    a, b = [w.clone().to(DEV) for w in w0], [w.clone().to(DEV) for w in w0]
    oa, ob = _kernel(kind, [dict(params=a, **hp)]), _kernel(kind, [dict(params=b, **hp)])
    static = [torch.zeros(s, device=DEV) for s in shapes]

    def feed(gs):
        for buf, p, q, g in zip(static, a, b, gs):
            buf.copy_(g)
            p.grad = buf
            q.grad = g.to(DEV)

    rows = iter(grads)
    feed(next(rows))
    oa.step()
    ob.step()
    _same("eager step", kind, a, oa, b, ob)
    oa.graph_prepare()
    graph = _capture(oa)
    _same("after the capture (nothing ran)", kind, a, oa, b, ob)
    for replay in range(1, 7):
        if replay == 4:
            for opt in (oa, ob):
                opt.param_groups[0].update(lr=0.37 * lr, weight_decay=0.05)
        feed(next(rows))
        oa.graph_pre_replay()
        graph.replay()
        ob.step()
        torch.cuda.synchronize()
        _same(f"replay {replay}", kind, a, oa, b, ob)
        assert torch.equal(_ratios(oa), _ratios(ob)) and _ratios(oa).numel() == len(shapes), f"replay {replay}: trust ratios"
        if replay == 5:
            feed(next(rows))
            oa.step()
            oa.graph_note_eager_step()
            ob.step()
            _same("interposed eager step", kind, a, oa, b, ob)
            assert torch.equal(_ratios(oa), _ratios(ob))
    if kind == "lamb":
        assert all(oa.state[p]["step"] == 8 for p in a)


@pytest.mark.parametrize("kind,hyper", [("lamb", "wd"), ("lars", "momentum")])
def test_capture_before_any_eager_step_is_refused(kind, hyper):
    from multimodal_supernovae_amd._lib import MsnHipError
    p = torch.zeros(1000, device=DEV, requires_grad=True)
    p.grad = torch.ones(1000, device=DEV)
    opt = _kernel(kind, [dict(params=[p], **HYPERS[kind][hyper])])
    opt.graph_prepare()
    with pytest.raises(MsnHipError, match="eager optimizer step"):
        _capture(opt)
    assert bool((p == 0).all()) and len(opt.state.get(p, {})) == 0


def test_capture_without_graph_prepare_is_refused():
    from multimodal_supernovae_amd._lib import MsnHipError
    p = torch.ones(1000, device=DEV, requires_grad=True)
    p.grad = torch.ones(1000, device=DEV)
    opt = _kernel("lars", [dict(params=[p], **LARS_HYPERS["no_momentum"])])
    with pytest.raises(MsnHipError, match="graph_prepare"):
        _capture(opt)
    assert bool((p == 1).all())


def test_lars_without_momentum_is_captured_before_any_eager_step():
    """momentum = 0: there is no state to wait for, and the scratch comes from graph_prepare().  3 replays against a twin."""
    hp = LARS_HYPERS["no_momentum"]
    w0 = _weights([(4099,), (7, 3)], seed=121)
    grads = _random_grads([(4099,), (7, 3)], 3, seed=122)
    a, b = [w.clone().to(DEV) for w in w0], [w.clone().to(DEV) for w in w0]
    oa, ob = _kernel("lars", [dict(params=a, **hp)]), _kernel("lars", [dict(params=b, **hp)])
    static = [torch.zeros_like(p) for p in a]
    for p, buf in zip(a, static):
        p.grad = buf
    oa.graph_prepare()
    graph = _capture(oa)
    for gs in grads:
        for buf, q, g in zip(static, b, gs):
            buf.copy_(g)
            q.grad = g.to(DEV)
        oa.graph_pre_replay()
        graph.replay()
        ob.step()
        torch.cuda.synchronize()
        _same("replay", "lars", a, oa, b, ob)
        assert torch.equal(_ratios(oa), _ratios(ob))
    assert not torch.equal(a[0], w0[0].to(DEV)) and all(len(oa.state.get(p, {})) == 0 for p in a)


# ---- 7. a NaN in a gradient ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,hyper", PLUMBING)
def test_a_nan_gradient_stays_in_its_tensor(kind, hyper):
    """One NaN in one gradient: that tensor's norm is NaN, the comparisons fail, its ratio is 1 and the NaN reaches p through the
    update; the other tensors step as if nothing had happened, and step() returns."""
    shapes = [(4099,), (129, 33), (7, 3)]
    w0 = _weights(shapes, seed=61)
    grads = _random_grads(shapes, 2, seed=62)
    a, b = [w.clone().to(DEV) for w in w0], [w.clone().to(DEV) for w in w0]
    oa, ob = _kernel(kind, [dict(params=a, **HYPERS[kind][hyper])]), _kernel(kind, [dict(params=b, **HYPERS[kind][hyper])])
    _steps(a, oa, grads[:1])
    _steps(b, ob, grads[:1])
    bad = [g.clone() for g in grads[1]]
    bad[1].view(-1)[777] = float("nan")
    ra, rb = _steps(a, oa, [bad])[0], _steps(b, ob, grads[1:])[0]
    torch.cuda.synchronize()
    assert float(ra[1]) == 1.0 and float(ra[0]) == float(rb[0]) and float(ra[2]) == float(rb[2])
    assert bool(torch.isnan(a[1].view(-1)[777])) and int(torch.isnan(a[1]).sum()) == 1
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and bool(torch.isfinite(a[0]).all())


# ---- 8. argument checks -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["lamb", "lars"])
def test_cpu_and_fp64_parameters_raise_at_step(kind):
    from multimodal_supernovae_amd._lib import MsnHipError
    for p in (torch.zeros(8, requires_grad=True), torch.zeros(8, device=DEV, dtype=torch.float64, requires_grad=True)):
        p.grad = torch.ones_like(p)
        opt = _kernel(kind, [dict(params=[p], **HYPERS[kind]["wd" if kind == "lamb" else "momentum"])])
        with pytest.raises(MsnHipError):
            opt.step()
        assert bool((p == 0).all())


# ---- 9. the Trainer -----------------------------------------------------------------------------------------------------------
def test_eager_fit_with_the_lamb_class_is_the_loop_by_hand():
    import test_trainer_optim_gpu as T
    from multimodal_supernovae_amd import optim
    from multimodal_supernovae_amd.trainer import Trainer
    batches = T._batches()
    base = T._model(optimizer=optim.LAMB)
    hand, fitted = copy.deepcopy(base), copy.deepcopy(base)
    oh, sh, lrs_h, losses_h = T._hand_loop(hand, batches, T.warmup)
    lrs = []
    tr = Trainer(max_epochs=T.EPOCHS).fit(T._scheduled(fitted, T._by_step(T.warmup), lrs), batches)
    assert type(tr.optimizer) is optim.LAMB and type(oh) is optim.LAMB and tr.global_step == 6
    assert lrs == lrs_h == [T.LR * f for f in (0.25, 0.5, 0.75, 1.0, 1.0, 1.0)]
    assert all(torch.equal(x, y) for x, y in zip(tr.step_losses, losses_h))
    T._bitwise(hand, oh, fitted, tr.optimizer)
    ratios = _ratios(tr.optimizer)
    assert torch.equal(ratios, _ratios(oh)) and bool(torch.isfinite(ratios).all()) and not bool((ratios == 1.0).all())


def test_graph_replayed_lars_with_a_step_interval_warmup_matches_eager():
    """Three eager warm-up calls, the capture, three replays; the lr changes in front of every replay (warmup_decay) and reaches
    the recorded launches through graph_pre_replay.  The graphed-against-eager bound of tests/test_trainer_optim_gpu.py."""
    import test_trainer_optim_gpu as T
    from multimodal_supernovae_amd import optim
    from multimodal_supernovae_amd.trainer import Trainer
    batches = T._batches()
    base = T._model(optimizer="lars")
    eager, graphed = copy.deepcopy(base), copy.deepcopy(base)
    te = Trainer(max_epochs=T.EPOCHS).fit(T._scheduled(eager, T._by_step(T.warmup_decay)), batches)
    tg = Trainer(max_epochs=T.EPOCHS, graphed_steps=True).fit(T._scheduled(graphed, T._by_step(T.warmup_decay)), batches)
    torch.cuda.synchronize()
    assert type(tg.optimizer) is optim.LARS and tg.graphed_step.graph is not None and tg.global_step == te.global_step == 6
    assert tg.optimizer.param_groups[0]["lr"] == te.optimizer.param_groups[0]["lr"] == T.LR * T.warmup_decay(6)
    for x, y in zip(te.history["train_loss"], tg.history["train_loss"]):
        assert abs(x - y) <= 1e-5 * abs(x), (te.history, tg.history)
    for (k, p), (_, q) in zip(eager.named_parameters(), graphed.named_parameters()):
        torch.testing.assert_close(q, p, rtol=1e-5, atol=1e-7, msg=lambda m: f"{k}: {m}")
    assert tg.optimizer._graph_hyper_seen[0][0] == T.LR * T.warmup_decay(5), "the last replay did not run with the scheduler's lr"
    rg, re_ = _ratios(tg.optimizer), _ratios(te.optimizer)
    assert rg.numel() == re_.numel() > 0 and bool(torch.isfinite(rg).all()) and not bool((rg == 1.0).all())


def test_two_ranks_end_with_identical_parameters_and_ratios():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "dist_check_layerwise.py")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "DIST CHECK OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
