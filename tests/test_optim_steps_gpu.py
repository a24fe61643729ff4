"""The fused Adam / AdamW / SGD steps (csrc/optim_steps.hip through optim.Adam / AdamW / SGD) against torch's own definitions in
float64, in the form of tests/test_radam_gpu.py.

Reference: the matching torch.optim class (foreach=False) on float64 CPU copies of the same weights, fed the same gradients.
Yardstick: the same class on float32 CPU copies.  Every accuracy assertion has the form

    kernel_err <= margin * yardstick_err + floor          (both errors against the float64 reference)

with margin 1.5 on RMS errors and 2.5 on max errors, and floor = one fp32 ulp of the largest reference magnitude (for the
relative error of exp_avg_sq: one fp32 ulp relative, 2^-23), which covers a yardstick that happens to be exact.  The margins
come from tools/emulate_optim_steps.py, a numpy fp32 emulation of exactly the kernels' operation order (fused multiply-adds
emulated through float64) run on the CPU over 200 003 elements and 40 steps for the hyper-parameter sets below, with unit-normal
gradients and with unit-normal gradients times exp(3 N(0, 1)) -- the very draws of the 200 003-element case below.  After the
floor the emulated kernels stay within 0.39x (RMS; exp_avg_sq, 0.34x for p under AdamW's decay, 0.00x elsewhere) of torch fp32,
and on max errors within 1.57x (momentum_buffer under the wide gradients: torch rounds buf * momentum, the kernel fuses it),
1.00x (relative error of exp_avg_sq), 0.92x (p), 0.81x (exp_avg_sq) and 0.50x (exp_avg); the headroom covers the device's own
sqrtf and division.  exp_avg is torch's lerp with the product fused, m + (1 - beta1) (g - m): the form fma(beta1, m, (1 - beta1) g)
reaches 6.72x on exp_avg under the wide gradients (`--exp-avg product`; an entry that one large gradient of k steps ago dominates
decays by (float)beta1 each step and ends k * 2.6e-8 off) and misses the max margin, on the emulation and on the device alike.
No number in this file was taken
from the kernels' own output.  Gradients are pre-generated from a seeded generator and do not depend on the weights, so an error
cannot feed back through the gradient.  profiles/optim_steps_accuracy.txt holds the ratios measured on an MI355X.

Every accuracy case prints one line `OPTIM-ACC <case>: <quantity>=<bounded>/<raw> ...` BEFORE it asserts, the largest values over
the case's checkpoints of: bounded = (kernel_err - floor) / yardstick_err, the figure the margin bounds, and raw = kernel_err /
yardstick_err (p, m, v, b = parameter, exp_avg, exp_avg_sq, momentum_buffer; rms / max / rel = RMS, max and max relative error)."""
import functools
import io
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
RMS_MARGIN, MAX_MARGIN = 1.5, 2.5
CHECK_STEPS = (1, 2, 5, 12, 40)
SENTINEL = 12345.0

ADAM_HYPERS = {                                        # the five sets of tests/test_radam_gpu.py
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
HYPERS = {"adam": ADAM_HYPERS, "adamw": ADAM_HYPERS, "sgd": SGD_HYPERS}
TORCH = {"adam": torch.optim.Adam, "adamw": torch.optim.AdamW, "sgd": torch.optim.SGD}
NAMES = {"adam": "Adam", "adamw": "AdamW", "sgd": "SGD"}
# (letter, state key, judged by relative error as well)
STATE = {"adam": (("m", "exp_avg", False), ("v", "exp_avg_sq", True)), "adamw": (("m", "exp_avg", False), ("v", "exp_avg_sq", True)),
         "sgd": (("b", "momentum_buffer", False),)}
SHAPE_SETS = {"one": [(200003,)], "mixed": [(), (5,), (7, 3), (129, 33), (1000,), (64, 384)]}
ACCURACY_CASES = [(kind, hyper) for kind in HYPERS for hyper in HYPERS[kind]]
# one representative per update rule for the cases that are about memory and plumbing, not about the arithmetic
PLUMBING = [("adam", "default_wd"), ("adamw", "fast_betas"), ("sgd", "nesterov_wd"), ("sgd", "dampening_wd"), ("sgd", "plain")]


def _kernel(kind, groups):
    from multimodal_supernovae_amd import optim
    return getattr(optim, NAMES[kind])(groups)


def _torch(kind, groups):
    return TORCH[kind](groups, foreach=False)


def _ulp32(x):
    """One fp32 ulp at magnitude x."""
    x = abs(float(x))
    return 2.0 ** (max(math.floor(math.log2(x)), -126) - 23) if x > 0.0 else 2.0 ** -149


def _flat64(ts):
    return torch.cat([t.detach().reshape(-1).cpu().double() for t in ts])


def _compare(tag, kern, yard, ref, worst, fails, relative=False):
    """kern / yard / ref: lists of tensors of one quantity (kernel fp32, yardstick fp32, reference fp64), judged as one vector."""
    k, y, r = _flat64(kern), _flat64(yard), _flat64(ref)
    assert k.shape == r.shape == y.shape and bool(torch.isfinite(k).all()), tag
    ek, ey = (k - r).abs(), (y - r).abs()
    floor = _ulp32(r.abs().max())
    checks = [("rms", float(ek.pow(2).mean().sqrt()), float(ey.pow(2).mean().sqrt()), RMS_MARGIN, floor),
              ("max", float(ek.max()), float(ey.max()), MAX_MARGIN, floor)]
    if relative:
        nz = r != 0
        if bool(nz.any()):
            checks.append(("rel", float((ek[nz] / r[nz].abs()).max()), float((ey[nz] / r[nz].abs()).max()), MAX_MARGIN, 2.0 ** -23))
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


class Trio:
    """The kernel optimizer on the GPU, the fp32 yardstick and the fp64 reference on copies of the same weights.
    groups: None (one group with `hyper`) or a list of (indices, hyper)."""

    def __init__(self, kind, w0, hyper=None, groups=None):
        self.kind = kind
        self.k = [w.clone().to(DEV) for w in w0]
        self.y = [w.clone() for w in w0]
        self.r = [w.double() for w in w0]

        def pg(ps):
            if groups is None:
                return [dict(params=list(ps), **hyper)]
            return [dict(params=[ps[i] for i in idx], **h) for idx, h in groups]
        self.ok, self.oy, self.orf = _kernel(kind, pg(self.k)), _torch(kind, pg(self.y)), _torch(kind, pg(self.r))

    def all(self):
        return ((self.k, self.ok), (self.y, self.oy), (self.r, self.orf))

    def step(self, grads):
        for ps, opt in self.all():
            for p, g in zip(ps, grads):
                p.grad = None if g is None else g.to(device=p.device, dtype=p.dtype, copy=True)
            opt.step()

    def edit(self, group=0, **kv):
        for _, opt in self.all():
            opt.param_groups[group].update(kv)

    def judge(self, tag, worst, fails):
        """p of every parameter; every state tensor and the step count of every parameter the reference holds them for."""
        _compare(f"p@{tag}", self.k, self.y, self.r, worst, fails)
        for i, p in enumerate(self.k):
            if len(self.orf.state.get(self.r[i], {})) == 0:
                assert len(self.ok.state.get(p, {})) == 0, f"{tag}: parameter {i} gained state the reference does not hold"
            elif "step" in self.orf.state[self.r[i]]:
                ks = self.ok.state[p]["step"]
                assert type(ks) is int and ks == int(self.orf.state[self.r[i]]["step"]), (tag, i)
        for letter, key, relative in STATE[self.kind]:
            seen = [i for i, p in enumerate(self.r) if _has(self.orf, p, key)]
            assert [i for i, p in enumerate(self.k) if _has(self.ok, p, key)] == seen, f"{tag}: {key} held for other parameters"
            if seen:
                _compare(f"{letter}@{tag}", [self.ok.state[self.k[i]][key] for i in seen], [self.oy.state[self.y[i]][key] for i in seen],
                         [self.orf.state[self.r[i]][key] for i in seen], worst, fails, relative=relative)


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


def _weights(shapes, scale=0.1, seed=7):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g) * scale for s in shapes]


def _random_grads(shapes, steps, seed):
    g = torch.Generator().manual_seed(seed)
    return [[torch.randn(s, generator=g) for s in shapes] for _ in range(steps)]


# ---- 1. accuracy trajectories -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spread", ["unit", "wide"])
@pytest.mark.parametrize("shapes", list(SHAPE_SETS))
@pytest.mark.parametrize("kind,hyper", ACCURACY_CASES)
def test_trajectory_matches_fp64_reference(kind, hyper, shapes, spread):
    """40 steps judged after steps 1, 2, 5, 12 and 40: p and every state tensor under the bound, step counts equal as ints."""
    trio = Trio(kind, _weights(SHAPE_SETS[shapes]), HYPERS[kind][hyper])
    worst, fails = {}, []
    for step, grads in enumerate(_grads(shapes, spread), start=1):
        trio.step(grads)
        if step in CHECK_STEPS:
            trio.judge(f"step{step}", worst, fails)
    _finish(f"trajectory[{kind}-{hyper}-{shapes}-{spread}]", worst, fails)


# ---- 2. alignment changes no bit ----------------------------------------------------------------------------------------------
SIZES = (1, 3, 4, 5, 1023, 1025)             # scalar loop only; float4 loop only (4); both


def _shifted(t):
    """The values of `t` in a view that starts 4 bytes into a larger 16-byte aligned buffer."""
    whole = torch.full((t.numel() + 8,), SENTINEL, dtype=torch.float32, device=DEV)
    view = whole[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4
    return view


@pytest.mark.parametrize("kind,hyper", PLUMBING)
def test_alignment_changes_no_bit(kind, hyper):
    """The same values in 16-byte aligned tensors (float4 loop + scalar tail) and with the parameter, the gradient or the state
    4 bytes off a 16-byte boundary (scalar loop): 5 steps, torch.equal on p and on every state tensor."""
    hp = HYPERS[kind][hyper]
    shapes = [(n,) for n in SIZES]
    w0 = _weights(shapes, seed=11)
    grads = _random_grads(shapes, 5, seed=12)
    keys = [key for _, key, _ in STATE[kind]]
    runs = {}
    for which in ("aligned", "p", "g", "state"):
        ps = [_shifted(w.to(DEV)) if which == "p" else w.clone().to(DEV) for w in w0]
        assert all(p.data_ptr() % 16 == (4 if which == "p" else 0) for p in ps)
        runs[which] = (ps, _kernel(kind, [dict(params=ps, **hp)]))
    for step, gs in enumerate(grads, start=1):
        for which, (ps, opt) in runs.items():
            for p, g in zip(ps, gs):
                p.grad = _shifted(g.to(DEV)) if which == "g" else g.clone().to(DEV)
            opt.step()
            if which == "state" and step == 1:
                # from the second step on the state lives 4 bytes off (the first SGD step stores the buffer, the others read it)
                for p in ps:
                    for key in keys:
                        if _has(opt, p, key):
                            opt.state[p][key] = _shifted(opt.state[p][key])
                            assert opt.state[p][key].data_ptr() % 16 == 4
    ref_ps, ref_opt = runs["aligned"]
    for which in ("p", "g", "state"):
        ps, opt = runs[which]
        for i, n in enumerate(SIZES):
            assert torch.equal(ps[i], ref_ps[i]), f"{which} misaligned, {n} elements: p differs"
            for key in keys:
                assert _has(opt, ps[i], key) == _has(ref_opt, ref_ps[i], key)
                if _has(opt, ps[i], key):
                    assert torch.equal(opt.state[ps[i]][key], ref_opt.state[ref_ps[i]][key]), f"{which} misaligned, {n} elements: {key}"
    if kind != "sgd":                                   # Adam / AdamW: the state misaligned from the very first step as well
        ps = [w.clone().to(DEV) for w in w0]
        opt = _kernel(kind, [dict(params=ps, **hp)])
        for p in ps:
            opt.state[p] = {"step": 0, "exp_avg": _shifted(torch.zeros_like(p)), "exp_avg_sq": _shifted(torch.zeros_like(p))}
        for gs in grads:
            for p, g in zip(ps, gs):
                p.grad = g.clone().to(DEV)
            opt.step()
        for i, n in enumerate(SIZES):
            assert torch.equal(ps[i], ref_ps[i]), f"state misaligned from step 1, {n} elements: p differs"
            for key in keys:
                assert torch.equal(opt.state[ps[i]][key], ref_opt.state[ref_ps[i]][key]), f"state misaligned from step 1, {n}: {key}"


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
    step and the gradients keep their bits; a parameter whose grad is None and a frozen one (requires_grad=False) keep their
    bits and gain no state."""
    hp = HYPERS[kind][hyper]
    shapes = [(5,), (7, 3), (1000,), (129, 33), (), (64,), (33,)]
    w0 = _weights(shapes, seed=21)
    grads = _random_grads(shapes, 3, seed=22)
    pflat, ps, pmask = _pack(w0, lead=4, gap=1)
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
        for i in range(5):
            assert torch.equal(gs[i], row[i].to(DEV)), f"gradient {i} was written"
            assert torch.equal(ps[i], twin[i]), f"parameter {i} differs from the run on plain tensors"
    for i in (5, 6):
        assert torch.equal(ps[i], w0[i].to(DEV)) and len(opt.state.get(ps[i], {})) == 0, f"parameter {i} was touched"
    flats = {opt.state[p][key]._base for p in ps[:5] for _, key, _ in STATE[kind] if _has(opt, p, key)}
    for flat in flats:                                  # the 16-byte padding between the state slices stays zero
        used = torch.zeros(flat.numel(), dtype=torch.bool, device=DEV)
        for p in ps[:5]:
            for _, key, _ in STATE[kind]:
                s = opt.state[p][key]
                used[s.storage_offset():s.storage_offset() + s.numel()] = True
        assert bool((flat[~used] == 0).all()), "a write into the padding of the state buffer"
    assert len(flats) == (0 if hp.get("momentum", 1.0) == 0 else 1)


# ---- 4. param groups ----------------------------------------------------------------------------------------------------------
SMALL = [(33,), (129, 33), (1000,), (7, 3)]
SECOND_GROUP = {"adam": dict(lr=2e-3, betas=(0.8, 0.95), eps=1e-5, weight_decay=0.0),
                "adamw": dict(lr=2e-3, betas=(0.8, 0.95), eps=1e-5, weight_decay=0.2),
                "sgd": dict(lr=3e-3, momentum=0.5, dampening=0.0, weight_decay=0.0, nesterov=False)}


@pytest.mark.parametrize("kind,hyper", [("adam", "default_wd"), ("adamw", "default_wd"), ("sgd", "nesterov_wd")])
def test_two_param_groups_and_an_lr_edited_between_steps(kind, hyper):
    """Two groups that differ in lr, weight_decay and betas / momentum; lr of the first group is halved before step 4 and lr and
    weight_decay of the second change before step 7, on all three sides.  Judged after every step: an edit that took effect a step
    late, or never, misses the bound at once (the yardstick's error is 1e-7 of the step, the edit moves the step by half)."""
    trio = Trio(kind, _weights(SMALL, seed=41), groups=[([0, 2], HYPERS[kind][hyper]), ([1, 3], SECOND_GROUP[kind])])
    worst, fails = {}, []
    for step, gs in enumerate(_random_grads(SMALL, 10, seed=42), start=1):
        if step == 4:
            trio.edit(0, lr=0.5 * HYPERS[kind][hyper]["lr"])
        if step == 7:
            trio.edit(1, lr=1.25e-3, weight_decay=0.05)
        trio.step(gs)
        trio.judge(f"step{step}", worst, fails)
    _finish(f"two_param_groups[{kind}]", worst, fails)


# ---- 5. state dict ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,hyper", [("adam", "default_wd"), ("adamw", "default_wd"), ("sgd", "nesterov_wd")])
def test_torch_state_dict_continues_on_the_gpu(kind, hyper):
    """3 steps of the torch.optim class (fp32, CPU), its state_dict() loaded into the kernel optimizer (step arrives as a tensor, the
    moments from the CPU), 5 more steps on the GPU: judged against the uninterrupted fp64 run with the uninterrupted fp32 run as
    the yardstick, under the bound of the trajectories."""
    hp = HYPERS[kind][hyper]
    w0 = _weights(SMALL, seed=81)
    grads = _random_grads(SMALL, 8, seed=82)
    y, r = [w.clone() for w in w0], [w.double() for w in w0]
    oy, orf = _torch(kind, [dict(params=y, **hp)]), _torch(kind, [dict(params=r, **hp)])

    def pair_step(gs):
        for ps, opt in ((y, oy), (r, orf)):
            for p, g in zip(ps, gs):
                p.grad = g.to(p.dtype, copy=True)
            opt.step()
    for gs in grads[:3]:
        pair_step(gs)
    k = [p.detach().clone().to(DEV) for p in y]
    ok = _kernel(kind, [dict(params=k, **hp)])
    ok.load_state_dict(oy.state_dict())
    for p in k:
        for _, key, _ in STATE[kind]:
            assert ok.state[p][key].device.type == DEV
        if kind != "sgd":
            assert type(ok.state[p]["step"]) is int and ok.state[p]["step"] == 3
    for gs in grads[3:]:
        pair_step(gs)
        for p, g in zip(k, gs):
            p.grad = g.to(DEV)
        ok.step()
    worst, fails = {}, []
    _compare("p@end", k, y, r, worst, fails)
    for letter, key, relative in STATE[kind]:
        _compare(f"{letter}@end", [ok.state[p][key] for p in k], [oy.state[p][key] for p in y], [orf.state[p][key] for p in r],
                 worst, fails, relative=relative)
    if kind != "sgd":
        assert [ok.state[p]["step"] for p in k] == [int(orf.state[p]["step"]) for p in r] == [8] * len(k)
    _finish(f"torch_to_kernel[{kind}]", worst, fails)


@pytest.mark.parametrize("kind,hyper", PLUMBING)
def test_own_state_dict_survives_save_and_load_and_aliases_nothing(kind, hyper):
    """3 steps, state_dict() through torch.save / torch.load(weights_only=True) into a fresh instance over copies of the weights:
    both continue for 3 steps with torch.equal.  Loaded directly (no file in between), the state aliases no tensor of the source."""
    hp = HYPERS[kind][hyper]
    w0 = _weights(SMALL, seed=91)
    grads = _random_grads(SMALL, 6, seed=92)
    keys = [key for _, key, _ in STATE[kind]]
    a = [w.clone().to(DEV) for w in w0]
    oa = _kernel(kind, [dict(params=a, **hp)])
    for gs in grads[:3]:
        for p, g in zip(a, gs):
            p.grad = g.to(DEV)
        oa.step()
    buf = io.BytesIO()
    torch.save(oa.state_dict(), buf)
    buf.seek(0)
    b = [p.detach().clone() for p in a]
    ob = _kernel(kind, [dict(params=b, **hp)])
    ob.load_state_dict(torch.load(buf, weights_only=True))
    c = [p.detach().clone() for p in a]
    oc = _kernel(kind, [dict(params=c, **hp)])
    oc.load_state_dict(oa.state_dict())                 # same device, same dtype: torch's own .to() would hand back the very tensors
    theirs = {oa.state[p][key].data_ptr() for p in a for key in keys if _has(oa, p, key)}
    mine = {oc.state[p][key].data_ptr() for p in c for key in keys if _has(oc, p, key)}
    assert len(mine) == len(theirs) and not (mine & theirs), "the loaded state shares storage with its source"
    for gs in grads[3:]:
        for ps, opt in ((a, oa), (b, ob), (c, oc)):
            for p, g in zip(ps, gs):
                p.grad = g.to(DEV)
            opt.step()
    for ps, opt in ((b, ob), (c, oc)):
        for p, q in zip(a, ps):
            assert torch.equal(p, q)
            for key in keys:
                assert _has(oa, p, key) == _has(opt, q, key)
                if _has(oa, p, key):
                    assert torch.equal(oa.state[p][key], opt.state[q][key]), key
            if kind != "sgd":
                assert opt.state[q]["step"] == oa.state[p]["step"] == 6


# ---- 6. the step recorded in a HIP graph --------------------------------------------------------------------------------------
def _capture(opt):
    """opt.step() recorded on a side stream, the way tests/test_radam_gpu.py and tests/test_graph_gpu.py record RAdam.  A single
    chain of nodes: no parallel branches."""
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    tick = graph.tick = torch.zeros(1, device=DEV)     # lives as long as the graph that writes it
    side.wait_stream(torch.cuda.current_stream())
    failure = None
    with torch.cuda.stream(side):
        graph.capture_begin(capture_error_mode="thread_local")
        tick.add_(1.0)                                  # a step that is refused records nothing: the graph is never empty
        try:
            opt.step()                                  # recorded, not run
        except Exception as exc:                        # noqa: BLE001 -- the stream must leave capture mode before the test goes on
            failure = exc
        graph.capture_end()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    if failure is not None:
        raise failure
    return graph


def _same(tag, kind, a, oa, b, ob):
    for i, (p, q) in enumerate(zip(a, b)):
        assert torch.equal(p, q), f"{tag}: p[{i}] differs by {float((p - q).abs().max()):.3e}"
        for _, key, _ in STATE[kind]:
            assert _has(oa, p, key) == _has(ob, q, key), (tag, key)
            if _has(oa, p, key):
                assert torch.equal(oa.state[p][key], ob.state[q][key]), f"{tag}: {key}[{i}]"
        if kind != "sgd":
            assert type(oa.state[p]["step"]) is int and oa.state[p]["step"] == ob.state[q]["step"], tag


@pytest.mark.parametrize("kind,hyper", [("adam", "default_wd"), ("adamw", "default_wd"), ("sgd", "nesterov_wd"), ("sgd", "dampening_wd")])
def test_recorded_step_equals_eager_steps(kind, hyper):
    """One eager step, graph_prepare(), the step captured, then 6 replays with graph_pre_replay() against 6 eager steps of a twin fed
    the same gradients: torch.equal on p and the state after every replay, host step counts equal.  lr and weight_decay change
    between replays 3 and 4 on both sides; after replay 5 one eager step runs on both (graph_note_eager_step)."""
    hp = HYPERS[kind][hyper]
    shapes = [(129, 33), (1000,), (7, 3)]
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
                opt.param_groups[0].update(lr=0.37 * hp["lr"], weight_decay=0.05)
        feed(next(rows))
        oa.graph_pre_replay()
        graph.replay()
        ob.step()
        torch.cuda.synchronize()
        _same(f"replay {replay}", kind, a, oa, b, ob)
        if replay == 5:
            feed(next(rows))
            oa.step()
            oa.graph_note_eager_step()
            ob.step()
            _same("interposed eager step", kind, a, oa, b, ob)
    if kind != "sgd":
        assert all(oa.state[p]["step"] == 8 for p in a)


@pytest.mark.parametrize("kind,hyper", [("adamw", "default_wd"), ("sgd", "momentum")])
def test_capture_before_any_eager_step_is_refused(kind, hyper):
    from multimodal_supernovae_amd._lib import MsnHipError
    p = torch.zeros(1000, device=DEV, requires_grad=True)
    p.grad = torch.ones(1000, device=DEV)
    opt = _kernel(kind, [dict(params=[p], **HYPERS[kind][hyper])])
    opt.graph_prepare()
    with pytest.raises(MsnHipError, match="eager optimizer step"):
        _capture(opt)
    assert bool((p == 0).all()) and len(opt.state.get(p, {})) == 0


def test_plain_sgd_is_captured_before_any_eager_step():
    """momentum = 0: there is no state to wait for.  3 replays against a twin's eager steps."""
    hp = SGD_HYPERS["plain"]
    w0 = _weights([(1000,), (7, 3)], seed=121)
    grads = _random_grads([(1000,), (7, 3)], 3, seed=122)
    a, b = [w.clone().to(DEV) for w in w0], [w.clone().to(DEV) for w in w0]
    oa, ob = _kernel("sgd", [dict(params=a, **hp)]), _kernel("sgd", [dict(params=b, **hp)])
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
        _same("replay", "sgd", a, oa, b, ob)
    assert not torch.equal(a[0], w0[0].to(DEV)) and all(len(oa.state.get(p, {})) == 0 for p in a)


# ---- 7. argument checks -------------------------------------------------------------------------------------------------------
def test_bad_hyper_parameters_raise_at_construction():
    from multimodal_supernovae_amd import optim
    p = [torch.zeros(3, device=DEV, requires_grad=True)]
    for cls in (optim.Adam, optim.AdamW):
        for bad in (dict(lr=-1.0), dict(eps=-1e-8), dict(betas=(1.0, 0.999)), dict(betas=(0.9, -0.1)), dict(weight_decay=-0.1),
                    dict(amsgrad=True), dict(maximize=True), dict(differentiable=True)):
            with pytest.raises(ValueError):
                cls(p, **bad)
        cls(p, foreach=True, capturable=True, fused=True, amsgrad=False, maximize=False, differentiable=False)
    for bad in (dict(lr=-1.0), dict(momentum=-0.5), dict(weight_decay=-0.1), dict(nesterov=True), dict(nesterov=True, momentum=0.9, dampening=0.1),
                dict(maximize=True), dict(differentiable=True)):
        with pytest.raises(ValueError):
            optim.SGD(p, **bad)
    optim.SGD(p, momentum=0.9, nesterov=True, foreach=True, fused=False)


@pytest.mark.parametrize("kind", ["adam", "adamw", "sgd"])
def test_cpu_and_fp64_parameters_raise_at_step(kind):
    from multimodal_supernovae_amd._lib import MsnHipError
    for p in (torch.zeros(8, requires_grad=True), torch.zeros(8, device=DEV, dtype=torch.float64, requires_grad=True)):
        p.grad = torch.ones_like(p)
        opt = _kernel(kind, [dict(params=[p])])
        with pytest.raises(MsnHipError):
            opt.step()
        assert bool((p == 0).all())
