"""The fused RAdam step (csrc/optim_steps.hip through optim.RAdam) against torch's own definition in float64.

Reference: torch.optim.RAdam(foreach=False) on float64 CPU copies of the same weights, fed the same gradients.
Yardstick: the same optimiser on float32 CPU copies.  Every accuracy assertion has the form

    kernel_err <= margin * yardstick_err + floor          (both errors against the float64 reference)

with margin 1.5 on RMS errors and 2 on max errors, and floor = one fp32 ulp of the largest reference magnitude (for the
relative error of exp_avg_sq: one fp32 ulp relative, 2^-23), which covers a yardstick that happens to be exact.  The margins
come from a CPU emulation of the kernel's operation order in numpy fp32 (200 003 elements, three beta pairs, 5 / 12 / 40
steps): with the betas kept in double for the scalars and 1 - beta rounded once, the emulated kernel stayed within 1.20x (RMS)
and 1.39x (max) of torch fp32; the headroom covers the device's fused multiply-adds.  No number in this file was taken from the
kernel's own output.  Gradients are pre-generated from a seeded generator and do not depend on the weights, so an error cannot
feed back through the gradient.  profiles/radam_accuracy.txt holds the ratios measured on an MI355X.

Every case prints one line `RADAM-ACC <case>: <quantity>=<bounded>/<raw> ...` BEFORE it asserts, the largest values over the
case's checkpoints of: bounded = (kernel_err - floor) / yardstick_err, the figure the margin bounds, and raw = kernel_err /
yardstick_err (p, m, v = parameter, exp_avg, exp_avg_sq; rms / max / rel = RMS, max and max relative error)."""
import copy
import functools
import io
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
RMS_MARGIN, MAX_MARGIN = 1.5, 2.0
CHECK_STEPS = (1, 5, 6, 12, 40)          # 6 = the first rectified step with beta2 = 0.999
SENTINEL = 12345.0

HYPERS = {
    "default": dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0),
    "default_wd": dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-3),
    "fast_betas": dict(lr=1e-2, betas=(0.8, 0.9), eps=1e-6, weight_decay=1e-2),
    "large_eps": dict(lr=3e-3, betas=(0.95, 0.99), eps=1e-3, weight_decay=0.1),
    "never_rectified": dict(lr=1e-2, betas=(0.0, 0.5), eps=1e-8, weight_decay=0.0),      # rho_inf = 3 <= 5
}
SHAPE_SETS = {"one": [(200003,)], "mixed": [(), (5,), (7, 3), (129, 33), (1000,), (64, 384)]}


def _kernel_radam(groups):
    from multimodal_supernovae_amd.optim import RAdam
    return RAdam(groups)


def _torch_radam(groups):
    return torch.optim.RAdam(groups, foreach=False)


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
    print(f"RADAM-ACC {case}: " + " ".join(f"{k}={v[0]:.2f}/{v[1]:.2f}" for k, v in worst.items()))
    assert not fails, f"{case}: {len(fails)} accuracy bound(s) missed\n" + "\n".join(fails[:20])


class Trio:
    """optim.RAdam on the GPU, the fp32 yardstick and the fp64 reference on copies of the same weights.
    groups: None (one group with `hyper`) or a list of (indices, hyper)."""

    def __init__(self, w0, hyper=None, groups=None, kernel_params=None):
        self.k = kernel_params if kernel_params is not None else [w.clone().to(DEV) for w in w0]
        self.y = [w.clone() for w in w0]
        self.r = [w.double() for w in w0]

        def pg(ps):
            if groups is None:
                return [dict(params=list(ps), **hyper)]
            return [dict(params=[ps[i] for i in idx], **h) for idx, h in groups]
        self.ok, self.oy, self.orf = _kernel_radam(pg(self.k)), _torch_radam(pg(self.y)), _torch_radam(pg(self.r))

    def all(self):
        return ((self.k, self.ok), (self.y, self.oy), (self.r, self.orf))

    def set_grads(self, grads, which=None):
        for ps, opt in which or self.all():
            for p, g in zip(ps, grads):
                p.grad = None if g is None else g.to(device=p.device, dtype=p.dtype, copy=True)

    def step(self, grads):
        self.set_grads(grads)
        for _, opt in self.all():
            opt.step()

    def edit(self, group=0, **kv):
        for _, opt in self.all():
            opt.param_groups[group].update(kv)

    def judge(self, tag, worst, fails):
        """p of every parameter; exp_avg, exp_avg_sq and the step count of every parameter the reference holds state for."""
        _compare(f"p@{tag}", self.k, self.y, self.r, worst, fails)
        seen = [i for i, p in enumerate(self.r) if len(self.orf.state.get(p, {}))]
        for i, p in enumerate(self.k):
            if i not in seen:
                assert len(self.ok.state.get(p, {})) == 0, f"{tag}: parameter {i} gained state without a gradient"
        if not seen:
            return
        for i in seen:
            assert int(self.ok.state[self.k[i]]["step"]) == int(self.orf.state[self.r[i]]["step"]), (tag, i)
        for name, key in (("m", "exp_avg"), ("v", "exp_avg_sq")):
            _compare(f"{name}@{tag}", [self.ok.state[self.k[i]][key] for i in seen], [self.oy.state[self.y[i]][key] for i in seen],
                     [self.orf.state[self.r[i]][key] for i in seen], worst, fails, relative=(name == "v"))


@functools.lru_cache(maxsize=None)
def _unit_grads(kind, steps=40):
    """steps x tensors of N(0,1) draws, independent of any weight."""
    g = torch.Generator().manual_seed(1234 + len(SHAPE_SETS[kind]))
    return [[torch.randn(s, generator=g) for s in SHAPE_SETS[kind]] for _ in range(steps)]


def _weights(shapes, scale, seed=7):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g) * scale for s in shapes]


# ---- a. accuracy trajectories ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gscale", [1e-4, 1.0, 1e3])
@pytest.mark.parametrize("wscale", [0.02, 1.0])
@pytest.mark.parametrize("kind", list(SHAPE_SETS))
@pytest.mark.parametrize("hyper", list(HYPERS))
def test_trajectory_matches_fp64_reference(hyper, kind, wscale, gscale):
    """40 steps (across the rectification switch) judged after steps 1, 5, 6, 12 and 40.  The relative error of exp_avg_sq is
    the sharpest figure: with the betas handed to the kernel as floats, 1.f - 0.999f = 0.00099998713 put a systematic 1.3e-5
    into exp_avg_sq, 13 times what fp32 arithmetic gives; that version misses this bound with the default betas."""
    trio = Trio(_weights(SHAPE_SETS[kind], wscale), HYPERS[hyper])
    worst, fails = {}, []
    for step, unit in enumerate(_unit_grads(kind), start=1):
        trio.step([u * gscale for u in unit])
        if step in CHECK_STEPS:
            trio.judge(f"step{step}", worst, fails)
    _finish(f"trajectory[{hyper}-{kind}-w{wscale:g}-g{gscale:g}]", worst, fails)


# ---- b. one update, whatever the memory path ------------------------------------------------------------------------------------
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


def _intact(flat, mask):
    return bool((flat[mask] == SENTINEL).all())


def _offsets_mod4(views):
    return {v.storage_offset() % 4 for v in views}


def test_memory_path_does_not_change_a_bit():
    """The update is elementwise, so aligned tensors (float4 path), views at odd element offsets of flat buckets (scalar path;
    GradientReducer's unpadded gradient views), unaligned parameters on aligned state, and non-contiguous gradients must all give
    the same bits -- and nothing outside a tensor may be written."""
    shapes = [(5,), (7, 3), (129, 33), (1000,), (), (64, 384)]
    hyper = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-3)
    w0 = _weights(shapes, 0.02, seed=11)
    g = torch.Generator().manual_seed(12)
    grads = [[torch.randn(s, generator=g) for s in shapes] for _ in range(7)]
    zeros = [torch.zeros(s) for s in shapes]

    # (i) fresh aligned tensors
    a = [w.clone().to(DEV) for w in w0]
    oa = _kernel_radam([dict(params=a, **hyper)])
    # (ii) parameters and gradients as views of flat buffers; the state comes from _init_state (aligned slices)
    pflat, b, pmask = _pack(w0, lead=3, gap=1)
    gflat, bg, gmask = _pack(zeros, lead=1, gap=0)                   # back to back, as GradientReducer packs a bucket
    assert _offsets_mod4(b) >= {1, 2, 3} and _offsets_mod4(bg) >= {1, 2, 3}
    ob = _kernel_radam([dict(params=b, **hyper)])
    for p, gv in zip(b, bg):
        p.grad = gv
    ob._init_state([(group, group["params"]) for group in ob.param_groups])
    sflat = ob.state[b[0]]["exp_avg"]._base
    smask = torch.ones(sflat.numel(), dtype=torch.bool, device=DEV)
    for p in b:
        for key in ("exp_avg", "exp_avg_sq"):
            s = ob.state[p][key]
            assert s._base is sflat
            smask[s.storage_offset():s.storage_offset() + s.numel()] = False
    assert int(smask.sum()) > 0
    sflat[smask] = SENTINEL
    # (ii') the state at odd offsets of sentinel-filled buffers as well
    p2flat, c, p2mask = _pack(w0, lead=2, gap=3)
    g2flat, cg, g2mask = _pack(zeros, lead=3, gap=0)
    mflat, cm, mmask = _pack(zeros, lead=1, gap=2)
    vflat, cv, vmask = _pack(zeros, lead=5, gap=0)
    assert _offsets_mod4(cm) >= {1, 2, 3} and _offsets_mod4(cv) >= {1, 2, 3}
    oc = _kernel_radam([dict(params=c, **hyper)])
    for p, gv, m, v in zip(c, cg, cm, cv):
        p.grad = gv
        oc.state[p] = {"step": 0, "exp_avg": m, "exp_avg_sq": v}
    # (iii) non-contiguous gradients
    d = [w.clone().to(DEV) for w in w0]
    od = _kernel_radam([dict(params=d, **hyper)])

    guarded = [(pflat, pmask, "p"), (gflat, gmask, "g"), (sflat, smask, "state of _init_state"), (p2flat, p2mask, "p'"),
               (g2flat, g2mask, "g'"), (mflat, mmask, "m'"), (vflat, vmask, "v'")]
    for step, gs in enumerate(grads, start=1):
        for i, gi in enumerate(gs):
            gd = gi.to(DEV)
            a[i].grad = gd.clone()
            bg[i].copy_(gd)
            cg[i].copy_(gd)
            if gd.dim() == 2:
                d[i].grad = gd.t().contiguous().t()
            elif gd.dim() == 1:
                d[i].grad = torch.stack([gd, gd + 1.0], dim=1)[:, 0]
            else:
                d[i].grad = gd.clone()
            assert gd.dim() == 0 or not d[i].grad.is_contiguous() or gd.numel() == 1
        for opt in (oa, ob, oc, od):
            opt.step()
        for flat, mask, what in guarded:
            assert _intact(flat, mask), f"step {step}: a write outside the tensors of {what}"
        for i in range(len(shapes)):
            for name, ps, opt in (("views", b, ob), ("views with unaligned state", c, oc), ("non-contiguous gradients", d, od)):
                assert torch.equal(ps[i], a[i]), f"step {step}, tensor {i}: p differs on the path '{name}'"
                for key in ("exp_avg", "exp_avg_sq"):
                    assert torch.equal(opt.state[ps[i]][key], oa.state[a[i]][key]), f"step {step}, tensor {i}: {key} differs ({name})"
        assert all(int(opt.state[ps[0]]["step"]) == step for ps, opt in ((a, oa), (b, ob), (c, oc), (d, od)))
    for i in range(len(shapes)):                      # the gradients themselves are inputs: untouched
        assert torch.equal(bg[i], grads[-1][i].to(DEV)) and torch.equal(cg[i], grads[-1][i].to(DEV))


def test_large_tensor_and_tiny_tensors_in_one_launch():
    """3 * 2^20 + 5 elements: the grid (1024 blocks x 256 threads x float4) strides over it four times and leaves a scalar tail;
    the tensors of 1, 3 and 1023 elements in the same launch leave nearly every block of theirs idle.  Three steps against the
    fp64 reference; the small tensors sit between sentinels."""
    shapes = [(3 * 2 ** 20 + 5,), (), (3,), (1023,)]
    w0 = _weights(shapes, 0.02, seed=21)
    g = torch.Generator().manual_seed(22)
    big = w0[0].clone().to(DEV)
    pflat, small, pmask = _pack(w0[1:], lead=4, gap=1)            # offsets 4, 6, 10: aligned and unaligned
    gflat, small_g, gmask = _pack([torch.zeros(s) for s in shapes[1:]], lead=4, gap=1)
    trio = Trio(w0, dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-3), kernel_params=[big] + small)
    worst, fails = {}, []
    for step in range(1, 4):
        grads = [torch.randn(s, generator=g) for s in shapes]
        trio.set_grads(grads, which=trio.all()[1:])
        big.grad = grads[0].to(DEV)
        for p, gv, gi in zip(small, small_g, grads[1:]):
            gv.copy_(gi)
            p.grad = gv
        for _, opt in trio.all():
            opt.step()
        assert _intact(pflat, pmask) and _intact(gflat, gmask), f"step {step}: a write outside the small tensors"
        trio.judge(f"step{step}", worst, fails)
    sflat = trio.ok.state[big]["exp_avg"]._base              # the slices of _init_state are padded to 16 bytes with zeros
    used = torch.zeros(sflat.numel(), dtype=torch.bool, device=DEV)
    for p in trio.k:
        for key in ("exp_avg", "exp_avg_sq"):
            s = trio.ok.state[p][key]
            used[s.storage_offset():s.storage_offset() + s.numel()] = True
    assert int((~used).sum()) > 0 and bool((sflat[~used] == 0).all()), "a write into the padding of the state buffer"
    _finish("large_and_tiny", worst, fails)


# ---- c. semantics against torch --------------------------------------------------------------------------------------------------
SMALL = [(33,), (129, 33), (1000,)]


def _random_grads(shapes, steps, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return [[torch.randn(s, generator=g) * scale for s in shapes] for _ in range(steps)]


def test_parameter_without_gradient_and_late_first_gradient():
    """grad is None: the bits stay and no state appears (models_finetune.configure_optimizers relies on it).  From step 4 on the
    parameter has gradients: its own step count starts at 1 while the others are at 4 (two launches per step)."""
    w0 = _weights(SMALL, 0.02, seed=31)
    trio = Trio(w0, dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-3))
    worst, fails = {}, []
    frozen = trio.k[1].clone()
    for step, gs in enumerate(_random_grads(SMALL, 11, seed=32), start=1):
        if step <= 3:
            gs[1] = None
        trio.step(gs)
        trio.judge(f"step{step}", worst, fails)
        if step <= 3:
            assert torch.equal(trio.k[1], frozen) and trio.k[1] not in trio.ok.state
    assert [int(trio.ok.state[p]["step"]) for p in trio.k] == [11, 8, 11]
    _finish("late_first_gradient", worst, fails)


def test_two_param_groups():
    w0 = _weights(SMALL + [(7, 3)], 0.02, seed=41)
    groups = [([0, 2], dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-3)),
              ([1, 3], dict(lr=2e-3, betas=(0.8, 0.95), eps=1e-5, weight_decay=0.0))]
    trio = Trio(w0, groups=groups)
    worst, fails = {}, []
    for step, gs in enumerate(_random_grads(SMALL + [(7, 3)], 12, seed=42), start=1):
        trio.step(gs)
        trio.judge(f"step{step}", worst, fails)
    _finish("two_param_groups", worst, fails)


def test_lr_and_weight_decay_edited_between_eager_steps():
    trio = Trio(_weights(SMALL, 0.02, seed=51), dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-3))
    worst, fails = {}, []
    for step, gs in enumerate(_random_grads(SMALL, 10, seed=52), start=1):
        if step == 4:
            trio.edit(lr=5e-3)
        if step == 7:
            trio.edit(lr=1.25e-3, weight_decay=0.05)
        trio.step(gs)
        trio.judge(f"step{step}", worst, fails)
    _finish("edited_between_steps", worst, fails)


@pytest.mark.parametrize("t", [10_000, 1_000_000])
def test_one_step_from_injected_state_at_a_large_step_count(t):
    """1 / (1 - beta1^t) -> 1 and beta2^t underflows to 0: one step from the same moments at step t - 1 on every side."""
    shapes = [(1000,), (129, 33)]
    trio = Trio(_weights(shapes, 0.02, seed=61), dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-3))
    g = torch.Generator().manual_seed(62)
    for i, s in enumerate(shapes):
        m0, v0 = torch.randn(s, generator=g) * 0.1, torch.randn(s, generator=g).square() + 1e-3
        trio.ok.state[trio.k[i]] = {"step": t - 1, "exp_avg": m0.to(DEV), "exp_avg_sq": v0.to(DEV)}
        trio.oy.state[trio.y[i]] = {"step": torch.tensor(float(t - 1)), "exp_avg": m0.clone(), "exp_avg_sq": v0.clone()}
        trio.orf.state[trio.r[i]] = {"step": torch.tensor(float(t - 1), dtype=torch.float64), "exp_avg": m0.double(),
                                     "exp_avg_sq": v0.double()}
    worst, fails = {}, []
    trio.step(_random_grads(shapes, 1, seed=63)[0])
    trio.judge("step", worst, fails)
    assert all(int(trio.ok.state[p]["step"]) == t for p in trio.k)
    _finish(f"injected_state[t={t}]", worst, fails)


def test_eps_zero_with_nonzero_gradients():
    trio = Trio(_weights(SMALL, 0.02, seed=71), dict(lr=1e-2, betas=(0.9, 0.999), eps=0.0, weight_decay=0.0))
    worst, fails = {}, []
    for step, gs in enumerate(_random_grads(SMALL, 12, seed=72), start=1):
        gs = [torch.where(x >= 0, x + 0.25, x - 0.25) for x in gs]          # |g| >= 0.25: exp_avg_sq > 0 from the first step
        trio.step(gs)
        trio.judge(f"step{step}", worst, fails)
    _finish("eps_zero", worst, fails)


# ---- d. state interchange with torch.optim.RAdam ---------------------------------------------------------------------------------
def _judge_continuation(case, params, opt, trio):
    """`params` / `opt`: the continued run (fp32, any device) judged against trio's uninterrupted fp64 run, with trio's
    uninterrupted fp32 run as the yardstick."""
    worst, fails = {}, []
    _compare("p@end", params, trio.y, trio.r, worst, fails)
    for name, key in (("m", "exp_avg"), ("v", "exp_avg_sq")):
        _compare(f"{name}@end", [opt.state[p][key] for p in params], [trio.oy.state[p][key] for p in trio.y],
                 [trio.orf.state[p][key] for p in trio.r], worst, fails, relative=(name == "v"))
    assert [int(opt.state[p]["step"]) for p in params] == [int(trio.orf.state[p]["step"]) for p in trio.r]
    _finish(case, worst, fails)


class _Pair:
    """Uninterrupted fp32 (yardstick) and fp64 (reference) runs only."""

    def __init__(self, w0, hyper):
        self.y, self.r = [w.clone() for w in w0], [w.double() for w in w0]
        self.oy, self.orf = _torch_radam([dict(params=self.y, **hyper)]), _torch_radam([dict(params=self.r, **hyper)])

    def step(self, grads):
        for ps, opt in ((self.y, self.oy), (self.r, self.orf)):
            for p, g in zip(ps, grads):
                p.grad = None if g is None else g.to(p.dtype, copy=True)
            opt.step()


INTERCHANGE = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-3)


def test_torch_state_dict_continues_on_the_gpu():
    """7 steps of torch.optim.RAdam (fp32, CPU), its state_dict() loaded into optim.RAdam (step arrives as a tensor, the moments
    from the CPU), 7 more steps on the GPU."""
    pair = _Pair(_weights(SMALL, 0.02, seed=81), INTERCHANGE)
    grads = _random_grads(SMALL, 14, seed=82)
    for gs in grads[:7]:
        pair.step(gs)
    k = [p.clone().to(DEV) for p in pair.y]
    ok = _kernel_radam([dict(params=k, **INTERCHANGE)])
    ok.load_state_dict(copy.deepcopy(pair.oy.state_dict()))
    assert all(ok.state[p]["exp_avg"].device.type == DEV for p in k)
    for gs in grads[7:]:
        pair.step(gs)
        for p, g in zip(k, gs):
            p.grad = g.to(DEV)
        ok.step()
    _judge_continuation("torch_to_kernel", k, ok, pair)


def test_kernel_state_dict_continues_in_torch():
    """The reverse: 7 steps on the GPU, state_dict() (step as a Python int, moments as views of one flat buffer) loaded into
    torch.optim.RAdam on the CPU, 7 more steps there."""
    w0 = _weights(SMALL, 0.02, seed=91)
    pair = _Pair(w0, INTERCHANGE)
    grads = _random_grads(SMALL, 14, seed=92)
    k = [w.clone().to(DEV) for w in w0]
    ok = _kernel_radam([dict(params=k, **INTERCHANGE)])
    for gs in grads[:7]:
        pair.step(gs)
        for p, g in zip(k, gs):
            p.grad = g.to(DEV)
        ok.step()
    c = [p.detach().cpu().clone() for p in k]
    oc = _torch_radam([dict(params=c, **INTERCHANGE)])
    oc.load_state_dict(ok.state_dict())
    assert all(oc.state[p]["exp_avg"].device.type == "cpu" for p in c)
    for gs in grads[7:]:
        pair.step(gs)
        for p, g in zip(c, gs):
            p.grad = g.clone()
        oc.step()
    _judge_continuation("kernel_to_torch", c, oc, pair)


def test_state_dict_survives_save_and_load_into_a_fresh_instance():
    """optim.RAdam.state_dict() through torch.save / torch.load into a fresh instance; the parameter that had no gradient before
    the save gets its state through _init_state afterwards (its step count starts at 1)."""
    w0 = _weights(SMALL, 0.02, seed=101)
    pair = _Pair(w0, INTERCHANGE)
    grads = _random_grads(SMALL, 14, seed=102)
    k = [w.clone().to(DEV) for w in w0]
    ok = _kernel_radam([dict(params=k, **INTERCHANGE)])
    for gs in grads[:7]:
        gs[2] = None
        pair.step(gs)
        for p, g in zip(k, gs):
            p.grad = None if g is None else g.to(DEV)
        ok.step()
    buf = io.BytesIO()
    torch.save(ok.state_dict(), buf)
    buf.seek(0)
    k2 = [p.detach().clone() for p in k]
    ok2 = _kernel_radam([dict(params=k2, **INTERCHANGE)])
    ok2.load_state_dict(torch.load(buf))
    assert len(ok2.state.get(k2[2], {})) == 0 and torch.equal(k2[2], w0[2].to(DEV))
    for gs in grads[7:]:
        pair.step(gs)
        for p, g in zip(k2, gs):
            p.grad = g.to(DEV)
        ok2.step()
    assert [int(ok2.state[p]["step"]) for p in k2] == [14, 14, 7]
    _judge_continuation("save_load_fresh_instance", k2, ok2, pair)


# ---- e. the step recorded in a HIP graph -----------------------------------------------------------------------------------------
def test_recorded_step_follows_hyper_parameter_changes():
    """The capture interface in the order trainer.GraphedTrainStep drives it, without a model: two eager steps, graph_prepare(),
    the step captured on a side stream, then 14 replays with graph_pre_replay() before each.  lr is halved before replays 5 and
    10, weight_decay changes before replay 8, and one eager step (graph_note_eager_step) runs after replay 7.  A single chain of
    nodes: no parallel branches."""
    shapes = [(129, 33), (1000,), (7, 3)]
    hyper = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-3)
    w0 = _weights(shapes, 0.02, seed=111)
    grads = _random_grads(shapes, 17, seed=112)
    trio = Trio(w0, hyper)
    e = [w.clone().to(DEV) for w in w0]                  # an all-eager optim.RAdam run of the same schedule
    oe = _kernel_radam([dict(params=e, **hyper)])
    static = [torch.zeros(s, device=DEV) for s in shapes]
    worst, fails = {}, []
    taken = [0]

    def feed(gs):
        for ps, opt in trio.all()[1:]:
            for p, g in zip(ps, gs):
                p.grad = g.to(p.dtype, copy=True)
            opt.step()
        for buf, p, q, g in zip(static, trio.k, e, gs):
            buf.copy_(g)
            p.grad = buf
            q.grad = g.to(DEV)
        oe.step()

    def edit(**kv):
        trio.edit(**kv)
        oe.param_groups[0].update(kv)

    def eager(gs):
        feed(gs)
        trio.ok.step()
        taken[0] += 1
        trio.judge(f"step{taken[0]}", worst, fails)

    eager(grads[0])
    eager(grads[1])
    trio.ok.graph_prepare()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        graph.capture_begin(capture_error_mode="thread_local")
        trio.ok.step()                                    # recorded, not run
        graph.capture_end()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert all(int(trio.ok.state[p]["step"]) == 2 for p in trio.k)
    rest = iter(grads[2:])
    lr = hyper["lr"]
    for replay in range(1, 15):
        if replay in (5, 10):
            lr *= 0.5
            edit(lr=lr)
        if replay == 8:
            edit(weight_decay=0.05)
        feed(next(rest))
        trio.ok.graph_pre_replay()
        graph.replay()
        taken[0] += 1
        trio.judge(f"step{taken[0]}", worst, fails)
        if replay == 7:
            eager(next(rest))
            trio.ok.graph_note_eager_step()
    torch.cuda.synchronize()
    assert taken[0] == 17 and all(int(trio.ok.state[p]["step"]) == 17 for p in trio.k)
    same = all(torch.equal(p, q) and torch.equal(trio.ok.state[p]["exp_avg"], oe.state[q]["exp_avg"])
               and torch.equal(trio.ok.state[p]["exp_avg_sq"], oe.state[q]["exp_avg_sq"]) for p, q in zip(trio.k, e))
    drift = max(float((p - q).abs().max()) for p, q in zip(trio.k, e))
    print(f"RADAM-ACC recorded_step vs all-eager optim.RAdam: bit-identical={same} max |dp|={drift:.3e}")
    _compare("p_eager@end", e, trio.y, trio.r, worst, fails)      # the all-eager run under the same criterion
    _finish("recorded_step", worst, fails)
    # The device derives 1 / (1 - beta1^t) and the rectification term with its own pow: nothing promises the host's last bit.
    # On an MI355X the two runs were measured bit-identical (profiles/radam_accuracy.txt), so equality is held.
    assert same, f"the recorded steps and the eager steps differ (max |dp| = {drift:.3e})"


# ---- f. the shared plumbing (optim._FusedStep) under RAdam -----------------------------------------------------------------------
def test_class_step_equals_the_raw_c_abi_bit_for_bit():
    """optim.RAdam.step() against a loop written here that builds the {p, g, m, v, numel} table itself and calls msn_radam_step
    with the group's values, one launch per (group, step count): the argument types and the bucketing of the class.  Two param
    groups with their own lr and weight_decay; one parameter of the second group gets its first gradient at step 3, so that group
    holds two step counts and takes two launches.  The moments of the loop are separate allocations, those of the class slices
    of one buffer: alignment changes no bit (test_memory_path_does_not_change_a_bit)."""
    from multimodal_supernovae_amd._lib import check, lib, ptr, stream_ptr
    shapes = [(), (5,), (7, 3), (129, 33)]
    hypers = [dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-3), dict(lr=3e-3, betas=(0.8, 0.95), eps=1e-6, weight_decay=0.05)]
    members, late = [[0, 1], [2, 3]], 2
    w0 = _weights(shapes, 0.02, seed=121)
    a, b = [w.clone().to(DEV) for w in w0], [w.clone().to(DEV) for w in w0]
    opt = _kernel_radam([dict(params=[a[i] for i in idx], **h) for idx, h in zip(members, hypers)])
    state = {}                                           # of the loop: index -> [step, exp_avg, exp_avg_sq]
    for step, gs in enumerate(_random_grads(shapes, 6, seed=122), start=1):
        grads = [None if (i == late and step < 3) else g.to(DEV) for i, g in enumerate(gs)]
        for p, g in zip(a, grads):
            p.grad = None if g is None else g.clone()
        opt.step()
        for idx, h in zip(members, hypers):
            buckets = {}
            for i in idx:
                if grads[i] is not None:
                    st = state.setdefault(i, [0, torch.zeros_like(b[i]), torch.zeros_like(b[i])])
                    st[0] += 1
                    buckets.setdefault(st[0], []).append(i)
            for count, items in buckets.items():
                words = []
                for i in items:
                    words += [b[i].data_ptr(), grads[i].data_ptr(), state[i][1].data_ptr(), state[i][2].data_ptr(), b[i].numel()]
                table = torch.tensor(words, dtype=torch.int64).to(DEV)
                check(lib().msn_radam_step(ptr(table), len(items), max(b[i].numel() for i in items), h["lr"], h["betas"][0],
                                           h["betas"][1], h["eps"], h["weight_decay"], count, stream_ptr()), "msn_radam_step")
        torch.cuda.synchronize()
    assert [state[i][0] for i in range(4)] == [6, 6, 4, 6]
    for i in range(4):
        st = opt.state[a[i]]
        assert type(st["step"]) is int and st["step"] == state[i][0], f"tensor {i}: step {st['step']!r} against {state[i][0]}"
        assert torch.equal(a[i], b[i]), f"tensor {i}: p differs"
        assert torch.equal(st["exp_avg"], state[i][1]) and torch.equal(st["exp_avg_sq"], state[i][2]), f"tensor {i}: moments differ"


def _record_one_step(opt, params):
    """One eager step, graph_prepare(), step() recorded on a side stream.  Returns the graph."""
    g = torch.Generator().manual_seed(131)
    for p in params:
        p.grad = torch.randn(p.shape, generator=g).to(DEV)
    opt.step()
    opt.graph_prepare()
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        graph.capture_begin(capture_error_mode="thread_local")
        opt.step()                                        # recorded, not run
        graph.capture_end()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    return graph


@pytest.mark.parametrize("name", ["RAdam", "AdamW", "SGD", "LAMB", "LARS"])
def test_every_optimizer_leaves_the_same_record_of_a_recorded_launch(name):
    """_graph_launches after a recorded step: (group, [(parameter, its state)], ..., device step counter) whatever the optimizer
    -- the shape bench.py's snapshot and the accumulation tests unpack by position.  With a step count (RAdam, AdamW, LAMB) the
    device counter and the host's `step` agree after a replay that graph_pre_replay() announced."""
    from multimodal_supernovae_amd import optim
    params = [w.to(DEV) for w in _weights([(7, 3), (7, 3)], 0.02, seed=130)]
    kwargs = {"SGD": dict(momentum=0.9), "LAMB": dict(weight_decay=1e-2), "LARS": dict(weight_decay=1e-2)}.get(name, {})
    opt = getattr(optim, name)(params, lr=1e-2, **kwargs)
    graph = _record_one_step(opt, params)
    assert len(opt._graph_launches) == 1
    opt.graph_pre_replay()
    graph.replay()
    torch.cuda.synchronize()
    for entry in opt._graph_launches:
        assert isinstance(entry, tuple) and len(entry) == 6
        assert entry[0] is opt.param_groups[0]
        assert isinstance(entry[1], list) and len(entry[1]) == 2
        for (p, st), q in zip(entry[1], params):
            assert p is q and st is opt.state[q]
        counter = entry[5]
        assert counter.dtype == torch.int64 and counter.numel() == 1 and counter.device.type == DEV
        if name in ("RAdam", "AdamW", "LAMB"):
            assert int(counter) == entry[1][0][1]["step"] == 2


def test_graph_prepare_invents_no_state():
    """A parameter that never had a gradient has no entry in `state` -- torch's own rule, which state_dict() (a checkpoint) shows
    -- and graph_prepare(), which looks at every parameter of a group, must not leave an empty one behind."""
    params = [w.to(DEV) for w in _weights(SMALL, 0.02, seed=141)]
    opt = _kernel_radam([dict(params=params, **INTERCHANGE)])
    for p, g in zip(params[:2], _random_grads(SMALL[:2], 1, seed=142)[0]):
        p.grad = g.to(DEV)
    opt.step()
    opt.graph_prepare()
    assert len(opt.state) == 2 and params[2] not in opt.state
    assert len(opt.state_dict()["state"]) == 2
