"""Gradient accumulation on the GPU (optim.grad_accumulate_ / GradAccumulator, csrc/grad_accum.hip): the kernel against torch's
fp32 add bit for bit, and Trainer / GraphedTrainStep(accumulate_grad_batches=k) against Lightning's loop written by hand with
torch's own AccumulateGrad.  Shapes: the tiny two-tower model of tests/test_grad_clip_gpu.py, 8 rows per batch."""
import copy
import math
import os
import subprocess
import sys

import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu

TK = dict(n_out=8, emb=16, heads=4, depth=2, dropout=0.0, time_norm=20583.37, agg="mean")
SK = dict(n_out=8, emb=8, heads=2, depth=2, dropout=0.0, time_norm=17945.14, agg="mean")
COMBOS = ["lightcurve", "spectral"]
PASS = 4 * 256 * 4                    # elements one block covers per pass (kMtBlockElems of csrc/multi_tensor.h)
GUARD, SENTINEL = 8, -12345.0         # floats in front of and behind every tensor that no launch may touch


def _cap(n_tensors):
    """Blocks per tensor of a table of n_tensors (the cap of mt_grid_x, csrc/multi_tensor.h)."""
    return min(1024, max(32, 8192 // n_tensors))


def _buffers(sizes, misaligned, seed, scale=1.0):
    """One (whole buffer, view) per size: the view starts GUARD floats in (16-byte aligned), or GUARD + 1 floats in (4 bytes off
    a 16-byte boundary) for the indices in `misaligned`; the guard words hold SENTINEL."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for i, n in enumerate(sizes):
        off = GUARD + (1 if i in misaligned else 0)
        whole = torch.full((n + 2 * GUARD + 1,), SENTINEL)
        whole[off:off + n] = torch.randn(n, generator=g) * scale
        whole = whole.cuda()
        out.append((whole, whole[off:off + n], off))
    return out


def _same_bits(got, want):
    got, want = got.cpu(), want.cpu()
    nan = torch.isnan(want)
    return torch.equal(torch.isnan(got), nan) and torch.equal(got[~nan].view(torch.int32), want[~nan].view(torch.int32))


def _guards_intact(bufs):
    for whole, view, off in bufs:
        n = view.numel()
        if not (bool((whole[:off] == SENTINEL).all()) and bool((whole[off + n:] == SENTINEL).all())):
            return False
    return True


def _tables():
    sizes = [1, 3, 4, 5, PASS - 1, PASS, PASS + 1, 2 * PASS + 7, 1023, 4097] + [17 + 13 * i for i in range(29)]
    sizes.append(_cap(len(sizes) + 1) * PASS + PASS + 5)          # longer than the cap times a pass: every block loops
    small = [1 + (7 * i) % 61 for i in range(300)] + [300_001]    # the cap at its minimum (32): 32 passes < 300 001 elements
    assert len(sizes) == 40 and sizes[-1] > _cap(40) * PASS and _cap(len(small)) == 32 and small[-1] > 32 * PASS
    return {"forty": (sizes, {"g": {8}, "acc": {9}}), "small": (small, {"g": {5}, "acc": {300}})}


@pytest.mark.parametrize("which", ["forty", "small"])
def test_kernel_is_torch_fp32_add_bit_for_bit(which):
    from multimodal_supernovae_amd import optim
    sizes, mis = _tables()[which]
    special = len(sizes) - 1 if which == "forty" else 300           # the largest tensor carries the planted values
    acc = _buffers(sizes, mis["acc"], seed=1)
    third = _buffers(sizes, set(), seed=2)
    assert acc[min(mis["acc"])][1].data_ptr() % 16 == 4
    rounds = []
    for r in range(5):
        g = _buffers(sizes, mis["g"], seed=10 + r, scale=10.0 ** (r - 2))
        assert g[min(mis["g"])][1].data_ptr() % 16 == 4
        v = g[special][1]
        if r == 0:
            v[0], v[1], v[2], v[3], v[PASS + 1] = math.nan, math.inf, -math.inf, 1e-40, -math.inf
        if r == 1:
            v[1], v[2], v[3], v[7] = math.inf, math.inf, 1e-40, math.inf       # inf + inf, -inf + inf = NaN, denormal + denormal
        rounds.append(g)
    a_views, t_views = [a for _, a, _ in acc], [t for _, t, _ in third]
    # store, then three adds with fresh gradients, each into the accumulator itself
    optim.grad_accumulate_(a_views, a_views, [g for _, g, _ in rounds[0]], add=False)
    want = [g.cpu().clone() for _, g, _ in rounds[0]]
    for a, w in zip(a_views, want):
        assert _same_bits(a, w)
    for r in (1, 2, 3):
        optim.grad_accumulate_(a_views, a_views, [g for _, g, _ in rounds[r]], add=True)
        want = [w + g.cpu() for w, (_, g, _) in zip(want, rounds[r])]       # torch's fp32 add on the CPU
        for i, (a, w) in enumerate(zip(a_views, want)):
            assert _same_bits(a, w), (r, i, sizes[i])
    sp = a_views[special].cpu()
    assert math.isnan(float(sp[0])) and float(sp[1]) == math.inf and math.isnan(float(sp[2])) and float(sp[7]) == math.inf
    assert 0.0 < float(rounds[0][special][1][3]) < 1.2e-38 and float(sp[PASS + 1]) == -math.inf
    # dst = a third buffer: the accumulator stays as it is
    before = [a.clone() for a in a_views]
    optim.grad_accumulate_(t_views, a_views, [g for _, g, _ in rounds[4]], add=True)
    for i, (t, a, b, w, (_, g, _)) in enumerate(zip(t_views, a_views, before, want, rounds[4])):
        assert _same_bits(a, b), i
        assert _same_bits(t, w + g.cpu()), i
    # dst = the gradient itself (what the optimizer reads)
    gs = [g.clone() for _, g, _ in rounds[4]]
    optim.grad_accumulate_(gs, a_views, gs, add=True)
    for i, (x, w, (_, g, _)) in enumerate(zip(gs, want, rounds[4])):
        assert _same_bits(x, w + g.cpu()), i
    torch.cuda.synchronize()
    assert _guards_intact(acc) and _guards_intact(third) and all(_guards_intact(g) for g in rounds)


def test_selector_from_device_memory_and_late_first_gradients():
    from multimodal_supernovae_amd import optim
    sizes = [5, PASS + 3, 70_000]
    acc, g1, g2 = _buffers(sizes, {1}, seed=3), _buffers(sizes, set(), seed=4), _buffers(sizes, {2}, seed=5)
    a = [x for _, x, _ in acc]
    word = torch.zeros(1, dtype=torch.int32, device="cuda")
    optim.grad_accumulate_(a, a, [x for _, x, _ in g1], add=True, add_dev=word)         # the device word says store
    for x, (_, g, _) in zip(a, g1):
        assert _same_bits(x, g)
    word.fill_(1)
    optim.grad_accumulate_(a, a, [x for _, x, _ in g2], add=False, add_dev=word)        # ... and now add
    want = [g.cpu() + h.cpu() for (_, g, _), (_, h, _) in zip(g1, g2)]
    for x, w in zip(a, want):
        assert _same_bits(x, w)
    # a tensor whose first gradient of the window comes late (acc None) is stored while the others are added
    optim.grad_accumulate_(a, [a[0], None, a[2]], [x for _, x, _ in g1], add=True)
    assert _same_bits(a[0], want[0] + g1[0][1].cpu()) and _same_bits(a[1], g1[1][1]) and _same_bits(a[2], want[2] + g1[2][1].cpu())
    torch.cuda.synchronize()
    assert _guards_intact(acc) and _guards_intact(g1) and _guards_intact(g2)


def test_python_side_refuses_what_the_kernel_cannot_take():
    from multimodal_supernovae_amd import _lib, optim
    a, g = torch.zeros(8, device="cuda"), torch.ones(8, device="cuda")
    with pytest.raises(_lib.MsnHipError, match="float32"):
        optim.grad_accumulate_([a], [a], [g.double()])
    with pytest.raises(_lib.MsnHipError, match="contiguous"):
        optim.grad_accumulate_([a[::2]], [a[::2]], [g[::2]])
    with pytest.raises(_lib.MsnHipError):
        optim.grad_accumulate_([a], [a], [g.cpu()])
    with pytest.raises(_lib.MsnHipError, match="same number"):
        optim.grad_accumulate_([a], [a], [g[:4]])
    p, q = torch.zeros(6, device="cuda", requires_grad=True), torch.zeros(3, device="cuda", requires_grad=True)
    acc = optim.GradAccumulator([p, q])
    p.grad = torch.full((6,), 1.0, device="cuda")
    acc.accumulate(False)                                   # q has no gradient: it contributes nothing
    assert acc.have == {p}
    p.grad, q.grad = torch.full((6,), 2.0, device="cuda"), torch.full((3,), 5.0, device="cuda")
    acc.accumulate(False)                                   # q's first gradient comes late: stored, not added to what was there
    p.grad, q.grad = torch.full((6,), 4.0, device="cuda"), None
    acc.accumulate(True)
    assert torch.equal(p.grad, torch.full((6,), 7.0, device="cuda")) and torch.equal(q.grad, torch.full((3,), 5.0, device="cuda"))
    assert not acc.window_open


# ------------------------------------------------------------------------------------------------------------ the Trainer
def _model(dropout=0.0):
    from multimodal_supernovae_amd.models_multimodal import LightCurveImageCLIP
    torch.manual_seed(0)
    tk, sk = dict(TK, dropout=dropout), dict(SK, dropout=dropout)
    return LightCurveImageCLIP(enc_dim=16, nband=2, transformer_kwargs=tk, transformer_spectral_kwargs=sk,
                               combinations=COMBOS, loss="softmax", lr=3e-3,
                               optimizer_kwargs={"weight_decay": 1e-3}).cuda().train()


def _batches(n, steps, device="cuda"):
    g = torch.Generator().manual_seed(5)
    out = []
    for _ in range(steps):
        mask = torch.ones(n, 12, dtype=torch.bool)
        mask[:, 9:] = torch.rand(n, 3, generator=g) > 0.5
        b = (None, torch.randn(n, 12, generator=g), torch.rand(n, 12, generator=g) * 100, mask,
             torch.randn(n, 10, generator=g), torch.rand(n, 10, generator=g) * 6000 + 3000,
             torch.ones(n, 10, dtype=torch.bool), None, None)
        out.append(tuple(t.to(device) if t is not None else None for t in b))
    return out


def _close(a, b):
    for (k, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        torch.testing.assert_close(q, p, rtol=1e-5, atol=1e-7, msg=lambda m: f"{k}: {m}")


def _hand_loop(model, batches, k, epochs=1, clip=None, boundaries=None):
    """Lightning's loop with torch's own AccumulateGrad: zero_grad only after a step, (loss / k).backward(), a step at
    (i + 1) % k == 0 and on the last batch (or where `boundaries` says).  clip: None | ("msn" | "torch", max_norm).
    Returns (undivided losses, optimizer, steps, total norms)."""
    from multimodal_supernovae_amd import optim
    opt = model.configure_optimizers()["optimizer"]
    params = [p for group in opt.param_groups for p in group["params"]]
    opt.zero_grad(set_to_none=True)
    losses, steps, totals = [], 0, []
    for _ in range(epochs):
        for i, batch in enumerate(batches):
            batch = tuple(t.cuda() if t is not None else None for t in batch)
            loss = model.training_step(batch, i)
            (loss / k).backward()
            losses.append(loss.detach().clone())
            step = boundaries[i] if boundaries is not None else ((i + 1) % k == 0 or i == len(batches) - 1)
            if step:
                if clip is not None:
                    fn = optim.clip_grad_norm_ if clip[0] == "msn" else torch.nn.utils.clip_grad_norm_
                    totals.append(float(fn(params, clip[1])))
                opt.step()
                steps += 1
                opt.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    return losses, opt, steps, totals


def _states(model, opt):
    out = [p.detach().clone() for p in model.parameters()]
    steps = []
    for group in opt.param_groups:
        for p in group["params"]:
            st = opt.state.get(p, {})
            if len(st):
                out += [st["exp_avg"].clone(), st["exp_avg_sq"].clone()]
                steps.append(st["step"])
    return out, steps


def _bitwise(model_a, opt_a, model_b, opt_b):
    (ta, sa), (tb, sb) = _states(model_a, opt_a), _states(model_b, opt_b)
    assert len(ta) == len(tb) and len(sa) == len(sb) > 0
    assert all(type(s) is int for s in sa + sb) and sa == sb, (sa, sb)
    names = [k for k, _ in model_a.named_parameters()]
    for i, (x, y) in enumerate(zip(ta, tb)):
        assert torch.equal(x, y), (names[i] if i < len(names) else f"moment {i - len(names)}", float((x - y).abs().max()))


@pytest.mark.parametrize("k,steps", [(2, 8), (3, 6)])
def test_eager_trainer_is_lightnings_loop_by_hand_bit_for_bit(k, steps):
    from multimodal_supernovae_amd.trainer import Trainer
    batches = _batches(8, 7, device="cpu")                        # windows 2 + 2 + 2 + 1 and 3 + 3 + 1, over two epochs
    base = _model()
    h1, h2, t = copy.deepcopy(base), copy.deepcopy(base), copy.deepcopy(base)
    l1, o1, n1, _ = _hand_loop(h1, batches, k, epochs=2)
    l2, o2, n2, _ = _hand_loop(h2, batches, k, epochs=2)
    _bitwise(h1, o1, h2, o2)                                      # the kernels are deterministic
    assert n1 == n2 == steps and all(torch.equal(a, b) for a, b in zip(l1, l2))
    tr = Trainer(max_epochs=2, accumulate_grad_batches=k).fit(t, batches)
    torch.cuda.synchronize()
    assert tr.global_step == steps and len(tr.step_losses) == 14 == len(l1)
    assert all(torch.equal(a, b) for a, b in zip(tr.step_losses, l1)), ([float(x) for x in tr.step_losses], [float(x) for x in l1])
    assert len(tr.history["train_loss"]) == 2
    _bitwise(h1, o1, t, tr.optimizer)
    assert sum(p.grad is not None for p in t.parameters()) > 20      # after the step p.grad holds the accumulated gradient
    assert tr.accumulator is not None and not tr.accumulator.window_open


def test_eager_trainer_with_clipping():
    from multimodal_supernovae_amd.trainer import Trainer
    k, v = 2, 0.05
    batches = _batches(8, 7, device="cpu")
    base = _model()
    hm, ht, t = copy.deepcopy(base), copy.deepcopy(base), copy.deepcopy(base)
    _, om, nm, totals_m = _hand_loop(hm, batches, k, epochs=2, clip=("msn", v))
    _, ot, nt, totals_t = _hand_loop(ht, batches, k, epochs=2, clip=("torch", v))
    assert nm == nt == 8 and all(x > v for x in totals_m) and all(x > v for x in totals_t)      # the clip engaged at every step
    tr = Trainer(max_epochs=2, accumulate_grad_batches=k, gradient_clip_val=v).fit(t, batches)
    torch.cuda.synchronize()
    assert tr.global_step == 8
    _bitwise(hm, om, t, tr.optimizer)                             # the package's clip in the hand loop: bit for bit
    _close(ht, t)                                                 # torch's clip: the bound of tests/test_grad_clip_gpu.py


def test_k_equal_one_is_the_plain_path(monkeypatch):
    from multimodal_supernovae_amd import optim
    from multimodal_supernovae_amd.trainer import Trainer
    batches = _batches(8, 6, device="cpu")
    base = _model()
    a, b = copy.deepcopy(base), copy.deepcopy(base)
    plain = Trainer(max_epochs=1).fit(a, batches)
    calls = []
    real = optim.grad_accumulate_
    monkeypatch.setattr(optim, "grad_accumulate_", lambda *x, **kw: (calls.append(1), real(*x, **kw))[1])
    one = Trainer(max_epochs=1, accumulate_grad_batches=1).fit(b, batches)
    torch.cuda.synchronize()
    assert calls == [] and one.accumulator is None and one.global_step == plain.global_step == 6
    _bitwise(a, plain.optimizer, b, one.optimizer)
    assert all(torch.equal(x, y) for x, y in zip(plain.step_losses, one.step_losses))
    monkeypatch.setattr(optim, "grad_accumulate_", lambda *x, **kw: (calls.append(1), real(*x, **kw))[1])
    Trainer(max_epochs=1, accumulate_grad_batches=2).fit(copy.deepcopy(base), batches)
    assert len(calls) == 6                                        # the counter does see the launches: one per micro-batch


def test_row_additive_loss_four_micro_batches_equal_the_big_batch():
    """ClipMLP(regression=True), transformer towers (no BatchNorm): 4 micro-batches of 8 rows against one batch of 32, the same
    rows in the same order; the loss is a mean over rows, so the gradients agree up to the order of the sums.  Against the fp64
    plain-PyTorch restatement of tests/test_supervised_gpu.py the accumulated gradient may be at most twice as far off as the
    one-batch gradient (the same operations in another order), with a floor of one fp32 ulp of the largest gradient entry.
    The test prints both errors before it asserts.  Measured on an MI355X: one batch of 32 rows 1.205e-07, 4 x 8 accumulated
    1.505e-07; largest gradient entry 1.410e+00 (one fp32 ulp 1.192e-07), so the bound was 2.410e-07."""
    import test_supervised_gpu as S
    from multimodal_supernovae_amd.trainer import Trainer
    model = S._head("regression", seed=3)
    P = {k: v.detach().double().clone().requires_grad_(v.is_floating_point()) for k, v in model.clip_model.state_dict().items()}
    H = {k: v.detach().double().clone().requires_grad_() for k, v in model.mlp.state_dict().items()}
    batch = S._batch(32, seed=9)
    b64 = tuple(t.double() if torch.is_tensor(t) and t.is_floating_point() else t for t in batch)
    S._restated_loss(P, H, b64, "regression", None).backward()
    want = {"clip_model." + k: v for k, v in P.items() if v.requires_grad}
    want.update({"mlp." + k: v for k, v in H.items()})
    model.cuda().train()
    accumulated = copy.deepcopy(model)
    model.training_step(S._cuda(batch), 0).backward()
    micro = [tuple(t[8 * i:8 * i + 8] if torch.is_tensor(t) else t for t in batch) for i in range(4)]
    tr = Trainer(max_epochs=1, accumulate_grad_batches=4).fit(accumulated, micro)
    torch.cuda.synchronize()
    assert tr.global_step == 1 and len(tr.step_losses) == 4
    err_one = err_acc = largest = 0.0
    compared = 0
    for (k, p), (_, q) in zip(model.named_parameters(), accumulated.named_parameters()):
        w = want[k].grad
        if p.grad is None:
            assert q.grad is None and (w is None or float(w.abs().max()) == 0.0), k
            continue
        compared += 1
        largest = max(largest, float(w.abs().max()))
        err_one = max(err_one, float((p.grad.cpu().double() - w).abs().max()))
        err_acc = max(err_acc, float((q.grad.cpu().double() - w).abs().max()))
    ulp = 2.0 ** (math.floor(math.log2(largest)) - 23)
    print(f"one batch of 32: max |error| {err_one:.3e}; 4 x 8 accumulated: {err_acc:.3e}; largest entry {largest:.3e}, ulp {ulp:.3e}")
    assert compared > 20 and err_acc <= max(2.0 * err_one, ulp)


# ------------------------------------------------------------------------------------------------------ graph replay
def _drive_graphed(model, batches, k, last_flags=None, warmup=3):
    from multimodal_supernovae_amd.trainer import GraphedTrainStep
    step = GraphedTrainStep(model, model.configure_optimizers()["optimizer"], warmup=warmup, accumulate_grad_batches=k)
    losses = []
    for i, b in enumerate(batches):
        losses.append(float(step(b, i, last_batch=bool(last_flags and last_flags[i])).detach()))
    torch.cuda.synchronize()
    return step, losses


def _check_graphed(step, losses, eager, eager_losses, graphed, steps):
    assert step.graph is not None and step.calls == len(losses)
    for a, b in zip(eager_losses, losses):
        assert abs(float(a) - b) <= 1e-5 * abs(float(a)), ([float(x) for x in eager_losses], losses)
    _close(eager, graphed)
    counters = [int(c) for _, _, _, _, _, c in step.optimizer._graph_launches]
    assert counters and all(c == steps for c in counters), counters           # RAdam's DEVICE step count: once per optimizer step
    host = {st["step"] for st in step.optimizer.state.values() if len(st)}
    assert host == {steps}


def test_graph_replay_equals_eager():
    batches = _batches(8, 10)                                     # 10 calls = 5 steps: across RAdam's rectification switch
    eager = _model()
    graphed = copy.deepcopy(eager)
    le, _, n, _ = _hand_loop(eager, batches, 2, boundaries=[i % 2 == 1 for i in range(10)])
    assert n == 5
    step, lg = _drive_graphed(graphed, batches, 2)
    _check_graphed(step, lg, eager, le, graphed, 5)
    assert step.graph.boundary_from is not None and step.graph.segments == 2


def test_graph_replay_with_an_odd_batch_and_a_window_of_one():
    batches = _batches(8, 10)
    batches[5] = tuple(t[:5] if t is not None else None for t in batches[5])     # runs eagerly, closes the window 4 .. 5
    flags = [i == 8 for i in range(10)]                                           # the last batch of an epoch: a window of one
    bounds = [True if i == 8 else (i % 2 == 1 if i < 8 else False) for i in range(10)]   # 9 opens a window that stays open
    eager = _model()
    graphed = copy.deepcopy(eager)
    le, _, n, _ = _hand_loop(eager, batches, 2, boundaries=bounds)
    assert n == 5
    step, lg = _drive_graphed(graphed, batches, 2, last_flags=flags)
    _check_graphed(step, lg, eager, le, graphed, 5)
    assert step.accum.window_open


def test_graph_replays_draw_new_dropout_masks():
    batch = _batches(8, 1)[0]
    model = _model(dropout=0.1)
    step, losses = _drive_graphed(model, [batch] * 8, 2)
    assert step.graph is not None and all(math.isfinite(x) for x in losses)
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
    # calls 4 and 5 are replays on the same batch with the same weights (the step comes at the end of call 5): only the masks differ
    assert losses[4] != losses[5]


def test_trainer_passes_accumulation_to_the_graphed_step():
    from multimodal_supernovae_amd.trainer import Trainer
    batches = _batches(8, 7, device="cpu")
    eager = _model()
    graphed = copy.deepcopy(eager)
    te = Trainer(max_epochs=2, accumulate_grad_batches=2).fit(eager, batches)
    tg = Trainer(max_epochs=2, accumulate_grad_batches=2, graphed_steps=True).fit(graphed, batches)
    torch.cuda.synchronize()
    assert tg.graphed_step.graph is not None and tg.global_step == te.global_step == 8
    for a, b in zip(te.step_losses, tg.step_losses):
        assert abs(float(a) - float(b)) <= 1e-5 * abs(float(a))
    _close(eager, graphed)


# ------------------------------------------------------------------------------------------------------------- resume
def test_resume_at_an_epoch_end_is_bitwise(tmp_path):
    from multimodal_supernovae_amd import checkpoint as C
    from multimodal_supernovae_amd.trainer import Trainer
    batches = _batches(8, 5, device="cpu")                        # windows 2 + 2 + 1: three steps per epoch
    base = _model()
    whole, first = copy.deepcopy(base), copy.deepcopy(base)
    tw = Trainer(max_epochs=2, accumulate_grad_batches=2).fit(whole, batches)
    cb = C.ModelCheckpoint(str(tmp_path / "ckpt"))
    t1 = Trainer(max_epochs=1, accumulate_grad_batches=2, callbacks=[cb]).fit(first, batches)
    assert t1.global_step == 3 and os.path.exists(cb.best_model_path)
    torch.manual_seed(77)
    other = _model()
    with torch.no_grad():
        for p in other.parameters():
            p.add_(0.01)
    t2 = Trainer(max_epochs=2, accumulate_grad_batches=2).fit(other, batches, ckpt_path=cb.best_model_path)
    torch.cuda.synchronize()
    assert tw.global_step == t2.global_step == 6
    _bitwise(whole, tw.optimizer, other, t2.optimizer)
    assert tw.history == t2.history


# ---------------------------------------------------------------------------------------------------------- two ranks
def test_two_ranks_accumulating_equal_one_process_at_twice_the_batch():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "dist_check_accumulate.py")], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0 and "DIST CHECK OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
