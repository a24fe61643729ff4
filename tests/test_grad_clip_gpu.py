"""Gradient clipping on the GPU (optim.clip_grad_norm_ / clip_grad_value_, csrc/grad_clip.hip) against torch.nn.utils on float64
copies, and the Trainer / GraphedTrainStep with pl.Trainer's gradient_clip_val against hand-written loops."""
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


def _params(sizes, seed=0, offsets=None, scale=1.0):
    """Leaf tensors with gradients; offsets[i] places gradient i at that storage offset of a larger buffer (misaligned view)."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for i, n in enumerate(sizes):
        p = torch.zeros(n, device="cuda", requires_grad=True)
        off = offsets[i] if offsets else 0
        buf = (torch.randn(n + off, generator=g) * scale).cuda()
        p.grad = buf[off:off + n]
        out.append(p)
    return out


def _ref(params, fn, *args, **kw):
    """torch.nn.utils on float64 CPU copies: (clipped gradients, return value)."""
    ref = [torch.zeros(p.shape, dtype=torch.float64, requires_grad=True) for p in params]
    for r, p in zip(ref, params):
        r.grad = p.grad.detach().cpu().double()
    out = fn(ref, *args, **kw)
    return [r.grad for r in ref], out


def _headline_params():
    sys.path.insert(0, ROOT)
    import bench
    model = bench.build_model(torch.device("cuda"))
    g = torch.Generator(device="cuda").manual_seed(3)
    ps = [p for p in model.parameters()]
    for p in ps:
        p.grad = torch.randn(p.shape, device="cuda", generator=g) * 1e-3
    return ps


SIZES = [1, 3, 5, 1023, 4097]
# The "small" table of tests/test_grad_accum_gpu.py: 301 tensors put mt_grid_x's cap (csrc/multi_tensor.h) at its minimum of 32
# blocks per tensor, and 32 x kMtBlockElems (4096) < 300 001, so every block of the large tensor takes three passes.
CAPPED = [1 + (7 * i) % 61 for i in range(300)] + [300_001]
SECOND_PASS = 32 * 4096                 # the first element of the large tensor that a block reaches in its second pass


def _capped_params(where, seed):
    """CAPPED with every gradient 16-byte aligned ("capped"), or tensor 5 one float and the large one three floats off."""
    offsets = [0] * len(CAPPED)
    if where == "capped_misaligned":
        offsets[5], offsets[300] = 1, 3
    params = _params(CAPPED, seed=seed, offsets=offsets)
    assert [p.grad.data_ptr() % 16 for p in (params[5], params[300])] == ([4, 12] if where == "capped_misaligned" else [0, 0])
    return params


@pytest.mark.parametrize("norm_type", [1.0, 2.0, math.inf])
@pytest.mark.parametrize("where", ["sizes", "misaligned", "headline", "capped", "capped_misaligned"])
@pytest.mark.parametrize("below", [True, False])
def test_clip_grad_norm_matches_torch_fp64(norm_type, where, below):
    from multimodal_supernovae_amd import optim
    if where == "headline":
        params = _headline_params()
        assert sum(p.numel() for p in params) > 20_000_000
    elif where.startswith("capped"):
        params = _capped_params(where, seed=8)
    elif where == "misaligned":
        params = _params(SIZES + [70000], seed=1, offsets=[1, 2, 3, 1, 2, 3])
        assert any(p.grad.data_ptr() % 16 for p in params)
    else:
        params = _params(SIZES + [70000], seed=2)
    norm = float(torch.linalg.vector_norm(torch.cat([p.grad.double().flatten() for p in params]), norm_type))
    max_norm = norm * (0.3 if below else 3.0)
    want_g, want_total = _ref(params, torch.nn.utils.clip_grad_norm_, max_norm, norm_type=norm_type)
    total = optim.clip_grad_norm_(params, max_norm, norm_type=norm_type)
    assert total.dim() == 0 and total.dtype == torch.float32 and total.is_cuda
    assert abs(float(total) - float(want_total)) <= 1e-6 * float(want_total)
    for p, w in zip(params, want_g):
        torch.testing.assert_close(p.grad.cpu().double(), w, rtol=1e-6, atol=0.0)


@pytest.mark.parametrize("norm_type", [1.0, 2.0, math.inf])
@pytest.mark.parametrize("bad", ["nan", "+inf", "-inf", "both_inf"])
def test_nonfinite_gradients_follow_torch(norm_type, bad):
    from multimodal_supernovae_amd import optim
    params = _params(SIZES + [9000], seed=4, offsets=[0, 1, 0, 2, 0, 3])
    if bad == "nan":
        params[4].grad[17] = math.nan
    if bad in ("+inf", "both_inf"):
        params[5].grad[4001] = math.inf
    if bad in ("-inf", "both_inf"):
        params[3].grad[5] = -math.inf
    want_g, want_total = _ref(params, torch.nn.utils.clip_grad_norm_, 1.0, norm_type=norm_type)
    total = optim.clip_grad_norm_(params, 1.0, norm_type=norm_type)
    t, w = float(total), float(want_total)
    assert (math.isnan(t) and math.isnan(w)) or t == w, (t, w)
    for p, w in zip(params, want_g):
        torch.testing.assert_close(p.grad.cpu().double(), w, rtol=1e-6, atol=0.0, equal_nan=True)
    if bad == "nan":
        assert all(torch.isnan(p.grad).all() for p in params)             # a NaN anywhere poisons every gradient
    else:
        assert float(total) == math.inf and not torch.isnan(params[0].grad).any()


def test_error_if_nonfinite_raises_eagerly_and_is_refused_under_capture():
    from multimodal_supernovae_amd import _lib, optim
    params = _params([100, 200], seed=5)
    params[1].grad[3] = math.inf
    before = [p.grad.clone() for p in params]
    with pytest.raises(RuntimeError, match="non-finite"):
        optim.clip_grad_norm_(params, 1.0, error_if_nonfinite=True)
    for p, b in zip(params, before):                                    # as torch: raised before any gradient is scaled
        assert torch.equal(p.grad, b)
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        graph.capture_begin()
        try:
            with pytest.raises(_lib.MsnHipError, match="capture"):
                optim.clip_grad_norm_(params, 1.0, error_if_nonfinite=True)
        finally:
            graph.capture_end()
    torch.cuda.current_stream().wait_stream(side)


@pytest.mark.parametrize("clip_value", [0.0, 0.25, 1.5])
def test_clip_grad_value_is_torch_clamp_bit_for_bit(clip_value):
    from multimodal_supernovae_amd import optim
    params = _params(SIZES + [70000], seed=6, offsets=[0, 1, 2, 3, 1, 0])
    params[5].grad[11] = math.nan
    params[5].grad[12] = math.inf
    params[3].grad[0] = -math.inf
    tables = [params]
    for where in ("capped", "capped_misaligned"):                       # the planted values sit in the large tensor's second pass
        params = _capped_params(where, seed=9)
        large = params[300].grad
        large[SECOND_PASS + 5], large[SECOND_PASS + 4102], large[SECOND_PASS + 70_001] = math.nan, math.inf, -math.inf
        tables.append(params)
    for params in tables:
        want = [torch.clamp(p.grad.cpu(), -clip_value, clip_value) for p in params]
        assert optim.clip_grad_value_(params, clip_value) is None
        for p, w in zip(params, want):
            got = p.grad.cpu()
            assert torch.equal(torch.isnan(got), torch.isnan(w))
            keep = ~torch.isnan(w)
            assert torch.equal(got[keep].view(torch.int32), w[keep].view(torch.int32))


def test_clipping_is_deterministic_and_skips_parameters_without_gradient():
    from multimodal_supernovae_amd import optim
    base = _headline_params()
    grads0 = [p.grad.clone() for p in base]
    runs = []
    for _ in range(3):
        for p, g in zip(base, grads0):
            p.grad = g.clone()
        total = optim.clip_grad_norm_(base, 0.05).clone()
        runs.append((total, [p.grad.clone() for p in base]))
    for total, gs in runs[1:]:
        assert torch.equal(total.view(torch.int32), runs[0][0].view(torch.int32))
        assert all(torch.equal(a, b) for a, b in zip(gs, runs[0][1]))
    params = _params([10, 20, 30], seed=7)
    lone = torch.zeros(5, device="cuda", requires_grad=True)             # no gradient: skipped
    want_g, want_total = _ref(params, torch.nn.utils.clip_grad_norm_, 0.5)
    total = optim.clip_grad_norm_([params[0], lone, params[1], params[2]], 0.5)
    assert lone.grad is None
    assert abs(float(total) - float(want_total)) <= 1e-6 * float(want_total)
    for p, w in zip(params, want_g):
        torch.testing.assert_close(p.grad.cpu().double(), w, rtol=1e-6, atol=0.0)
    assert float(optim.clip_grad_norm_([], 1.0)) == 0.0
    assert float(optim.clip_grad_norm_([lone], 1.0)) == 0.0


def _model():
    from multimodal_supernovae_amd.models_multimodal import LightCurveImageCLIP
    torch.manual_seed(0)
    return LightCurveImageCLIP(enc_dim=16, nband=2, transformer_kwargs=TK, transformer_spectral_kwargs=SK,
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


@pytest.mark.parametrize("algo", ["norm", "value"])
def test_trainer_clipping_matches_torch_hand_loop(algo):
    from multimodal_supernovae_amd.trainer import Trainer
    steps, v = 8, (0.05 if algo == "norm" else 1e-3)
    batches = _batches(8, steps, device="cpu")
    a = _model()
    b = copy.deepcopy(a)
    tr = Trainer(max_epochs=1, gradient_clip_val=v, gradient_clip_algorithm=None if algo == "norm" else "value").fit(a, batches)
    opt = b.configure_optimizers()["optimizer"]
    losses = []
    for i, batch in enumerate(batches):
        batch = tuple(t.cuda() if t is not None else None for t in batch)
        opt.zero_grad(set_to_none=True)
        loss = b.training_step(batch, i)
        loss.backward()
        params = [p for group in opt.param_groups for p in group["params"]]
        if algo == "norm":
            total = torch.nn.utils.clip_grad_norm_(params, v)
            assert float(total) > v                                       # the clip engaged at every step
        else:
            assert max(float(p.grad.abs().max()) for p in params if p.grad is not None) > v
            torch.nn.utils.clip_grad_value_(params, v)
        opt.step()
        losses.append(float(loss.detach()))
    torch.cuda.synchronize()
    got = [float(x) for x in tr.step_losses]
    for x, y in zip(got, losses):
        assert abs(x - y) <= 1e-5 * abs(y), (got, losses)
    _close(b, a)
    # after the step p.grad holds the clipped gradient, as under Lightning (logit_bias: analytically zero, rounding noise only)
    scale = max(float(q.grad.abs().max()) for q in b.parameters() if q.grad is not None)
    for (k, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        if q.grad is not None and k != "logit_bias":
            torch.testing.assert_close(p.grad, q.grad, rtol=1e-5, atol=1e-5 * scale, msg=lambda m: f"grad {k}: {m}")


def _eager_clipped(model, batches, v, algo):
    from multimodal_supernovae_amd import optim
    opt = model.configure_optimizers()["optimizer"]
    losses = []
    for batch in batches:
        opt.zero_grad(set_to_none=True)
        loss = model.training_step(batch, 0)
        loss.backward()
        params = [p for group in opt.param_groups for p in group["params"]]
        if algo == "norm":
            assert float(optim.clip_grad_norm_(params, v)) > v
        else:
            optim.clip_grad_value_(params, v)
        opt.step()
        losses.append(float(loss.detach()))
    return losses


@pytest.mark.parametrize("algo", ["norm", "value"])
def test_graphed_step_with_clipping_equals_eager_steps(algo):
    from multimodal_supernovae_amd.trainer import GraphedTrainStep
    steps, v = 9, (0.05 if algo == "norm" else 1e-3)                    # 9 steps cross RAdam's rectification switch
    batches = _batches(8, steps)
    eager = _model()
    graphed = copy.deepcopy(eager)
    losses_e = _eager_clipped(eager, batches, v, algo)
    step = GraphedTrainStep(graphed, graphed.configure_optimizers()["optimizer"], warmup=3, gradient_clip_val=v,
                            gradient_clip_algorithm=algo)
    losses_g = [float(step(b).detach()) for b in batches]
    assert step.graph is not None and step.calls == steps
    torch.cuda.synchronize()
    for a, b in zip(losses_e, losses_g):
        assert abs(a - b) <= 1e-5 * abs(a), (losses_e, losses_g)
    _close(eager, graphed)


def test_graphed_step_with_clipping_and_an_odd_batch_in_between():
    from multimodal_supernovae_amd.trainer import GraphedTrainStep
    batches = _batches(8, 8)
    batches[5] = tuple(t[:5] if t is not None else None for t in batches[5])
    eager = _model()
    graphed = copy.deepcopy(eager)
    _eager_clipped(eager, batches, 0.05, "norm")
    step = GraphedTrainStep(graphed, graphed.configure_optimizers()["optimizer"], warmup=2, gradient_clip_val=0.05)
    for b in batches:
        step(b)
    assert step.graph is not None
    torch.cuda.synchronize()
    _close(eager, graphed)


def test_two_ranks_with_clipping_equal_one_process_at_twice_the_batch():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "dist_check.py"), "--clip"], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0 and "DIST CHECK OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
