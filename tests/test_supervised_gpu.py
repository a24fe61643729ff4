"""Supervised heads on the GPU (csrc/supervised.hip, models_finetune.py): the cross-entropy kernels against torch in fp64,
the metric kernels against exact host constructions, ClipMLP against a plain-PyTorch restatement built from oracle/, and its
behaviour under the Trainer's three modes (eager, graph-replayed, data parallel)."""
import copy
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(1, 2), (2, 2), (7, 5), (256, 5), (1024, 5), (4096, 17), (1024, 64), (513, 1000), (3, 1024), (100000, 5)]
GATE = 1e-6            # against fp64, as tests/test_grad_clip_gpu.py


def _ce_case(N, C, scale, weighted, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, generator=g) * scale
    y = torch.randint(0, C, (N,), generator=g)
    w = torch.rand(C, generator=g) + 0.25 if weighted else None
    return x, y, w


def _run_ce(x, y, w, x_dev=None):
    """loss and dlogits of the HIP path; x_dev: a prepared (possibly row-strided) device view of x."""
    from multimodal_supernovae_amd.models_finetune import cross_entropy
    xd = (x.cuda() if x_dev is None else x_dev).detach().requires_grad_()
    loss = cross_entropy(xd, y.cuda(), None if w is None else w.cuda())
    loss.backward()
    return loss.detach().cpu(), xd.grad.cpu()


def _ref_ce(x, y, w):
    xr = x.double().requires_grad_()
    loss = F.cross_entropy(xr, y, weight=None if w is None else w.double(), reduction="mean")
    loss.backward()
    return loss.detach(), xr.grad


def _check_ce(got, want, what):
    (loss, dx), (rl, rdx) = got, want
    le = abs(float(loss) - float(rl)) / abs(float(rl))
    ge = float((dx.double() - rdx).abs().max()) / float(rdx.abs().max())
    print(f"{what}: loss {float(loss):.9g} ref {float(rl):.9g} rel {le:.3e}; max|dx - ref| / max|ref| {ge:.3e}")
    assert le <= GATE, (what, le)
    assert ge <= GATE, (what, ge)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("scale", [1.0, 30.0])
@pytest.mark.parametrize("N,C", SHAPES)
def test_cross_entropy_matches_torch_fp64(N, C, scale, weighted):
    """The draws are those on which fp32 arithmetic was checked against this reference on the CPU beforehand (seed
    1000 N + C: torch's own fp32 op stays within 2.2e-7 of it).  The fp64 reference has a resolution of its own: it forms
    log(1 + t) from the rounded 1 + t, so a loss below about 1e-9 -- a single row whose target wins by 25 or more -- is
    only known to 2.2e-16 / loss, which is coarser than the gate; none of these draws is of that kind."""
    x, y, w = _ce_case(N, C, scale, weighted, seed=1000 * N + C)
    _check_ce(_run_ce(x, y, w), _ref_ce(x, y, w), f"N={N} C={C} scale={scale} weighted={weighted}")


@pytest.mark.parametrize("N,C", [(300, 5), (70, 40), (5000, 5), (200, 300)])
def test_cross_entropy_strided_ignored_and_out_of_range(N, C):
    x, y, w = _ce_case(N, C, 3.0, True, seed=N + C)
    big = torch.randn(N, C + 7).cuda()
    big[:, :C] = x.cuda()
    _check_ce(_run_ce(x, y, w, x_dev=big[:, :C]), _ref_ce(x, y, w), f"row-strided N={N} C={C}")
    yi = y.clone()
    yi[::3] = -100
    got = _run_ce(x, yi, w)
    _check_ce(got, _ref_ce(x, yi, w), f"ignore_index N={N} C={C}")
    assert float(got[1][::3].abs().max()) == 0.0
    # any other target outside [0, C) is ignored in the same way (torch itself refuses it): never an out-of-bounds read
    yo = yi.clone()
    yo[1], yo[2] = C + 3, -5
    yref = yo.clone()
    yref[1], yref[2] = -100, -100
    got = _run_ce(x, yo, w)
    _check_ce(got, _ref_ce(x, yref, w), f"out-of-range target N={N} C={C}")
    assert float(got[1][1:3].abs().max()) == 0.0
    loss, dx = _run_ce(x, torch.full((N,), -100), w)
    assert torch.isnan(loss)                                   # all rows ignored: nan, as torch
    assert torch.isnan(F.cross_entropy(x, torch.full((N,), -100), weight=w))


def test_cross_entropy_with_the_callers_denominator():
    """The kernel's own interface: out = {loss, denom, numerator}, and a device denominator of the caller's replaces the local one."""
    from multimodal_supernovae_amd._lib import check, lib, ptr, stream_ptr
    for N, C in [(100, 5), (9000, 5), (300, 100)]:
        x, y, w = _ce_case(N, C, 2.0, True, seed=N)
        xd, yd, wd = x.cuda(), y.cuda(), w.cuda()
        lse = torch.empty(N, device="cuda")
        pred = torch.empty(N, dtype=torch.int32, device="cuda")
        nb = lib().msn_cross_entropy_workspace_bytes(N, C)
        ws = torch.empty(max(nb, 8), dtype=torch.uint8, device="cuda")
        outs = []
        for denom_in in (None, torch.tensor([123.5], device="cuda")):
            out = torch.empty(3, device="cuda")
            check(lib().msn_cross_entropy_fwd(ptr(xd), C, ptr(yd), ptr(wd), N, C, ptr(denom_in), ptr(lse), ptr(pred), ptr(out),
                                              ptr(ws), nb, stream_ptr()), "msn_cross_entropy_fwd")
            outs.append(out.cpu().double())
        ref_num = float(F.cross_entropy(x.double(), y, weight=w.double(), reduction="sum"))
        ref_den = float(w.double()[y].sum())
        for out in outs:
            assert abs(float(out[2]) - ref_num) <= GATE * ref_num and abs(float(out[1]) - ref_den) <= GATE * ref_den
        assert abs(float(outs[0][0]) - ref_num / ref_den) <= GATE * ref_num / ref_den
        assert abs(float(outs[1][0]) - ref_num / 123.5) <= GATE * ref_num / 123.5
        ref_lse = torch.logsumexp(x.double(), dim=1)
        assert float((lse.cpu().double() - ref_lse).abs().max()) <= GATE * float(ref_lse.abs().max())


@pytest.mark.parametrize("N,C", SHAPES + [(5000, 16), (5000, 65), (777, 257)])
def test_prediction_is_torch_argmax_and_runs_are_bit_identical(N, C):
    from multimodal_supernovae_amd.models_finetune import _cross_entropy
    g = torch.Generator().manual_seed(N + C)
    y = torch.randint(0, C, (N,), generator=g).cuda()
    for x in (torch.randn(N, C, generator=g), torch.randint(0, 3, (N, C), generator=g).float()):     # the second: ties everywhere
        runs = []
        for _ in range(2):
            xd = x.cuda().requires_grad_()
            loss, pred = _cross_entropy(xd, y)
            loss.backward()
            runs.append((loss.detach().clone(), pred.clone(), xd.grad.clone()))
        assert runs[0][1].dtype == torch.int32
        assert torch.equal(runs[0][1].cpu().long(), torch.argmax(x, dim=1))
        assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[1]))


@pytest.mark.parametrize("C", [5, 16, 17, 64, 200, 1000])
def test_prediction_on_rows_without_a_finite_maximum(C):
    """Rows of -inf only and rows holding NaN: the class is torch.argmax's on both kernel families (a lane per row up to
    C = 16, a wave per row beyond), never an index outside [0, C)."""
    from multimodal_supernovae_amd.models_finetune import argmax_rows
    g = torch.Generator().manual_seed(C)
    x = torch.randn(6, C, generator=g)
    x[1] = float("-inf")
    x[2, C // 2] = float("nan")
    x[3, 0], x[3, C - 1] = float("nan"), float("nan")
    x[4, : C - 1] = float("-inf")
    pred = argmax_rows(x.cuda()).cpu().long()
    assert torch.equal(pred, torch.argmax(x, dim=1)), (pred, torch.argmax(x, dim=1))


def test_metric_updates_with_an_empty_batch_count_nothing():
    from multimodal_supernovae_amd.models_finetune import ClassificationMetrics, RegressionMetrics
    cm, rm = ClassificationMetrics(5), RegressionMetrics()
    cm.update(torch.tensor([1, 2], dtype=torch.int32).cuda(), torch.tensor([1, 3]).cuda())
    rm.update(torch.tensor([0.5]).cuda(), torch.tensor([0.25]).cuda())
    before = cm.cm.clone(), rm.sums.clone()
    cm.update(torch.empty(0, dtype=torch.int32).cuda(), torch.empty(0, dtype=torch.int64).cuda())
    cm.update(torch.empty(0, 5).cuda(), torch.empty(0, dtype=torch.int64).cuda())
    rm.update(torch.empty(0).cuda(), torch.empty(0).cuda())
    assert torch.equal(cm.cm, before[0]) and torch.equal(rm.sums, before[1]) and int(cm.cm.sum()) == 2


@pytest.mark.parametrize("C", [2, 5, 64, 1000])
def test_confusion_matrix_equals_bincount(C):
    from multimodal_supernovae_amd.models_finetune import ClassificationMetrics, classification_metrics
    g = torch.Generator().manual_seed(C)
    m = ClassificationMetrics(C)
    want = torch.zeros(C, C, dtype=torch.int64)
    for i, n in enumerate((1000, 37, 50000)):
        y = torch.randint(0, C, (n,), generator=g)
        p = torch.randint(0, C, (n,), generator=g)
        if i == 2:                                              # skewed: 90 % of the rows in one cell
            hot = torch.rand(n, generator=g) < 0.9
            y[hot], p[hot] = C - 1, 1
        y[5] = -100                                             # an ignored row does not count
        m.update(p.to(torch.int32).cuda(), y.cuda())
        keep = y >= 0
        want += torch.bincount(y[keep] * C + p[keep], minlength=C * C).view(C, C)
    assert m.cm.dtype == torch.int32 and torch.equal(m.cm.cpu().long(), want)
    assert m.compute() == classification_metrics(want)
    m.reset()
    assert int(m.cm.sum()) == 0
    logits = torch.randn(100, C, generator=g)                   # update() from logits takes the kernel's arg-max
    y = torch.randint(0, C, (100,), generator=g)
    m.update(logits.cuda(), y.cuda())
    assert torch.equal(m.cm.cpu().long(), torch.bincount(y * C + logits.argmax(1), minlength=C * C).view(C, C))


@pytest.mark.parametrize("N", [1, 1000, 100000])
def test_regression_sums_match_fp64(N):
    from multimodal_supernovae_amd.models_finetune import RegressionMetrics, regression_metrics
    g = torch.Generator().manual_seed(N)
    m = RegressionMetrics()
    want = torch.zeros(6, dtype=torch.float64)
    for _ in range(3):
        y = torch.rand(N, generator=g)
        p = y + 0.1 * torch.randn(N, generator=g)
        m.update(p.cuda(), y.cuda())
        yd, d = y.double(), p.double() - y.double()
        want += torch.stack([torch.tensor(float(N), dtype=torch.float64), d.abs().sum(), (d * d).sum(), yd.sum(), (yd * yd).sum(),
                             (d.abs() / (1 + yd) > 0.15).sum().double()])
    got = m.sums.cpu()
    rel = ((got - want).abs() / want.abs().clamp(min=1e-300)).tolist()
    print(f"N={N}: relative differences of the six sums {rel}")
    assert got[0] == want[0] and got[5] == want[5]
    assert max(rel) <= 1e-12
    res = m.compute()
    assert res == regression_metrics(got.tolist()) and set(res) == {"L1", "L2", "R2", "OLF"}


# ------------------------------------------------------------------------------------------------------- the module
CFG = dict(enc_dim=16, nband=2, combinations=["lightcurve", "spectral"],
           transformer_kwargs=dict(n_out=8, emb=16, heads=2, depth=2, dropout=0.0, time_norm=1000.0, agg="mean"),
           transformer_spectral_kwargs=dict(n_out=8, emb=16, heads=4, depth=1, dropout=0.0, time_norm=5000.0, agg="max"),
           conv_kwargs=dict(dim=8, depth=1, channels=3, kernel_size=5, patch_size=8, n_out=8, dropout_prob=0.0),
           meta_kwargs=None)
T_LC, T_SP, N_CLASSES = 10, 9, 5


def _clip(seed=0):
    from multimodal_supernovae_amd.models_multimodal import LightCurveImageCLIP
    torch.manual_seed(seed)
    return LightCurveImageCLIP(enc_dim=CFG["enc_dim"], logit_scale=10.0, nband=CFG["nband"],
                               transformer_kwargs=CFG["transformer_kwargs"],
                               transformer_spectral_kwargs=CFG["transformer_spectral_kwargs"], conv_kwargs=CFG["conv_kwargs"],
                               combinations=CFG["combinations"], loss="softmax")


def _head(task, seed=0, n_classes=N_CLASSES, **kw):
    from multimodal_supernovae_amd.models_finetune import ClipMLP
    clip = _clip(seed)
    torch.manual_seed(seed + 1)
    kw.setdefault("hidden_dim", 24)
    return ClipMLP(clip, classification=task == "classification", regression=task == "regression", n_classes=n_classes, **kw)


def _batch(B, seed, n_classes=N_CLASSES, separable=False):
    g = torch.Generator().manual_seed(seed)
    mask_lc = torch.arange(T_LC)[None, :] < torch.randint(1, T_LC + 1, (B, 1), generator=g)
    mask_sp = torch.arange(T_SP)[None, :] < torch.randint(1, T_SP + 1, (B, 1), generator=g)
    x_lc = torch.randn(B, T_LC, generator=g)
    cls = torch.randint(0, n_classes, (B,), generator=g)
    if separable:                                               # class = sign of the light curve's mean
        mask_lc = torch.ones(B, T_LC, dtype=torch.bool)
        cls = torch.randint(0, 2, (B,), generator=g)
        x_lc = 0.5 * x_lc + (2.0 * cls.float() - 1.0)[:, None]
    return (None, x_lc, torch.rand(B, T_LC, generator=g) * 100, mask_lc, torch.randn(B, T_SP, generator=g),
            torch.rand(B, T_SP, generator=g) * 6000 + 3000, mask_sp, torch.rand(B, generator=g), cls)


def _cuda(batch):
    return tuple(t.cuda() if torch.is_tensor(t) else t for t in batch)


def _restated_loss(P, H, batch, task, weights):
    """oracle towers -> concatenated embeddings -> plain-torch MLP (Linear, ReLU, ..., Linear) -> F.cross_entropy / F.mse_loss."""
    from oracle import clip as oclip
    h = torch.cat(oclip.embeddings(P, CFG, batch, training=True), dim=1)
    idx = sorted({int(k.split(".")[1]) for k in H})
    for j, i in enumerate(idx):
        h = F.linear(h, H[f"layers.{i}.weight"], H[f"layers.{i}.bias"])
        if j < len(idx) - 1:
            h = F.relu(h)
    if task == "classification":
        return F.cross_entropy(h, batch[8], weight=weights)
    return F.mse_loss(h.squeeze(1), batch[7])


@pytest.mark.parametrize("task,weighted", [("classification", False), ("classification", True), ("regression", False)])
@pytest.mark.parametrize("B", [1, 3, 7, 64])
def test_module_matches_plain_torch_restatement(B, task, weighted):
    weights = torch.tensor([0.5, 1.0, 2.0, 0.25, 1.25]) if weighted else None
    model = _head(task, seed=40 + B, class_weights=weights)
    P = {k: v.detach().clone().requires_grad_(v.is_floating_point()) for k, v in model.clip_model.state_dict().items()}
    H = {k: v.detach().clone().requires_grad_() for k, v in model.mlp.state_dict().items()}
    batch = _batch(B, seed=B)
    ref = _restated_loss(P, H, batch, task, weights)
    ref.backward()
    model.cuda().train()
    loss = model.training_step(_cuda(batch), 0)
    err = abs(float(loss.detach()) - float(ref.detach()))
    print(f"B={B} {task} weighted={weighted}: loss {float(loss.detach()):.7g} restated {float(ref.detach()):.7g}")
    assert err <= 1e-5 + 1e-3 * abs(float(ref.detach()))
    assert float(model.logged["train_loss"]) == float(loss.detach())
    loss.backward()
    want_all = {"clip_model." + k: v for k, v in P.items() if v.requires_grad}
    want_all.update({"mlp." + k: v for k, v in H.items()})
    for k, p in model.named_parameters():
        want = want_all[k].grad if want_all[k].grad is not None else torch.zeros_like(want_all[k])
        got = p.grad.cpu() if p.grad is not None else torch.zeros_like(want)
        if k in ("clip_model.logit_scale", "clip_model.logit_bias"):
            assert p.grad is None and float(want.abs().max()) == 0.0          # the contrastive scale / bias take no part
            continue
        scale = float(want.abs().max()) + 1e-6
        assert float((got - want).abs().max()) <= 2e-3 * scale + 1e-6, (k, B, float((got - want).abs().max()), scale)


def test_class_weights_refused_for_regression():
    from multimodal_supernovae_amd.models_finetune import ClipMLP
    with pytest.raises(ValueError):
        ClipMLP(_clip(), regression=True, class_weights=[1.0] * 5)


def _graph_nodes(loss):
    seen, stack, names, leaves = set(), [loss.grad_fn], [], []
    while stack:
        fn = stack.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        names.append(type(fn).__name__)
        if hasattr(fn, "variable"):
            leaves.append(fn.variable)
        stack += [f for f, _ in fn.next_functions]
    return names, leaves


TOWER_NODES = ("ProjectNormalise", "PostNorm", "TimeEmbed", "MaskedPool", "Attention", "MaskTokens")


@pytest.mark.parametrize("task", ["classification", "regression"])
def test_frozen_backbone_stays_bit_identical_and_has_no_tower_backward(task):
    from multimodal_supernovae_amd.trainer import Trainer
    model = _head(task, seed=3, freeze_backbone=True, learning_rate=1e-2)
    batches = [_batch(16, seed=s) for s in range(3)]
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    tr = Trainer(max_epochs=1).fit(model, batches)
    torch.cuda.synchronize()
    assert tr.global_step == 3 and model.training and not model.clip_model.training
    after = model.state_dict()
    for k, v in before.items():
        if k.startswith("clip_model."):
            assert torch.equal(after[k].cpu(), v), k
    assert all(not torch.equal(after[k].cpu(), before[k]) for k in before if k.startswith("mlp."))
    loss = model.training_step(_cuda(batches[0]), 0)
    names, leaves = _graph_nodes(loss)
    assert not [n for n in names if any(t in n for t in TOWER_NODES)], names
    head = {id(p) for p in model.mlp.parameters()}
    assert leaves and all(id(v) in head for v in leaves)
    assert any("LinearChain" in n for n in names)
    # the same walk does find the towers when they train
    names, leaves = _graph_nodes(_head(task, seed=3).cuda().train().training_step(_cuda(batches[0]), 0))
    assert any("ProjectNormalise" in n for n in names) and len(leaves) > len(head)


def _predict(model, batches):
    model.eval()
    outs = []
    with torch.no_grad():
        for b in batches:
            outs.append(model(*_cuda(b)).cpu())
    return torch.cat(outs)


def test_trainer_fit_classification_logs_metrics_and_learns():
    from multimodal_supernovae_amd.models_finetune import classification_metrics
    from multimodal_supernovae_amd.trainer import Trainer
    model = _head("classification", seed=5, n_classes=2, learning_rate=1e-2)
    train = [_batch(32, seed=s, n_classes=2, separable=True) for s in range(8)]
    val = [_batch(32, seed=100, n_classes=2, separable=True), _batch(11, seed=101, n_classes=2, separable=True)]
    tr = Trainer(max_epochs=2).fit(model, train, val)
    print("train_loss", tr.history["train_loss"], "val_loss", tr.history["val_loss"], {k: model.logged[k] for k in ("f1_val", "f1_micro_val", "acc_val")})
    assert len(tr.history["train_loss"]) == 2 and len(tr.history["val_loss"]) == 2
    assert tr.history["train_loss"][1] < tr.history["train_loss"][0]
    logits = _predict(model, val)
    y = torch.cat([b[8] for b in val])
    cm = torch.bincount(y * 2 + logits.argmax(1), minlength=4).view(2, 2)
    want = classification_metrics(cm)
    assert model.logged["f1_val"] == pytest.approx(want["f1_macro"], abs=1e-12)
    assert model.logged["f1_micro_val"] == pytest.approx(want["f1_micro"], abs=1e-12)
    assert model.logged["acc_val"] == pytest.approx(want["acc"], abs=1e-12)
    rows = torch.tensor([32.0, 11.0], dtype=torch.float64)
    per_batch = torch.stack([F.cross_entropy(l.double(), b[8]) for l, b in zip(logits.split([32, 11]), val)])
    assert tr.history["val_loss"][-1] == pytest.approx(float((per_batch * rows).sum() / rows.sum()), rel=1e-5)


def test_trainer_fit_regression_logs_metrics():
    from multimodal_supernovae_amd.models_finetune import regression_metrics
    from multimodal_supernovae_amd.trainer import Trainer
    model = _head("regression", seed=6, learning_rate=1e-2)
    train = [_batch(32, seed=s) for s in range(8)]
    val = [_batch(32, seed=100), _batch(11, seed=101)]
    tr = Trainer(max_epochs=2).fit(model, train, val)
    print("train_loss", tr.history["train_loss"], "val_loss", tr.history["val_loss"], {k: model.logged[k + "_val"] for k in ("L1", "L2", "R2", "OLF")})
    assert len(tr.history["train_loss"]) == 2 and len(tr.history["val_loss"]) == 2
    p = _predict(model, val).squeeze(1).double()
    y = torch.cat([b[7] for b in val]).double()
    d = p - y
    want = regression_metrics([43.0, float(d.abs().sum()), float((d * d).sum()), float(y.sum()), float((y * y).sum()),
                               float((d.abs() / (1 + y) > 0.15).sum())])
    for k in ("L1", "L2", "R2", "OLF"):
        assert model.logged[k + "_val"] == pytest.approx(want[k], rel=1e-9, abs=1e-12), k
    assert tr.history["val_loss"][-1] == pytest.approx(want["L2"], rel=1e-5)


@pytest.mark.parametrize("frozen", [False, True])
@pytest.mark.parametrize("task", ["classification", "regression"])
def test_graphed_step_equals_eager_steps(task, frozen):
    from multimodal_supernovae_amd.trainer import GraphedTrainStep
    steps = 9                                           # crosses RAdam's rectification switch (rho_t > 5 from step 6)
    batches = [_cuda(_batch(8, seed=s)) for s in range(steps)]
    eager = _head(task, seed=7, freeze_backbone=frozen, learning_rate=3e-3, optimizer_kwargs={"weight_decay": 1e-3}).cuda().train()
    graphed = copy.deepcopy(eager)
    opt_e = eager.configure_optimizers()["optimizer"]
    losses_e = []
    for b in batches:
        opt_e.zero_grad(set_to_none=True)
        loss = eager.training_step(b, 0)
        loss.backward()
        opt_e.step()
        losses_e.append(float(loss.detach()))
    opt_g = graphed.configure_optimizers()["optimizer"]
    step = GraphedTrainStep(graphed, opt_g, warmup=3)
    losses_g = [float(step(b).detach()) for b in batches]
    assert step.graph is not None and step.calls == steps
    torch.cuda.synchronize()
    for a, b in zip(losses_e, losses_g):
        assert abs(a - b) <= 1e-5 * abs(a), (losses_e, losses_g)
    for (k, p), (_, q) in zip(eager.named_parameters(), graphed.named_parameters()):
        torch.testing.assert_close(q, p, rtol=1e-5, atol=1e-7, msg=lambda m: f"{k}: {m}")
    for (k, p), (_, q) in zip(eager.named_buffers(), graphed.named_buffers()):
        torch.testing.assert_close(q, p, rtol=1e-5, atol=1e-7, msg=lambda m: f"buffer {k}: {m}")
    assert all(int(st["step"]) == steps for st in opt_g.state.values())
    assert losses_e[0] != losses_e[-1]


@pytest.mark.parametrize("task", ["classification", "regression"])
def test_trainer_with_graphed_steps_matches_eager_trainer(task):
    """Trainer(graphed_steps=True) over two epochs whose last batch is short == the eager Trainer (losses, parameters)."""
    from multimodal_supernovae_amd.trainer import Trainer
    batches = [_batch(8, seed=s) for s in range(6)]
    batches[-1] = tuple(t[:3] if t is not None else None for t in batches[-1])
    val = [_batch(8, seed=50)]
    a = _head(task, seed=8, learning_rate=3e-3)
    b = copy.deepcopy(a)
    ta = Trainer(max_epochs=2).fit(a, batches, val)
    tb = Trainer(max_epochs=2, graphed_steps=True).fit(b, batches, val)
    torch.cuda.synchronize()
    for key in ("train_loss", "val_loss"):
        assert len(ta.history[key]) == 2
        for x, y in zip(ta.history[key], tb.history[key]):
            assert abs(x - y) <= 1e-5 * abs(x), key
    for (k, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        torch.testing.assert_close(q, p, rtol=1e-5, atol=1e-7, msg=lambda m: f"{k}: {m}")


def test_two_rank_supervised_step_equals_single_process_global_batch():
    """Two ranks sharing the GPU over gloo (tools/dist_check_supervised.py): loss and gradients of the data-parallel step
    equal the single-process step at the doubled batch, unweighted, with class weights whose sums differ between the ranks,
    and for the regression loss; both ranks report the same train_loss."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "dist_check_supervised.py")], capture_output=True, text=True,
                       timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "DIST CHECK OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
