"""Focal loss and label smoothing on the GPU (csrc/focal_loss.hip, models_finetune.py): the kernels against the longdouble
reference, cross-checks with torch and with this package's cross-entropy, ignored rows, predictions, determinism, the C-ABI
and its refusals, and ClipMLP(loss="focal") eager, graph-replayed, under the Trainer and on two ranks."""
import copy
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_supervised_gpu as S          # the tiny towers, their batches, and the gate of the cross-entropy tests

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GATE = S.GATE                  # 1e-6 against the reference
FLOOR = 2.0 ** -126            # one smallest fp32 normal: a focal loss of confident rows underflows fp32
# the smallest shapes that reach every path: one workgroup / several + the finishing block, a lane per row (C <= 16) / a wave
# per row with 1, 4 or 16 registers per lane, and both sides of every switch -- the kernel's own single-workgroup thresholds
# (256 rows a lane per row, 4 rows a wave per row) among them, and (8200, 17), where a wave walks on to a second row
SHAPES = [(1, 2), (2, 2), (7, 5), (256, 5), (257, 5), (4096, 16), (4096, 17), (5000, 16), (4, 17), (5, 17), (64, 64), (65, 65), (70, 257),
          (513, 1000), (3, 1024), (8200, 17), (100000, 5)]
GAMMAS = [0.0, 0.5, 2.0, 5.0]
SMOOTHINGS = [0.0, 0.1]


@functools.lru_cache(maxsize=4)
def _case(N, C, scale, weighted):
    g = torch.Generator().manual_seed(1000 * N + C)
    x = torch.randn(N, C, generator=g) * scale
    y = torch.randint(0, C, (N,), generator=g)
    w = torch.rand(C, generator=g) + 0.25 if weighted else None
    return x, y, w


def _run(x, y, w, gamma, eps, x_dev=None):
    """loss, dlogits and pred of the HIP path; x_dev: a prepared (possibly row-strided) device view of x."""
    from multimodal_supernovae_amd.models_finetune import _focal_loss
    xd = (x.cuda() if x_dev is None else x_dev).detach().requires_grad_()
    loss, pred = _focal_loss(xd, y.cuda(), None if w is None else w.cuda(), gamma, eps)
    loss.backward()
    return loss.detach().cpu(), xd.grad.cpu(), pred.cpu()


def _check(got, want, what):
    """|loss - ref| <= GATE |ref| + FLOOR and max|dx - ref| <= GATE max|ref| + FLOOR; prints the ratios to the bounds."""
    (loss, dx), (rl, rdx) = got[:2], want
    le, lb = abs(float(loss.double()) - rl), GATE * abs(rl) + FLOOR
    ge, gb = float(np.abs(dx.double().numpy() - rdx).max()), GATE * float(np.abs(rdx).max()) + FLOOR
    print(f"{what}: loss {float(loss):.9g} ref {rl:.9g} error / bound {le / lb:.3e}; max|dx - ref| / bound {ge / gb:.3e}")
    assert le <= lb, (what, le, lb)
    assert ge <= gb, (what, ge, gb)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("scale", [1.0, 30.0])
@pytest.mark.parametrize("eps", SMOOTHINGS)
@pytest.mark.parametrize("gamma", GAMMAS)
@pytest.mark.parametrize("N,C", SHAPES)
def test_focal_loss_matches_the_reference(N, C, gamma, eps, scale, weighted):
    """Expected, since the rows are computed in fp64: one fp32 rounding of the loss (6e-8, 0.06 of the bound) and two of a
    gradient entry, its own and that of the fp32 denominator the backward divides by (0.12 of the bound).  Measured on an
    MI355X over the 544 cases: the worst error / bound is 0.058 for the loss and 0.092 for the gradient
    (profiles/focal_loss_accuracy.txt)."""
    from multimodal_supernovae_amd.models_finetune import focal_loss_reference
    x, y, w = _case(N, C, scale, weighted)
    _check(_run(x, y, w, gamma, eps), focal_loss_reference(x, y, w, gamma, eps),
           f"N={N} C={C} gamma={gamma} eps={eps} scale={scale} weighted={weighted}")


def test_focal_loss_where_a_lane_walks_on_to_a_second_row():
    """The grid stops at 2048 workgroups of 256 lanes: from N = 524289 on, lanes of the lane-per-row kernels take a second
    row.  One case, the smallest round size past that."""
    from multimodal_supernovae_amd.models_finetune import focal_loss_reference
    N, C = 530000, 5
    x, y, w = _case(N, C, 1.0, True)
    got = _run(x, y, w, 2.0, 0.1)
    _check(got, focal_loss_reference(x, y, w, 2.0, 0.1), f"N={N} C={C} gamma=2.0 eps=0.1 scale=1.0 weighted=True")
    assert torch.equal(got[2].long(), torch.argmax(x, dim=1))


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("eps", [0.1, 0.5, 1.0])
@pytest.mark.parametrize("N,C", [(7, 5), (256, 5), (4096, 17), (513, 1000), (100000, 5)])
def test_smoothed_cross_entropy_matches_torch_fp64(N, C, eps, weighted):
    from multimodal_supernovae_amd.models_finetune import cross_entropy
    x, y, w = _case(N, C, 1.0, weighted)
    y = y.clone()
    y[::5] = -100
    xd = x.cuda().requires_grad_()
    loss = cross_entropy(xd, y.cuda(), None if w is None else w.cuda(), label_smoothing=eps)
    loss.backward()
    xr = x.double().requires_grad_()
    ref = F.cross_entropy(xr, y, weight=None if w is None else w.double(), label_smoothing=eps, reduction="mean")
    ref.backward()
    le = abs(float(loss.detach().double().cpu()) - float(ref.detach())) / abs(float(ref.detach()))
    ge = float((xd.grad.cpu().double() - xr.grad).abs().max()) / float(xr.grad.abs().max())
    print(f"N={N} C={C} eps={eps} weighted={weighted}: loss rel {le:.3e}, max|dx - ref| / max|ref| {ge:.3e}")
    assert le <= GATE and ge <= GATE
    assert float(xd.grad[::5].abs().max()) == 0.0


@pytest.mark.parametrize("N,C", [(7, 5), (256, 5), (4096, 17), (513, 1000), (100000, 5)])
def test_gamma_zero_without_smoothing_is_this_packages_cross_entropy(N, C):
    from multimodal_supernovae_amd.models_finetune import cross_entropy, focal_loss
    x, y, w = _case(N, C, 1.0, True)
    res = []
    for fn in (lambda a: focal_loss(a, y.cuda(), w.cuda(), gamma=0.0, label_smoothing=0.0), lambda a: cross_entropy(a, y.cuda(), w.cuda())):
        xd = x.cuda().requires_grad_()
        loss = fn(xd)
        loss.backward()
        res.append((loss.detach().cpu(), xd.grad.cpu()))
    (fl, fdx), (cl, cdx) = res
    le = abs(float(fl) - float(cl)) / abs(float(cl))
    ge = float((fdx - cdx).abs().max()) / float(cdx.abs().max())
    print(f"N={N} C={C}: focal(gamma=0) against cross_entropy: loss rel {le:.3e} (bits {'agree' if torch.equal(fl, cl) else 'differ'}), "
          f"gradient {ge:.3e} of its largest entry (bits {'agree' if torch.equal(fdx, cdx) else 'differ'})")
    assert le <= GATE and ge <= GATE
    # label_smoothing = 0.0 takes the cross-entropy kernels themselves: today's bits
    xd = x.cuda().requires_grad_()
    loss = cross_entropy(xd, y.cuda(), w.cuda(), label_smoothing=0.0)
    loss.backward()
    assert torch.equal(loss.detach().cpu(), cl) and torch.equal(xd.grad.cpu(), cdx)


@pytest.mark.parametrize("N,C", [(300, 5), (70, 40), (5000, 5), (200, 300)])
def test_strided_ignored_and_out_of_range(N, C):
    from multimodal_supernovae_amd.models_finetune import focal_loss_reference
    gamma, eps = 2.0, 0.1
    g = torch.Generator().manual_seed(N + C)
    x = torch.randn(N, C, generator=g) * 3.0
    y = torch.randint(0, C, (N,), generator=g)
    w = torch.rand(C, generator=g) + 0.25
    big = torch.randn(N, C + 7).cuda()
    big[:, :C] = x.cuda()
    want = focal_loss_reference(x, y, w, gamma, eps)
    strided = _run(x, y, w, gamma, eps, x_dev=big[:, :C])
    _check(strided, want, f"row-strided N={N} C={C}")
    dense = _run(x, y, w, gamma, eps)
    assert all(torch.equal(a, b) for a, b in zip(strided, dense))          # the same bits for every row stride
    yo = y.clone()
    yo[::3] = -100
    yo[1], yo[2] = C + 3, -5                                             # ignored like -100, never used as an index
    yref = yo.clone()
    yref[1], yref[2] = -100, -100
    got = _run(x, yo, w, gamma, eps)
    _check(got, focal_loss_reference(x, yref, w, gamma, eps), f"ignored rows N={N} C={C}")
    assert float(got[1][::3].abs().max()) == 0.0 and float(got[1][1:3].abs().max()) == 0.0
    loss, dx, pred = _run(x, torch.full((N,), -100), w, gamma, eps)
    assert torch.isnan(loss)                                             # all rows ignored: nan, as torch
    assert torch.equal(pred.long(), torch.argmax(x, dim=1))              # the predictions do not depend on the targets


@pytest.mark.parametrize("N,C", SHAPES + [(5000, 65), (777, 257)])
def test_prediction_is_argmax_and_runs_are_bit_identical(N, C):
    from multimodal_supernovae_amd.models_finetune import _focal_loss, argmax_rows
    g = torch.Generator().manual_seed(N + C)
    y = torch.randint(0, C, (N,), generator=g).cuda()
    for x in (torch.randn(N, C, generator=g), torch.randint(0, 3, (N, C), generator=g).float()):     # the second: ties everywhere
        runs = []
        for _ in range(2):
            xd = x.cuda().requires_grad_()
            loss, pred = _focal_loss(xd, y, None, 2.0, 0.1)
            loss.backward()
            runs.append((loss.detach().clone(), pred.clone(), xd.grad.clone()))
        assert runs[0][1].dtype == torch.int32
        assert torch.equal(runs[0][1], argmax_rows(x.cuda()))
        assert torch.equal(runs[0][1].cpu().long(), torch.argmax(x, dim=1))
        assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[1]))


@pytest.mark.parametrize("C", [5, 16, 17, 64, 200, 1000])
def test_prediction_and_loss_on_rows_without_a_finite_maximum(C):
    """Rows of -inf only and rows holding NaN: the class is argmax_rows' (torch.argmax's) on both kernel families, and the
    non-finite logits reach the loss."""
    from multimodal_supernovae_amd.models_finetune import _focal_loss, argmax_rows
    g = torch.Generator().manual_seed(C)
    x = torch.randn(6, C, generator=g)
    x[1] = float("-inf")
    x[2, C // 2] = float("nan")
    x[3, 0], x[3, C - 1] = float("nan"), float("nan")
    x[4, : C - 1] = float("-inf")
    y = torch.zeros(6, dtype=torch.int64).cuda()
    loss, pred = _focal_loss(x.cuda(), y, None, 2.0, 0.0)
    assert torch.equal(pred, argmax_rows(x.cuda())) and torch.equal(pred.cpu().long(), torch.argmax(x, dim=1))
    assert torch.isnan(loss)
    # a -inf logit beside the target is a class of probability zero: finite without smoothing
    x = torch.randn(6, C, generator=g)
    x[:, 1] = float("-inf")
    xd = x.cuda().requires_grad_()
    loss, _ = _focal_loss(xd, y, None, 2.0, 0.0)
    loss.backward()
    assert torch.isfinite(loss) and bool(torch.isfinite(xd.grad).all()) and float(xd.grad[:, 1].abs().max()) == 0.0


def _fwd_args(x, y, w, N, C, gamma, eps, denom_in, pred, out, ws, nb, ld=None):
    from multimodal_supernovae_amd._lib import ptr, stream_ptr
    return (ptr(x), C if ld is None else ld, ptr(y), ptr(w), N, C, gamma, eps, ptr(denom_in), ptr(pred), ptr(out), ptr(ws), nb,
            stream_ptr())


def test_the_callers_denominator_replaces_the_local_one():
    """The kernel's own interface: out = {numerator / denom_in, denominator, numerator}."""
    from multimodal_supernovae_amd._lib import check, lib
    from multimodal_supernovae_amd.models_finetune import focal_loss_reference
    for N, C in [(100, 5), (9000, 5), (300, 100)]:
        x, y, w = _case(N, C, 1.0, True)
        xd, yd, wd = x.cuda(), y.cuda(), w.cuda()
        pred = torch.empty(N, dtype=torch.int32, device="cuda")
        nb = lib().msn_focal_loss_workspace_bytes(N, C)
        ws = torch.empty(max(nb, 8), dtype=torch.uint8, device="cuda")
        outs = []
        for denom_in in (None, torch.tensor([123.5], device="cuda")):
            out = torch.empty(3, device="cuda")
            check(lib().msn_focal_loss_fwd(*_fwd_args(xd, yd, wd, N, C, 2.0, 0.1, denom_in, pred, out, ws, nb)), "msn_focal_loss_fwd")
            outs.append(out.cpu().double())
        ref_den = float(w.double()[y].sum())
        ref_num = focal_loss_reference(x, y, w, 2.0, 0.1)[0] * ref_den
        for out in outs:
            assert abs(float(out[2]) - ref_num) <= GATE * ref_num and abs(float(out[1]) - ref_den) <= GATE * ref_den
        assert abs(float(outs[0][0]) - ref_num / ref_den) <= GATE * ref_num / ref_den
        assert abs(float(outs[1][0]) - ref_num / 123.5) <= GATE * ref_num / 123.5


def test_every_refusal_returns_one_and_writes_nothing():
    from multimodal_supernovae_amd._lib import lib, ptr, stream_ptr
    L = lib()
    N, C = 200, 5                                                         # one workgroup: the calls that are in order need no workspace
    x, y, w = _case(N, C, 1.0, True)
    wide = torch.randn(2, 1025).cuda()
    xd, yd, wd = x.cuda(), y.cuda(), w.cuda()
    pred = torch.full((N,), -7, dtype=torch.int32, device="cuda")
    out = torch.full((3,), -7.0, device="cuda")
    dx = torch.full((N, C), -7.0, device="cuda")
    ws = torch.full((64,), 7, dtype=torch.uint8, device="cuda")
    one = torch.ones(1, device="cuda")
    off = torch.zeros(N * C + 1, device="cuda")[1:]                       # 4 bytes past a 16-byte boundary: fine for floats
    y_off = torch.zeros(2 * N + 1, dtype=torch.int32, device="cuda")[1:]   # 4 bytes past an 8-byte boundary: not for int64
    assert L.msn_focal_loss_workspace_bytes(6000, 5) > 64

    def fwd(x_=xd, y_=yd, w_=wd, N_=N, C_=C, gamma=2.0, eps=0.1, pred_=pred, out_=out, ws_=None, nb=0, ld=None):
        return L.msn_focal_loss_fwd(*_fwd_args(x_, y_, w_, N_, C_, gamma, eps, None, pred_, out_, ws_, nb, ld))

    def bwd(x_=xd, y_=yd, N_=N, C_=C, gamma=2.0, eps=0.1, denom=one, g=one, dx_=dx, ld=C, lddx=C):
        return L.msn_focal_loss_bwd(ptr(x_), ld, ptr(y_), ptr(wd), N_, C_, gamma, eps, ptr(denom), ptr(g), ptr(dx_), lddx, stream_ptr())

    refused = {
        "fwd C = 1": fwd(C_=1, ld=5), "fwd C = 1025": fwd(x_=wide, N_=2, C_=1025), "fwd N = 0": fwd(N_=0), "fwd N = 2^31": fwd(N_=2 ** 31),
        "fwd gamma < 0": fwd(gamma=-0.5), "fwd gamma = inf": fwd(gamma=float("inf")), "fwd gamma = nan": fwd(gamma=float("nan")),
        "fwd smoothing < 0": fwd(eps=-0.1), "fwd smoothing > 1": fwd(eps=1.5), "fwd smoothing = nan": fwd(eps=float("nan")),
        "fwd row stride below C": fwd(ld=C - 1), "fwd null logits": fwd(x_=None), "fwd null target": fwd(y_=None),
        "fwd null pred": fwd(pred_=None), "fwd null out": fwd(out_=None), "fwd misaligned target": fwd(y_=y_off),
        "fwd workspace missing": fwd(N_=6000), "fwd workspace too small": fwd(N_=6000, ws_=ws, nb=64),
        "bwd C = 1": bwd(C_=1), "bwd C = 1025": bwd(C_=1025, ld=1025, lddx=1025), "bwd N = 0": bwd(N_=0), "bwd N = 2^31": bwd(N_=2 ** 31),
        "bwd gamma < 0": bwd(gamma=-1.0), "bwd gamma = nan": bwd(gamma=float("nan")), "bwd smoothing > 1": bwd(eps=1.01),
        "bwd row stride below C": bwd(ld=C - 1), "bwd gradient stride below C": bwd(lddx=C - 1), "bwd null denominator": bwd(denom=None),
        "bwd null grad_out": bwd(g=None), "bwd null dlogits": bwd(dx_=None), "bwd misaligned target": bwd(y_=y_off),
    }
    torch.cuda.synchronize()
    assert {k: v for k, v in refused.items() if v != 1} == {}
    assert L.msn_last_error()
    assert bool((pred == -7).all()) and bool((out == -7.0).all()) and bool((dx == -7.0).all()) and bool((ws == 7).all())
    # the same buffers are written once the arguments are in order (a float pointer 4 bytes past a 16-byte boundary included)
    off.copy_(xd.reshape(-1))
    assert fwd(x_=off) == 0 and bwd(x_=off) == 0
    torch.cuda.synchronize()
    assert not bool((pred == -7).any()) and not bool((out == -7.0).any()) and not bool((dx == -7.0).any())


# ------------------------------------------------------------------------------------------------------- the module
LOSS = dict(loss="focal", loss_kwargs={"gamma": 2.0, "label_smoothing": 0.1})
WEIGHTS = [0.5, 1.0, 2.0, 0.25, 1.25]


def test_module_step_is_the_focal_loss_of_its_logits_with_a_gradient_everywhere():
    from multimodal_supernovae_amd.models_finetune import focal_loss_reference
    model = S._head("classification", seed=11, class_weights=WEIGHTS, **LOSS).cuda().train()
    batch = S._cuda(S._batch(16, seed=3))
    loss = model.training_step(batch, 0)
    loss.backward()
    torch.cuda.synchronize()
    assert torch.isfinite(loss) and float(model.logged["train_loss"]) == float(loss.detach())
    with torch.no_grad():
        logits = model(*batch).cpu()
    want = focal_loss_reference(logits, batch[8].cpu(), torch.tensor(WEIGHTS), 2.0, 0.1)[0]
    assert abs(float(loss.detach()) - want) <= 1e-5 * want
    for k, p in model.named_parameters():
        if k in ("clip_model.logit_scale", "clip_model.logit_bias"):
            assert p.grad is None
            continue
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0.0, k
    # the default model on the same weights runs the cross-entropy: another number
    plain = S._head("classification", seed=11, class_weights=WEIGHTS).cuda().train()
    assert float(plain.training_step(batch, 0).detach()) != float(loss.detach())


def test_twenty_radam_steps_on_one_batch_lower_the_focal_loss():
    model = S._head("classification", seed=12, learning_rate=1e-2, **LOSS).cuda().train()
    batch = S._cuda(S._batch(32, seed=4))
    opt = model.configure_optimizers()["optimizer"]
    losses = []
    for _ in range(20):
        opt.zero_grad(set_to_none=True)
        loss = model.training_step(batch, 0)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print("focal loss over twenty steps:", [round(v, 5) for v in losses])
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]


@pytest.mark.parametrize("frozen", [False, True])
def test_graphed_focal_step_equals_eager_steps(frozen):
    from multimodal_supernovae_amd.trainer import GraphedTrainStep
    steps = 9                                           # crosses RAdam's rectification switch (rho_t > 5 from step 6)
    batches = [S._cuda(S._batch(8, seed=s)) for s in range(steps)]
    eager = S._head("classification", seed=7, freeze_backbone=frozen, learning_rate=3e-3, class_weights=WEIGHTS,
                    optimizer_kwargs={"weight_decay": 1e-3}, **LOSS).cuda().train()
    graphed = copy.deepcopy(eager)
    opt_e = eager.configure_optimizers()["optimizer"]
    losses_e = []
    for b in batches:
        opt_e.zero_grad(set_to_none=True)
        loss = eager.training_step(b, 0)
        loss.backward()
        opt_e.step()
        losses_e.append(float(loss.detach()))
    step = GraphedTrainStep(graphed, graphed.configure_optimizers()["optimizer"], warmup=3)
    losses_g = [float(step(b).detach()) for b in batches]
    assert step.graph is not None and step.calls == steps
    torch.cuda.synchronize()
    for a, b in zip(losses_e, losses_g):
        assert abs(a - b) <= 1e-5 * abs(a), (losses_e, losses_g)
    for (k, p), (_, q) in zip(eager.named_parameters(), graphed.named_parameters()):
        torch.testing.assert_close(q, p, rtol=1e-5, atol=1e-7, msg=lambda m: f"{k}: {m}")
    assert losses_e[0] != losses_e[-1]


@pytest.mark.parametrize("graphed", [False, True])
def test_trainer_fit_logs_the_focal_validation_loss_and_the_metrics(graphed):
    from multimodal_supernovae_amd.models_finetune import classification_metrics, focal_loss_reference
    from multimodal_supernovae_amd.trainer import Trainer
    model = S._head("classification", seed=5, n_classes=2, learning_rate=1e-2, **LOSS)
    train = [S._batch(32, seed=s, n_classes=2, separable=True) for s in range(8)]
    val = [S._batch(32, seed=100, n_classes=2, separable=True), S._batch(11, seed=101, n_classes=2, separable=True)]
    tr = Trainer(max_epochs=2, graphed_steps=graphed).fit(model, train, val)
    print("train_loss", tr.history["train_loss"], "val_loss", tr.history["val_loss"], {k: model.logged[k] for k in ("f1_val", "acc_val")})
    assert len(tr.history["train_loss"]) == 2 and len(tr.history["val_loss"]) == 2
    assert tr.history["train_loss"][1] < tr.history["train_loss"][0]
    logits = S._predict(model, val)
    y = torch.cat([b[8] for b in val])
    want = classification_metrics(torch.bincount(y * 2 + logits.argmax(1), minlength=4).view(2, 2))
    assert model.logged["f1_val"] == pytest.approx(want["f1_macro"], abs=1e-12)
    assert model.logged["acc_val"] == pytest.approx(want["acc"], abs=1e-12)
    rows = [32.0, 11.0]
    per_batch = [focal_loss_reference(l, b[8], None, 2.0, 0.1)[0] for l, b in zip(logits.split([32, 11]), val)]
    assert tr.history["val_loss"][-1] == pytest.approx(sum(p * r for p, r in zip(per_batch, rows)) / sum(rows), rel=1e-5)


def test_two_rank_focal_step_equals_single_process_global_batch():
    """Two ranks sharing the GPU over gloo (tools/dist_check_focal.py): loss and gradients of the data-parallel focal step
    with label smoothing equal the single-process step at the doubled batch, unweighted and with class weights whose sums
    differ between the ranks; both ranks report the same train_loss."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "dist_check_focal.py")], capture_output=True, text=True,
                       timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "DIST CHECK OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
