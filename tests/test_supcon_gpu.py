"""The label-aware contrastive kernels of csrc/supcon.hip against the fp64 references and derived bounds of tests/supcon_refs.py,
launch by launch through loss.HipSupConKernels.forward / .backward: the exact counts, both log-sum-exp vectors, the loss share, dE1,
dE2, dlogit_scale and dlogit_bias.  The backward is fed the fp32-rounded reference log-sum-exps of every gathered row and the
reference counts, not the forward kernel's output.  The cases are the narrow, square cases of infonce_refs.CASES (the smallest
shapes that reach each path of the key-split plan; their plan features are asserted), the label patterns are dealt over the (case,
family) pairs.  Before every launch the blocks the allocator hands out next are filled with NaN.  Then the public functions against
loss.supcon_reference, and the model under loss="supcon": eager, twenty optimizer steps, and recorded as a graph.

The gate on every bound is 1; the measured ratios are recorded in the docstring of tests/supcon_refs.py."""
import copy
import functools
import gc
import math

import pytest
import torch

import infonce_refs as R
import supcon_refs as SR

pytestmark = pytest.mark.gpu


def _dev(n):
    """where the fp64 reference is evaluated: on the card once the score slabs are large"""
    return "cuda" if n >= 2000 else "cpu"


def poison(*shapes):
    """fill what the caching allocator will hand out next with NaN (as float32 words: a NaN there is a huge int32 too)"""
    junk = [torch.full(s if isinstance(s, tuple) else (s,), math.nan, dtype=torch.float32, device="cuda") for s in shapes]
    del junk


def ws_floats(case):
    from multimodal_supernovae_amd._lib import lib
    nb = lib().msn_supcon_workspace_bytes(case.b1, case.b2, case.n1, case.n2, case.D)
    pl = R.plan(case.b1, case.b2, case.n1, case.n2, case.D)
    assert nb == pl.total + R.cdiv(4 * 2 * pl.ksplit * pl.maxq, 256) * 256
    return max(nb, 16) // 4 + 1


@functools.lru_cache(maxsize=None)
def bundle(name, family, pattern, grad_out=None):
    """operands on the card and the references (computed once, never modified)"""
    case = R.CASES[name][0]
    inp = R.make_inputs(family, case)
    y = SR.labels_for(name, pattern)
    g = R.grad_out_of(name, family) if grad_out is None else grad_out
    args, fref, lses, bref = SR.refs(inp, case, y, g, _dev(case.n1))
    cu = lambda t: t.cuda() if torch.is_tensor(t) else t
    e1a, e2a = cu(args[2]), cu(args[3])
    o = case.q_offset
    dargs = (e1a[o:o + case.b1], e2a[o:o + case.b2], e1a, e2a, y.to(torch.int32).cuda(), o, cu(args[6]), cu(args[7]))
    return case, g, dargs, fref, tuple(cu(t) for t in lses), bref


def show(what, name, family, pattern, ratios):
    print(f"\nRATIO {what} {family} {pattern} {name} " + " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))


def launch_forward(case, dargs):
    from multimodal_supernovae_amd.loss import HipSupConKernels as K
    poison(ws_floats(case), case.b2, case.b1, case.b1, 1)
    lr, lc, cnt, loss = K.forward(*dargs)
    return dict(lse_row=lr, lse_col=lc, cnt=cnt, loss=loss)


def launch_backward(case, dargs, lses, cnt, g):
    from multimodal_supernovae_amd.loss import HipSupConKernels as K
    poison(ws_floats(case), (case.b1, case.D), (case.b2, case.D), 2)
    d1, d2, ds, db = K.backward(*dargs, *lses, cnt, torch.tensor(g, dtype=torch.float32, device="cuda"))
    return dict(dE1=d1, dE2=d2, dscale=ds, dbias=db)


def ref_cnt(fref):
    return fref["cnt"].to(torch.int32).cuda()


@pytest.mark.parametrize("name,family,pattern", SR.RUNS + [SR.BIG])
def test_forward_and_backward(name, family, pattern):
    case, g, dargs, fref, lses, bref = bundle(name, family, pattern)
    assert R.plan_features(case) == R.CASES[name][1]
    fwd = launch_forward(case, dargs)
    assert torch.equal(fwd["cnt"].cpu().long(), fref["cnt"].cpu().long())
    bad_f, r_f = SR.failures(fwd, fref)
    bad_b, r_b = SR.failures(launch_backward(case, dargs, lses, ref_cnt(fref), g), bref)
    show("supcon", name, family, pattern, {**r_f, **r_b})
    assert not bad_f + bad_b, (bad_f + bad_b, g)


@pytest.mark.parametrize("name,pattern", [("n300_d100", "strided"), ("sh2100_o1056", "sparse")])
@pytest.mark.parametrize("g", R.GRAD_OUTS)
def test_every_gradient_follows_grad_out(name, pattern, g):
    case, g, dargs, fref, lses, bref = bundle(name, "hot", pattern, g)
    bad, ratios = SR.failures(launch_backward(case, dargs, lses, ref_cnt(fref), g), bref)
    show(f"grad_out={g}", name, "hot", pattern, ratios)
    assert not bad, bad


@pytest.mark.parametrize("name", ["n33_d5", "n300_d130", "sh2100_o2068"])
def test_rows_past_b_are_never_written(name):
    """outputs handed over as the first rows of larger buffers: the sentinel rows behind them keep their bits"""
    from multimodal_supernovae_amd._lib import check, lib, ptr, stream_ptr
    case, g, dargs, fref, lses, bref = bundle(name, "flat", "five")
    e1l, e2l, e1a, e2a, y, o, ls, bias = dargs
    b, D, n = case.b1, case.D, case.n1
    L = lib()
    nb = L.msn_supcon_workspace_bytes(b, b, n, n, D)
    sent = 12345.0
    ws = torch.full((max(nb, 16) // 4 + 1 + 64,), math.nan, device="cuda")
    lr, lc = torch.full((b + 7,), sent, device="cuda"), torch.full((b + 7,), sent, device="cuda")
    cnt = torch.full((b + 7,), -77, dtype=torch.int32, device="cuda")
    loss = torch.full((3,), sent, device="cuda")
    check(L.msn_supcon_fwd(ptr(e1l), e1l.stride(0), b, ptr(e2l), e2l.stride(0), b, ptr(e1a), e1a.stride(0), n, ptr(e2a), e2a.stride(0), n,
                           D, o, ptr(y), ptr(ls), ptr(bias), ptr(lr), ptr(lc), ptr(cnt), ptr(loss), ptr(ws), nb, stream_ptr()), "msn_supcon_fwd")
    assert bool((lr[b:] == sent).all()) and bool((lc[b:] == sent).all()) and bool((cnt[b:] == -77).all()) and bool((loss[1:] == sent).all())
    assert bool(torch.isnan(ws[nb // 4 + 1:]).all())
    bad, _ = SR.failures(dict(lse_row=lr[:b], lse_col=lc[:b], cnt=cnt[:b], loss=loss[0]), fref)
    assert not bad, bad
    d1, d2 = torch.full((b + 5, D + 3), sent, device="cuda"), torch.full((b + 5, D + 3), sent, device="cuda")
    dsb = torch.full((5,), sent, device="cuda")
    gt = torch.tensor(g, dtype=torch.float32, device="cuda")
    ws.fill_(math.nan)
    check(L.msn_supcon_bwd(ptr(e1l), e1l.stride(0), b, ptr(e2l), e2l.stride(0), b, ptr(e1a), e1a.stride(0), n, ptr(e2a), e2a.stride(0), n,
                           D, o, ptr(y), ptr(ls), ptr(bias), ptr(lses[0]), ptr(lses[1]), ptr(ref_cnt(fref)), ptr(gt), ptr(d1), D + 3,
                           ptr(d2), D + 3, ptr(dsb), ptr(ws), nb, stream_ptr()), "msn_supcon_bwd")
    for d in (d1, d2):
        assert bool((d[b:] == sent).all()) and bool((d[:, D:] == sent).all())
    assert bool((dsb[2:] == sent).all()) and bool(torch.isnan(ws[nb // 4 + 1:]).all())
    bad, _ = SR.failures(dict(dE1=d1[:b, :D], dE2=d2[:b, :D], dscale=dsb[0], dbias=dsb[1]), bref)
    assert not bad, bad


@pytest.mark.parametrize("name,pattern", [("n33_d5", "unknown"), ("n300_d100", "strided"), ("sh2100_o1056", "five")])
def test_the_same_call_twice_gives_the_same_bits(name, pattern):
    case, g, dargs, fref, lses, _ = bundle(name, "hot", pattern)
    a, b = launch_forward(case, dargs), launch_forward(case, dargs)
    assert all(torch.equal(a[k], b[k]) for k in a)
    a, b = launch_backward(case, dargs, lses, ref_cnt(fref), g), launch_backward(case, dargs, lses, ref_cnt(fref), g)
    assert all(torch.equal(a[k], b[k]) for k in a)


def test_strided_and_misaligned_views_give_the_same_bits():
    """The operands as column slices of one packed (n, 2 D + 4) buffer (the all-gather layout): E1 at column 0 (row-strided, 16-byte
    aligned: the vector loads), E2 one float past column D (not aligned: the scalar loads).  Held to the reference bounds, and to
    the contiguous call bit for bit."""
    name, pattern = "n300_d100", "strided"
    case, g, dargs, fref, lses, bref = bundle(name, "hot", pattern)
    D = case.D
    pack = torch.full((case.n1, 2 * D + 4), math.nan, device="cuda")
    pack[:, :D], pack[:, D + 1:2 * D + 1] = dargs[2], dargs[3]
    e1, e2 = pack[:, :D], pack[:, D + 1:2 * D + 1]
    assert e1.stride(0) % 4 == 0 and e1.data_ptr() % 16 == 0 and e2.data_ptr() % 16 != 0
    sargs = (e1, e2, e1, e2) + dargs[4:]
    fwd, bwd = launch_forward(case, sargs), launch_backward(case, sargs, lses, ref_cnt(fref), g)
    bad_f, r_f = SR.failures(fwd, fref)
    bad_b, r_b = SR.failures(bwd, bref)
    show("strided", name, "hot", pattern, {**r_f, **r_b})
    assert not bad_f + bad_b, bad_f + bad_b
    cf, cb = launch_forward(case, dargs), launch_backward(case, dargs, lses, ref_cnt(fref), g)
    assert all(torch.equal(fwd[k], cf[k]) for k in fwd) and all(torch.equal(bwd[k], cb[k]) for k in bwd)


@pytest.mark.parametrize("name", ["n33_d12", "n300_d130", "sh2100_o1056"])
def test_distinct_labels_agree_with_the_infonce_kernels(name):
    """all labels distinct: the loss is clip_loss -- both kernels are within their own bounds of their fp64 references, and those
    references are the same numbers, so the kernels differ by no more than the sum of the two bounds"""
    from multimodal_supernovae_amd.loss import HipPairKernels as K
    case, g, dargs, fref, lses, bref = bundle(name, "flat", "distinct")
    e1l, e2l, e1a, e2a, y, o, ls, bias = dargs
    inp = R.make_inputs("flat", case)
    _, nfref, _, nbref = R.softmax_refs(inp, case, g, _dev(case.n1))
    fwd, bwd = launch_forward(case, dargs), launch_backward(case, dargs, lses, ref_cnt(fref), g)
    assert bool((fwd["cnt"] == 1).all())
    lr, lc, loss = K.forward(e1l, e2l, e1a, e2a, o, ls, bias)
    d1, d2, ds, db = K.backward(e1l, e2l, e1a, e2a, o, ls, bias, *lses, torch.tensor(g, dtype=torch.float32, device="cuda"))
    for key, ours, theirs, r1, r2 in (("lse_row", fwd["lse_row"], lr, fref, nfref), ("lse_col", fwd["lse_col"], lc, fref, nfref),
                                      ("loss", fwd["loss"], loss, fref, nfref), ("dE1", bwd["dE1"], d1, bref, nbref),
                                      ("dE2", bwd["dE2"], d2, bref, nbref), ("dscale", bwd["dscale"], ds, bref, nbref),
                                      ("dbias", bwd["dbias"], db, bref, nbref)):
        bound = (r1["b_" + key] + r2["b_" + key]).to("cuda")
        err = (ours.double() - theirs.double()).abs()
        assert bool((err <= bound).all()), (key, float((err / bound).max()))


def test_the_c_abi_refuses_before_a_launch():
    from multimodal_supernovae_amd import _lib
    L = _lib.lib()
    p, s = _lib.ptr, _lib.stream_ptr()
    X = torch.zeros(8, 300, device="cuda")
    y = torch.zeros(8, dtype=torch.int32, device="cuda")
    f = torch.zeros(8, device="cuda")
    one = torch.zeros((), device="cuda")
    ws = torch.zeros(1 << 14, device="cuda")
    fwd = lambda b1, b2, n1, n2, D, o, nb: L.msn_supcon_fwd(p(X), 300, b1, p(X), 300, b2, p(X), 300, n1, p(X), 300, n2, D, o, p(y), p(one),
                                                           p(one), p(f), p(f), p(y), p(one), p(ws), nb, s)
    assert fwd(8, 8, 8, 8, 257, 0, 1 << 16) == 1            # D > 256
    assert fwd(8, 7, 8, 8, 16, 0, 1 << 16) == 1             # b1 != b2
    assert fwd(8, 8, 8, 7, 16, 0, 1 << 16) == 1             # n1 != n2
    assert fwd(4, 4, 8, 8, 16, 5, 1 << 16) == 1             # q_offset + b > n
    assert fwd(8, 8, 8, 8, 16, 0, 8) == 1                   # workspace too small
    assert L.msn_supcon_workspace_bytes(8, 8, 8, 8, 257) == 0 and L.msn_supcon_workspace_bytes(8, 7, 8, 8, 16) == 0
    torch.cuda.synchronize()
    assert float(f.abs().sum()) == 0.0 and float(one) == 0.0 and int(y.abs().sum()) == 0


def test_non_finite_inputs_propagate():
    case, g, dargs, fref, lses, _ = bundle("n33_d5", "flat", "five")
    e1a = dargs[2].clone()
    e1a[7, 2] = math.nan
    nargs = (e1a, dargs[1], e1a, dargs[3]) + dargs[4:]
    fwd = launch_forward(case, nargs)
    assert bool(torch.isnan(fwd["loss"])) and torch.equal(fwd["cnt"].cpu().long(), fref["cnt"].cpu().long())
    bwd = launch_backward(case, nargs, lses, ref_cnt(fref), g)
    assert bool(torch.isnan(bwd["dE2"]).any()) and bool(torch.isnan(bwd["dscale"]))


# ------------------------------------------------------------------------------------------------------------ through Python
def _loss_bound(embs, y, scales, biases):
    """the loss bound of supcon_refs summed over the pairs"""
    total = 0.0
    pairs = [(i, j) for i in range(len(embs)) for j in range(i + 1, len(embs))]
    for k, (i, j) in enumerate(pairs):
        s = scales if scales.dim() == 0 else scales[k]
        b = biases if biases.dim() == 0 else biases[k]
        total += float(SR.forward_ref(embs[i], embs[j], embs[i], embs[j], y, 0, float(s), float(b))["b_loss"])
    return total


@pytest.mark.parametrize("m", [2, 3])
def test_public_functions_against_the_reference(m):
    from multimodal_supernovae_amd.loss import supcon_loss, supcon_loss_multimodal, supcon_reference
    n, d, up = 150, 24, -1.7
    g = R.gen(40 + m)
    cpu = [torch.nn.functional.normalize(torch.randn(n, d, generator=g), dim=1) for _ in range(m)]
    y = SR.make_labels("unknown", n, seed=m)
    pairs = m * (m - 1) // 2
    scales = torch.tensor([2.0, 2.5, 1.5][:pairs]) if m == 3 else torch.tensor(2.3)
    biases = torch.tensor([0.2, -1.0, 0.0][:pairs]) if m == 3 else torch.tensor(-0.5)
    embs = [e.cuda().requires_grad_(True) for e in cpu]
    sc, bi = scales.cuda().requires_grad_(True), biases.cuda().requires_grad_(True)
    labels = y.cuda() if m == 3 else y.to(torch.float32).cuda()          # integer and floating labels
    loss = supcon_loss_multimodal(embs, labels, sc, bi) if m == 3 else supcon_loss(embs[0], embs[1], labels, sc, bi)
    (up * loss).backward()
    rl, rdE, rds, rdb = supcon_reference(cpu, y, scales, biases)
    assert abs(float(loss.detach()) - float(rl)) <= _loss_bound(cpu, y, scales, biases) + 2.0 ** -24 * pairs * abs(float(rl))
    # the gradients: the backward of the public path takes the forward kernel's LSEs, which are within their bounds of the fp64
    # ones, so each pair's launch is within backward_ref's bounds widened by that (d_lse_*); the pairs' bounds add up, with one
    # more rounding per addition of two pairs' gradients
    u = 2.0 ** -24
    bE = [torch.zeros(n, d, dtype=torch.float64) for _ in range(m)]
    bs, bb = torch.zeros(pairs, dtype=torch.float64), torch.zeros(pairs, dtype=torch.float64)
    for k, (i, j) in enumerate([(i, j) for i in range(m) for j in range(i + 1, m)]):
        s = float(scales if scales.dim() == 0 else scales[k])
        b = float(biases if biases.dim() == 0 else biases[k])
        fr = SR.forward_ref(cpu[i], cpu[j], cpu[i], cpu[j], y, 0, s, b)
        br = SR.backward_ref(cpu[i], cpu[j], cpu[i], cpu[j], y, 0, s, b, fr["lse_row"], fr["lse_col"], fr["cnt"], up,
                             d_lse_row=fr["b_lse_row"] / SR.MARGIN, d_lse_col=fr["b_lse_col"] / SR.MARGIN)
        bE[i] += br["b_dE1"]
        bE[j] += br["b_dE2"]
        bs[k], bb[k] = br["b_dscale"], br["b_dbias"]
    for k in range(m):
        want = up * rdE[k]
        err = (embs[k].grad.cpu().double() - want).abs()
        bound = bE[k] + u * (m - 1) * want.abs()
        print(f"\nRATIO python m={m} tower {k} dE={float((err / bound).max()):.3f}")
        assert bool((err <= bound).all()), (k, float((err / bound).max()))
    if scales.dim() == 0:
        bs, bb = bs.sum(0, keepdim=True), bb.sum(0, keepdim=True)
    ds_want, db_want = (up * rds).reshape(-1), (up * rdb).reshape(-1)
    ds_err = (sc.grad.cpu().double().reshape(-1) - ds_want).abs()
    db_err = (bi.grad.cpu().double().reshape(-1) - db_want).abs()
    assert bool((ds_err <= bs + u * pairs * ds_want.abs()).all()), (ds_err, bs)
    assert bool((db_err <= bb + u * pairs * db_want.abs()).all()), (db_err, bb)
    assert labels.grad is None


def test_refusals_on_the_card():
    from multimodal_supernovae_amd import _lib
    from multimodal_supernovae_amd.loss import supcon_loss
    e = torch.randn(6, 8, device="cuda")
    with pytest.raises(_lib.MsnHipError, match="labels must live on the embeddings' device"):
        supcon_loss(e, e, torch.arange(6))
    with pytest.raises(_lib.MsnHipError, match=r"embeddings\[1\] must live on the GPU"):
        supcon_loss(e, e.cpu(), torch.arange(6, device="cuda"))
    with pytest.raises(ValueError, match="labels must hold integer values"):
        supcon_loss(e, e, torch.tensor([0.0, 1.0, 2.5, 1.0, 0.0, 3.0], device="cuda"))


# ------------------------------------------------------------------------------------------------------------ the model
TK = dict(n_out=16, emb=16, heads=2, depth=1, dropout=0.0, time_norm=20583.37, agg="mean")
SK = dict(n_out=16, emb=16, heads=2, depth=1, dropout=0.0, time_norm=17945.14, agg="mean")


def _clip(loss="supcon", **kw):
    from multimodal_supernovae_amd.models_multimodal import LightCurveImageCLIP
    torch.manual_seed(0)
    return LightCurveImageCLIP(enc_dim=32, nband=2, transformer_kwargs=TK, transformer_spectral_kwargs=SK,
                               combinations=["lightcurve", "spectral"], loss=loss, **kw).cuda().train()


def _batch(g, B, T=12, Ts=16, labels=True):
    t = torch.sort(torch.rand(B, T // 2, generator=g) * 100, dim=1)[0].repeat(1, 2)
    y = torch.randint(0, 5, (B,), generator=g)
    return tuple(x.cuda() if x is not None else None for x in (
        None, torch.randn(B, T, generator=g), t, torch.ones(B, T, dtype=torch.bool), torch.randn(B, Ts, generator=g),
        torch.sort(torch.rand(B, Ts, generator=g) * 6000 + 3000, dim=1)[0], torch.ones(B, Ts, dtype=torch.bool),
        torch.rand(B, generator=g), y if labels else None))


def test_one_eager_step_matches_the_loss_of_the_models_own_embeddings():
    from multimodal_supernovae_amd.loss import supcon_reference
    model = _clip()
    batch = _batch(torch.Generator().manual_seed(5), 16)
    seen, inner = {}, model._loss

    def spy(embs, labels=None):
        seen.update(embs=[e.detach().cpu() for e in embs], labels=labels)
        return inner(embs, labels)

    model._loss = spy
    loss = model.training_step(batch, 0)
    assert loss.dtype == torch.float32 and bool(torch.isfinite(loss)) and seen["labels"] is batch[8]
    loss.backward()
    for k, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
    assert float(model.logit_scale.grad.abs()) > 0
    assert torch.equal(model.logged["train_loss"], loss.detach())
    ls, lb = model.logit_scale.detach().cpu(), model.logit_bias.detach().cpu()
    want = supcon_reference(seen["embs"], batch[8].cpu(), ls, lb)[0]
    assert abs(float(loss.detach()) - float(want)) <= _loss_bound(seen["embs"], batch[8].cpu(), ls, lb)
    # the validation step passes the labels too
    model.on_validation_start()
    with torch.no_grad():
        val = model.validation_step(batch, 0)
    assert seen["labels"] is batch[8] and abs(float(val) - float(loss.detach())) <= 1e-5 * abs(float(loss.detach()))


def test_twenty_radam_steps_on_one_batch_lower_the_loss():
    model = _clip(lr=3e-3)
    batch = _batch(torch.Generator().manual_seed(6), 16)
    opt = model.configure_optimizers()["optimizer"]
    losses = []
    for _ in range(20):
        opt.zero_grad(set_to_none=True)
        loss = model.training_step(batch, 0)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    with torch.no_grad():
        losses.append(float(model.training_step(batch, 0)))
    assert all(math.isfinite(v) for v in losses) and losses[-1] < losses[0], losses


def test_graphed_step_equals_eager_steps():
    """The step has no host read: it records into a graph, the labels one more static batch tensor, and replays to what the eager
    steps give (the tolerance of tests/test_graph_gpu.py for its own model)."""
    from multimodal_supernovae_amd.trainer import GraphedTrainStep
    steps = 9
    g = torch.Generator().manual_seed(7)
    batches = [_batch(g, 16) for _ in range(steps)]
    eager = _clip(lr=3e-3, optimizer_kwargs={"weight_decay": 1e-3})
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
    del step, graphed, losses_g                         # the recorded graph is destroyed here, not by a later collection
    gc.collect()


def test_a_batch_without_labels_raises_and_softmax_ignores_them():
    g = torch.Generator().manual_seed(8)
    with_labels = _batch(g, 16)
    without = with_labels[:8] + (None,)
    with pytest.raises(ValueError, match=r"classification.*batch\[8\]"):
        _clip().training_step(without, 0)
    model = _clip(loss="softmax")
    with torch.no_grad():
        a, b = model.training_step(with_labels, 0), model.training_step(without, 0)
    assert torch.equal(a, b)
