"""tests/infonce_refs.py against itself and against the oracle, on the CPU: the plan mirror reproduces the library's workspace size,
the fp64 references agree with oracle/loss.py and oracle/sharded.py, every input family has the property it is built for, the fp32
emulation of the kernels' arithmetic order stays inside every derived bound, and each injected defect makes the comparison that
tests/test_infonce_pinned_gpu.py runs fail on a named case."""
import functools
import math

import pytest
import torch

import infonce_refs as R

F64 = torch.float64
CPU_CASES = [n for n in R.CASES if n != "sh8187_o4000"] + ["sh8187_o4000"]


@functools.lru_cache(maxsize=None)
def bundle(name, family, swapped=False, grad_out=None):
    case = R.CASES[name][0]
    inp = R.make_inputs(family, case, swapped)
    g = R.grad_out_of(name, family) if grad_out is None else grad_out
    args, fref, lses, bref = R.softmax_refs(inp, case, g)
    return case, inp, g, args, fref, lses, bref


def run_softmax(name, family, swapped=False, defect=None, grad_out=None):
    case, inp, g, args, fref, lses, bref = bundle(name, family, swapped, grad_out)
    fwd = R.emulate_softmax_forward(*args, defect=defect)
    bwd = R.emulate_softmax_backward(*args, *lses, g, defect=defect)
    bad_f, r_f = R.failures(fwd, fref)
    bad_b, r_b = R.failures(bwd, bref)
    return bad_f + bad_b, {**r_f, **r_b}


@functools.lru_cache(maxsize=None)
def sigmoid_bundle(name, family, grad_out):
    case = R.CASES[name][0]
    inp = R.make_inputs(family, case)
    e1l, e2l = R.local_rows(inp, case)
    args = (e1l, e2l, inp["e1_all"], inp["e2_all"], case.q_offset, inp["log_scale"], inp["bias"])
    return args, R.sigmoid_forward_ref(*args), R.sigmoid_backward_ref(*args, grad_out)


def run_sigmoid(name, family, grad_out=0.37, defect=None):
    args, fref, bref = sigmoid_bundle(name, family, grad_out)
    bad_f, r_f = R.failures(R.emulate_sigmoid_forward(*args, defect=defect), fref)
    bad_b, r_b = R.failures(R.emulate_sigmoid_backward(*args, grad_out, defect=defect), bref)
    return bad_f + bad_b, {**r_f, **r_b}


# ------------------------------------------------------------------------------------------------------------ the plan
def test_plan_mirror_reproduces_the_workspace_size():
    import __graft_entry__ as entry
    entry.build()
    from multimodal_supernovae_amd import _lib
    L = _lib.lib()
    shapes = [(c.b1, c.b2, c.n1, c.n2, c.D) for c, _ in R.CASES.values()]
    shapes += [(n, n, n, n, d) for n in (1, 128, 129, 1000, 1024, 4096, 8192, 20000) for d in (1, 64, 128, 256, 288, 512, 1024)]
    shapes += [(96, 96, 768, 768, 128), (96, 96, 768, 768, 512), (7, 300, 9000, 700, 96), (2048, 2048, 16384, 16384, 768)]
    for s in shapes:
        assert L.msn_infonce_workspace_bytes(*s) == R.plan(*s).total, s


@pytest.mark.parametrize("name", list(R.CASES))
def test_cases_reach_the_plan_features_they_claim(name):
    case, want = R.CASES[name]
    assert R.plan_features(case) == want
    pl = R.plan(case.b1, case.b2, case.n1, case.n2, case.D)
    assert pl.wide == name.startswith("w")
    if name in ("sh8187_o4000", "wsh2040_d512"):
        assert pl.ksplit == 64
    if name == "wsh2080_d512":
        assert pl.capped and pl.ksplit == 33
    if name.startswith("sh2100"):
        assert math.ceil(pl.ksplit / 8) == 3 and case.q_offset // pl.keys_per_split == {0: 0, 1056: 8, 2068: 16}[case.q_offset]


# ------------------------------------------------------------------------------------------------------------ references == oracle
@pytest.mark.parametrize("name", ["n33_d8", "n300_d100", "r70x45_d32", "r45x200_d32"])
def test_softmax_reference_is_the_oracle_loss_and_its_gradient(name):
    from oracle.loss import clip_loss
    case, inp, _, args, fref, (lr, lc), _ = bundle(name, "flat")
    g = -2.5
    a, b = inp["e1_all"].double().requires_grad_(), inp["e2_all"].double().requires_grad_()
    s, c = inp["log_scale"].double().requires_grad_(), inp["bias"].double().requires_grad_()
    loss = clip_loss(a, b, s, c)
    (g * loss).backward()
    bref = R.softmax_backward_ref(*args, fref["lse_row"], fref["lse_col"], g)          # the unrounded log-sum-exps: the true gradient
    torch.testing.assert_close(fref["loss"], loss.detach(), rtol=1e-12, atol=1e-13)
    torch.testing.assert_close(bref["dE1"], a.grad, rtol=1e-9, atol=1e-13)
    torch.testing.assert_close(bref["dE2"], b.grad, rtol=1e-9, atol=1e-13)
    torch.testing.assert_close(bref["dscale"], s.grad, rtol=1e-9, atol=1e-12)
    torch.testing.assert_close(bref["dbias"], c.grad, rtol=0, atol=1e-12)


@pytest.mark.parametrize("name", ["sh2100_o1056", "sh300_b40x24", "r70x45_d32"])
def test_sharded_reference_is_the_sharded_oracle(name):
    from oracle.sharded import OraclePairKernels as O
    case, inp, g, args, fref, (lr, lc), bref = bundle(name, "unnormalised")
    d = [t.double() for t in args[:4]]
    ls, b = inp["log_scale"].double(), inp["bias"].double()
    o_lr, o_lc, o_loss = O.forward(*d, case.q_offset, ls, b)
    torch.testing.assert_close(fref["lse_row"], o_lr, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(fref["lse_col"], o_lc, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(fref["loss"], o_loss, rtol=1e-12, atol=1e-14)
    o1, o2, os_, ob = O.backward(*d, case.q_offset, ls, b, lr.double(), lc.double(), torch.tensor(g, dtype=F64))
    for got, want in ((bref["dE1"], o1), (bref["dE2"], o2), (bref["dscale"], os_), (bref["dbias"], ob)):
        torch.testing.assert_close(got, want, rtol=1e-9, atol=1e-14)


def test_sharded_shares_sum_to_the_dense_oracle():
    """two ranks' loss shares and dscale / dbias add up to the unsharded values; their dE rows are the unsharded rows"""
    from oracle.loss import clip_loss, sigmoid_loss
    n, D, b = 70, 12, 35
    inp = R.make_inputs("unnormalised", R.make_case(n, n, n, n, D))
    e1, e2, ls, bias = inp["e1_all"], inp["e2_all"], inp["log_scale"], inp["bias"]
    lr, lc = R.lse_all_ref(e1, e2, ls, bias)
    for fn, fwd, bwd in ((clip_loss, R.softmax_forward_ref, lambda *a: R.softmax_backward_ref(*a[:-1], lr, lc, a[-1])),
                         (sigmoid_loss, R.sigmoid_forward_ref, R.sigmoid_backward_ref)):
        a, c = e1.double().requires_grad_(), e2.double().requires_grad_()
        s, bb = ls.double().requires_grad_(), bias.double().requires_grad_()
        want = fn(a, c, s, bb)
        (0.37 * want).backward()
        tot, ds, db = 0.0, 0.0, 0.0
        for o in (0, b):
            args = (e1[o:o + b], e2[o:o + b], e1, e2, o, ls, bias)
            tot = tot + fwd(*args)["loss"]
            r = bwd(*args, 0.37)
            torch.testing.assert_close(r["dE1"], a.grad[o:o + b], rtol=1e-9, atol=1e-14)
            torch.testing.assert_close(r["dE2"], c.grad[o:o + b], rtol=1e-9, atol=1e-14)
            ds, db = ds + r["dscale"], db + r["dbias"]
        torch.testing.assert_close(tot, want.detach(), rtol=1e-12, atol=1e-14)
        torch.testing.assert_close(ds, s.grad, rtol=1e-9, atol=1e-13)
        torch.testing.assert_close(db, bb.grad, rtol=1e-9, atol=1e-13)


def test_rank_reference_is_the_oracle_rank():
    from oracle.clip import roc_data
    inp = R.make_inputs("flat", R.make_case(300, 300, 300, 300, 100))
    ref, _ = R.rank_ref(inp["e1_all"], inp["e2_all"])
    _, _, want = roc_data(inp["e1_all"].double(), inp["e2_all"].double())
    assert (ref.numpy() == want).mean() > 0.99          # the oracle normalises once more: a last-bit tie may move


# ------------------------------------------------------------------------------------------------------------ family properties
@pytest.mark.parametrize("name", CPU_CASES)
def test_hot_family_has_a_hot_key_per_query_at_every_boundary(name):
    case = R.CASES[name][0]
    inp = R.make_inputs("hot", case)
    if case.n1 < 2:
        return
    w = R.hot_weights(inp, case)
    qg = case.q_offset + torch.arange(case.b2)
    assert bool((inp["hot"] != qg).all()) and float(w.min()) >= 0.25 and float(w.max()) <= 0.75, (float(w.min()), float(w.max()))
    pl = R.plan(case.b1, case.b2, case.n1, case.n2, case.D)
    if case.D >= 2:
        for t in range(0, case.b2 - R.QT + 1, R.QT):         # every full query tile aims at every boundary index of its own
            seen = set(inp["hot"][t:t + R.QT].tolist())
            for i in (t, t + R.QT - 1):
                want = set(R.boundaries(pl, case.n1, case.q_offset + i)) - set(range(case.q_offset + t, case.q_offset + t + R.QT))
                assert want <= seen, (t, want - seen)


@pytest.mark.parametrize("name", CPU_CASES)
def test_large_family_overflows_a_plain_exponential_and_stays_finite(name):
    case, inp, _, args, fref, _, bref = bundle(name, "large")
    S = args[1].double() @ args[2].double().T * math.exp(float(inp["log_scale"])) + float(inp["bias"])
    assert 90.0 <= float(S.abs().max()) <= 110.001
    assert not bool(torch.isfinite(torch.exp(S.float()).sum()))
    assert all(bool(torch.isfinite(v).all()) for v in list(fref.values()) + list(bref.values()))


@pytest.mark.parametrize("name", R.SIGMOID_CASES)
def test_large_family_saturates_the_sigmoid_both_ways(name):
    args, fref, bref = sigmoid_bundle(name, "large", 0.37)
    u = fref["z"] * fref["Z"]
    assert float(u.max()) > 88 and float(u.min()) < -88             # both softplus branches, far out
    sg = 1.0 / (1.0 + torch.exp(-u.float()))
    assert bool((sg == 0).any()) and bool((sg == 1).any())
    assert all(bool(torch.isfinite(v).all()) for v in bref.values()) and bool(torch.isfinite(fref["loss"]))


def test_unnormalised_and_integer_families():
    case = R.make_case(300, 300, 300, 300, 100)
    inp = R.make_inputs("unnormalised", case)
    for e in (inp["e1_all"], inp["e2_all"]):
        nrm = e.double().norm(dim=1)
        assert 0.0999 <= float(nrm.min()) < 0.5 and 2.5 < float(nrm.max()) <= 3.0001
    for n, d in R.RANK_CASES:
        inp = R.make_inputs("integer", R.make_case(n, n, n, n, d))
        e1, e2 = inp["e1_all"], inp["e2_all"]
        assert bool((e1 == e1.round()).all()) and float(e1.abs().max()) <= 2 and float(e2.abs().max()) <= 2
        x32, (_, x) = e2 @ e1.T, R.rank_ref(e1, e2)
        assert torch.equal(x32.double(), x)                  # exact in fp32 whatever the order: |x| <= 4 D < 2^24
        ties = (x == x.diagonal()[:, None]).sum(1) - 1
        assert int((ties > 0).sum()) >= n // 8, "exact ties with the partner"


# ------------------------------------------------------------------------------------------------------------ emulation in bounds
@pytest.mark.parametrize("name", CPU_CASES)
def test_emulation_stays_inside_the_softmax_bounds(name):
    worst = {}
    variants = [("hot", False), ("hot", True), ("large", False), ("flat", False), ("unnormalised", False)]
    for family, swapped in variants if name != "sh8187_o4000" else variants[:1]:
        bad, ratios = run_softmax(name, family, swapped)
        assert not bad, (family, swapped, bad)
        worst[family + ("/swapped" if swapped else "")] = max(ratios.values())
    print("\nRATIO emulation softmax", name, " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 0.5          # the head room MARGIN was chosen with


@pytest.mark.parametrize("name", R.SIGMOID_CASES)
def test_emulation_stays_inside_the_sigmoid_bounds(name):
    for family in ("large", "unnormalised"):
        bad, ratios = run_sigmoid(name, family)
        print("\nRATIO emulation sigmoid", name, family, " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))
        assert not bad and max(ratios.values()) <= 0.5, (family, bad)


# ------------------------------------------------------------------------------------------------------------ defects are caught
KEY_CASES = ["n33_d8", "n129_d64", "n300_d100", "sh2100_o1056", "w129_d320", "wsh2040_d512"]


@pytest.mark.parametrize("name", KEY_CASES)
@pytest.mark.parametrize("kind", ["skip_key", "double_key"])
def test_a_key_lost_or_doubled_at_any_boundary_is_caught(kind, name):
    """in one query tile, at every tile, wave and split edge of the case: the log-sum-exp and the gradient both show it"""
    case = R.CASES[name][0]
    pl = R.plan(case.b1, case.b2, case.n1, case.n2, case.D)
    for qtile in sorted({0, (case.b2 - 1) // R.QT}):
        own = range(case.q_offset + qtile * R.QT, case.q_offset + (qtile + 1) * R.QT)
        for at in R.boundaries(pl, case.n1, case.q_offset + qtile * R.QT):
            if at in own and case.D < 2:
                continue
            bad, ratios = run_softmax(name, "hot", defect=(kind, at, qtile))
            assert any(b.startswith("lse_row") for b in bad) and any(b.startswith("dE2") for b in bad), (at, qtile, ratios)


def test_a_lost_key_hides_in_the_flat_family_at_the_old_tolerance():
    """why the hot family exists: on flat inputs at n = 300 the loss moves by less than 1e-3 relative"""
    case, inp, g, args, fref, _, _ = bundle("n300_d100", "flat")
    fwd = R.emulate_softmax_forward(*args, defect=("skip_key", 127, 0))
    assert abs(float(fwd["loss"]) - float(fref["loss"])) < 1e-3 * abs(float(fref["loss"]))


@pytest.mark.parametrize("kind,name,family", [
    ("no_max_subtraction", "n33_d8", "large"), ("no_max_subtraction", "w129_d320", "large"),
    ("merge_without_rescale", "n300_d100", "hot"), ("merge_without_rescale", "sh2100_o1056", "large"),
    ("no_inf_guard", "n129_d64", "flat"), ("no_inf_guard", "r45x200_d32", "flat"), ("no_inf_guard", "w33_d288", "hot"),
    ("local_positive", "sh2100_o1056", "hot"), ("local_positive", "sh300_b40x24", "flat"),
    ("n1_normaliser", "r70x45_d32", "flat"), ("finite_lse_k", "r70x45_d32", "flat"), ("finite_lse_k", "r45x200_d32", "hot"),
    ("no_minus_2_delta", "n33_d8", "flat"), ("no_minus_2_delta", "sh2100_o2068", "large"),
    ("grad_out_ignored", "n5_d5", "hot"), ("dscale_with_bias", "sh2100_o0", "hot"),
])
def test_softmax_defects_are_caught(kind, name, family):
    swapped = kind == "finite_lse_k" and name == "r45x200_d32"          # the keys beyond n are E2 rows there
    bad, ratios = run_softmax(name, family, swapped=swapped, defect=(kind,), grad_out=0.37)
    assert bad, ratios


@pytest.mark.parametrize("kind", ["sigmoid_diag_sign", "grad_out_ignored", "dscale_with_bias"])
@pytest.mark.parametrize("name", ["n33_d8", "sh2100_o1056"])
def test_sigmoid_defects_are_caught(kind, name):
    bad, ratios = run_sigmoid(name, "large", defect=(kind,))
    assert bad, ratios


def test_rank_counting_ties_is_caught():
    for n, d in R.RANK_CASES:
        inp = R.make_inputs("integer", R.make_case(n, n, n, n, d))
        ref, _ = R.rank_ref(inp["e1_all"], inp["e2_all"])
        assert torch.equal(R.emulate_rank(inp["e1_all"], inp["e2_all"]), ref)
        assert not torch.equal(R.emulate_rank(inp["e1_all"], inp["e2_all"], defect=("rank_ge",)), ref)


# ------------------------------------------------------------------------------------------------------------ the rank rule
@pytest.mark.parametrize("n,d,seed", [(1000, 128, 1000), (4096, 128, 4096), (33, 8, 33), (500, 100, 500), (33, 320, 353), (1000, 512, 1512), (33, 1024, 1057)])
def test_rank_rule_leaves_few_rows_undecided_on_the_inputs_of_the_oracle_tests(n, d, seed):
    """The inputs of test_retrieval_ranks_against_oracle in tests/test_infonce_gpu.py and tests/test_infonce_wide_gpu.py: the fp64
    margin alone keeps the rows the rule leaves out far below 1 %, and an fp32 product of fp32-normalised rows passes the rule."""
    g = torch.Generator().manual_seed(seed)
    e1 = torch.randn(n, d, generator=g)
    e2 = e1 + 2.0 * torch.randn(n, d, generator=g)
    a, q = e1 / e1.norm(dim=-1, keepdim=True), e2 / e2.norm(dim=-1, keepdim=True)
    wrong, undecided, rows = R.rank_rule(R.emulate_rank(a, q), e1, e2, normalised=True)
    assert wrong == 0 and undecided <= 0.01 * rows
