"""The contrastive-loss kernels of csrc/infonce.hip and csrc/infonce_wide.hip against the fp64 references and derived per-element
bounds of tests/infonce_refs.py, launch by launch through loss.HipPairKernels.forward / .backward, msn_sigmoid_loss_fwd / _bwd and
msn_retrieval_rank: both log-sum-exp vectors, the loss share, dE1, dE2, dlogit_scale and dlogit_bias, and the ranks.  The backward
is fed the fp32-rounded reference log-sum-exps of every gathered row, not the forward kernel's output.  The cases (infonce_refs.CASES)
are the smallest shapes that reach each path of the key-split plan; their plan features are asserted through the mirror, so a
change of make_plan cannot silently empty one.  Before every launch the blocks the allocator hands out next are filled with NaN:
the workspace and the outputs come from torch.empty, and the kernels promise to need no zeroed scratch.

The gate on every bound is 1; the measured ratios are recorded in the docstring of tests/infonce_refs.py."""
import functools
import math

import pytest
import torch

import infonce_refs as R

pytestmark = pytest.mark.gpu

VARIANTS = (("hot", False), ("hot", True), ("large", False), ("flat", False), ("unnormalised", False))
BIG = ("sh8187_o4000",)                      # forward and backward once per family; hot and large only
SOFTMAX_RUNS = [(n, f, s) for n in R.CASES for f, s in VARIANTS if n not in BIG or f in ("hot", "large") and not s]


def _dev(n):
    """where the fp64 reference is evaluated: on the card once the score slabs are large"""
    return "cuda" if n >= 2000 else "cpu"


def poison(*shapes):
    """fill what the caching allocator will hand out next with NaN"""
    junk = [torch.full(s if isinstance(s, tuple) else (s,), math.nan, dtype=torch.float32, device="cuda") for s in shapes]
    del junk


def ws_floats(case):
    from multimodal_supernovae_amd._lib import lib
    nb = lib().msn_infonce_workspace_bytes(case.b1, case.b2, case.n1, case.n2, case.D)
    assert nb == R.plan(case.b1, case.b2, case.n1, case.n2, case.D).total
    return max(nb, 16) // 4 + 1


@functools.lru_cache(maxsize=None)
def bundle(name, family, swapped, grad_out=None):
    """operands on the card and the references (computed once, never modified)"""
    case = R.CASES[name][0]
    inp = R.make_inputs(family, case, swapped)
    g = R.grad_out_of(name, family) if grad_out is None else grad_out
    args, fref, lses, bref = R.softmax_refs(inp, case, g, _dev(max(case.n1, case.n2)))
    cu = lambda t: t.cuda() if torch.is_tensor(t) else t
    e1a, e2a = cu(args[2]), cu(args[3])
    o = case.q_offset
    dargs = (e1a[o:o + case.b1], e2a[o:o + case.b2], e1a, e2a, o, cu(args[5]), cu(args[6]))
    return case, g, dargs, fref, tuple(cu(t) for t in lses), bref


def show(what, name, family, swapped, ratios):
    print(f"\nRATIO {what} {family}{'/swapped' if swapped else ''} {name} " + " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))


def launch_forward(case, dargs):
    from multimodal_supernovae_amd.loss import HipPairKernels as K
    poison(ws_floats(case), case.b2, case.b1, 1)
    lr, lc, loss = K.forward(*dargs)
    return dict(lse_row=lr, lse_col=lc, loss=loss)


def launch_backward(case, dargs, lses, g):
    from multimodal_supernovae_amd.loss import HipPairKernels as K
    poison(ws_floats(case), (case.b1, case.D), (case.b2, case.D), 2)
    d1, d2, ds, db = K.backward(*dargs, *lses, torch.tensor(g, dtype=torch.float32, device="cuda"))
    return dict(dE1=d1, dE2=d2, dscale=ds, dbias=db)


@pytest.mark.parametrize("name,family,swapped", SOFTMAX_RUNS)
def test_softmax_forward_and_backward(name, family, swapped):
    case, g, dargs, fref, lses, bref = bundle(name, family, swapped)
    assert R.plan_features(case) == R.CASES[name][1]
    bad_f, r_f = R.failures(launch_forward(case, dargs), fref)
    bad_b, r_b = R.failures(launch_backward(case, dargs, lses, g), bref)
    show("softmax", name, family, swapped, {**r_f, **r_b})
    assert not bad_f + bad_b, (bad_f + bad_b, g)


@pytest.mark.parametrize("name", ["n300_d100", "sh2100_o1056", "w129_d320"])
@pytest.mark.parametrize("g", R.GRAD_OUTS)
def test_every_gradient_follows_grad_out(name, g):
    case, g, dargs, _, lses, bref = bundle(name, "hot", False, g)
    bad, ratios = R.failures(launch_backward(case, dargs, lses, g), bref)
    show(f"grad_out={g}", name, "hot", False, ratios)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------ sigmoid loss
def _sigmoid_launch(case, dargs, g):
    from multimodal_supernovae_amd._lib import check, lib, ptr, stream_ptr
    e1l, e2l, e1a, e2a, o, ls, bias = dargs
    L = lib()
    b, D, n = case.b1, case.D, case.n1
    nws = ws_floats(case)
    nb = L.msn_infonce_workspace_bytes(b, b, n, n, D)
    poison(nws, 1)
    ws = torch.empty(nws, dtype=torch.float32, device="cuda")
    loss = torch.empty((), dtype=torch.float32, device="cuda")
    check(L.msn_sigmoid_loss_fwd(ptr(e1l), e1l.stride(0), ptr(e2l), e2l.stride(0), b, ptr(e1a), e1a.stride(0), ptr(e2a), e2a.stride(0),
                                 n, D, o, ptr(ls), ptr(bias), ptr(loss), ptr(ws), nb, stream_ptr()), "msn_sigmoid_loss_fwd")
    out = dict(loss=loss.clone())
    del ws, loss
    poison(nws, (b, D), (b, D), 2)
    ws = torch.empty(nws, dtype=torch.float32, device="cuda")
    d1, d2 = torch.empty((b, D), dtype=torch.float32, device="cuda"), torch.empty((b, D), dtype=torch.float32, device="cuda")
    dsb = torch.empty(2, dtype=torch.float32, device="cuda")
    gt = torch.tensor(g, dtype=torch.float32, device="cuda")
    check(L.msn_sigmoid_loss_bwd(ptr(e1l), e1l.stride(0), ptr(e2l), e2l.stride(0), b, ptr(e1a), e1a.stride(0), ptr(e2a), e2a.stride(0),
                                 n, D, o, ptr(ls), ptr(bias), ptr(gt), ptr(d1), D, ptr(d2), D, ptr(dsb), ptr(ws), nb, stream_ptr()),
          "msn_sigmoid_loss_bwd")
    out.update(dE1=d1, dE2=d2, dscale=dsb[0], dbias=dsb[1])
    return out


@pytest.mark.parametrize("family", ["large", "unnormalised"])
@pytest.mark.parametrize("name", R.SIGMOID_CASES)
def test_sigmoid_forward_and_backward(name, family):
    case = R.CASES[name][0]
    assert R.plan_features(case) == R.CASES[name][1]
    inp = R.make_inputs(family, case)
    g = R.grad_out_of(name, family)
    dev = _dev(case.n1)
    e1a, e2a = inp["e1_all"].to(dev), inp["e2_all"].to(dev)
    o = case.q_offset
    args = (e1a[o:o + case.b1], e2a[o:o + case.b2], e1a, e2a, o, inp["log_scale"], inp["bias"])
    fref, bref = R.sigmoid_forward_ref(*args), R.sigmoid_backward_ref(*args, g)
    c1, c2 = e1a.cuda(), e2a.cuda()
    got = _sigmoid_launch(case, (c1[o:o + case.b1], c2[o:o + case.b2], c1, c2, o, inp["log_scale"].cuda(), inp["bias"].cuda()), g)
    bad_f, r_f = R.failures({"loss": got.pop("loss")}, fref)
    bad_b, r_b = R.failures(got, bref)
    show("sigmoid", name, family, False, {**r_f, **r_b})
    assert not bad_f + bad_b, (bad_f + bad_b, g)
    if family == "large":                     # the saturated entries gave exact zeros and ones, nothing non-finite
        assert all(bool(torch.isfinite(v).all()) for v in got.values())


# ------------------------------------------------------------------------------------------------------------ ranks
def _rank_launch(e1, e2):
    from multimodal_supernovae_amd._lib import check, lib, ptr, stream_ptr
    n, d = e1.shape
    L = lib()
    nb = L.msn_infonce_workspace_bytes(n, n, n, n, d)
    poison(max(nb, 16) // 4 + 1, n)
    ws = torch.empty(max(nb, 16) // 4 + 1, dtype=torch.float32, device="cuda")
    rank = torch.empty(n, dtype=torch.int32, device="cuda")
    check(L.msn_retrieval_rank(ptr(e1), e1.stride(0), ptr(e2), e2.stride(0), n, d, ptr(rank), ptr(ws), nb, stream_ptr()), "msn_retrieval_rank")
    return rank


@pytest.mark.parametrize("n,d", R.RANK_CASES)
def test_ranks_are_exact_on_integers_ties_included(n, d):
    inp = R.make_inputs("integer", R.make_case(n, n, n, n, d))
    ref, x = R.rank_ref(inp["e1_all"], inp["e2_all"])
    assert int(((x == x.diagonal()[:, None]).sum(1) > 1).sum()) > 0
    got = _rank_launch(inp["e1_all"].cuda(), inp["e2_all"].cuda())
    assert torch.equal(got.cpu().long(), ref)


# ------------------------------------------------------------------------------------------------------------ layout, determinism
@pytest.mark.parametrize("name", ["n300_d100", "w129_d320"])
def test_strided_and_misaligned_views_against_the_reference(name):
    """The operands as column slices of one packed (n, 2 D + 4) buffer (the all-gather layout): E1 at column 0 (row-strided, 16-byte
    aligned: the vector loads), E2 one float past column D (not aligned: the scalar loads).  Compared with the reference bounds,
    and with the contiguous call bit for bit."""
    case, g, dargs, fref, lses, bref = bundle(name, "hot", False)
    D = case.D
    pack = torch.full((case.n1, 2 * D + 4), math.nan, device="cuda")
    pack[:, :D], pack[:, D + 1:2 * D + 1] = dargs[2], dargs[3]
    e1, e2 = pack[:, :D], pack[:, D + 1:2 * D + 1]
    assert e1.stride(0) % 4 == 0 and e1.data_ptr() % 16 == 0 and e2.data_ptr() % 16 != 0
    sargs = (e1, e2, e1, e2, 0, dargs[5], dargs[6])
    fwd, bwd = launch_forward(case, sargs), launch_backward(case, sargs, lses, g)
    bad_f, r_f = R.failures(fwd, fref)
    bad_b, r_b = R.failures(bwd, bref)
    show("strided", name, "hot", False, {**r_f, **r_b})
    assert not bad_f + bad_b, bad_f + bad_b
    cf, cb = launch_forward(case, dargs), launch_backward(case, dargs, lses, g)
    assert all(torch.equal(fwd[k], cf[k]) for k in fwd) and all(torch.equal(bwd[k], cb[k]) for k in bwd)


@pytest.mark.parametrize("name", ["n33_d5", "sh2100_o1056", "wsh2040_d512"])
def test_the_same_call_twice_gives_the_same_bits(name):
    case, g, dargs, _, lses, _ = bundle(name, "hot", False)
    a, b = launch_forward(case, dargs), launch_forward(case, dargs)
    assert all(torch.equal(a[k], b[k]) for k in a)
    a, b = launch_backward(case, dargs, lses, g), launch_backward(case, dargs, lses, g)
    assert all(torch.equal(a[k], b[k]) for k in a)
