"""tests/rownorm_refs.py against itself, against torch and against the oracle, on the CPU: the mirrors of the launch rules reproduce
the library's workspace sizes and every case reaches the path it claims, the fp64 references agree with torch's layer_norm and its
autograd and with oracle.encoders.time_positional_encoding, every input family has the property it is built for, the fp32
emulation of the kernels' arithmetic order stays inside every derived bound, and each injected defect makes the comparison that
tests/test_rownorm_pinned_gpu.py runs fail on a named case."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import rownorm_refs as R

F32, F64 = torch.float32, torch.float64


def strided(t, extra):
    """the same values as rows of a wider NaN-filled buffer (leading dimension cols + extra)"""
    buf = torch.full((t.shape[0], t.shape[1] + extra), math.nan, dtype=t.dtype)
    buf[:, :t.shape[1]] = t
    return buf[:, :t.shape[1]]


@functools.lru_cache(maxsize=None)
def ln_bundle(rows, cols, family, eps, with_add=True):
    inp = R.ln_inputs(family, rows, cols)
    fref = R.ln_forward_ref(inp["x"], inp["gamma"], inp["beta"], eps)
    mean, rstd = fref["mean"].to(F32), fref["rstd"].to(F32)
    bref = R.ln_backward_ref(inp["dy"], inp["x"], mean, rstd, inp["gamma"], inp["add"] if with_add else None)
    return inp, fref, (mean, rstd), bref


def run_ln(rows, cols, family="normal", eps=1e-5, defect=None, with_add=True, ld_extra=0):
    inp, fref, (mean, rstd), bref = ln_bundle(rows, cols, family, eps, with_add)
    x, dy, add = inp["x"], inp["dy"], inp["add"] if with_add else None
    if ld_extra:
        x, dy, add = strided(x, ld_extra), strided(dy, ld_extra + 4), None if add is None else strided(add, ld_extra + 8)
    bad_f, r_f = R.failures(R.emulate_ln_forward(x, inp["gamma"], inp["beta"], eps, defect), fref)
    bad_b, r_b = R.failures(R.emulate_ln_backward(dy, x, mean, rstd, inp["gamma"], add, defect), bref)
    return bad_f + bad_b, {**r_f, **r_b}


@functools.lru_cache(maxsize=None)
def l2_bundle(rows, cols, family):
    inp = R.l2_inputs(family, rows, cols)
    fref = R.l2_forward_ref(inp["x"])
    y, inv = fref["y"].to(F32), fref["inv"].to(F32)
    return inp, fref, (y, inv), R.l2_backward_ref(inp["dy"], y, inv)


def run_l2(rows, cols, family="normal", defect=None):
    inp, fref, (y, inv), bref = l2_bundle(rows, cols, family)
    bad_f, r_f = R.failures(R.emulate_l2_forward(inp["x"], defect), fref)
    bad_b, r_b = R.failures(R.emulate_l2_backward(inp["dy"], y, inv, defect), bref)
    return bad_f + bad_b, {**r_f, **r_b}


def run_te(name, regime, defect=None, integer=False):
    B, T, e, nband = R.TE_CASES[name]
    inp = R.te_inputs(B, T, e, nband, regime, integer)
    args = (inp["x"], inp["t"], inp["w"], inp["bw"], inp["omega"], inp["band"])
    bad_f, r_f = R.failures(R.emulate_te_forward(*args, defect=defect), R.te_forward_ref(*args))
    bad_b, r_b = R.failures(R.emulate_te_backward(inp["dy"], inp["x"], nband, defect), R.te_backward_ref(inp["dy"], inp["x"], nband))
    return bad_f + bad_b, {**r_f, **r_b}


# ------------------------------------------------------------------------------------------------------------ the launch rules
def test_mirrors_reproduce_the_workspace_sizes():
    import __graft_entry__ as entry
    entry.build()
    from multimodal_supernovae_amd import _lib
    L = _lib.lib()
    shapes = [(r, c) for r, c, _ in R.LN_CASES.values()] + [(66560, 384), (204800, 64), (50001, 12), (300, 768)]
    for rows, cols in shapes:
        assert L.msn_layernorm_bwd_workspace_bytes(rows, cols) == R.ln_plan(rows, cols).ws_bytes, (rows, cols)
    for B, T, e, nband in R.TE_CASES.values():
        assert L.msn_time_embed_bwd_workspace_bytes(B, e, nband) == R.te_plan(B, T, e, nband).ws_bytes


def test_dispatch_edges_of_the_row_kernels():
    assert [R.pick_lpr(c) for c in (4, 12, 60, 64, 68, 200, 256, 260, 384, 1020, 1024)] == [4] * 4 + [16] * 3 + [64] * 4
    for lpr, widths in R.WIDTHS.items():
        assert all(R.pick_lpr(c) == lpr for c in widths)
    # partly filled last chunk rounds (padding lanes exist) at every width that is not a multiple of 4 LPR
    assert [R.ln_plan(1, c).padded - c for c in (12, 60, 64, 68, 200, 256, 260, 1020, 1024)] == [4, 4, 0, 60, 56, 0, 252, 4, 0]


@pytest.mark.parametrize("name", list(R.LN_CASES))
def test_layernorm_cases_reach_the_paths_they_claim(name):
    rows, cols, want = R.LN_CASES[name]
    assert R.ln_features(rows, cols) == want
    assert all(n in R.LN_CASES for n in R.FAMILY_CASES + R.BIG_CASES)


def test_case_set_covers_every_path_of_the_issue():
    feats = {R.ln_features(r, c) for r, c, _ in R.LN_CASES.values()}
    for lpr in (4, 16, 64):
        assert {s for l, _, s, _ in feats if l == lpr} >= {1, 15, 16, 17, 64, 65, 512}
        assert (lpr, 2, 512, 5) in feats                   # the second grid-stride pass of the forward, five rounds of the backward
    assert [R.LN_CASES[n][:2] for n in R.BIG_CASES] == [(131137, 64), (32785, 68), (8197, 260)]
    assert all(R.ln_plan(r, c).passes == 2 for r, c in R.TIE_CASES)
    te = {n: R.te_plan(*c) for n, c in R.TE_CASES.items()}
    assert {p.groups for p in te.values()} >= {128, 42, 4, 2, 1}
    assert any(p.col_passes == 2 for p in te.values()) and any(p.idle_groups > 0 for p in te.values())
    assert te[R.TE_BIG].passes == 2 and all(p.passes == 1 for n, p in te.items() if n != R.TE_BIG)
    # the finish kernel: no unrolled trip, the edge b + 48 < B at 48 | 49, one and two unrolled trips, with and without a tail
    assert [R.finish_trips(b) for b in (1, 15, 16, 17, 48, 49, 64, 65, 130)] == [(0, 1), (0, 1), (0, 1), (0, 2), (0, 3), (1, 0), (1, 0), (1, 1), (2, 1)]


# ------------------------------------------------------------------------------------------------------------ references
@pytest.mark.parametrize("rows,cols,eps", [(17, 68, 1e-5), (65, 12, 1e-6), (5, 1020, 1e-5)])
def test_layernorm_reference_is_torch_layer_norm_and_its_gradient(rows, cols, eps):
    inp = R.ln_inputs("normal", rows, cols)
    x, g, b = (inp[k].double().requires_grad_() for k in ("x", "gamma", "beta"))
    y = F.layer_norm(x, (cols,), g, b, eps)
    y.backward(inp["dy"].double())
    fref = R.ln_forward_ref(inp["x"], inp["gamma"], inp["beta"], eps)
    bref = R.ln_backward_ref(inp["dy"], inp["x"], fref["mean"], fref["rstd"], inp["gamma"], inp["add"])   # unrounded statistics
    torch.testing.assert_close(fref["y"], y.detach(), rtol=1e-12, atol=1e-13)
    torch.testing.assert_close(fref["rstd"], 1 / torch.sqrt(x.detach().var(1, unbiased=False) + eps), rtol=1e-12, atol=0)
    torch.testing.assert_close(bref["dx"], x.grad + inp["add"].double(), rtol=1e-10, atol=1e-12)
    torch.testing.assert_close(bref["dgamma"], g.grad, rtol=1e-10, atol=1e-12)
    torch.testing.assert_close(bref["dbeta"], b.grad, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(bref["colsum"], bref["dx"].sum(0), rtol=0, atol=0)


def test_l2norm_reference_is_torch_and_its_gradient():
    inp = R.ln_inputs("normal", 17, 200)
    x = inp["x"].double().requires_grad_()
    y = x / x.norm(dim=-1, keepdim=True)
    y.backward(inp["dy"].double())
    fref = R.l2_forward_ref(inp["x"])
    torch.testing.assert_close(fref["y"], y.detach(), rtol=1e-13, atol=0)
    torch.testing.assert_close(R.l2_backward_ref(inp["dy"], fref["y"], fref["inv"])["dx"], x.grad, rtol=1e-10, atol=1e-13)


@pytest.mark.parametrize("e,nband", [(6, 1), (64, 2), (258, 3)])
def test_time_embed_reference_is_the_oracle_on_benign_arguments(e, nband):
    from oracle.encoders import time_positional_encoding
    B, T, norm = 3, 6, 17945.14
    inp = R.te_inputs(B, T, e, nband, "hundred", norm=norm)
    t = inp["t"] / 100.0                                        # |t omega| <= 1: fp32 sine and cosine are good to 1e-7
    w, bw = inp["w"].clone().requires_grad_(), inp["bw"].clone().requires_grad_()
    want = inp["x"][:, :, None] * w + bw + time_positional_encoding(t, e, norm)
    band = None
    if nband > 1:
        band = inp["band"].clone().requires_grad_()
        want = want + band[torch.arange(nband).repeat_interleave(T // nband)][None]
    ref = R.te_forward_ref(inp["x"], t, inp["w"], inp["bw"], inp["omega"], inp["band"])
    torch.testing.assert_close(ref["out"], want.detach().double(), rtol=0, atol=2e-6)
    want.backward(inp["dy"])
    bref = R.te_backward_ref(inp["dy"], inp["x"], nband)
    torch.testing.assert_close(bref["dw"], w.grad.double(), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(bref["dbw"], bw.grad.double(), rtol=1e-5, atol=1e-5)
    if nband > 1:
        torch.testing.assert_close(bref["dband"], band.grad.double(), rtol=1e-5, atol=1e-5)


# ------------------------------------------------------------------------------------------------------------ family properties
def test_families_have_the_properties_they_are_built_for():
    rows, cols = 65, 64
    inp = R.ln_inputs("constant", rows, cols)
    assert bool((inp["x"] == inp["x"][:, :1]).all()) and bool((inp["x"] != 0).all())
    ref = R.ln_forward_ref(inp["x"], inp["gamma"], inp["beta"], 1e-5)
    assert torch.equal(ref["y"], inp["beta"].double().expand(rows, cols))            # exactly beta in fp64
    assert float(ref["b_y"].min()) > 0
    off = R.ln_inputs("offset", rows, cols)["x"].double()
    assert abs(float(off[0].mean()) - 100) < 1 and abs(float(off[1].mean()) - 1000) < 1 and 0.5 < float(off.std(1).mean()) < 1.5
    wide = R.ln_inputs("wide", rows, cols)["x"].abs()
    assert 2.0 ** -6 <= float(wide.min()) < 2.0 ** -5 and 2.0 ** 5 < float(wide.max()) <= 2.0 ** 6
    assert 1e-16 < float(R.ln_inputs("tiny", rows, cols)["x"].abs().mean()) < 1e-14
    huge = R.ln_inputs("huge", 5, 1024)["x"]
    assert 1e14 < float(huge.abs().mean()) < 1e16 and bool(torch.isfinite((huge * huge).sum(1)).all())   # the contract: finite in fp32
    it = R.ln_inputs("integer", 3585, 64)
    assert all(bool((it[k] == it[k].round()).all()) for k in ("x", "dy", "add")) and bool((it["gamma"] == 1).all()) and bool((it["beta"] == 0).all())
    emu = R.emulate_ln_backward(it["dy"], it["x"], torch.zeros(3585), torch.ones(3585), it["gamma"])
    assert torch.equal(emu["dbeta"].double(), it["dy"].double().sum(0))              # exact whatever the order
    assert torch.equal(R.emulate_ln_forward(it["x"], it["gamma"], it["beta"], 1e-5)["mean"].double(), it["x"].double().mean(1))
    l2 = R.l2_inputs("normal", 17, 68)
    ref = R.l2_forward_ref(l2["x"])
    assert bool(torch.isnan(ref["y"][1]).all()) and math.isinf(float(ref["inv"][1])) and bool(torch.isfinite(ref["y"][[0, 2]]).all())


# ------------------------------------------------------------------------------------------------------------ emulation in bounds
HEADROOM = 0.5               # the head room MARGIN was chosen with


@pytest.mark.parametrize("name", [n for n in R.LN_CASES if n not in R.BIG_CASES] + list(R.BIG_CASES[1:]))
def test_emulation_stays_inside_the_layernorm_bounds(name):
    rows, cols, _ = R.LN_CASES[name]
    worst = {}
    families = R.LN_FAMILIES if name in R.FAMILY_CASES else ("normal", "integer")
    for family in families:
        for eps in R.EPS if name in R.FAMILY_CASES else R.EPS[:1]:
            for ld_extra in (0, 4) if name in R.FAMILY_CASES and family == "normal" else (0,):
                bad, ratios = run_ln(rows, cols, family, eps, ld_extra=ld_extra)
                assert not bad, (family, eps, ld_extra, bad)
                for k, v in ratios.items():
                    worst[k] = max(worst.get(k, 0.0), v)
    print("\nRATIO emulation layernorm", name, " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= HEADROOM


@pytest.mark.parametrize("name", [n for n in R.LN_CASES if n in R.FAMILY_CASES or R.LN_CASES[n][0] in (1, 3, 15, 63)])
def test_emulation_stays_inside_the_l2norm_bounds(name):
    rows, cols, _ = R.LN_CASES[name]
    worst = {}
    for family in R.LN_FAMILIES if name in R.FAMILY_CASES else ("normal",):
        bad, ratios = run_l2(rows, cols, family)
        assert not bad, (family, bad)
        for k, v in ratios.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("\nRATIO emulation l2norm", name, " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= HEADROOM


@pytest.mark.parametrize("name", list(R.TE_CASES))
def test_emulation_stays_inside_the_time_embed_bounds(name):
    worst = {}
    for regime in R.TE_REGIMES if name != R.TE_BIG else R.TE_REGIMES[2:]:
        bad, ratios = run_te(name, regime)
        assert not bad, (regime, bad)
        for k, v in ratios.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("\nRATIO emulation time_embed", name, " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= HEADROOM
    B, T, e, nband = R.TE_CASES[name]
    inp = R.te_inputs(B, T, e, nband, "hundred", integer=True)
    emu, ref = R.emulate_te_backward(inp["dy"], inp["x"], nband), R.te_backward_ref(inp["dy"], inp["x"], nband)
    assert all(torch.equal(emu[k].double(), ref[k]) for k in ("dw", "dbw", "dband"))   # integers: exact whatever the order


# ------------------------------------------------------------------------------------------------------------ defects are caught
# kind -> (runner, arguments of the named case, the outputs that must leave their bound)
DEFECT_CASES = {
    "one_pass_variance": (run_ln, dict(rows=17, cols=68, family="offset"), ("rstd", "y")),
    "padding_in_variance": (run_ln, dict(rows=17, cols=68, family="normal"), ("rstd", "y")),
    "padded_n": (run_ln, dict(rows=65, cols=60, family="normal"), ("mean", "rstd", "y")),
    "eps_dropped": (run_ln, dict(rows=65, cols=64, family="tiny"), ("rstd", "y")),
    "m2_dropped": (run_ln, dict(rows=5, cols=260, family="normal"), ("dx", "colsum")),
    "add_ignored": (run_ln, dict(rows=65, cols=12, family="normal"), ("dx", "colsum")),
    "last_slab_dropped": (run_ln, dict(rows=257, cols=260, family="integer"), ("dgamma", "dbeta", "colsum")),
    "lds_group_dropped": (run_ln, dict(rows=17, cols=200, family="integer"), ("dgamma", "dbeta", "colsum")),
    "stride_as_cols": (run_ln, dict(rows=17, cols=256, family="normal", ld_extra=4), ("mean", "y", "dx")),
    "band_edge_shifted": (run_te, dict(name="b5_t12_e64_n2", regime="hundred"), ("out", "dband")),
    "l2_no_projection": (run_l2, dict(rows=17, cols=68, family="normal"), ("dx",)),
    "sincos_swapped": (run_te, dict(name="b5_t6_e6_n1", regime="hundred"), ("out",)),
    "omega_index": (run_te, dict(name="b5_t6_e6_n1", regime="hundred"), ("out",)),
}


def test_every_defect_has_a_named_case():
    assert set(DEFECT_CASES) == set(R.DEFECTS)


@pytest.mark.parametrize("kind", R.DEFECTS)
def test_injected_defect_is_rejected_on_its_named_case(kind):
    run, kw, must = DEFECT_CASES[kind]
    clean, _ = run(**kw)
    assert not clean                                            # the same case passes without the defect
    bad, ratios = run(defect=kind, **kw)
    for out in must:
        assert any(b.startswith(out + " ") for b in bad), (out, ratios)


@pytest.mark.parametrize("kind", ["last_slab_dropped", "lds_group_dropped"])
@pytest.mark.parametrize("name", ["r3585_c64", "r1025_c68", "r65_c60", "r1025_c260", "r257_c1020"])
def test_a_lost_partial_sum_shows_on_integers_at_every_width(kind, name):
    rows, cols, _ = R.LN_CASES[name]
    if kind == "last_slab_dropped" and R.ln_plan(rows, cols).slabs == 1:
        return
    bad, ratios = run_ln(rows, cols, "integer", defect=kind)
    assert any(b.startswith("dbeta ") for b in bad), ratios


def test_one_pass_variance_hides_in_the_suite_data_at_its_tolerance():
    """why the offset family exists: on randn * 2 + 0.5 rows the one-pass form passes rtol 1e-4 / atol 1e-5"""
    inp, fref, _, _ = ln_bundle(17, 68, "normal", 1e-5)
    y = R.emulate_ln_forward(inp["x"], inp["gamma"], inp["beta"], 1e-5, "one_pass_variance")["y"]
    torch.testing.assert_close(y.double(), fref["y"], rtol=1e-4, atol=1e-5)
    inp, fref, _, _ = ln_bundle(17, 68, "offset", 1e-5)
    y = R.emulate_ln_forward(inp["x"], inp["gamma"], inp["beta"], 1e-5, "one_pass_variance")["y"]
    assert not float((y.double() - fref["y"]).abs().max()) < 0.1                      # wrong in the first digit (or NaN)
