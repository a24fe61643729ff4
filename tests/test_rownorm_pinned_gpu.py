"""The row kernels of csrc/rowops.hip against the fp64 references and derived per-element bounds of tests/rownorm_refs.py, launch by
launch: msn_layernorm_fwd / _bwd (mean, rstd, y, dx with and without the fused residual gradient, dgamma, dbeta, the column sums
of dx), msn_l2norm_fwd / _bwd and msn_time_embed_fwd / _bwd, through ops.* and, where the wrapper fixes a leading dimension,
through the C ABI.  The backward launches are fed the fp32-rounded REFERENCE statistics (mean and rstd, y and inv), not the forward
kernel's, so an error shared by both directions cannot cancel.  The cases (rownorm_refs.LN_CASES, TE_CASES) are the smallest
shapes that reach each path -- the three lane instantiations, both sides of the 64 | 68 and 256 | 260 dispatch edges, partly filled
last chunks, the slab counts around 16 and 64, the second grid-stride pass of the forward and the backward, every edge of the time
embedding's backward -- and the path is asserted through the mirrors, so a retune cannot silently empty one.  Before every launch
the blocks the allocator hands out next are filled with NaN, and strided outputs are written into NaN-filled buffers whose gaps
must still be NaN afterwards.

The gate on every bound is 1; the measured ratios are recorded in the docstring of tests/rownorm_refs.py."""
import functools
import math

import pytest
import torch

import rownorm_refs as R

pytestmark = pytest.mark.gpu
F32 = torch.float32


def _dev(numel):
    """where the fp64 reference is evaluated: on the card once the matrices are large"""
    return "cuda" if numel >= 1 << 20 else "cpu"


def poison(*shapes):
    """fill what the caching allocator will hand out next with NaN"""
    junk = [torch.full(s if isinstance(s, tuple) else (s,), math.nan, dtype=F32, device="cuda") for s in shapes]
    del junk


def show(what, name, family, ratios):
    print(f"\nRATIO {what} {family} {name} " + " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))


def wide(t, ld):
    """the same values as rows of a NaN-filled (rows, ld) buffer on the card: a view with row stride ld"""
    buf = torch.full((t.shape[0], ld), math.nan, dtype=t.dtype, device="cuda")
    buf[:, :t.shape[1]] = t
    return buf[:, :t.shape[1]]


def nan_out(rows, cols, ld):
    return torch.full((rows, ld), math.nan, dtype=F32, device="cuda")


def gaps_untouched(buf, cols):
    return bool(torch.isnan(buf[:, cols:]).all())


# ------------------------------------------------------------------------------------------------------------ the launches
def ln_forward(x, gamma, beta, eps, ldy=None):
    """through ops.layernorm_fwd, or (ldy given) through the C ABI into a NaN-filled (rows, ldy) buffer -> outputs, the buffer"""
    from multimodal_supernovae_amd import ops
    from multimodal_supernovae_amd._lib import check, lib, ptr, stream_ptr
    rows, cols = x.shape
    if ldy is None:
        poison((rows, cols), rows, rows)
        y, mean, rstd = ops.layernorm_fwd(x, gamma, beta, eps)
        return dict(mean=mean, rstd=rstd, y=y), None
    buf = nan_out(rows, cols, ldy)
    poison(rows, rows)
    mean, rstd = torch.empty(rows, dtype=F32, device="cuda"), torch.empty(rows, dtype=F32, device="cuda")
    check(lib().msn_layernorm_fwd(ptr(x), x.stride(0), rows, cols, ptr(gamma), ptr(beta), eps, ptr(buf), ldy, ptr(mean), ptr(rstd),
                                  stream_ptr()), "msn_layernorm_fwd")
    return dict(mean=mean, rstd=rstd, y=buf[:, :cols]), buf


def ln_ws_floats(rows, cols, nacc=2):
    from multimodal_supernovae_amd._lib import lib
    nb = lib().msn_layernorm_bwd_workspace_bytes(rows, cols)
    assert nb == R.ln_plan(rows, cols).ws_bytes
    return nb * nacc // 2 // 4


def ln_backward(dy, x, mean, rstd, gamma, add=None, lddx=None):
    from multimodal_supernovae_amd import ops
    from multimodal_supernovae_amd._lib import check, lib, ptr, stream_ptr
    rows, cols = x.shape
    if lddx is None:
        poison(ln_ws_floats(rows, cols), (rows, cols), cols, cols)
        dx, dg, db = ops.layernorm_bwd(dy, x, mean, rstd, gamma, add=add)
        return dict(dx=dx, dgamma=dg, dbeta=db), None
    buf = nan_out(rows, cols, lddx)
    nws = ln_ws_floats(rows, cols)
    poison(nws, cols, cols)
    ws = torch.empty(nws, dtype=F32, device="cuda")
    dg, db = torch.empty(cols, dtype=F32, device="cuda"), torch.empty(cols, dtype=F32, device="cuda")
    check(lib().msn_layernorm_bwd(ptr(dy), dy.stride(0), ptr(x), x.stride(0), rows, cols, ptr(mean), ptr(rstd), ptr(gamma), ptr(add),
                                  add.stride(0) if add is not None else 0, ptr(buf), lddx, ptr(dg), ptr(db), ptr(ws), nws * 4, stream_ptr()),
          "msn_layernorm_bwd")
    return dict(dx=buf[:, :cols], dgamma=dg, dbeta=db), buf


def ln_backward_colsum(dy, x, mean, rstd, gamma, add):
    """the bf16 form with the third accumulator: its fp32 outputs and the column sums of dx"""
    from multimodal_supernovae_amd import ops
    rows, cols = x.shape
    poison(ln_ws_floats(rows, cols, 3), (rows, cols), (rows, cols // 2), cols, cols, cols)
    dx, dxb, dg, db, cs = ops.layernorm_bwd_bf16(dy, x, mean, rstd, gamma, add=add, want_colsum=True)
    return dict(dx=dx, dgamma=dg, dbeta=db, colsum=cs), dxb


@functools.lru_cache(maxsize=None)
def ln_bundle(name, family, eps):
    """operands on the card and the references (computed once, never modified)"""
    rows, cols, _ = R.LN_CASES[name]
    inp = R.ln_inputs(family, rows, cols)
    dev = _dev(rows * cols)
    on = {k: v.to(dev) for k, v in inp.items()}
    fref = R.ln_forward_ref(on["x"], on["gamma"], on["beta"], eps)
    mean, rstd = fref["mean"].to(F32), fref["rstd"].to(F32)
    bref = R.ln_backward_ref(on["dy"], on["x"], mean, rstd, on["gamma"])
    return {k: v.cuda() for k, v in inp.items()}, fref, (mean.cuda(), rstd.cuda()), bref, R.ln_add_ref(bref, on["add"])


LN_RUNS = [(n, f, 1e-5) for n in R.LN_CASES for f in ("normal", "integer")]
LN_RUNS += [(n, f, e) for n in R.FAMILY_CASES for f in R.LN_FAMILIES for e in R.EPS if (n, f, e) not in LN_RUNS]


@pytest.mark.parametrize("name,family,eps", LN_RUNS)
def test_layernorm_forward_and_backward(name, family, eps):
    rows, cols, want = R.LN_CASES[name]
    assert R.ln_features(rows, cols) == want
    c, fref, (mean, rstd), bref, aref = ln_bundle(name, family, eps)
    fwd, _ = ln_forward(c["x"], c["gamma"], c["beta"], eps)
    bad, r = R.failures(fwd, fref)
    bwd, _ = ln_backward(c["dy"], c["x"], mean, rstd, c["gamma"])
    bad_b, r_b = R.failures(bwd, bref)
    bwa, _ = ln_backward(c["dy"], c["x"], mean, rstd, c["gamma"], add=c["add"])
    bad_a, r_a = R.failures({"dx": bwa["dx"]}, aref)
    third, dxb = ln_backward_colsum(c["dy"], c["x"], mean, rstd, c["gamma"], c["add"])
    bad_c, r_c = R.failures({"colsum": third["colsum"]}, aref)
    show(f"layernorm eps={eps:g}", name, family, {**r, **r_b, "dx+add": r_a["dx"], **r_c})
    assert not bad + bad_b + bad_a + bad_c, bad + bad_b + bad_a + bad_c
    # the column sums do not depend on `add`, nor the fp32 outputs on the third accumulator or the bf16 copy
    assert torch.equal(bwa["dgamma"], bwd["dgamma"]) and torch.equal(bwa["dbeta"], bwd["dbeta"])
    assert all(torch.equal(third[k], bwa[k]) for k in ("dx", "dgamma", "dbeta")) and torch.equal(dxb, bwa["dx"].to(torch.bfloat16))
    if family == "integer":                                  # every sum is exact there, whatever its order
        assert torch.equal(bwd["dbeta"].double(), bref["dbeta"].to("cuda"))
        if cols & (cols - 1) == 0:
            assert torch.equal(fwd["mean"].double(), fref["mean"].to("cuda"))
    if family == "constant":
        assert bool(torch.isfinite(fwd["y"]).all())


STRIDED = ("r65_c12", "r65_c60", "r4097_c64", "r17_c68", "r1025_c200", "r17_c256", "r5_c260", "r257_c1020", "r5_c1024")


@pytest.mark.parametrize("name", STRIDED)
@pytest.mark.parametrize("eps", R.EPS)
def test_layernorm_strided_operands_and_outputs(name, eps):
    """x, dy and add are slices of wider buffers with three different leading dimensions, y and dx go into NaN-filled wider buffers
    through the C ABI: the payload is inside its bound and equals the contiguous launch bit for bit, every gap is still NaN."""
    rows, cols, _ = R.LN_CASES[name]
    c, fref, (mean, rstd), bref, aref = ln_bundle(name, "normal", eps)
    x, dy, add = wide(c["x"], cols + 4), wide(c["dy"], cols + 8), wide(c["add"], cols + 12)
    assert {t.stride(0) for t in (x, dy, add)} == {cols + 4, cols + 8, cols + 12}
    fwd, ybuf = ln_forward(x, c["gamma"], c["beta"], eps, ldy=cols + 16)
    bwd, dbuf = ln_backward(dy, x, mean, rstd, c["gamma"], add=add, lddx=cols + 20)
    bad_f, r_f = R.failures(fwd, fref)
    bad_b, r_b = R.failures(bwd, aref)
    show(f"layernorm strided eps={eps:g}", name, "normal", {**r_f, **r_b})
    assert not bad_f + bad_b, bad_f + bad_b
    assert gaps_untouched(ybuf, cols) and gaps_untouched(dbuf, cols)
    plain_f, _ = ln_forward(c["x"], c["gamma"], c["beta"], eps)
    plain_b, _ = ln_backward(c["dy"], c["x"], mean, rstd, c["gamma"], add=c["add"])
    assert all(torch.equal(fwd[k], plain_f[k]) for k in fwd) and all(torch.equal(bwd[k], plain_b[k]) for k in bwd)


@pytest.mark.parametrize("B,T,e", [(65, 3, 64), (17, 5, 200), (9, 7, 384)])
def test_layernorm_of_the_class_row_view(B, T, e):
    """rows [:, 0, :] of a (B, T, e) tensor (row stride T e), as the ViT head normalises its class token"""
    from multimodal_supernovae_amd import ops
    inp = R.ln_inputs("normal", B, e)
    x3 = torch.full((B, T, e), math.nan, device="cuda")
    x3[:, 0] = inp["x"].cuda()
    view = x3[:, 0, :]
    assert view.stride(0) == T * e and not view.is_contiguous()
    fref = R.ln_forward_ref(inp["x"], inp["gamma"], inp["beta"], 1e-6)
    fwd, _ = ln_forward(view, inp["gamma"].cuda(), inp["beta"].cuda(), 1e-6)
    mean, rstd = fref["mean"].to(F32), fref["rstd"].to(F32)
    bwd, _ = ln_backward(inp["dy"].cuda(), view, mean.cuda(), rstd.cuda(), inp["gamma"].cuda())
    bad_f, r_f = R.failures(fwd, fref)
    bad_b, r_b = R.failures(bwd, R.ln_backward_ref(inp["dy"], inp["x"], mean, rstd, inp["gamma"]))
    show("layernorm class row", f"b{B}_t{T}_e{e}", "normal", {**r_f, **r_b})
    assert not bad_f + bad_b, bad_f + bad_b
    assert bool(torch.isnan(x3[:, 1:]).all())


@pytest.mark.parametrize("rows,cols", R.TIE_CASES)
def test_bf16_and_plane_forms_are_the_fp32_kernel_cast_or_split(rows, cols):
    """the forms tied to the fp32 kernel, at the new edge widths and one row count past the forward's cap each: bit for bit"""
    from multimodal_supernovae_amd import ops
    assert R.ln_plan(rows, cols).passes == 2 and R.ln_plan(rows, cols).rounds == 5
    g = R.gen(rows + cols)
    x = (torch.randn(rows, cols, generator=g) * 2 + 0.5).cuda()
    gm, bt = (torch.randn(cols, generator=g) + 1).cuda(), torch.randn(cols, generator=g).cuda()
    dy, add = torch.randn(rows, cols, generator=g).cuda(), torch.randn(rows, cols, generator=g).cuda()
    y, mean, rstd = ops.layernorm_fwd(x, gm, bt, 1e-6)
    yb, mb, rb = ops.layernorm_fwd_bf16(x, gm, bt, 1e-6)
    assert torch.equal(yb, y.to(torch.bfloat16)) and torch.equal(mb, mean) and torch.equal(rb, rstd)
    dx, dg, db = ops.layernorm_bwd(dy, x, mean, rstd, gm, add=add)
    for colsum in (False, True):
        out = ops.layernorm_bwd_bf16(dy, x, mean, rstd, gm, add=add, want_colsum=colsum)
        assert torch.equal(out[0], dx) and torch.equal(out[1], dx.to(torch.bfloat16)) and torch.equal(out[2], dg) and torch.equal(out[3], db)
    cs = out[4]
    for planes in (2, 3):
        yp, mp, rp = ops.layernorm_fwd_planes(x, gm, bt, 1e-6, planes)
        assert torch.equal(mp, mean) and torch.equal(rp, rstd) and torch.equal(yp.buf, ops.plane_split(y, planes).buf)
        dx2, dxp, dg2, db2, cs2 = ops.layernorm_bwd_planes(dy, x, mean, rstd, gm, planes, add=add, want_colsum=True)
        assert torch.equal(dx2, dx) and torch.equal(dxp.buf, ops.plane_split(dx, planes).buf)
        assert torch.equal(dg2, dg) and torch.equal(db2, db) and torch.equal(cs2, cs)


# ------------------------------------------------------------------------------------------------------------ L2 normalise
def l2_forward(x, ldy=None):
    from multimodal_supernovae_amd import ops
    from multimodal_supernovae_amd._lib import check, lib, ptr, stream_ptr
    rows, cols = x.shape
    if ldy is None:
        poison((rows, cols), rows)
        y, inv = ops.l2norm_fwd(x)
        return dict(y=y, inv=inv), None
    buf = nan_out(rows, cols, ldy)
    poison(rows)
    inv = torch.empty(rows, dtype=F32, device="cuda")
    check(lib().msn_l2norm_fwd(ptr(x), x.stride(0), rows, cols, ptr(buf), ldy, ptr(inv), stream_ptr()), "msn_l2norm_fwd")
    return dict(y=buf[:, :cols], inv=inv), buf


def l2_backward(dy, y, inv, lddx=None):
    from multimodal_supernovae_amd import ops
    from multimodal_supernovae_amd._lib import check, lib, ptr, stream_ptr
    rows, cols = y.shape
    if lddx is None:
        poison((rows, cols))
        return dict(dx=ops.l2norm_bwd(dy, y, inv)), None
    buf = nan_out(rows, cols, lddx)
    check(lib().msn_l2norm_bwd(ptr(dy), dy.stride(0), ptr(y), y.stride(0), rows, cols, ptr(inv), ptr(buf), lddx, stream_ptr()), "msn_l2norm_bwd")
    return dict(dx=buf[:, :cols]), buf


L2_NAMES = [n for n in R.LN_CASES if n in R.FAMILY_CASES or n in R.BIG_CASES or R.LN_CASES[n][0] in (1, 3, 15, 63)]
L2_RUNS = [(n, f) for n in L2_NAMES for f in (R.LN_FAMILIES if n in R.FAMILY_CASES else ("normal",))]


@pytest.mark.parametrize("name,family", L2_RUNS)
def test_l2norm_forward_and_backward(name, family):
    rows, cols, want = R.LN_CASES[name]
    assert R.ln_features(rows, cols) == want
    inp = R.l2_inputs(family, rows, cols)
    dev = _dev(rows * cols)
    fref = R.l2_forward_ref(inp["x"].to(dev))
    y, inv = fref["y"].to(F32), fref["inv"].to(F32)
    bref = R.l2_backward_ref(inp["dy"].to(dev), y, inv)
    x, dy = inp["x"].cuda(), inp["dy"].cuda()
    fwd, _ = l2_forward(x)
    bwd, _ = l2_backward(dy, y.cuda(), inv.cuda())
    bad_f, r_f = R.failures(fwd, fref)
    bad_b, r_b = R.failures(bwd, bref)
    show("l2norm", name, family, {**r_f, **r_b})
    assert not bad_f + bad_b, bad_f + bad_b
    if rows >= 3:            # the zero row is NaN like the reference; its neighbours in the same wave are ordinary (inside their bounds above)
        assert bool(torch.isnan(fwd["y"][1]).all()) and math.isinf(float(fwd["inv"][1]))
        assert bool(torch.isfinite(fwd["y"][[0, 2]]).all()) and bool(torch.isfinite(fwd["inv"][[0, 2]]).all())
    # strided operands and outputs through the C ABI: the same bits, the gaps still NaN
    if rows * cols < 1 << 20:
        sf, ybuf = l2_forward(wide(x, cols + 4), ldy=cols + 8)
        sb, dbuf = l2_backward(wide(dy, cols + 12), wide(y.cuda(), cols + 4), inv.cuda(), lddx=cols + 16)
        eq = lambda a, b: torch.equal(a, b) or torch.equal(torch.nan_to_num(a, nan=7.0), torch.nan_to_num(b, nan=7.0))
        assert eq(sf["y"], fwd["y"]) and eq(sf["inv"], fwd["inv"]) and eq(sb["dx"], bwd["dx"])
        assert gaps_untouched(ybuf, cols) and gaps_untouched(dbuf, cols)


# ------------------------------------------------------------------------------------------------------------ time embedding
def te_launch(c, nband):
    from multimodal_supernovae_amd import ops
    from multimodal_supernovae_amd._lib import lib
    B, T, e = c["dy"].shape
    poison((B, T, e))
    out = ops.time_embed_fwd(c["x"], c["t"], c["w"], c["bw"], c["omega"], c["band"])
    nb = lib().msn_time_embed_bwd_workspace_bytes(B, e, nband)
    assert nb == R.te_plan(B, T, e, nband).ws_bytes
    poison(max(nb, 16) // 4 + 1, e, e, (nband, e))
    dw, dbw, dband = ops.time_embed_bwd(c["dy"], c["x"], nband)
    return dict(out=out), dict(dw=dw, dbw=dbw, **({"dband": dband} if nband > 1 else {}))


TE_RUNS = [(n, r) for n in R.TE_CASES for r in (R.TE_REGIMES if n != R.TE_BIG else R.TE_REGIMES[2:])]


@pytest.mark.parametrize("name,regime", TE_RUNS)
def test_time_embed_forward_and_backward(name, regime):
    B, T, e, nband = R.TE_CASES[name]
    p = R.te_plan(B, T, e, nband)
    assert p.passes == (2 if name == R.TE_BIG else 1) and p.col_passes == (2 if e > 256 else 1) and p.groups == 256 // min(e, 256)
    inp = R.te_inputs(B, T, e, nband, regime)
    dev = _dev(B * T * e)
    on = {k: (v.to(dev) if v is not None else None) for k, v in inp.items()}
    fref = R.te_forward_ref(on["x"], on["t"], on["w"], on["bw"], on["omega"], on["band"])
    bref = R.te_backward_ref(on["dy"], on["x"], nband)
    fwd, bwd = te_launch({k: (v.cuda() if v is not None else None) for k, v in inp.items()}, nband)
    bad_f, r_f = R.failures(fwd, fref)
    bad_b, r_b = R.failures(bwd, bref)
    show("time_embed", name, regime, {**r_f, **r_b})
    assert not bad_f + bad_b, bad_f + bad_b
    if nband > 1:            # dbw is the fp32 sum of the dband rows, in the kernel's order
        assert torch.equal(bwd["dbw"].cpu(), R.sequential_sum(bwd["dband"].cpu()))
    if regime == "hundred":  # integers: every sum is exact, whatever its order
        it = R.te_inputs(B, T, e, nband, regime, integer=True)
        _, ib = te_launch({k: (v.cuda() if v is not None else None) for k, v in it.items()}, nband)
        iref = R.te_backward_ref(it["dy"], it["x"], nband)
        assert all(torch.equal(v.cpu().double(), iref[k]) for k, v in ib.items())
