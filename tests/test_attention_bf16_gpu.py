"""The bf16 attention kernels of csrc/attention_bf16.hip (battn_fwd_kernel, battn_bwd_dq_kernel, battn_bwd_dkv_kernel) against
the fp64 references and derived per-element bounds of tests/attention_bf16_refs.py, launch by launch: the backward is fed
out = bf16(Oref) and lse = fp32(lse_ref) made on the host, not the forward kernel's outputs.  Four input families (flat, peaked,
uniform, one-hot; the last two have exact expectations) at every tile and block edge of the token count, then column sums and
determinism, strides through the C ABI, independence of samples and heads, and the argument contract.  Below them the bf16
LayerNorm forms the same trunk uses (msn_layernorm_fwd_bf16 / msn_layernorm_bwd_bf16, csrc/rowops.hip) against the fp32 kernel
bit for bit, the bf16-dy branch included, at all three lanes-per-row variants.

The gate on every bound is 1.  Largest error / bound ratios observed on an MI355X over all lengths, for information (the
emulation of attention_bf16_refs.py reaches 0.65 / 0.78 / 0.82 / 0.78 on the peaked family at its four lengths):
    family     O      dQ     dK     dV
    flat       0.485  0.688  0.586  0.523
    peaked     0.733  0.810  0.830  0.848
    uniform    0.290  0.569  0      0.648     (q = 0: dK is exactly 0)
    one-hot    0      -      -      -         (held to its exact expectations)"""
import functools

import pytest
import torch

import attention_bf16_refs as R

pytestmark = pytest.mark.gpu

LENGTHS = (1, 15, 16, 17, 31, 32, 33, 63, 65, 128, 129, 197, 255, 256)      # 129: a wave's second 16-token tile
SHAPES = ((1, 1), (2, 3), (3, 2))       # (B, H), dealt over the lengths: each meets a ragged and a full 32-key block count


def shape_of(T):
    return SHAPES[LENGTHS.index(T) % 3]


@functools.lru_cache(maxsize=None)
def case(family, T, B=None, H=None):
    """Inputs on the card, the fp64 references (computed once, never modified) and the host-made operands of the backward."""
    if B is None:
        B, H = shape_of(T)
    inp = R.make_inputs(family, B, H, T)
    fref = R.forward_ref(inp["qkv"], B, T, H)
    out, lse = fref["out"].to(R.BF16), fref["lse"].to(R.F32)
    bref = R.backward_ref(inp["qkv"], out, inp["dout"], lse, B, T, H)
    dev = dict(qkv=inp["qkv"].cuda(), dout=inp["dout"].cuda(), out=out.cuda(), lse=lse.cuda())
    return B, H, inp, fref, bref, dev


def show(what, family, T, ratios):
    print(f"\nRATIO {what} {family} T={T} " + " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))


@pytest.mark.parametrize("T", LENGTHS)
@pytest.mark.parametrize("family", R.FAMILIES)
def test_forward(family, T):
    from multimodal_supernovae_amd import ops
    B, H, inp, fref, _, dev = case(family, T)
    out, lse = ops.attention_bf16_fwd(dev["qkv"], B, T, H, R.SCALE)
    bad, ratios = R.forward_failures(family, inp, fref, out, lse, B, T, H)
    show("fwd", family, T, ratios)
    assert not bad, (bad, ratios)


@pytest.mark.parametrize("T", LENGTHS)
@pytest.mark.parametrize("family", R.FAMILIES)
def test_backward_per_launch(family, T):
    from multimodal_supernovae_amd import ops
    B, H, inp, _, bref, dev = case(family, T)
    dqkv = ops.attention_bf16_bwd(dev["qkv"], dev["out"], dev["dout"], dev["lse"], B, T, H, R.SCALE)
    bad, ratios = R.backward_failures(family, inp, bref, dqkv, B, T, H)
    show("bwd", family, T, ratios)
    assert not bad, (bad, ratios)


@pytest.mark.parametrize("T", LENGTHS)
def test_column_sums_and_determinism(T):
    """want_colsum leaves dqkv bit-identical, the sums are those of the gradients AS STORED, and a second identical launch
    gives identical bits in every output."""
    from multimodal_supernovae_amd import ops
    B, H, _, _, _, dev = case("flat", T)
    args = (dev["qkv"], dev["out"], dev["dout"], dev["lse"], B, T, H, R.SCALE)
    plain = ops.attention_bf16_bwd(*args)
    dqkv, cs = ops.attention_bf16_bwd(*args, want_colsum=True)
    assert R.same_bits(dqkv, plain)
    assert R.close(cs, dqkv.cpu().double().sum(0), **R.COLSUM_TOL)
    dqkv2, cs2 = ops.attention_bf16_bwd(*args, want_colsum=True)
    assert R.same_bits(dqkv2, dqkv) and torch.equal(cs2, cs)
    (o1, l1), (o2, l2) = (ops.attention_bf16_fwd(dev["qkv"], B, T, H, R.SCALE) for _ in range(2))
    assert R.same_bits(o1, o2) and torch.equal(l1, l2)


SENTINEL = 0x5A5A


def _wide(rows, cols, lo, src=None):
    """A (rows, cols) bf16 matrix filled with a sentinel bit pattern, `src` copied into its columns lo .. lo + src.shape[1]."""
    w = torch.full((rows, cols), SENTINEL, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    if src is not None:
        w[:, lo:lo + src.shape[1]] = src
    return w


def _padding_intact(w, lo, hi):
    bits = w.view(torch.int16)
    return bool((bits[:, :lo] == SENTINEL).all()) and bool((bits[:, hi:] == SENTINEL).all())


@pytest.mark.parametrize("T", [33, 256])
def test_strides_through_the_c_abi(T):
    """qkv and dqkv as column slices of a wider matrix (ld = 3E + 8), out with ldo = E + 8, dout with ldd = E + 16: the bits of the
    packed call, padding columns untouched."""
    from multimodal_supernovae_amd import _lib, ops
    from multimodal_supernovae_amd._lib import check, ptr, stream_ptr
    B, H, _, _, _, dev = case("flat", T)
    E, n = 64 * H, B * T
    L = _lib.lib()
    out_p, lse_p = ops.attention_bf16_fwd(dev["qkv"], B, T, H, R.SCALE)
    dqkv_p, cs_p = ops.attention_bf16_bwd(dev["qkv"], dev["out"], dev["dout"], dev["lse"], B, T, H, R.SCALE, want_colsum=True)

    qkv_w = _wide(n, 3 * E + 8, 8, dev["qkv"])            # the slice starts 8 columns (16 bytes) in
    qkv_s = qkv_w[:, 8:]
    out_w = _wide(n, E + 8, 0)
    lse = torch.empty((B, H, T), dtype=torch.float32, device="cuda")
    check(L.msn_attention_bf16_fwd(ptr(qkv_s), 3 * E + 8, B, H, T, R.SCALE, ptr(out_w), E + 8, ptr(lse), stream_ptr()), "fwd")
    assert R.same_bits(out_w[:, :E], out_p) and torch.equal(lse, lse_p) and _padding_intact(out_w, 0, E)

    saved_w = _wide(n, E + 8, 0, dev["out"])
    dout_w = _wide(n, E + 16, 8, dev["dout"])
    dqkv_w = _wide(n, 3 * E + 8, 0)
    delta = torch.empty((B, H, T), dtype=torch.float32, device="cuda")
    cs = torch.empty(3 * E, dtype=torch.float32, device="cuda")
    ws = torch.empty((B, 3 * E), dtype=torch.float32, device="cuda")
    check(L.msn_attention_bf16_bwd(ptr(qkv_s), 3 * E + 8, ptr(saved_w), E + 8, ptr(dout_w[:, 8:]), E + 16, ptr(dev["lse"]), B, H, T,
                                   R.SCALE, ptr(dqkv_w), ptr(delta), ptr(cs), ptr(ws), stream_ptr()), "bwd")
    assert R.same_bits(dqkv_w[:, :3 * E], dqkv_p) and torch.equal(cs, cs_p) and _padding_intact(dqkv_w, 0, 3 * E)


def _poison(t, B, T, H, sample=None, head=None):
    """NaN in one sample's rows or in one head's columns of a (B*T, k H 64) bf16 / (B, H, T) fp32 operand."""
    t = t.clone()
    if t.dim() == 3:
        t[sample if sample is not None else slice(None), head if head is not None else slice(None)] = float("nan")
    elif sample is not None:
        t[sample * T:(sample + 1) * T] = float("nan")
    else:
        for third in range(t.shape[1] // (64 * H)):
            t[:, 64 * (third * H + head):64 * (third * H + head + 1)] = float("nan")
    return t


@pytest.mark.parametrize("T", [17, 197])
def test_samples_and_heads_are_independent(T):
    """NaN in sample 1 leaves sample 0 of the B = 2 launch equal to the B = 1 launch on sample 0, NaN in head 1 leaves head 0
    unchanged: bit for bit, and finite."""
    from multimodal_supernovae_amd import ops
    B, H, _, _, _, dev = case("flat", T, 2, 3)
    E = 64 * H
    names = ("qkv", "out", "dout", "lse")

    def run(d, B):
        o, l = ops.attention_bf16_fwd(d["qkv"], B, T, H, R.SCALE)
        return o, l, ops.attention_bf16_bwd(d["qkv"], d["out"], d["dout"], d["lse"], B, T, H, R.SCALE)

    first = {k: dev[k][:1].contiguous() if dev[k].dim() == 3 else dev[k][:T].contiguous() for k in names}
    o1, l1, g1 = run(first, 1)
    o2, l2, g2 = run({k: _poison(dev[k], B, T, H, sample=1) for k in names}, B)
    assert R.same_bits(o2[:T], o1) and torch.equal(l2[:1], l1) and R.same_bits(g2[:T], g1)
    assert bool(torch.isfinite(o2[:T].float()).all()) and bool(torch.isfinite(g2[:T].float()).all()) and bool(torch.isfinite(l2[:1]).all())
    assert bool(torch.isnan(o2[T:].float()).all())           # the poison did reach the kernel

    oc, lc, gc = run(dev, B)
    oh, lh, gh = run({k: _poison(dev[k], B, T, H, head=1) for k in names}, B)
    assert R.same_bits(oh[:, :64], oc[:, :64]) and torch.equal(lh[:, 0], lc[:, 0])
    for third in range(3):
        assert R.same_bits(gh[:, third * E:third * E + 64], gc[:, third * E:third * E + 64])
    assert bool(torch.isfinite(oh[:, :64].float()).all()) and bool(torch.isnan(oh[:, 64:128].float()).all())


def test_contract():
    """MsnHipError in front of any launch (the sentinel-filled outputs stay untouched) for T = 0, T = 257, ld not a multiple of 8,
    ld < 3E and a column-sum request without its workspace."""
    from multimodal_supernovae_amd import _lib
    from multimodal_supernovae_amd._lib import MsnHipError, check, ptr, stream_ptr
    B, H = 1, 1
    E = 64
    L = _lib.lib()
    qkv = torch.zeros((257, 3 * E + 8), dtype=torch.bfloat16, device="cuda")
    saved, dout = torch.zeros((257, E), dtype=torch.bfloat16, device="cuda"), torch.zeros((257, E), dtype=torch.bfloat16, device="cuda")
    lse_in = torch.zeros((B, H, 257), dtype=torch.float32, device="cuda")
    out, dqkv = _wide(257, E, 0), _wide(257, 3 * E + 8, 0)
    stat = torch.full((2, B, H, 257), 7.0, device="cuda")       # lse (forward) | delta (backward)
    cs = torch.full((3 * E,), 7.0, device="cuda")
    ws = torch.full((B, 3 * E), 7.0, device="cuda")

    def fwd(T, ld):
        check(L.msn_attention_bf16_fwd(ptr(qkv), ld, B, H, T, R.SCALE, ptr(out), E, ptr(stat[0]), stream_ptr()), "msn_attention_bf16_fwd")

    def bwd(T, ld, cs=None, ws=None):
        check(L.msn_attention_bf16_bwd(ptr(qkv), ld, ptr(saved), E, ptr(dout), E, ptr(lse_in), B, H, T, R.SCALE, ptr(dqkv),
                                       ptr(stat[1]), ptr(cs), ptr(ws), stream_ptr()), "msn_attention_bf16_bwd")

    for T, ld in [(0, 3 * E), (257, 3 * E), (16, 3 * E + 4), (16, 3 * E - 8)]:
        with pytest.raises(MsnHipError):
            fwd(T, ld)
        with pytest.raises(MsnHipError):
            bwd(T, ld)
    with pytest.raises(MsnHipError, match="workspace"):
        bwd(16, 3 * E, cs=cs, ws=None)
    torch.cuda.synchronize()
    assert _padding_intact(out, 0, 0) and _padding_intact(dqkv, 0, 0)
    assert bool((stat == 7.0).all()) and bool((cs == 7.0).all()) and bool((ws == 7.0).all())
    fwd(16, 3 * E + 8)                                        # the same buffers do pass with a valid geometry
    bwd(16, 3 * E + 8, cs=cs, ws=ws)
    torch.cuda.synchronize()
    assert not _padding_intact(out, 0, 0)


# ------------------------------------------------------------------------------------- the bf16 LayerNorm forms of the same trunk
LN_COLS = (8, 64, 68, 256, 260, 768, 1024)       # 4 lanes per row up to 64 columns, 16 up to 256, 64 beyond: both edges of each
LN_ROWS = (1, 37, 513)


@functools.lru_cache(maxsize=None)
def ln_case(rows, cols):
    g = R.gen(rows * 4099 + cols)
    rn = lambda *s: torch.randn(*s, generator=g).cuda()
    return dict(x=rn(rows, cols) * 1.5 + 0.3, gamma=rn(cols), beta=rn(cols), dy=rn(rows, cols), add=rn(rows, cols))


def _same(a, b):
    return all(torch.equal(s, t) for s, t in zip(a, b))


@pytest.mark.parametrize("rows", LN_ROWS)
@pytest.mark.parametrize("cols", LN_COLS)
def test_layernorm_bf16_forms_equal_the_fp32_kernel(rows, cols):
    """y_bf16 = bf16(y) with identical statistics; dx, dgamma, dbeta identical and dx_bf16 = bf16(dx), with and without the
    residual gradient and the column sums (which are those of dx to fp32 summation error: n 2^-24 sum |dx|)."""
    from multimodal_supernovae_amd import ops
    c = ln_case(rows, cols)
    y, mean, rstd = ops.layernorm_fwd(c["x"], c["gamma"], c["beta"], 1e-6)
    yb, mb, rb = ops.layernorm_fwd_bf16(c["x"], c["gamma"], c["beta"], 1e-6)
    assert yb.dtype == torch.bfloat16 and torch.equal(yb, y.to(torch.bfloat16)) and torch.equal(mb, mean) and torch.equal(rb, rstd)
    for add in (None, c["add"]):
        ref = ops.layernorm_bwd(c["dy"], c["x"], mean, rstd, c["gamma"], add=add)
        for want_colsum in (False, True):
            got = ops.layernorm_bwd_bf16(c["dy"], c["x"], mean, rstd, c["gamma"], add=add, want_colsum=want_colsum)
            dx, dxb, dg, db = got[:4]
            assert _same((dx, dg, db), ref) and dxb.dtype == torch.bfloat16 and torch.equal(dxb, ref[0].to(torch.bfloat16))
            if want_colsum:
                d64 = ref[0].double()
                assert bool(((got[4].double() - d64.sum(0)).abs() <= rows * 2.0 ** -24 * d64.abs().sum(0)).all())


@pytest.mark.parametrize("rows", LN_ROWS)
@pytest.mark.parametrize("cols", LN_COLS)
def test_layernorm_bwd_bf16_dy_equals_the_call_on_its_float_copy(rows, cols):
    """dy given AS bf16 (the dy_is_bf16 branch of ln_bwd_kernel, the trunk's default) == the call on dy.float(), every output bit for
    bit: the conversion is exact.  Packed, and as a row-strided view of a wider bf16 matrix."""
    from multimodal_supernovae_amd import ops
    c = ln_case(rows, cols)
    _, mean, rstd = ops.layernorm_fwd(c["x"], c["gamma"], c["beta"], 1e-6)
    dyb = c["dy"].to(torch.bfloat16)
    wide = _wide(rows, cols + 8, 8, dyb)
    for add, want_colsum in ((None, False), (c["add"], True)):
        want = ops.layernorm_bwd_bf16(dyb.float(), c["x"], mean, rstd, c["gamma"], add=add, want_colsum=want_colsum)
        for dy in (dyb, wide[:, 8:]):
            got = ops.layernorm_bwd_bf16(dy, c["x"], mean, rstd, c["gamma"], add=add, want_colsum=want_colsum)
            assert len(got) == len(want) and _same(got, want)
