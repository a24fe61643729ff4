"""The gather, mask and pooling glue kernels of csrc/conv.hip and csrc/rowops.hip, kernel by kernel, against plain torch / numpy
on the CPU (tests/glue_refs.py, itself checked by tests/test_glue_refs_cpu.py).

Three kinds of comparison:
  * data movement (im2col in both column orders, channel padding, weight re-layouts, the ViT token compaction, token masking, the
    series features, max-pool values and arg-max, the dropout mask) is bit equality;
  * kernels that add a few terms (col2im in both orders, add_rows, the ViT token assembly, the max-pool backward gather, the masked
    pooling backward) get integer-valued inputs in [-8, 8], so every sum is exact in float32 and the result must EQUAL the float64
    reference, plus one random-normal case held to convmixer_refs.check_all;
  * the two long float32 reductions (masked MSE, masked mean pool) are held to convmixer_refs.check_all only.
Every elementwise kernel caps its grid (8192 blocks of 256 in conv.hip and dropout, 4096 elsewhere, 2048 for the masked-MSE
backward): each has one case above its cap, so a kernel without its grid-stride loop leaves a tail unwritten.

Two cases of the im2col table do NOT pass the cap they were written for (34*256*144 = 1.25 M float4 groups and 64*256*108 =
1.77 M elements, against 8192*256 = 2.10 M threads); they stay, and B = 58 / B = 80 of the same geometry are added, which do.
The stride-3 geometry is an addition too: with strides 1 and 2 only, a col2im_tap that skips its `ty % sh` test for even ty
computes the same result.

Measured on an MI355X: every check_all line (54: col2im x 2, maxpool_bwd, masked pool, vit_tokens, add_rows, masked MSE) has
err <= 1.02e-7 of max|ref64| against the bound 3.8e-6 (e32 <= 1.09e-7: the floor of the bound decides everywhere); the masked-MSE
loss at n = 600001 is within 6e-8.  The NaN cases fail on kernels that select with a bare `>` ("0 NaN outputs, 15 windows cover
a NaN pixel"; "0 NaN outputs, the reference has 3")."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import convmixer_refs as R
import glue_refs as G

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64, F32 = torch.float64, torch.float32
NAN = float("nan")


def _ops():
    from multimodal_supernovae_amd import ops
    return ops


def _dev(t):
    return t.to(DEV).contiguous()


# -------------------------------------------------------------------------------- 1. im2col / col2im, both column orders
CONV_GEOMS = [
    (2, 5, 7, 3, 3, 3, 1, 1, 1, 1),          # 3-channel stem: scalar order only
    (2, 9, 7, 4, 3, 3, 2, 2, 1, 1),          # odd sizes, stride 2: the last window stops short of the border
    (1, 16, 16, 4, 7, 7, 2, 2, 3, 3),        # the ResNet stem after channel padding
    (3, 1, 33, 8, 1, 7, 1, 2, 0, 3),         # 1-D series, H = 1
    (2, 6, 6, 8, 1, 1, 2, 2, 0, 0),          # 1x1 stride 2: col2im leaves the skipped pixels exactly 0
    (2, 4, 5, 12, 3, 2, 1, 2, 1, 0),         # kh != kw, sh != sw, ph != pw
    (2, 10, 7, 4, 3, 2, 3, 1, 1, 0),         # stride 3: rows that no tap of a window reaches, even and odd
    (34, 16, 16, 64, 3, 3, 1, 1, 1, 1),      # tap order: 1.25 M float4 groups
    (64, 16, 16, 12, 3, 3, 1, 1, 1, 1),      # scalar order: 1.77 M elements
    (58, 16, 16, 64, 3, 3, 1, 1, 1, 1),      # tap order: 58*256*144 = 2 101 248 float4 groups > 8192*256
    (80, 16, 16, 12, 3, 3, 1, 1, 1, 1),      # scalar order: 80*256*108 = 2 211 840 elements > 8192*256
]


def _geom_id(c):
    return "-".join(str(v) for v in c)


@pytest.mark.parametrize("case", CONV_GEOMS, ids=_geom_id)
def test_im2col_both_orders_bit_exact(case):
    ops = _ops()
    B, H, W, C = case[:4]
    geom = case[4:]
    x = torch.randn(B, H, W, C, generator=G.gen(sum(case)))
    want = G.im2col_ref(x, *geom)
    cols = ops.im2col(_dev(x), *geom).cpu()
    assert cols.shape == want.shape
    assert torch.equal(cols, want)
    if C % 4 == 0:
        tap = ops.im2col_tap(_dev(x), *geom).cpu()
        assert torch.equal(tap, G.im2col_tap_ref(x, *geom))
        assert torch.equal(tap, cols[:, G.tap_perm(C, geom[0] * geom[1])])


@pytest.mark.parametrize("case", CONV_GEOMS + [(40, 32, 32, 52, 1, 1, 1, 1, 0, 0)], ids=_geom_id)   # the last: B H W C > 8192*256
def test_col2im_both_orders_equal_fold_on_integers(case):
    ops = _ops()
    shape, geom = case[:4], case[4:]
    B, H, W, C = shape
    rows = B * G.conv_out(H, geom[0], geom[2], geom[4]) * G.conv_out(W, geom[1], geom[3], geom[5])
    d = G.ints((rows, C * geom[0] * geom[1]), G.gen(sum(case) + 1))
    want = G.col2im_ref(d, shape, *geom).to(F32)
    dx = ops.col2im(_dev(d), shape, *geom).cpu()
    assert torch.equal(dx, want)
    if geom[:4] == (1, 1, 2, 2):
        assert bool((dx[:, 1::2] == 0).all()) and bool((dx[:, :, 1::2] == 0).all())
    if C % 4 == 0:
        dx_tap = ops.col2im_tap(_dev(d), shape, *geom).cpu()
        assert torch.equal(dx_tap, G.col2im_tap_ref(d, shape, *geom).to(F32))
        perm = G.tap_perm(C, geom[0] * geom[1])
        assert torch.equal(ops.col2im_tap(_dev(d[:, perm]), shape, *geom).cpu(), dx)      # the adjoints agree up to the column order


def test_col2im_both_orders_random_normal():
    ops = _ops()
    case = (2, 9, 7, 4, 3, 3, 2, 2, 1, 1)
    shape, geom = case[:4], case[4:]
    d = torch.randn(2 * 5 * 4, 4 * 9, generator=G.gen(11))
    got = {"col2im": ops.col2im(_dev(d), shape, *geom), "col2im_tap": ops.col2im_tap(_dev(d), shape, *geom)}
    ref64, ref32 = ({"col2im": G.col2im_ref(d, shape, *geom, dtype=dt), "col2im_tap": G.col2im_tap_ref(d, shape, *geom, dtype=dt)}
                    for dt in (F64, F32))
    R.check_all(f"col2im{case}", got, ref32, ref64)


# ------------------------------------------------------------------------------------------------ 2. weight re-layouts
@pytest.mark.parametrize("co,ci,taps,cp", [(5, 3, 49, 4), (8, 4, 9, 4), (16, 64, 9, 64), (7, 3, 5, 8), (600, 64, 64, 64)])
def test_conv_weight_relayout_all_modes_bit_exact(co, ci, taps, cp):
    ops = _ops()
    g = G.gen(co + ci + taps + cp)
    w = torch.randn(co, ci * taps, generator=g)
    t = ops.conv_weight_relayout(_dev(w), co, ci, taps, 1, ci_pad=cp).cpu()
    assert t.shape == (co, taps * cp)
    assert torch.equal(t, G.relayout_ref(w, co, ci, taps, 1, cp))
    assert bool((t.view(co, taps, cp)[:, :, ci:] == 0).all())
    src = torch.randn(co, taps, cp, generator=g)
    src[:, :, ci:] = 12345.0                                   # a sentinel in the padded slots: mode 0 must not read them
    back = ops.conv_weight_relayout(_dev(src.view(co, -1)), co, ci, taps, 0, ci_pad=cp).cpu()
    assert back.shape == (co, ci * taps)
    assert torch.equal(back, G.relayout_ref(src, co, ci, taps, 0, cp)) and not bool((back == 12345.0).any())
    assert torch.equal(ops.conv_weight_relayout(_dev(t), co, ci, taps, 0, ci_pad=cp).cpu(), w)      # the exact inverse of mode 1
    k = ops.conv_weight_relayout(_dev(w), co, ci, taps, 2).cpu()
    assert k.shape == (taps * co, ci)
    assert torch.equal(k, G.relayout_ref(w, co, ci, taps, 2))


@pytest.mark.parametrize("rows,C,cp", [(7, 3, 4), (1, 1, 4), (5, 4, 4), (530000, 3, 4)])
def test_pad_channels_bit_exact(rows, C, cp):
    ops = _ops()
    x = torch.randn(rows, C, generator=G.gen(rows + C))
    out = ops.pad_channels(_dev(x), cp).cpu()
    assert out.shape == (rows, cp)
    assert torch.equal(out, G.pad_channels_ref(x, cp))
    assert bool((out[:, C:] == 0).all())


# ------------------------------------------------------------------------------------------------------ 3. maxpool2d
POOL_GEOMS = [
    (2, 9, 11, 5, 3, 2, 1),          # scalar kernel
    (2, 9, 11, 8, 3, 2, 1),          # 4-channel kernel
    (1, 4, 4, 4, 2, 2, 0),           # windows tile the image
    (2, 7, 5, 6, 3, 1, 1),           # stride 1: every pixel in up to 9 windows
    (1, 6, 6, 4, 3, 3, 0),           # stride = kernel
    (3, 8, 8, 3, 2, 1, 0),           # even kernel, no padding
    (2, 200, 200, 27, 3, 1, 1),      # scalar: 2.16 M outputs and pixels > 8192*256
    (2, 257, 257, 64, 3, 1, 1),      # 4-channel: 2.11 M float4 groups > 8192*256
]


@pytest.mark.parametrize("kind", ["normal", "ties"])
@pytest.mark.parametrize("case", POOL_GEOMS, ids=_geom_id)
def test_maxpool2d_values_argmax_and_backward(case, kind):
    ops = _ops()
    B, H, W, C, k, s, p = case
    g = G.gen(sum(case))
    x = torch.randn(B, H, W, C, generator=g) if kind == "normal" else G.ints((B, H, W, C), g, 0, 3)
    y_ref, idx_ref = G.maxpool_ref(x, k, s, p)
    y, arg = ops.maxpool2d_fwd(_dev(x), k, s, p)
    assert y.shape == y_ref.shape
    assert torch.equal(y.cpu(), y_ref)
    assert torch.equal(arg.cpu(), idx_ref)                     # on ties: the first maximum in (u, v) scan order
    dy = G.ints(y_ref.shape, g)
    dx = ops.maxpool2d_bwd(_dev(dy), arg, (B, H, W, C), k, s, p)
    assert torch.equal(dx.cpu(), G.maxpool_bwd_ref(dy, idx_ref, (B, H, W, C)).to(F32))


def test_maxpool2d_backward_random_normal():
    ops = _ops()
    B, H, W, C, k, s, p = case = (2, 7, 5, 6, 3, 1, 1)
    g = G.gen(21)
    x = G.ints((B, H, W, C), g, 0, 3)                          # ties: several windows share an arg-max, the gather adds up to 9 terms
    _, idx = G.maxpool_ref(x, k, s, p)
    dy = torch.randn(idx.shape, generator=g)
    y, arg = ops.maxpool2d_fwd(_dev(x), k, s, p)
    got = {"dx": ops.maxpool2d_bwd(_dev(dy), arg, (B, H, W, C), k, s, p)}
    ref64, ref32 = ({"dx": G.maxpool_bwd_ref(dy, idx, (B, H, W, C), dt)} for dt in (F64, F32))
    R.check_all(f"maxpool_bwd{case}", got, ref32, ref64)


@pytest.mark.parametrize("case", [(2, 9, 11, 5, 3, 2, 1), (2, 9, 11, 8, 3, 2, 1), (2, 7, 5, 6, 3, 1, 1), (2, 7, 5, 8, 3, 1, 1)],
                         ids=_geom_id)
def test_maxpool2d_propagates_nan_like_torch(case):
    """One NaN pixel per image: every window covering it is NaN in y, and the backward routes those windows' gradient to it.
    The second image has a second NaN right of the first in one channel: a window over both reports the last, as torch does."""
    ops = _ops()
    B, H, W, C, k, s, p = case
    g = G.gen(sum(case) + 5)
    x = torch.randn(B, H, W, C, generator=g)
    pix = [(H // 2, W // 2), (H - 1, 0)]                       # an interior pixel, a corner
    for b, (yy, xx) in enumerate(pix):
        x[b, yy, xx, :] = NAN
    x[1, H - 1, 1, C - 1] = NAN
    y_ref, idx_ref = G.maxpool_ref(x, k, s, p)
    cover = F.max_pool2d(torch.isnan(x).float().permute(0, 3, 1, 2), k, s, p).permute(0, 2, 3, 1) > 0
    assert torch.equal(torch.isnan(y_ref), cover) and int(cover.sum()) > 0
    y, arg = ops.maxpool2d_fwd(_dev(x), k, s, p)
    got_nan = torch.isnan(y.cpu())
    assert torch.equal(got_nan, cover), f"maxpool {case}: {int(got_nan.sum())} NaN outputs, {int(cover.sum())} windows cover a NaN pixel"
    assert G.equal_nan(y, y_ref)
    assert torch.equal(arg.cpu(), idx_ref)
    dy = G.ints(y_ref.shape, g)
    dx = ops.maxpool2d_bwd(_dev(dy), arg, (B, H, W, C), k, s, p).cpu()
    assert torch.equal(dx, G.maxpool_bwd_ref(dy, idx_ref, (B, H, W, C)).to(F32))
    yy, xx = pix[0]
    assert torch.equal(dx[0, yy, xx], (dy[0] * cover[0]).sum((0, 1)))
    both = (idx_ref[1, :, :, C - 1] == (H - 1) * W + 1) & cover[1, :, :, 0]
    assert int(both.sum()) > 0                                 # windows over both NaNs of that channel point at the second


# -------------------------------------------------------------------------------------------------- 4. masked pooling
MP_SIZES = [(2, 1, 8), (3, 2, 16), (3, 3, 100), (2, 5, 70), (2, 7, 130), (4, 9, 64),
            (33, 130, 250)]                                    # the last: B T e > 4096*256, the backward's grid-stride loop


def _pool_mask(B, T, g):
    """Ragged masks; row 0 has its single valid token at position 0, row 1 at the last position."""
    mask = torch.rand(B, T, generator=g) > 0.4
    mask[:, 0] = True
    mask[0] = False
    mask[0, 0] = True
    mask[1] = False
    mask[1, T - 1] = True
    return mask


def _mode(ops, mode):
    return ops.POOL_MEAN if mode == "mean" else ops.POOL_MAX


@pytest.mark.parametrize("B,T,e", MP_SIZES)
def test_masked_max_pool_bit_exact(B, T, e):
    ops = _ops()
    g = G.gen(B * T + e)
    mask = _pool_mask(B, T, g)
    mu8 = ops._mask_u8(_dev(mask))
    for kind in ("normal", "ties"):
        x = torch.randn(B, T, e, generator=g) if kind == "normal" else G.ints((B, T, e), g, -2, 2)
        x[:, :, 1] = -x[:, :, 1].abs() - 1.0                   # negative at every token: with any padded token the maximum is a padded 0
        dout = G.ints((B, e), g)
        out_ref, dx_ref, arg_ref = G.masked_pool_ref(x, mask, "max", dout)
        out, arg, _ = ops.masked_pool_fwd(_dev(x), mu8, ops.POOL_MAX)
        assert torch.equal(out.cpu(), out_ref.to(F32)), kind
        assert torch.equal(arg.cpu(), arg_ref), kind           # the first maximum over the whole sequence, padded zeros included
        dx = ops.masked_pool_bwd(_dev(dout), mu8, T, ops.POOL_MAX, arg, None).cpu()
        assert torch.equal(dx, dx_ref.to(F32)), kind
        padded_rows = ~mask.all(1)
        assert bool((out.cpu()[padded_rows, 1] == 0).all()) and bool((dx[padded_rows, :, 1] == 0).all())


@pytest.mark.parametrize("B,T,e", MP_SIZES)
def test_masked_pool_backward_on_integers_and_mean_forward(B, T, e):
    ops = _ops()
    g = G.gen(B * T + e + 1)
    mask = _pool_mask(B, T, g)
    mu8 = ops._mask_u8(_dev(mask))
    x, dout = G.ints((B, T, e), g), G.ints((B, e), g)
    ref64, ref32 = (G.masked_pool_ref(x, mask, "mean", dout, dt) for dt in (F64, F32))
    out, _, cnt = ops.masked_pool_fwd(_dev(x), mu8, ops.POOL_MEAN)
    assert torch.equal(cnt.cpu(), mask.sum(1).to(F32))
    dx = ops.masked_pool_bwd(_dev(dout), mu8, T, ops.POOL_MEAN, None, cnt)
    # one correctly rounded division of two small integers per element: the float64 quotient rounds to the same float32
    assert torch.equal(dx.cpu(), ref64[1].to(F32))
    R.check_all(f"masked_mean_int{(B, T, e)}", {"out": out}, {"out": ref32[0]}, {"out": ref64[0]})


@pytest.mark.parametrize("mode", ["mean", "max"])
@pytest.mark.parametrize("B,T,e", [(2, 1, 8), (2, 7, 130), (4, 9, 64)])
def test_masked_pool_random_normal(mode, B, T, e):
    ops = _ops()
    g = G.gen(B * T + e + 2)
    mask = _pool_mask(B, T, g)
    mu8 = ops._mask_u8(_dev(mask))
    x, dout = torch.randn(B, T, e, generator=g), torch.randn(B, e, generator=g)
    ref64, ref32 = (G.masked_pool_ref(x, mask, mode, dout, dt) for dt in (F64, F32))
    out, arg, cnt = ops.masked_pool_fwd(_dev(x), mu8, _mode(ops, mode))
    dx = ops.masked_pool_bwd(_dev(dout), mu8, T, _mode(ops, mode), arg, cnt)
    R.check_all(f"masked_{mode}{(B, T, e)}", {"out": out, "dx": dx}, {"out": ref32[0], "dx": ref32[1]},
                {"out": ref64[0], "dx": ref64[1]})


@pytest.mark.parametrize("B,T,e", [(3, 2, 16), (3, 3, 100), (2, 7, 130), (4, 9, 64)])
def test_masked_max_pool_propagates_nan_like_the_reference(B, T, e):
    """One NaN at a valid token and one at a padded token (NaN * 0 = NaN): the pooled value is NaN in both channels, the arg-max
    is the NaN position, and the gradient lands there (times the mask, as autograd gives: 0 at the padded token)."""
    ops = _ops()
    g = G.gen(B * T + e + 3)
    mask = torch.ones(B, T, dtype=torch.bool)
    mask[:, T - 1] = False                                     # the last token is padding in every row
    mask[B - 1, 0] = False
    x = torch.randn(B, T, e, generator=g)
    x[0, 0, 3] = NAN                                           # valid, first quarter of the sequence
    x[1, T - 1, 5] = NAN                                       # padded, last quarter
    x[B - 1, T // 2, e - 1] = NAN                              # valid (T > 2) or padded (T = 2), a middle quarter, the last channel
    dout = G.ints((B, e), g, 1, 8)
    out_ref, dx_ref, arg_ref = G.masked_pool_ref(x, mask, "max", dout)
    assert int(torch.isnan(out_ref).sum()) == 3
    mu8 = ops._mask_u8(_dev(mask))
    out, arg, _ = ops.masked_pool_fwd(_dev(x), mu8, ops.POOL_MAX)
    got_nan = int(torch.isnan(out).sum())
    assert got_nan == 3, f"masked max pool {(B, T, e)}: {got_nan} NaN outputs, the reference has 3"
    assert G.equal_nan(out, out_ref.to(F32))
    assert torch.equal(arg.cpu(), arg_ref)
    dx = ops.masked_pool_bwd(_dev(dout), mu8, T, ops.POOL_MAX, arg, None).cpu()
    assert torch.equal(dx, dx_ref.to(F32))
    assert float(dx[0, 0, 3]) == float(dout[0, 3]) and float(dx[1, T - 1, 5]) == 0.0


# ----------------------------------------------------------------------------------------------------- 5. mask_tokens
@pytest.mark.parametrize("rows,e", [(1, 1), (7, 6), (50, 384), (4100, 257)])
def test_mask_tokens_forward_and_as_its_own_backward(rows, e):
    ops = _ops()
    g = G.gen(rows + e)
    x = torch.randn(rows, e, generator=g)
    mask = torch.rand(rows, generator=g) > 0.5
    mask[0] = False
    mask[rows - 1] = rows > 1
    x[0, 0] = NAN                                              # under a false mask: 0 * NaN stays NaN
    if rows > 1:
        x[rows - 1, e - 1] = NAN                               # under a true mask
        x[0, 1] = -2.0                                         # under a false mask: 0 * -2 = -0.0
    mu8 = ops._mask_u8(_dev(mask))
    assert mu8.dtype == torch.uint8 and set(mu8.unique().tolist()) <= {0, 1}
    want = G.mask_tokens_ref(x, mask)
    assert bool(torch.isnan(want[0, 0])) and (rows == 1 or (bool(torch.signbit(want[0, 1])) and float(want[0, 1]) == 0.0))
    y = ops.mask_tokens(_dev(x), mu8)
    assert G.same_bits(y, want)                                # int32 views: -0.0 keeps its sign bit
    dy = torch.randn(rows, e, generator=g)
    assert G.same_bits(ops.mask_tokens(_dev(dy), mu8), G.mask_tokens_ref(dy, mask))
    x3 = x.view(1, rows, e) if rows % 5 else x.view(5, rows // 5, e)      # the (B, T, e) form the towers pass
    assert G.same_bits(ops.mask_tokens(_dev(x3), mu8).view(rows, e), want)


# ------------------------------------------------------------------------------------------------------ 6. vit_tokens
VIT_SIZES = [(1, 2, 4), (3, 5, 6), (2, 65, 384), (70, 65, 256)]       # the last: B T e and B (T-1) e > 4096*256


@pytest.mark.parametrize("B,T,e", VIT_SIZES)
def test_vit_tokens_forward_on_integers_and_backward_bit_exact(B, T, e):
    ops = _ops()
    g = G.gen(B + T + e)
    patch, cls, pos = G.ints((B * (T - 1), e), g), G.ints((e,), g), G.ints((T, e), g)
    tok = ops.vit_tokens_fwd(_dev(patch), _dev(cls), _dev(pos), B, T)
    assert tok.shape == (B, T, e)
    assert torch.equal(tok.cpu(), G.vit_tokens_ref(patch, cls, pos, B, T).to(F32))
    dtok = torch.randn(B, T, e, generator=g)
    dpatch = ops.vit_tokens_bwd(_dev(dtok))
    assert torch.equal(dpatch.cpu(), dtok[:, 1:].reshape(-1, e))


def test_vit_tokens_forward_random_normal():
    ops = _ops()
    B, T, e = 3, 5, 6
    g = G.gen(31)
    patch, cls, pos = torch.randn(B * (T - 1), e, generator=g), torch.randn(e, generator=g), torch.randn(T, e, generator=g)
    got = {"tok": ops.vit_tokens_fwd(_dev(patch), _dev(cls), _dev(pos), B, T)}
    ref64, ref32 = ({"tok": G.vit_tokens_ref(patch, cls, pos, B, T, dt)} for dt in (F64, F32))
    R.check_all(f"vit_tokens{(B, T, e)}", got, ref32, ref64)


# ------------------------------------------------------------------------------------------------- 7. series_features
@pytest.mark.parametrize("B,T", [(1, 1), (5, 50), (1030, 1024)])
def test_series_features_bit_exact(B, T):
    ops = _ops()
    g = G.gen(B + T)
    x, t = torch.randn(B, T, generator=g), torch.rand(B, T, generator=g) * 9000.0
    mask = torch.rand(B, T, generator=g) > 0.3
    mask[0, 0] = B * T > 1
    mask[-1, -1] = False
    inv_norm = 1.0 / 17945.14
    feat = ops.series_features(_dev(x), _dev(t), ops._mask_u8(_dev(mask)), inv_norm)
    assert feat.shape == (B, T, 4)
    assert torch.equal(feat.cpu(), G.series_features_ref(x, t, mask, inv_norm))
    assert bool((feat[..., 3] == 0).all()) and torch.equal(feat[..., 2].cpu() != 0, mask)


# -------------------------------------------------------------------------------------------------------- 8. add_rows
def _add_rows_case(B, T, e, src_strided, g, integers):
    draw = (lambda shape: G.ints(shape, g)) if integers else (lambda shape: torch.randn(shape, generator=g))
    buf = draw((B, T, e))
    if src_strided:
        sbuf = draw((B, 2, e + 4))
        src = sbuf[:, 1, 4:]                                   # row stride 2 (e + 4), an offset of 4 floats: 16-byte aligned
    else:
        sbuf = draw((B, e))
        src = sbuf
    return buf, sbuf, src


@pytest.mark.parametrize("B,T,e,src_strided", [(5, 7, 8, False), (300, 3, 384, False), (4200, 2, 1024, False), (5, 7, 8, True),
                                               (300, 3, 384, True)])
def test_add_rows_on_strided_views_leaves_the_rest_untouched(B, T, e, src_strided):
    ops = _ops()
    buf, sbuf, src = _add_rows_case(B, T, e, src_strided, G.gen(B + T + e), integers=True)
    dbuf, dsbuf = _dev(buf), _dev(sbuf)
    dsrc = dsbuf[:, 1, 4:] if src_strided else dsbuf
    assert (not dsrc.is_contiguous()) == src_strided
    ret = ops.add_rows(dbuf[:, 0, :], dsrc)
    assert ret.data_ptr() == dbuf.data_ptr()
    got = dbuf.cpu()
    assert torch.equal(got[:, 0, :], (buf[:, 0, :].double() + src.double()).to(F32))
    assert G.same_bits(got[:, 1:, :], buf[:, 1:, :])           # every element outside the view keeps its bits
    assert G.same_bits(dsbuf, sbuf)                            # and so does the source


def test_add_rows_random_normal():
    ops = _ops()
    B, T, e = 300, 3, 384
    buf, sbuf, src = _add_rows_case(B, T, e, True, G.gen(41), integers=False)
    dbuf, dsbuf = _dev(buf), _dev(sbuf)
    ops.add_rows(dbuf[:, 0, :], dsbuf[:, 1, 4:])
    ref64, ref32 = ({"dst": buf[:, 0, :].to(dt) + src.to(dt)} for dt in (F64, F32))
    R.check_all(f"add_rows{(B, T, e)}", {"dst": dbuf[:, 0, :]}, ref32, ref64)
    assert G.same_bits(dbuf.cpu()[:, 1:, :], buf[:, 1:, :])


# ------------------------------------------------------------------------------------------------------ 9. masked MSE
MSE_SIZES = [1, 63, 1025, 204800, 600001]                      # the last: > 2048*256, the backward's grid-stride loop


def _mse_inputs(n, g):
    shape = (n,) if n % 1024 else (n // 1024, 1024)            # the model passes (B, T, 1) predictions: the kernel sees numel()
    return torch.randn(shape, generator=g), torch.randn(shape, generator=g) * 0.5 + 0.2


def _selection(kind, shape, g):
    n = int(np.prod(shape))
    if kind == "all":
        return torch.ones(shape, dtype=torch.bool)
    if kind == "third":
        sel = torch.rand(shape, generator=g) < 0.3
        sel.view(-1)[n - 1] = True                             # never empty, and the tail element takes part
        return sel
    sel = torch.zeros(shape, dtype=torch.bool)
    if kind == "one":
        sel.view(-1)[(2 * n) // 3] = True
    return sel


@pytest.mark.parametrize("kind", ["all", "third", "one"])
@pytest.mark.parametrize("n", MSE_SIZES)
def test_masked_mse_forward_and_backward(n, kind):
    from multimodal_supernovae_amd.models_pretraining import masked_mse
    g = G.gen(n + len(kind))
    pred, target = _mse_inputs(n, g)
    sel = _selection(kind, pred.shape, g)
    grad_out = -1.75
    ref64, ref32 = (G.masked_mse_ref(pred, target, sel, grad_out, dt) for dt in (F64, F32))
    pd = _dev(pred).requires_grad_()
    loss = masked_mse(pd, _dev(target), _dev(sel))
    (loss * grad_out).backward()
    R.check_all(f"masked_mse[{n},{kind}]", {"loss": loss.detach().reshape(1), "dpred": pd.grad},
                {"loss": ref32[0], "dpred": ref32[1]}, {"loss": ref64[0], "dpred": ref64[1]})
    assert bool((pd.grad.cpu()[~sel] == 0).all())
    assert torch.equal(pd.grad.cpu() != 0, ref64[1] != 0)


@pytest.mark.parametrize("n", [1, 1025, 600001])
def test_masked_mse_with_nothing_selected_is_nan_with_a_zero_gradient(n):
    from multimodal_supernovae_amd.models_pretraining import masked_mse
    pred, target = _mse_inputs(n, G.gen(n))
    sel = _selection("none", pred.shape, None)
    loss_ref, d_ref = G.masked_mse_ref(pred, target, sel, 2.5)
    assert bool(torch.isnan(loss_ref).all()) and bool((d_ref == 0).all())
    pd = _dev(pred).requires_grad_()
    loss = masked_mse(pd, _dev(target), _dev(sel))
    (loss * 2.5).backward()
    assert bool(torch.isnan(loss))
    assert torch.equal(pd.grad.cpu(), torch.zeros_like(pred))


def test_masked_mse_count_is_exact():
    """stats[1], the number of selected elements (<= 2^24: exact in float32), through the C entry point."""
    from multimodal_supernovae_amd import ops
    from multimodal_supernovae_amd._lib import check, lib, ptr, stream_ptr
    g = G.gen(51)
    for n in MSE_SIZES:
        pred, target = _mse_inputs(n, g)
        sel = _selection("third", pred.shape, g)
        stats = torch.empty(2, dtype=F32, device=DEV)
        pd, td, sd = _dev(pred), _dev(target), ops._mask_u8(_dev(sel))
        check(lib().msn_masked_mse_fwd(ptr(pd), ptr(td), ptr(sd), n, ptr(stats), stream_ptr()), "msn_masked_mse_fwd")
        assert float(stats[1]) == float(sel.sum()), n


# --------------------------------------------------------------------------------------------------------- 10. dropout
SEEDS = [0, 1, (1 << 62) - 12345678901]
DROPOUT_N = [1, 257, 8192 * 256 + 257]                         # the last: above the 8192 x 256 grid


def _dropout_check(y, x, res, seed, p):
    """y (device) against the reference mask of `seed`: the zero pattern exactly, the kept values within 2 ulp."""
    n = x.numel()
    keep = torch.from_numpy(G.keep_mask(seed, n, p)).view(x.shape)
    y = y.cpu()
    base = res if res is not None else torch.zeros_like(x)
    assert torch.equal(y[~keep], base[~keep])                  # dropped: exactly 0 (+ residual)
    inv_keep = 1.0 / (1.0 - float(np.float32(p)))
    scaled = x.double() * inv_keep
    want = scaled + base.double()
    ulp = torch.from_numpy(np.spacing(np.abs(scaled.to(F32).numpy()))).double()
    tol = 2.0 * ulp
    if res is not None:                                        # one more rounding, of the sum
        tol = tol + torch.from_numpy(np.spacing(np.abs(want.to(F32).numpy()))).double()
    else:
        assert torch.equal(y != 0, keep)                       # x has no zeros: the zero pattern IS the mask
    assert bool(((y.double() - want).abs()[keep] <= tol[keep]).all())


@pytest.mark.parametrize("p", [0.0, 0.1, 0.5, 0.999])
@pytest.mark.parametrize("n", DROPOUT_N)
@pytest.mark.parametrize("seed", SEEDS)
def test_dropout_mask_is_the_reference_hash(seed, n, p):
    ops = _ops()
    x = torch.randn(n, generator=G.gen(n)).abs() + 0.25         # no zeros
    xd = _dev(x)
    y = ops.dropout(xd, p, seed)
    _dropout_check(y, x, None, seed, p)
    assert torch.equal(ops.dropout(xd.clone(), p, seed), y)    # the same (p, seed) reproduces the mask
    xin = xd.clone()
    assert ops.dropout(xin, p, seed, out=xin) is xin and G.same_bits(xin, y)       # in place: the same bytes


@pytest.mark.parametrize("n", [257, 8192 * 256 + 257])
def test_dropout_adds_the_residual_after_scaling(n):
    ops = _ops()
    g = G.gen(n + 1)
    x, res = torch.randn(n, generator=g).abs() + 0.25, torch.randn(n, generator=g)
    seed, p = SEEDS[2], 0.5
    y = ops.dropout(_dev(x), p, seed, residual=_dev(res))
    _dropout_check(y, x, res, seed, p)
    keep = torch.from_numpy(G.keep_mask(seed, n, p))
    # p = 0.5: the scale is exactly 2, so the kept values are one rounding of 2 x + res -- not 2 (x + res)
    assert torch.equal(y.cpu()[keep], (2.0 * x.double() + res.double()).to(F32)[keep])


def test_dropout_seed_token_adds_base_and_offset_mod_2_64(monkeypatch):
    ops = _ops()
    n, p = 1000, 0.3
    x = torch.randn(n, generator=G.gen(61)).abs() + 0.25
    base, offset = (1 << 63) + 5, (1 << 63) + (1 << 40) + 7       # the sum wraps
    seed = (base + offset) & G.MASK64
    assert seed == (1 << 40) + 12
    base_t = torch.tensor([G.as_i64(base)], dtype=torch.int64, device=DEV)
    y = ops.dropout(_dev(x), p, ops.SeedToken(base_t, offset))
    _dropout_check(y, x, None, seed, p)
    assert torch.equal(y, ops.dropout(_dev(x), p, seed))
    # msn_seed_advance: the base becomes the next value of the LCG (Python integers mod 2^64)
    monkeypatch.setattr(ops, "GRAPH_SEED", [base_t, 0])
    for _ in range(3):
        ops.graph_seed_advance()
        base = G.lcg_next(base)
        assert int(base_t.cpu()[0]) == G.as_i64(base)
    y2 = ops.dropout(_dev(x), p, ops.SeedToken(base_t, offset))
    _dropout_check(y2, x, None, (base + offset) & G.MASK64, p)
    assert not torch.equal(y2, y)
