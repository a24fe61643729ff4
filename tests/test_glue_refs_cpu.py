"""The references of tests/glue_refs.py against torch itself, on the CPU: the column orders against F.conv2d, the adjoints
against the inner-product identity, the convolution with its gradients against those two, the pooling backward against autograd,
the dropout hash against its statistics."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import glue_refs as G

F64 = torch.float64
GEOMS = [(2, 9, 7, 4, 3, 3, 2, 2, 1, 1), (3, 1, 33, 8, 1, 7, 1, 2, 0, 3), (2, 4, 5, 12, 3, 2, 1, 2, 1, 0)]


@pytest.mark.parametrize("B,H,W,C,kh,kw,sh,sw,ph,pw", GEOMS)
def test_im2col_refs_times_the_weight_are_conv2d(B, H, W, C, kh, kw, sh, sw, ph, pw):
    g = G.gen(B + H + W + C)
    co = 5
    x, w = torch.randn(B, H, W, C, generator=g, dtype=F64), torch.randn(co, C, kh, kw, generator=g, dtype=F64)
    want = F.conv2d(x.permute(0, 3, 1, 2), w, stride=(sh, sw), padding=(ph, pw)).permute(0, 2, 3, 1).reshape(-1, co)
    got = G.im2col_ref(x, kh, kw, sh, sw, ph, pw) @ w.reshape(co, -1).t()
    assert got.shape == want.shape == (B * G.conv_out(H, kh, sh, ph) * G.conv_out(W, kw, sw, pw), co)
    torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12)
    w_tap = G.relayout_ref(w.reshape(co, -1), co, C, kh * kw, 1)
    got_tap = G.im2col_tap_ref(x, kh, kw, sh, sw, ph, pw) @ w_tap.t()
    torch.testing.assert_close(got_tap, want, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("B,H,W,C,kh,kw,sh,sw,ph,pw", GEOMS + [(2, 6, 6, 8, 1, 1, 2, 2, 0, 0)])
def test_col2im_refs_are_the_exact_adjoints(B, H, W, C, kh, kw, sh, sw, ph, pw):
    g = G.gen(B * H + W * C)
    geom = (kh, kw, sh, sw, ph, pw)
    x = G.ints((B, H, W, C), g).double()                  # integer-valued: both inner products are exact
    cols = G.im2col_ref(x, *geom)
    d = G.ints(cols.shape, g).double()
    assert float((cols * d).sum()) == float((x * G.col2im_ref(d, x.shape, *geom)).sum())
    cols_tap = G.im2col_tap_ref(x, *geom)
    assert float((cols_tap * d).sum()) == float((x * G.col2im_tap_ref(d, x.shape, *geom)).sum())
    if kh == kw == 1 and sh == 2:                         # pixels no window covers
        dx = G.col2im_ref(d, x.shape, *geom)
        assert bool((dx[:, 1::2] == 0).all()) and bool((dx[:, :, 1::2] == 0).all())


def test_relayout_refs_invert_each_other_and_pad_with_zeros():
    g = G.gen(3)
    co, ci, taps, cp = 7, 3, 5, 8
    w = torch.randn(co, ci * taps, generator=g)
    t = G.relayout_ref(w, co, ci, taps, 1, cp)
    assert t.shape == (co, taps * cp) and bool((t.view(co, taps, cp)[:, :, ci:] == 0).all())
    assert torch.equal(t.view(co, taps, cp)[2, 4, :ci], w.view(co, ci, taps)[2, :, 4])
    assert torch.equal(G.relayout_ref(t, co, ci, taps, 0, cp), w)
    assert torch.equal(G.relayout_ref(w, co, ci, taps, 2).view(taps, co, ci)[4, 2], w.view(co, ci, taps)[2, :, 4])


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("case", G.IMPLICIT_GEOMS, ids=lambda c: "-".join(map(str, c)))
def test_conv2d_ref_is_the_verified_column_references_on_integers(case, relu):
    """conv2d_ref (F.conv2d + autograd) against im2col_tap_ref / col2im_tap_ref / relayout_ref, which the tests above verify, in
    float64 on the integer inputs the GPU tests use: equality, and every sum stays inside float32's exact range in any order."""
    B, H, W, C, co, kh, kw = case[:7]
    geom, taps = case[5:], kh * kw
    x, w, b, dy = (t.double() for t in G.conv_inputs(case, True))
    y, dx, dw_tap, db = G.conv2d_ref(x, w, b, case[7:9], case[9:11], dy, relu)
    cols, w_tap = G.im2col_tap_ref(x, *geom), G.conv_w_tap(w)
    assert y.shape == dy.shape == (cols.shape[0], co) and w_tap.shape == (co, taps * C)
    assert dx.shape == x.shape and dw_tap.shape == w_tap.shape and db.shape == (co,)
    pre = cols @ w_tap.t() + b
    assert 0 < int((pre == 0).sum()) < pre.numel() // 20            # ReLU'(0) = 0 is exercised, and does not dominate
    d = dy * (pre > 0) if relu else dy
    assert torch.equal(torch.relu(pre) if relu else pre, y)
    assert torch.equal(G.col2im_tap_ref(d @ w_tap, x.shape, *geom), dx)
    assert torch.equal(d.t() @ cols, dw_tap)
    assert torch.equal(G.relayout_ref(dw_tap, co, C, taps, 0), d.t() @ G.im2col_ref(x, *geom))     # tap-major back to torch's (c, u, v)
    assert torch.equal(d.sum(0), db)
    w_tco = G.conv_w_tco(w)
    assert w_tco.shape == (taps * co, C) and torch.equal(w_tco.view(kh, kw, co, C)[kh - 1, 0, 3], w[3, :, kh - 1, 0])
    # exactness in float32, whatever the order of summation: the sum of the magnitudes of any result's terms is below 2^24
    assert max(4 * taps * C + 3, 4 * taps * co, 4 * cols.shape[0]) < 2 ** 24
    assert max(float(t.abs().max()) for t in (y, dx, dw_tap, db)) < 1024
    y32 = G.conv2d_ref(x.float(), w.float(), b.float(), case[7:9], case[9:11], dy.float(), relu, torch.float32)
    assert all(t.dtype == torch.float32 for t in y32)                # the yardstick really runs at float32


def test_conv2d_ref_without_bias_and_on_normal_inputs():
    case = G.IMPLICIT_GEOMS[3]
    x, w, b, dy = G.conv_inputs(case, False)
    assert x.dtype == torch.float32 and abs(float(w.std()) - 0.1) < 0.01 and abs(float(x.std()) - 1.0) < 0.05
    y0, dx0, dw0, db0 = G.conv2d_ref(x, w, None, case[7:9], case[9:11], dy, False)
    y1, dx1, dw1, db1 = G.conv2d_ref(x, w, b, case[7:9], case[9:11], dy, False)
    assert y0.dtype == F64
    torch.testing.assert_close(y0 + b.double(), y1, rtol=1e-12, atol=1e-12)
    assert torch.equal(dx0, dx1) and torch.equal(dw0, dw1) and torch.equal(db0, db1) and torch.equal(db0, dy.double().sum(0))
    assert not x.requires_grad and not w.requires_grad           # the caller's tensors stay as they are


@pytest.mark.parametrize("B,H,W,C,k,s,p", [(2, 9, 11, 5, 3, 2, 1), (1, 4, 4, 4, 2, 2, 0), (2, 7, 5, 6, 3, 1, 1)])
@pytest.mark.parametrize("ties", [False, True])
def test_maxpool_ref_backward_is_autograd(B, H, W, C, k, s, p, ties):
    g = G.gen(B + H + W + C + k)
    x = (G.ints((B, H, W, C), g, 0, 3) if ties else torch.randn(B, H, W, C, generator=g)).double()
    y, idx = G.maxpool_ref(x, k, s, p)
    assert y.shape == (B, G.conv_out(H, k, s, p), G.conv_out(W, k, s, p), C)
    assert torch.equal(x.reshape(B, H * W, C).gather(1, idx.reshape(B, -1, C).long()).reshape(y.shape), y)
    xr = x.permute(0, 3, 1, 2).clone().requires_grad_()
    dy = G.ints(y.shape, g).double()
    F.max_pool2d(xr, k, s, p).backward(dy.permute(0, 3, 1, 2))
    assert torch.equal(G.maxpool_bwd_ref(dy, idx, x.shape), xr.grad.permute(0, 2, 3, 1))


def test_maxpool_ref_propagates_nan_and_takes_the_first_maximum():
    x = torch.zeros(1, 4, 4, 1)
    y, idx = G.maxpool_ref(x, 3, 1, 1)
    assert int(idx[0, 1, 1, 0]) == 0 and int(idx[0, 0, 0, 0]) == 0 and int(idx[0, 3, 3, 0]) == 2 * 4 + 2   # first in (u, v) order
    x[0, 2, 1, 0] = float("nan")
    y, idx = G.maxpool_ref(x, 3, 1, 1)
    cover = F.max_pool2d(torch.isnan(x).float().permute(0, 3, 1, 2), 3, 1, 1).permute(0, 2, 3, 1) > 0
    assert torch.equal(torch.isnan(y), cover) and int(cover.sum()) == 9
    assert bool((idx[cover] == 2 * 4 + 1).all())
    x[0, 2, 2, 0] = float("nan")                            # a second NaN later in the scan: torch reports the last one
    _, idx = G.maxpool_ref(x, 3, 1, 1)
    assert int(idx[0, 2, 1, 0]) == 2 * 4 + 2 and int(idx[0, 2, 0, 0]) == 2 * 4 + 1


def test_masked_max_ref_takes_the_first_maximum_and_the_first_nan():
    g = G.gen(5)
    x = G.ints((3, 7, 6), g, -2, 2)
    mask = torch.rand(3, 7, generator=g) > 0.3
    mask[:, 0] = True
    x[1, 2, 3] = float("nan")                              # valid or padded: x * mask is NaN either way
    x[2, 5, 0] = float("nan")
    mask[2, 5] = False
    out, dx, arg = G.masked_pool_ref(x, mask, "max", torch.ones(3, 6))
    z = (x * mask[:, :, None]).numpy()
    assert np.array_equal(arg.numpy(), np.argmax(z, axis=1).astype(np.int32))      # numpy: first occurrence, NaN counts as the maximum
    assert bool(torch.isnan(out[1, 3])) and bool(torch.isnan(out[2, 0])) and int(arg[1, 3]) == 2 and int(arg[2, 0]) == 5
    assert int(torch.isnan(out).sum()) == 2
    assert float(dx[2, 5, 0]) == 0.0 and float(dx[1, 2, 3]) == float(mask[1, 2])


def test_mask_tokens_ref_keeps_nan_and_the_sign_of_zero():
    x = torch.tensor([[-1.5, float("nan"), 2.0]])
    y = G.mask_tokens_ref(x, torch.tensor([False]))
    assert torch.signbit(y[0, 0]) and torch.isnan(y[0, 1]) and not torch.signbit(y[0, 2]) and float(y[0, 2]) == 0.0
    assert G.same_bits(G.mask_tokens_ref(x, torch.tensor([True])), x)
    assert not G.same_bits(torch.tensor([0.0]), torch.tensor([-0.0]))


def test_masked_mse_ref_with_nothing_selected_is_nan_with_a_zero_gradient():
    pred, target = torch.randn(9), torch.randn(9)
    loss, d = G.masked_mse_ref(pred, target, torch.zeros(9, dtype=torch.bool), 1.7)
    assert bool(torch.isnan(loss).all()) and bool((d == 0).all())
    sel = torch.tensor([False, True] + [False] * 7)
    loss, d = G.masked_mse_ref(pred, target, sel, 1.7)
    assert float(loss) == float((pred[1].double() - target[1].double()) ** 2)
    assert float(d[1]) == 2 * 1.7 * float(pred[1].double() - target[1].double()) and int((d != 0).sum()) == 1


@pytest.mark.parametrize("p", [0.1, 0.5, 0.999])
def test_keep_mask_keeps_its_share(p):
    n = 10 ** 6
    kept = int(G.keep_mask(12345, n, p).sum())
    q = 1.0 - float(np.float32(p))
    assert abs(kept - n * q) <= 3.0 * (n * q * (1 - q)) ** 0.5 + 1.0, (kept, n * q)


def test_keep_mask_depends_on_the_seed_and_p_zero_keeps_all():
    a, b = G.keep_mask(0, 4096, 0.5), G.keep_mask(1, 4096, 0.5)
    assert not np.array_equal(a, b) and 0.3 < float((a != b).mean()) < 0.7
    assert bool(G.keep_mask(7, 4096, 0.0).all())
    assert np.array_equal(G.keep_mask((1 << 64) + 5, 100, 0.5), G.keep_mask(5, 100, 0.5))      # the seed is taken mod 2^64


def test_keep_mask_one_element_by_hand():
    """Element 3 of seed 11 in Python integers mod 2^64."""
    m = G.MASK64
    x = (3 * 0x9E3779B97F4A7C15 + 11) & m
    x ^= x >> 33
    x = (x * 0xFF51AFD7ED558CCD) & m
    x ^= x >> 33
    x = (x * 0xC4CEB9FE1A85EC53) & m
    x ^= x >> 33
    u = (x >> 40) / 2.0 ** 24
    for p in (0.1, 0.5, 0.9):
        assert bool(G.keep_mask(11, 4, p)[3]) == (u >= float(np.float32(p)))


def test_lcg_next_and_as_i64():
    assert G.lcg_next(0) == 1442695040888963407
    assert G.lcg_next((1 << 64) - 1) == (1442695040888963407 - 6364136223846793005) % (1 << 64)
    assert G.as_i64((1 << 63) + 5) == -(1 << 63) + 5 and G.as_i64(5) == 5
