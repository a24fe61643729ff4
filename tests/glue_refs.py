"""Plain torch / numpy references for the gather, mask and pooling glue kernels of csrc/conv.hip and csrc/rowops.hip: im2col and
its adjoint in both column orders, the convolution weight re-layouts, channel padding, 2-D max pooling, masked pooling, token
masking, ViT token assembly, the 1-D CNN's input features, the masked MSE and the counter-based dropout mask; and for the
implicit-GEMM convolutions of csrc/gemm.hip: the convolution with its three gradients in the layouts of the C ABI.  Shared by
tests/test_glue_kernels_gpu.py and tests/test_conv_implicit_gpu.py (the kernels against these, on the card) and
tests/test_glue_refs_cpu.py (these against F.conv2d, autograd and numpy, on any machine).

Nothing here imports the package under test.  Data movement is compared bit for bit; references that add take a `dtype`:
float64 gives the reference, float32 the yardstick e32 of convmixer_refs.check_all."""
import numpy as np
import torch
import torch.nn.functional as F

MASK64 = (1 << 64) - 1


def gen(seed):
    return torch.Generator().manual_seed(seed)


def ints(shape, g, lo=-8, hi=8):
    """Integer-valued float32 in [lo, hi]: sums of a few of them are exact in float32."""
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).to(torch.float32)


def same_bits(a, b):
    """Bit equality of two float32 tensors (tells -0.0 from +0.0 and compares NaNs by payload)."""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(a.view(torch.int32), b.view(torch.int32))


def equal_nan(a, b):
    """torch.equal with NaN == NaN."""
    a, b = a.detach().cpu(), b.detach().cpu()
    return a.shape == b.shape and torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a.nan_to_num(0.0), b.nan_to_num(0.0))


# ------------------------------------------------------------------------------------------- im2col and its adjoint
def conv_out(n, k, s, p):
    return (n + 2 * p - k) // s + 1


def im2col_ref(x_cl, kh, kw, sh, sw, ph, pw):
    """(B, H, W, C) channels-last -> rows (b, oh, ow) x columns (c, u, v): F.unfold on the NCHW view."""
    B = x_cl.shape[0]
    u = F.unfold(x_cl.permute(0, 3, 1, 2).contiguous(), (kh, kw), padding=(ph, pw), stride=(sh, sw))      # (B, C kh kw, L)
    return u.permute(0, 2, 1).reshape(B * u.shape[2], u.shape[1])


def tap_perm(C, taps):
    """Column j of the (u, v, c) order holds column tap_perm[j] of the (c, u, v) order."""
    return torch.arange(C * taps).view(C, taps).t().reshape(-1)


def im2col_tap_ref(x_cl, kh, kw, sh, sw, ph, pw):
    """The same rows with the columns in (u, v, c) order (channels fastest)."""
    return im2col_ref(x_cl, kh, kw, sh, sw, ph, pw)[:, tap_perm(x_cl.shape[-1], kh * kw)].contiguous()


def col2im_ref(dcols, shape, kh, kw, sh, sw, ph, pw, dtype=torch.float64):
    """Adjoint of im2col_ref: F.fold of the (c, u, v) columns at `dtype`; returns channels-last (B, H, W, C)."""
    B, H, W, C = shape
    d = dcols.to(dtype).reshape(B, -1, C * kh * kw).permute(0, 2, 1)
    return F.fold(d, (H, W), (kh, kw), padding=(ph, pw), stride=(sh, sw)).permute(0, 2, 3, 1).contiguous()


def col2im_tap_ref(dcols, shape, kh, kw, sh, sw, ph, pw, dtype=torch.float64):
    """Adjoint of im2col_tap_ref: the columns go back to (c, u, v) order, then col2im_ref."""
    inv = torch.argsort(tap_perm(shape[3], kh * kw))
    return col2im_ref(dcols[:, inv], shape, kh, kw, sh, sw, ph, pw, dtype)


# ----------------------------------------------------------------------------------------------- weight re-layouts
def relayout_ref(w, co, ci, taps, mode, ci_pad=None):
    """mode 1: (co, ci, taps) -> (co, taps, ci_pad), zeros in the channels ci .. ci_pad - 1;  mode 0: its inverse (the padded
    channels are dropped);  mode 2: (co, ci, taps) -> (tap, co, ci).  Flat 2-D results as the kernel's wrapper returns them."""
    ci_pad = ci if ci_pad is None else ci_pad
    if mode == 1:
        return F.pad(w.reshape(co, ci, taps).permute(0, 2, 1), (0, ci_pad - ci)).reshape(co, taps * ci_pad)
    if mode == 2:
        return w.reshape(co, ci, taps).permute(2, 0, 1).reshape(taps * co, ci)
    return w.reshape(co, taps, ci_pad)[:, :, :ci].permute(0, 2, 1).reshape(co, ci * taps)


def pad_channels_ref(x, cp):
    return F.pad(x, (0, cp - x.shape[-1]))


# ---------------------------------------------------------------------------------- the convolution and its gradients
def conv_w_tap(w):
    """(Cout, C, kh, kw) -> (Cout, kh*kw*C), tap-major with the channel fastest: the weight operand of the forward launch."""
    co, ci, kh, kw = w.shape
    return relayout_ref(w.reshape(co, -1), co, ci, kh * kw, 1).contiguous()


def conv_w_tco(w):
    """(Cout, C, kh, kw) -> (kh*kw*Cout, C), rows (tap, c_out): the weight operand of the dgrad launch."""
    co, ci, kh, kw = w.shape
    return relayout_ref(w.reshape(co, -1), co, ci, kh * kw, 2).contiguous()


def conv2d_ref(x_cl, w, bias, stride, padding, dy_rows, relu, dtype=torch.float64):
    """[relu](F.conv2d(x, w, bias)) and its autograd gradients under the cotangent `dy_rows`, at `dtype`, on the NCHW view of the
    channels-last x_cl (B, H, W, C); w is (Cout, C, kh, kw), dy_rows is (B*OH*OW, Cout).  Returns, in the layouts of the C ABI:
    y as rows (B*OH*OW, Cout), dx channels-last (B, H, W, C), dw_tap (Cout, kh*kw*C) tap-major, db (Cout).  bias = None is a zero
    bias: db is then the gradient such a bias would get.  With relu the cotangent goes through relu(conv): ReLU'(0) = 0."""
    co = w.shape[0]
    x = x_cl.detach().to(dtype).permute(0, 3, 1, 2).contiguous().requires_grad_()
    wr = w.detach().to(dtype, copy=True).requires_grad_()
    br = (torch.zeros(co, dtype=dtype) if bias is None else bias.detach().to(dtype, copy=True)).requires_grad_()
    y = F.conv2d(x, wr, br, stride=tuple(stride), padding=tuple(padding))
    if relu:
        y = torch.relu(y)
    y_rows = y.permute(0, 2, 3, 1).reshape(-1, co)
    dx, dw, db = torch.autograd.grad(y_rows, (x, wr, br), dy_rows.to(dtype).reshape(y_rows.shape))
    return y_rows.detach().contiguous(), dx.permute(0, 2, 3, 1).contiguous(), conv_w_tap(dw), db


# (B, H, W, C, Cout, kh, kw, sh, sw, ph, pw) of tests/test_conv_implicit_gpu.py (what each one is for: its docstring)
IMPLICIT_GEOMS = [
    (2, 6, 10, 64, 96, 3, 5, 1, 1, 0, 1),
    (4, 6, 6, 96, 96, 3, 3, 1, 1, 0, 0),
    (2, 6, 6, 96, 64, 3, 3, 1, 1, 2, 2),
    (16, 5, 12, 64, 64, 2, 3, 1, 2, 1, 0),
    (16, 7, 9, 64, 64, 3, 3, 2, 3, 1, 1),
    (32, 7, 9, 64, 128, 1, 1, 2, 2, 0, 0),
    (8, 1, 64, 64, 128, 1, 5, 1, 1, 0, 0),
    (2, 8, 8, 160, 128, 3, 3, 1, 1, 1, 1),
    (2, 8, 8, 128, 160, 3, 3, 1, 1, 1, 1),
    (4, 8, 8, 256, 256, 3, 3, 1, 1, 1, 1),
    (128, 8, 8, 64, 64, 3, 3, 1, 1, 1, 1),
]


def conv_inputs(case, integers):
    """x_cl (B, H, W, C), w (Cout, C, kh, kw), bias (Cout), dy (B*OH*OW, Cout) of one geometry, seeded by it.  integers: values
    in [-2, 2], the bias in [-3, 3] (every sum of the convolution and its gradients is exact in float32, in any order:
    test_glue_refs_cpu.py checks that);  else x, dy ~ N(0, 1), w ~ 0.1 N(0, 1), bias ~ N(0, 1)."""
    B, H, W, C, co, kh, kw, sh, sw, ph, pw = case
    g = gen(sum(case) + 1000 * integers)
    rows = B * conv_out(H, kh, sh, ph) * conv_out(W, kw, sw, pw)
    if integers:
        return ints((B, H, W, C), g, -2, 2), ints((co, C, kh, kw), g, -2, 2), ints((co,), g, -3, 3), ints((rows, co), g, -2, 2)
    return (torch.randn(B, H, W, C, generator=g), 0.1 * torch.randn(co, C, kh, kw, generator=g), torch.randn(co, generator=g),
            torch.randn(rows, co, generator=g))


# ---------------------------------------------------------------------------------------------------- 2-D max pool
def maxpool_ref(x_cl, k, s, p):
    """F.max_pool2d on the CPU: values and flat arg-max yy * W + xx (int32), both channels-last (B, OH, OW, C)."""
    y, idx = F.max_pool2d(x_cl.permute(0, 3, 1, 2).contiguous(), k, s, p, return_indices=True)
    return y.permute(0, 2, 3, 1).contiguous(), idx.permute(0, 2, 3, 1).contiguous().to(torch.int32)


def maxpool_bwd_ref(dy_cl, idx_cl, shape, dtype=torch.float64):
    """dx[b, pixel, c] = sum of dy over the windows whose arg-max is that pixel."""
    B, H, W, C = shape
    dy = dy_cl.to(dtype).permute(0, 3, 1, 2).reshape(B, C, -1)
    idx = idx_cl.to(torch.int64).permute(0, 3, 1, 2).reshape(B, C, -1)
    dx = torch.zeros(B, C, H * W, dtype=dtype).scatter_add_(2, idx, dy)
    return dx.view(B, C, H, W).permute(0, 2, 3, 1).contiguous()


# -------------------------------------------------------------------------------------------------- masked pooling
def masked_pool_ref(x, mask, mode, dout, dtype=torch.float64):
    """z = x * mask;  mean: sum_t z / sum_t mask;  max: max over ALL t of z (padded zeros take part).  Returns the pooled value,
    its gradient under the cotangent `dout` (autograd) and, for max, the arg-max torch reports."""
    xr = x.detach().to(dtype, copy=True).requires_grad_()
    z = xr * mask[:, :, None]
    arg = None
    if mode == "mean":
        out = z.sum(1) / mask.sum(1)[:, None]
    else:
        out, arg = z.max(dim=1)
        arg = arg.to(torch.int32)
    (dx,) = torch.autograd.grad(out, xr, dout.to(dtype))
    return out.detach(), dx, arg


def mask_tokens_ref(x, mask):
    """x * mask as the reference writes it: 0 * NaN stays NaN, 0 * negative is -0.0."""
    return x * mask[..., None].to(x.dtype)


# ----------------------------------------------------------------------------------------------- ViT token assembly
def vit_tokens_ref(patch, cls, pos, B, T, dtype=torch.float64):
    e = patch.shape[-1]
    tok = torch.cat([cls.to(dtype).reshape(1, 1, e).expand(B, 1, e), patch.to(dtype).reshape(B, T - 1, e)], 1)
    return tok + pos.to(dtype).reshape(1, T, e)


def series_features_ref(x, t, mask, inv_norm):
    """(x m, (t inv_norm) m, m, 0) in float32, the products taken left to right."""
    m = mask.to(torch.float32)
    inv = torch.tensor(inv_norm, dtype=torch.float32)
    return torch.stack([x * m, (t * inv) * m, m, torch.zeros_like(m)], dim=-1)


# ------------------------------------------------------------------------------------------------------ masked MSE
def masked_mse_ref(pred, target, sel, grad_out, dtype=torch.float64):
    """((pred - target)^2)[sel].mean() and d/dpred under the upstream gradient `grad_out`."""
    pr = pred.detach().to(dtype, copy=True).requires_grad_()
    loss = ((pr - target.to(dtype)) ** 2)[sel].mean()
    (d,) = torch.autograd.grad(loss, pr, torch.tensor(grad_out, dtype=dtype))
    return loss.detach().reshape(1), d


# --------------------------------------------------------------------------------------------------------- dropout
def keep_mask(seed, n, p):
    """The keep decision of the counter-based dropout for elements 0 .. n-1, in numpy uint64 (every step wraps mod 2^64):
    x = i * 0x9E3779B97F4A7C15 + seed; three xor-shift-multiply rounds; u = float32(x >> 40) * 2^-24; keep = u >= float32(p)."""
    x = np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.full(n, seed & MASK64, dtype=np.uint64)
    x ^= x >> np.uint64(33)
    x *= np.uint64(0xFF51AFD7ED558CCD)
    x ^= x >> np.uint64(33)
    x *= np.uint64(0xC4CEB9FE1A85EC53)
    x ^= x >> np.uint64(33)
    u = (x >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)
    return u >= np.float32(p)


def lcg_next(base):
    """The next value of the 64-bit LCG that moves the device-resident seed base once per recorded step."""
    return (base * 6364136223846793005 + 1442695040888963407) & MASK64


def as_i64(v):
    """A value mod 2^64 as the int64 torch stores."""
    v &= MASK64
    return v - (1 << 64) if v >= (1 << 63) else v
