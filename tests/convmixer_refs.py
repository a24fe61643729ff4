"""Plain-torch references for the streaming kernels of csrc/convmixer.hip (patch gather / scatter, depthwise 'same' convolution
+ GELU, BatchNorm with fused residual / ReLU / GELU', the split kernels of synchronised BatchNorm) and the error bound they are
held to.  Shared by tests/test_convmixer_kernels_gpu.py (the kernels against these, on the card) and
tests/test_convmixer_refs_cpu.py (these against autograd / F.conv2d / F.batch_norm, on any machine).

Nothing here imports the package under test.  Every reference takes a `dtype`: float64 gives the reference, float32 gives the
yardstick e32 of the bound

    max|got - ref64| <= MARGIN * max(e32, 4 * 2^-23) * max|ref64|,       e32 = max|ref32 - ref64| / max|ref64|

MARGIN = 8 allows for another summation order (four-way unrolled partials, 16 groups, up to 1024 block partials) and for
erff / __expf in place of libm, and for nothing else."""
import torch
import torch.nn.functional as F

MARGIN = 8.0
FLOOR = 4.0 * 2.0 ** -23
NEAR_ZERO = 1e-3          # |pre-ReLU value| below this (and not exactly 0): the cotangent is zeroed
NEAR_ZERO_CAP = 5e-3      # at most this share of a tensor may be zeroed that way
MOMENTUM, EPS = 0.1, 1e-5


def gen(seed):
    return torch.Generator().manual_seed(seed)


def leaf(t, dtype):
    """A copy of `t` at `dtype` that requires grad (a copy also at float32: the caller's tensor stays as it is)."""
    return t.detach().to(dtype, copy=True).requires_grad_()


# ------------------------------------------------------------------------------------------------------ the bound
def scaled_err(got, ref64):
    """max|got - ref64| / max|ref64| (max|ref64| = 0: the absolute error)."""
    got, ref64 = got.detach().cpu().double(), ref64.detach().double()
    assert got.shape == ref64.shape, (tuple(got.shape), tuple(ref64.shape))
    assert bool(torch.isfinite(got).all()), "non-finite values"
    if got.numel() == 0:
        return 0.0
    scale = float(ref64.abs().max())
    return float((got - ref64).abs().max()) / (scale if scale > 0.0 else 1.0)


def bound(ref32, ref64):
    """The right-hand side of the bound, relative to max|ref64|."""
    return MARGIN * max(scaled_err(ref32, ref64), FLOOR)


def check_all(tag, got, ref32, ref64, keys=None):
    """Every tensor of `got` against the bound; prints one line `tag key: err / bound (e32)` per tensor BEFORE asserting, and
    reports every miss at once.  Returns {key: (err, bound)}."""
    out, misses = {}, []
    for k in (keys or sorted(got)):
        err, e32 = scaled_err(got[k], ref64[k]), scaled_err(ref32[k], ref64[k])
        lim = MARGIN * max(e32, FLOOR)
        print(f"CONVMIXER-ACC {tag} {k}: err {err:.3e} bound {lim:.3e} (e32 {e32:.3e})")
        out[k] = (err, lim)
        if not err <= lim:
            misses.append(f"{k}: {err:.3e} > {lim:.3e}")
    assert not misses, f"{tag}: " + "; ".join(misses)
    return out


# ------------------------------------------------------------------------------------------------- patch gather
def patchify_ref(img, p):
    """(B, C, H, W) -> rows (b, i, j) x columns (c, u, v) of the floor(H/p) x floor(W/p) grid of p x p patches."""
    B, C, H, W = img.shape
    gh, gw = H // p, W // p
    t = img[:, :, :gh * p, :gw * p].reshape(B, C, gh, p, gw, p)
    return t.permute(0, 2, 4, 1, 3, 5).reshape(B * gh * gw, C * p * p)


def unpatchify_ref(dpatches, shape, p):
    """The exact adjoint of patchify_ref: zeros in the pixels beyond the floor grid."""
    B, C, H, W = shape
    gh, gw = H // p, W // p
    dimg = torch.zeros(shape, dtype=dpatches.dtype)
    dimg[:, :, :gh * p, :gw * p] = dpatches.reshape(B, gh, gw, C, p, p).permute(0, 3, 1, 4, 2, 5).reshape(B, C, gh * p, gw * p)
    return dimg


# ----------------------------------------------------------------------------------- depthwise 'same' conv + GELU
def to_cl(t):
    """(B, C, H, W) -> contiguous (B, H, W, C)."""
    return t.permute(0, 2, 3, 1).contiguous()


def from_cl(t):
    return t.permute(0, 3, 1, 2).contiguous()


def dwconv_gelu_ref(x_cl, w, b, dpre_cl, add_cl, dtype):
    """x_cl, dpre_cl, add_cl: channels-last (B, gh, gw, C); w (C, 1, k, k); b (C).  s = conv2d(x, w, b, 'same', groups = C),
    act = gelu(s), pre = d gelu(s) / ds (what the kernel stores in place of s); dx / dw / dbias = the gradients of s under the
    cotangent dpre, dx_add = dx + add.  All activations returned channels-last."""
    C = x_cl.shape[-1]
    x, w, b = leaf(from_cl(x_cl), dtype), leaf(w, dtype), leaf(b, dtype)
    s = F.conv2d(x, w, b, padding="same", groups=C)
    act = F.gelu(s)
    (gp,) = torch.autograd.grad(act, s, torch.ones_like(act), retain_graph=True)
    dx, dw, db = torch.autograd.grad(s, (x, w, b), from_cl(dpre_cl).to(dtype))
    dx = to_cl(dx)
    return {"act": to_cl(act.detach()), "pre": to_cl(gp), "dx": dx, "dx_add": dx + add_cl.to(dtype), "dw": dw, "dbias": db}


# --------------------------------------------------------------------------------------------- BatchNorm variants
def near_zero_mask(v64):
    """Elements of the fp64 pre-ReLU value within NEAR_ZERO of zero but not exactly zero: a ReLU mask computed in fp32 may
    flip there, so the cotangent is zeroed and the mask cannot matter.  Exact zeros stay in: relu'(0) = 0 is part of the
    contract (a column with gamma = beta = 0 tests it).  Asserts the share is at most NEAR_ZERO_CAP."""
    m = (v64.abs() < NEAR_ZERO) & (v64 != 0)
    share = float(m.double().mean())
    assert share <= NEAR_ZERO_CAP, f"{share:.2e} of the elements sit within {NEAR_ZERO} of the ReLU kink"
    return m


def bn_inputs(rows, C, seed, zero_column=True):
    """fp32 inputs of one BatchNorm case.  Column 0 has gamma = beta = 0 and a zero residual: its output is exactly 0 with and
    without the residual, so a ReLU mask taken with >= instead of > shows in d gamma / d beta."""
    g = gen(seed)
    d = {"x": torch.randn(rows, C, generator=g) * 1.5 + 0.3, "gamma": torch.randn(C, generator=g) + 1,
         "beta": torch.randn(C, generator=g), "rm": torch.randn(C, generator=g) * 0.1, "rv": torch.rand(C, generator=g) + 0.5,
         "res": torch.randn(rows, C, generator=g), "dy": torch.randn(rows, C, generator=g),
         "pre": torch.randn(rows, C, generator=g)}
    if zero_column:
        d["gamma"][0] = 0.0
        d["beta"][0] = 0.0
        d["res"][:, 0] = 0.0
    return d


def bn_pre_relu(inp, training, residual):
    """The fp64 value the ReLU sees: BatchNorm(x) (+ residual)."""
    x = inp["x"].double()
    v = F.batch_norm(x, inp["rm"].double().clone(), inp["rv"].double().clone(), inp["gamma"].double(), inp["beta"].double(),
                     training=training, momentum=MOMENTUM, eps=EPS)
    return v + inp["res"].double() if residual else v


def bn_ref(inp, dy, training, residual, relu, dtype):
    """y = [relu](batch_norm(x) [+ res]) and its gradients under the cotangent dy, plus the updated running statistics.
    dx_pre = dx * pre: what the kernel's backward returns when handed the GELU' multiplier `pre`."""
    x, gamma, beta, res = (leaf(inp[k], dtype) for k in ("x", "gamma", "beta", "res"))
    rm, rv = inp["rm"].to(dtype).clone(), inp["rv"].to(dtype).clone()
    v = F.batch_norm(x, rm, rv, gamma, beta, training=training, momentum=MOMENTUM, eps=EPS)
    if residual:
        v = v + res
    y = torch.relu(v) if relu else v
    grads = torch.autograd.grad(y, (x, gamma, beta) + ((res,) if residual else ()), dy.to(dtype))
    out = {"y": y.detach(), "dx": grads[0], "dgamma": grads[1], "dbeta": grads[2], "dx_pre": grads[0] * inp["pre"].to(dtype)}
    if residual:
        out["dres"] = grads[3]
    if training:
        out["running_mean"], out["running_var"] = rm, rv
    return out


# ------------------------------------------------------------------- synchronised BatchNorm: cut, run per block, add
class TorchSplitBN:
    """The six split entry points of synchronised BatchNorm restated in torch at one dtype (the primitives split_bn drives)."""

    def __init__(self, dtype):
        self.dtype = dtype

    def colsum(self, x, center):
        return x.sum(0) if center is None else ((x - center) ** 2).sum(0)

    def mean_from_sum(self, s, count):
        return s / count

    def rstd_from_sqdev(self, sq, count, mean, rm, rv):
        """Returns rstd; updates rm / rv in place (unbiased variance over the global count)."""
        rm.mul_(1 - MOMENTUM).add_(MOMENTUM * mean)
        rv.mul_(1 - MOMENTUM).add_(MOMENTUM * sq / (count - 1))
        return 1.0 / torch.sqrt(sq / count + EPS)

    def apply(self, x, mean, rstd, gamma, beta):
        return (x - mean) * rstd * gamma + beta

    def bwd_sums(self, dy, x, mean, rstd):
        """(sum dy, sum dy * xhat) as one 2C vector."""
        return torch.cat([dy.sum(0), (dy * (x - mean) * rstd).sum(0)])

    def bwd_apply(self, dy, x, count, mean, rstd, gamma, sums):
        C = x.shape[1]
        xhat = (x - mean) * rstd
        return gamma * rstd * (dy - (sums[:C] + xhat * sums[C:]) / count)


def split_bn(prim, xs, dys, gamma, beta, rm, rv):
    """Synchronised BatchNorm over the row blocks `xs` (cotangents `dys`) with the all-reduces played by `+`:
    column sums per block added, mean over the global count, centred column sums per block added, rstd + running statistics,
    apply per block; backward sums per block added, apply per block with the added sums and the global count.
    rm / rv are updated in place.  Returns y, dx (blocks concatenated), mean, rstd, and the blocks' local d gamma / d beta added."""
    count = sum(int(x.shape[0]) for x in xs)
    C = xs[0].shape[1]
    total = None
    for x in xs:
        s = prim.colsum(x, None)
        total = s if total is None else total + s
    mean = prim.mean_from_sum(total, count)
    sq = None
    for x in xs:
        s = prim.colsum(x, mean)
        sq = s if sq is None else sq + s
    rstd = prim.rstd_from_sqdev(sq, count, mean, rm, rv)
    ys = [prim.apply(x, mean, rstd, gamma, beta) for x in xs]
    local = [prim.bwd_sums(dy, x, mean, rstd) for dy, x in zip(dys, xs)]
    sums = local[0].clone()
    for s in local[1:]:
        sums = sums + s
    dxs = [prim.bwd_apply(dy, x, count, mean, rstd, gamma, sums) for dy, x in zip(dys, xs)]
    return {"y": torch.cat(ys), "dx": torch.cat(dxs), "mean": mean, "rstd": rstd, "dbeta": sums[:C].clone(),
            "dgamma": sums[C:].clone(), "running_mean": rm, "running_var": rv}


def sync_bn_ref(inp, dtype):
    """One F.batch_norm over all rows: what split_bn has to reproduce."""
    x, gamma, beta = (leaf(inp[k], dtype) for k in ("x", "gamma", "beta"))
    rm, rv = inp["rm"].to(dtype).clone(), inp["rv"].to(dtype).clone()
    y = F.batch_norm(x, rm, rv, gamma, beta, training=True, momentum=MOMENTUM, eps=EPS)
    dx, dg, db = torch.autograd.grad(y, (x, gamma, beta), inp["dy"].to(dtype))
    xd = x.detach()
    mean = xd.mean(0)
    rstd = 1.0 / torch.sqrt(((xd - mean) ** 2).mean(0) + EPS)
    return {"y": y.detach(), "dx": dx, "dgamma": dg, "dbeta": db, "mean": mean, "rstd": rstd, "running_mean": rm,
            "running_var": rv}
