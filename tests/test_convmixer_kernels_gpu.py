"""The streaming kernels of csrc/convmixer.hip, kernel by kernel, against plain torch on the CPU in float64.

References (tests/convmixer_refs.py, checked on the CPU by tests/test_convmixer_refs_cpu.py) are built from F.conv2d,
F.batch_norm, F.gelu, autograd and indexing only; none of them calls the package.  Patch gather / scatter is data movement
and compared bit for bit.  Every other tensor is held to

    max|got - ref64| <= 8 * max(e32, 4 * 2^-23) * max|ref64|

where e32 is the same error of torch's own float32 CPU evaluation of the same reference on the same inputs (computed in the
test, never taken from the kernel).  Each case prints `CONVMIXER-ACC <case> <tensor>: err .. bound .. (e32 ..)` before it
asserts.

A ReLU mask may flip where the pre-ReLU value is within rounding of zero: the cotangent is zeroed where the fp64 pre-ReLU value
is within 1e-3 of zero (at most 0.5 % of a tensor, asserted on the reference), so no element leaves the comparison.  Exact zeros
are kept: column 0 of every BatchNorm case has gamma = beta = 0 (and a zero residual), its output is exactly 0 and relu'(0) = 0
must show as d gamma = d beta = 0.

Largest figures measured on an MI355X per group (err as a multiple of max|ref64|; ratio = err / bound, 1 would miss):
    depthwise conv (9 cases)         err <= 9.7e-7 (dbias at B = 1100), e32 <= 1.8e-6, ratio <= 0.26
    BatchNorm variants (32 cases)    err <= 2.4e-7, e32 <= 2.2e-6, ratio <= 0.06
    synchronised BatchNorm (3)       err <= 1.3e-7, e32 <= 4.8e-7, ratio <= 0.04
    patch gather / scatter           bit-exact
The autograd half of the residual + ReLU cases and the module cases (5.) have not been measured on the card yet."""
import contextlib
import warnings

import pytest
import torch
import torch.nn as nn

import convmixer_refs as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64, F32 = torch.float64, torch.float32


def _ops():
    from multimodal_supernovae_amd import ops
    return ops


def _dev(t):
    return t.to(DEV).contiguous()


@contextlib.contextmanager
def _quiet():
    """padding='same' with an even kernel warns about a padded copy: expected here."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        yield


# --------------------------------------------------------------------------------- 1. depthwise 'same' conv + GELU
DW_CASES = [
    (2, 8, 8, 32, 5),        # the headline grid: interior and border taps together
    (3, 9, 6, 5, 5),         # non-square grid, channels no multiple of 4
    (2, 3, 5, 7, 4),         # even kernel, grid smaller than the kernel in one direction
    (2, 2, 2, 4, 7),         # kernel larger than the grid both ways
    (1, 1, 6, 3, 3),         # a single row
    (2, 7, 4, 70, 2),        # k = 2, more than 64 channels
    (3, 5, 5, 8, 1),         # k = 1
    (1100, 4, 4, 8, 3),      # B > 1024: the batch-strided loop of the dW partials, a finish pass over 1024 blocks
    (9, 32, 32, 128, 3),     # 1.18 M elements: the grid-stride loop of the forward and dX kernels
]


@pytest.mark.parametrize("B,gh,gw,C,k", DW_CASES)
def test_dwconv_gelu_forward_and_backward(B, gh, gw, C, k):
    ops = _ops()
    g = R.gen(7 * B + 100 * gh + 10 * gw + C + k)
    x = torch.randn(B, gh, gw, C, generator=g)
    w, b = torch.randn(C, 1, k, k, generator=g) / k, torch.randn(C, generator=g) * 0.5
    dpre, add = torch.randn(B, gh, gw, C, generator=g), torch.randn(B, gh, gw, C, generator=g)
    with _quiet():
        ref64, ref32 = (R.dwconv_gelu_ref(x, w, b, dpre, add, dt) for dt in (F64, F32))
    M = B * gh * gw
    xd, wd, bd, dd, ad = _dev(x).view(M, C), _dev(w), _dev(b), _dev(dpre).view(M, C), _dev(add).view(M, C)
    pre, act = ops.dwconv_gelu_fwd(xd, wd, bd, B, gh, gw)
    dx, dw, dbias = ops.dwconv_bwd(dd, xd, wd, B, gh, gw)
    dx_add, dw2, none = ops.dwconv_bwd(dd, xd, wd, B, gh, gw, add=ad, want_bias=False)
    torch.cuda.synchronize()
    assert none is None
    assert torch.equal(dw2, dw), "dW depends on add= / want_bias= (or is not deterministic)"
    shape = (B, gh, gw, C)
    got = {"act": act.view(shape), "pre": pre.view(shape), "dx": dx.view(shape), "dx_add": dx_add.view(shape), "dw": dw,
           "dbias": dbias}
    R.check_all(f"dwconv{(B, gh, gw, C, k)}", got, ref32, ref64)


# ----------------------------------------------------------------------------------------- 2. patchify / unpatchify
PATCH_CASES = [
    (2, 3, 16, 16, 4),       # the golden's own shape
    (3, 1, 23, 17, 10),      # non-square, floor in both directions
    (2, 4, 5, 9, 1),         # p = 1 (to_channels_last)
    (1, 3, 8, 8, 8),         # one patch
    (2, 3, 7, 12, 5),        # floor in both directions, small
    (5, 3, 300, 300, 4),     # 1.35 M elements: the grid-stride loop
]


@pytest.mark.parametrize("B,C,H,W,p", PATCH_CASES)
def test_patchify_and_unpatchify_bit_exact(B, C, H, W, p):
    ops = _ops()
    g = R.gen(B + 10 * C + 100 * H + W + p)
    img = torch.randn(B, C, H, W, generator=g)
    patches = ops.patchify(_dev(img), p)
    want = R.patchify_ref(img, p)
    assert patches.shape == want.shape
    assert torch.equal(patches.cpu(), want)
    d = torch.randn(want.shape, generator=g)
    dimg = ops.unpatchify(_dev(d), (B, C, H, W), p)
    assert torch.equal(dimg.cpu(), R.unpatchify_ref(d, (B, C, H, W), p))


@pytest.mark.parametrize("B,C,H,W,p", [(3, 1, 23, 17, 10), (2, 3, 7, 12, 5)])
def test_patch_columns_follow_the_conv_weight_layout(B, C, H, W, p):
    """patches @ w0.view(dim, -1).T is the stride-p convolution: ties the column order (c, u, v) to the weight layout."""
    import torch.nn.functional as F
    g = R.gen(17 * p + W)
    img, dim = torch.randn(B, C, H, W, generator=g), 6
    w0 = torch.randn(dim, C, p, p, generator=g, dtype=F64)
    patches = _ops().patchify(_dev(img), p).cpu().double()
    conv = F.conv2d(img.double(), w0, stride=p).permute(0, 2, 3, 1).reshape(-1, dim)
    torch.testing.assert_close(patches @ w0.view(dim, -1).T, conv, rtol=1e-12, atol=1e-12)


def test_to_channels_last_and_its_backward():
    from multimodal_supernovae_amd import functional as F_
    B, C, H, W = 2, 4, 5, 9
    g = R.gen(59)
    img, cot = torch.randn(B, C, H, W, generator=g), torch.randn(B, H, W, C, generator=g)
    xd = _dev(img).requires_grad_()
    out = F_.to_channels_last(xd)
    assert out.shape == (B, H, W, C) and torch.equal(out.detach().cpu(), img.permute(0, 2, 3, 1))
    out.backward(_dev(cot))
    assert torch.equal(xd.grad.cpu(), cot.permute(0, 3, 1, 2))


# --------------------------------------------------------------------------------------- 3. fused BatchNorm variants
BN_SHAPES = [(7, 8), (1000, 32), (4100, 70), (70000, 12)]
BN_VARIANTS = ["pre", "residual", "relu", "residual_relu"]


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("variant", BN_VARIANTS)
@pytest.mark.parametrize("rows,C", BN_SHAPES)
def test_batchnorm_variants(rows, C, variant, training):
    """Forward with residual= / relu=; backward with the pre= (GELU') multiplier, with relu_out= (msn_batchnorm_relu_bwd) and
    with ops.relu_mask followed by the plain backward (the residual + ReLU path of _BatchNormAct, which is also run through
    autograd so that the residual's gradient is checked)."""
    from multimodal_supernovae_amd.functional import _BatchNormAct
    ops = _ops()
    residual, relu = "residual" in variant, "relu" in variant
    inp = R.bn_inputs(rows, C, seed=rows + C)
    dy = inp["dy"].clone()
    if relu:
        dy[R.near_zero_mask(R.bn_pre_relu(inp, training, residual))] = 0.0
    ref64, ref32 = (R.bn_ref(inp, dy, training, residual, relu, dt) for dt in (F64, F32))
    d = {k: _dev(v) for k, v in inp.items()}
    dyd = _dev(dy)
    tag = f"bn{(rows, C)} {variant} {'train' if training else 'eval'}"

    def stats(got, rm, rv):
        if training:
            got["running_mean"], got["running_var"] = rm, rv
        else:
            assert torch.equal(rm.cpu(), inp["rm"]) and torch.equal(rv.cpu(), inp["rv"]), "eval mode changed the running statistics"
        return got

    rm, rv = d["rm"].clone(), d["rv"].clone()
    y, mean, rstd = ops.batchnorm_fwd(d["x"], d["gamma"], d["beta"], rm, rv, training,
                                      residual=d["res"] if residual else None, relu=relu)
    got = stats({"y": y}, rm, rv)
    if variant == "pre":
        got["dx_pre"], got["dgamma"], got["dbeta"] = ops.batchnorm_bwd(dyd, d["x"], d["pre"], mean, rstd, d["gamma"], training)
    elif variant == "residual":
        got["dx"], got["dgamma"], got["dbeta"] = ops.batchnorm_bwd(dyd, d["x"], None, mean, rstd, d["gamma"], training)
    elif variant == "relu":
        got["dx"], got["dgamma"], got["dbeta"] = ops.batchnorm_bwd(dyd, d["x"], None, mean, rstd, d["gamma"], training, relu_out=y)
    else:
        dm = ops.relu_mask(dyd, y)
        got["dres"] = dm
        got["dx"], got["dgamma"], got["dbeta"] = ops.batchnorm_bwd(dm, d["x"], None, mean, rstd, d["gamma"], training)
    torch.cuda.synchronize()
    if relu:      # forward / backward consistency at exact zeros: relu(0) = 0 and relu'(0) = 0
        assert not bool(y[:, 0].any()), "column 0 (gamma = beta = 0) must be exactly zero"
        assert float(got["dgamma"][0]) == 0.0 and float(got["dbeta"][0]) == 0.0, "relu'(0) must be 0"
    R.check_all(tag, got, ref32, ref64)
    if variant != "residual_relu":
        return
    xa, ga, ba, ra = (d[k].clone().requires_grad_() for k in ("x", "gamma", "beta", "res"))
    rm, rv = d["rm"].clone(), d["rv"].clone()
    out = _BatchNormAct.apply(xa, ga, ba, rm, rv, training, ra, True)
    out.backward(dyd)
    torch.cuda.synchronize()
    got = stats({"y": out.detach(), "dx": xa.grad, "dgamma": ga.grad, "dbeta": ba.grad, "dres": ra.grad}, rm, rv)
    assert float(ga.grad[0]) == 0.0 and float(ba.grad[0]) == 0.0 and not bool(ra.grad[:, 0].any()), "relu'(0) must be 0"
    R.check_all(tag + " autograd", got, ref32, ref64)


# ------------------------------------------------------------- 4. synchronised-BatchNorm split kernels, one process
class LibSplitBN:
    """The split entry points of libmsn_hip behind the interface of convmixer_refs.TorchSplitBN."""

    def __init__(self):
        from multimodal_supernovae_amd import _lib
        self.L, self.check, self.ptr, self.stream = _lib.lib(), _lib.check, _lib.ptr, _lib.stream_ptr

    def _ws(self, rows, C):
        nb = self.L.msn_bn_workspace_bytes(rows, C)
        return _ops()._workspace(nb, DEV), nb

    def colsum(self, x, center):
        rows, C = x.shape
        out, (ws, nb), p = torch.empty(C, dtype=F32, device=DEV), self._ws(rows, C), self.ptr
        self.check(self.L.msn_bn_colsum(p(x), rows, C, p(center), p(out), p(ws), nb, self.stream()), "msn_bn_colsum")
        return out

    def mean_from_sum(self, s, count):
        mean, p = torch.empty_like(s), self.ptr
        self.check(self.L.msn_bn_mean_from_sum(p(s), count, s.numel(), p(mean), self.stream()), "msn_bn_mean_from_sum")
        return mean

    def rstd_from_sqdev(self, sq, count, mean, rm, rv):
        rstd, p = torch.empty_like(sq), self.ptr
        self.check(self.L.msn_bn_rstd_from_sqdev(p(sq), count, sq.numel(), R.EPS, R.MOMENTUM, p(mean), p(rm), p(rv), p(rstd),
                                                 self.stream()), "msn_bn_rstd_from_sqdev")
        return rstd

    def apply(self, x, mean, rstd, gamma, beta):
        rows, C = x.shape
        y, p = torch.empty_like(x), self.ptr
        self.check(self.L.msn_batchnorm_apply(p(x), rows, C, p(mean), p(rstd), p(gamma), p(beta), p(None), 0, p(y),
                                              self.stream()), "msn_batchnorm_apply")
        return y

    def bwd_sums(self, dy, x, mean, rstd):
        rows, C = x.shape
        sums, (ws, nb), p = torch.empty(2 * C, dtype=F32, device=DEV), self._ws(rows, C), self.ptr
        self.check(self.L.msn_bn_bwd_sums(p(dy), p(x), rows, C, p(mean), p(rstd), p(sums), p(ws), nb, self.stream()),
                   "msn_bn_bwd_sums")
        return sums

    def bwd_apply(self, dy, x, count, mean, rstd, gamma, sums):
        rows, C = x.shape
        dx, p = torch.empty_like(x), self.ptr
        self.check(self.L.msn_bn_bwd_apply(p(dy), p(x), p(None), rows, count, C, p(mean), p(rstd), p(gamma), p(sums), p(dx),
                                           self.stream()), "msn_bn_bwd_apply")
        return dx


@pytest.mark.parametrize("n,rows,C", [(2, 512, 32), (3, 1367, 70), (4, 16, 8)])
def test_sync_batchnorm_split_kernels_in_one_process(n, rows, C):
    """n row blocks of `rows` rows each; the all-reduces are `+`.  Against ONE fp64 F.batch_norm over all n * rows rows: the
    unbiased running variance and the 1/count of the backward use the global count."""
    inp = R.bn_inputs(n * rows, C, seed=n * 100 + C, zero_column=False)
    ref64, ref32 = (R.sync_bn_ref(inp, dt) for dt in (F64, F32))
    d = {k: _dev(v) for k, v in inp.items()}
    xs, dys = [t.contiguous() for t in d["x"].chunk(n)], [t.contiguous() for t in d["dy"].chunk(n)]
    assert len(xs) == n and all(t.shape == (rows, C) for t in xs)
    got = R.split_bn(LibSplitBN(), xs, dys, d["gamma"], d["beta"], d["rm"].clone(), d["rv"].clone())
    torch.cuda.synchronize()
    R.check_all(f"syncbn{(n, rows, C)}", got, ref32, ref64)


# ------------------------------------------------------------------- 5. the module at shapes the goldens never take
MODULE_CASES = [
    (dict(dim=12, depth=2, channels=2, kernel_size=4, patch_size=3), (5, 2, 14, 20)),    # 4 x 6 grid, even kernel, floors
    (dict(dim=32, depth=1, channels=3, kernel_size=5, patch_size=4), (4, 3, 32, 48)),    # 8 x 12 grid
]
TRACKED = 3


def _seeded_state(m, g):
    """Every parameter and buffer drawn from `g`: fan-in scaled weights, BatchNorm scales around 1, non-trivial running
    statistics."""
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, nn.BatchNorm2d):
                mod.weight.copy_(torch.randn(mod.weight.shape, generator=g) * 0.2 + 1.0)
                mod.bias.copy_(torch.randn(mod.bias.shape, generator=g) * 0.2)
                mod.running_mean.copy_(torch.randn(mod.running_mean.shape, generator=g) * 0.1)
                mod.running_var.copy_(torch.rand(mod.running_var.shape, generator=g) + 0.5)
                mod.num_batches_tracked.fill_(TRACKED)
            elif isinstance(mod, (nn.Conv2d, nn.Linear)):
                fan_in = mod.weight[0].numel()
                mod.weight.copy_(torch.randn(mod.weight.shape, generator=g) / fan_in ** 0.5)
                if mod.bias is not None:
                    mod.bias.copy_(torch.randn(mod.bias.shape, generator=g) * 0.1)


def _oracle(state, x, cot, cfg, training, dtype):
    from oracle import encoders as oenc
    P = {k: (R.leaf(v, dtype) if v.is_floating_point() else v.clone()) for k, v in state.items()}
    x = R.leaf(x, dtype)
    stats = {}
    with _quiet():
        y = oenc.convmixer(P, "", x, depth=cfg["depth"], patch_size=cfg["patch_size"], training=training, stats_out=stats)
    y.backward(cot.to(dtype))
    out = {"y": y.detach(), "dx": x.grad}
    for k, v in P.items():
        if v.is_floating_point() and not k.endswith(("running_mean", "running_var")):
            out["grad " + k] = v.grad if v.grad is not None else torch.zeros_like(v)
    out.update({k: v.detach() for k, v in stats.items()})
    return out


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("cfg,shape", MODULE_CASES, ids=["dim12_k4_p3_14x20", "dim32_k5_p4_32x48"])
def test_convmixer_module_against_the_oracle_in_fp64(cfg, shape, training):
    from multimodal_supernovae_amd.models_multimodal import ConvMixer
    g = R.gen(cfg["dim"] + shape[-1])
    m = ConvMixer(n_out=8, dropout_prob=0.0, **cfg)
    _seeded_state(m, g)
    state = {k: v.detach().clone() for k, v in m.state_dict().items()}
    x, cot = torch.rand(shape, generator=g), torch.randn(shape[0], 8, generator=g)
    ref64, ref32 = (_oracle(state, x, cot, cfg, training, dt) for dt in (F64, F32))
    m.to(DEV).train(training)
    xd = _dev(x).requires_grad_()
    y = m(xd)
    y.backward(_dev(cot))
    torch.cuda.synchronize()
    got = {"y": y.detach(), "dx": xd.grad}
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        got["grad " + k] = p.grad
    sd = m.state_dict()
    for k, v in sd.items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == TRACKED + (1 if training else 0), k
        elif k.endswith(("running_mean", "running_var")):
            if training:
                got[k] = v
            else:
                assert torch.equal(v.cpu(), state[k]), f"eval mode changed {k}"
    assert sorted(got) == sorted(ref64), (sorted(set(got) ^ set(ref64)))
    R.check_all(f"module {cfg['dim']}/{cfg['kernel_size']}/{cfg['patch_size']} {'train' if training else 'eval'}", got, ref32, ref64)
