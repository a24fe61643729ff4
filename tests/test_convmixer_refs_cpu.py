"""The hand-written references of tests/convmixer_refs.py against autograd, F.unfold, F.conv2d and F.batch_norm in float64, so
that what tests/test_convmixer_kernels_gpu.py holds the ConvMixer streaming kernels to is itself checked where no GPU exists."""
import math

import pytest
import torch
import torch.nn.functional as F

import convmixer_refs as R

PATCH_CASES = [(2, 3, 16, 16, 4), (3, 1, 23, 17, 10), (2, 4, 5, 9, 1), (1, 3, 8, 8, 8), (2, 3, 7, 12, 5)]
BN_SHAPES = [(7, 8), (1000, 32), (4100, 70), (70000, 12)]


@pytest.mark.parametrize("B,C,H,W,p", PATCH_CASES)
def test_patchify_ref_is_unfold_and_matches_the_conv_weight_layout(B, C, H, W, p):
    g = R.gen(B * 1000 + H * 10 + p)
    img = torch.randn(B, C, H, W, generator=g, dtype=torch.float64)
    gh, gw = H // p, W // p
    patches = R.patchify_ref(img, p)
    assert patches.shape == (B * gh * gw, C * p * p)
    unfolded = F.unfold(img[:, :, :gh * p, :gw * p], p, stride=p).transpose(1, 2).reshape(B * gh * gw, C * p * p)
    assert torch.equal(patches, unfolded)
    dim = 6
    w0 = torch.randn(dim, C, p, p, generator=g, dtype=torch.float64)
    conv = F.conv2d(img, w0, stride=p).permute(0, 2, 3, 1).reshape(B * gh * gw, dim)
    torch.testing.assert_close(patches @ w0.view(dim, -1).T, conv, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("B,C,H,W,p", PATCH_CASES)
def test_unpatchify_ref_is_the_adjoint(B, C, H, W, p):
    g = R.gen(B * 1000 + W * 10 + p)
    img = torch.randn(B, C, H, W, generator=g, dtype=torch.float64).requires_grad_()
    patches = R.patchify_ref(img, p)
    d = torch.randn(patches.shape, generator=g, dtype=torch.float64)
    (dimg,) = torch.autograd.grad(patches, img, d)
    got = R.unpatchify_ref(d, tuple(img.shape), p)
    assert torch.equal(got, dimg)
    gh, gw = H // p, W // p
    assert not bool(got[:, :, gh * p:, :].any()) and not bool(got[:, :, :, gw * p:].any())


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 7])
def test_dwconv_ref_pads_like_the_kernel_and_stores_gelu_prime(k):
    """padding='same' puts (k-1)//2 zeros on the left / top and the rest on the right / bottom (even k: one more on the right),
    which is what dw_geom of csrc/convmixer.hip assumes; `pre` is Phi(s) + s * phi(s)."""
    g = R.gen(40 + k)
    B, gh, gw, C = 2, 3, 5, 4
    x = torch.randn(B, gh, gw, C, generator=g)
    w, b = torch.randn(C, 1, k, k, generator=g) / k, torch.randn(C, generator=g)
    dpre, add = torch.randn(B, gh, gw, C, generator=g), torch.randn(B, gh, gw, C, generator=g)
    ref = R.dwconv_gelu_ref(x, w, b, dpre, add, torch.float64)
    lo = (k - 1) // 2
    hi = k - 1 - lo
    xp = F.pad(R.from_cl(x).double(), (lo, hi, lo, hi))
    s = F.conv2d(xp, w.double(), b.double(), groups=C)
    torch.testing.assert_close(ref["act"], R.to_cl(F.gelu(s)), rtol=1e-13, atol=1e-13)
    gp = 0.5 * (1 + torch.erf(s / math.sqrt(2))) + s * torch.exp(-0.5 * s * s) / math.sqrt(2 * math.pi)
    torch.testing.assert_close(ref["pre"], R.to_cl(gp), rtol=1e-12, atol=1e-12)
    # dx / dw / dbias are the gradients of <dpre, s>: written out tap by tap for one (channel, tap) and one pixel
    c, u, v = C - 1, k - 1, 0
    d, xc = R.from_cl(dpre).double()[:, c], xp[:, c]
    want = sum(float(d[:, i, j] @ xc[:, i + u, j + v]) for i in range(gh) for j in range(gw))
    assert abs(float(ref["dw"][c, 0, u, v]) - want) <= 1e-12 * max(1.0, abs(want))
    torch.testing.assert_close(ref["dbias"], dpre.double().sum(dim=(0, 1, 2)), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(ref["dx_add"] - ref["dx"], add.double(), rtol=0, atol=1e-14)


@pytest.mark.parametrize("n,R_,C", [(2, 512, 32), (3, 1367, 70), (4, 16, 8)])
def test_split_bn_bookkeeping_reproduces_one_batch_norm(n, R_, C):
    inp = R.bn_inputs(n * R_, C, seed=n * 100 + C, zero_column=False)
    ref = R.sync_bn_ref(inp, torch.float64)
    d = {k: v.double() for k, v in inp.items()}
    got = R.split_bn(R.TorchSplitBN(torch.float64), list(d["x"].chunk(n)), list(d["dy"].chunk(n)), d["gamma"], d["beta"],
                     d["rm"].clone(), d["rv"].clone())
    assert sorted(got) == sorted(ref)
    for k in ref:
        torch.testing.assert_close(got[k], ref[k], rtol=1e-11, atol=1e-11, msg=lambda m, k=k: f"{k}: {m}")


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("rows,C", BN_SHAPES)
def test_near_zero_share_stays_under_the_cap_on_the_reference(rows, C, training):
    inp = R.bn_inputs(rows, C, seed=rows + C)
    for residual in (False, True):
        v = R.bn_pre_relu(inp, training, residual)
        m = R.near_zero_mask(v)                                  # asserts the cap
        assert bool((v[:, 0] == 0).all()) and not bool(m[:, 0].any())   # the exact-zero column stays in the comparison
        assert float(m.double().mean()) <= 1.5e-3


def test_near_zero_rule():
    v = torch.tensor([0.0, -0.0, 5e-4, -9.9e-4, 1e-3, -2e-3, 1.0] + [3.0] * 1000, dtype=torch.float64)
    assert R.near_zero_mask(v)[:7].tolist() == [False, False, True, True, False, False, False]
    with pytest.raises(AssertionError):
        R.near_zero_mask(torch.full((10,), 1e-4, dtype=torch.float64))


@pytest.mark.parametrize("training", [True, False])
def test_bn_ref_relu_at_exact_zero_and_the_gelu_prime_multiplier(training):
    inp = R.bn_inputs(50, 6, seed=3)
    ref = R.bn_ref(inp, inp["dy"], training, residual=True, relu=True, dtype=torch.float64)
    assert float(ref["dgamma"][0]) == 0.0 and float(ref["dbeta"][0]) == 0.0 and not bool(ref["dres"][:, 0].any())
    assert torch.equal(ref["dres"], inp["dy"].double() * (ref["y"] > 0))
    plain = R.bn_ref(inp, inp["dy"], training, residual=False, relu=False, dtype=torch.float64)
    assert torch.equal(plain["dx_pre"], plain["dx"] * inp["pre"].double())
    assert ("running_mean" in plain) == training
    R.bn_ref(inp, inp["dy"], training, residual=True, relu=True, dtype=torch.float32)
    assert not any(t.requires_grad for t in inp.values()), "a reference changed its float32 inputs in place"


def test_bound_and_check_all():
    ref64 = torch.tensor([1.0, -2.0, 4.0], dtype=torch.float64)
    ref32 = ref64 + torch.tensor([0.0, 0.0, 4e-6], dtype=torch.float64)             # e32 = 1e-6
    assert R.scaled_err(ref32, ref64) == pytest.approx(1e-6)
    assert R.bound(ref32, ref64) == pytest.approx(8e-6)
    assert R.bound(ref64, ref64) == R.MARGIN * R.FLOOR                              # an exact yardstick leaves the floor
    ok = ref64 + torch.tensor([0.0, 3.0e-5, 0.0], dtype=torch.float64)              # 7.5e-6 of the scale
    bad = ref64 + torch.tensor([0.0, 3.4e-5, 0.0], dtype=torch.float64)             # 8.5e-6
    R.check_all("t", {"a": ok}, {"a": ref32}, {"a": ref64})
    with pytest.raises(AssertionError):
        R.check_all("t", {"a": bad}, {"a": ref32}, {"a": ref64})
    with pytest.raises(AssertionError):
        R.check_all("t", {"a": torch.tensor([1.0, float("nan"), 4.0])}, {"a": ref32}, {"a": ref64})
