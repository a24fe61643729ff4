"""Heads wider than 128 columns (132 - 512, attention_wide.hip) through ops.attention_fwd / attention_bwd against the reference's
formula in fp64 (scores * scale, -1e7 key fill, softmax, @ v): widths, sequence lengths (also Tq != Tk, up to 1024), masks,
packed column slices, the shared query of the pooling head, host padding of odd widths, determinism and the path modes."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

WIDTHS = [132, 144, 192, 256, 320, 384, 512]
LENGTHS = [(1, 1), (9, 9), (17, 17), (64, 64), (65, 65), (128, 128), (129, 129), (200, 200), (220, 220), (40, 128), (77, 300),
           (1, 200)]


def _ref(q, k, v, mask, heads, scale):
    B, Tq, E = q.shape
    s = E // heads
    qh, kh, vh = (t.view(B, -1, heads, s) for t in (q, k, v))
    dot = torch.einsum("bihs,bjhs->bhij", qh, kh) * scale
    if mask is not None:
        dot = torch.where(mask[:, None, None, :], dot, torch.full_like(dot, -1e7))
    return torch.einsum("bhij,bjhs->bihs", torch.softmax(dot, dim=-1), vh).reshape(B, Tq, E)


def _mask(kind, B, Tk, g):
    """none | random (key 0 always on, the last sample fully padded) | a masked stretch across the 16-key chunk boundaries"""
    if kind == "none":
        return None
    mask = torch.rand(B, Tk, generator=g) > 0.3
    mask[:, 0] = True
    if kind == "random":
        if B > 1:
            mask[-1] = False
    else:
        mask[:, 10:41] = False
    return mask


def _check(qc, kc, vc, mask, heads, scale, dout, qr, kr, vr, what, q_shared=False):
    """forward and backward through ops against the fp64 gradients of qr / kr / vr (already computed); backward outputs
    filled with NaN beforehand, so every element must be written"""
    from multimodal_supernovae_amd import ops
    mu8 = ops._mask_u8(mask.cuda()) if mask is not None else None
    B, Tk = kc.shape[0], kc.shape[1]
    Tq = qc.shape[1]
    out, lse = ops.attention_fwd(qc, kc, vc, mu8, heads, scale, q_shared=q_shared)
    ref = _ref(qr.expand(B, Tq, -1) if q_shared else qr, kr, vr, mask, heads, scale)
    torch.testing.assert_close(out.cpu().double(), ref.detach(), rtol=1e-4, atol=3e-5, msg=lambda m: f"out {what}: {m}")
    ref.backward(dout.double())
    dq = torch.full((B, Tq, qc.shape[2]), float("nan"), device="cuda")
    dk, dv = torch.full_like(kc, float("nan")), torch.full_like(vc, float("nan"))
    ops.attention_bwd(qc, kc, vc, mu8, heads, scale, out, lse, dout.cuda(), dq, dk, dv, q_shared=q_shared)
    want_dq = qr.grad if not q_shared else None
    for got, want, name in ((dq, want_dq, "dq"), (dk, kr.grad, "dk"), (dv, vr.grad, "dv")):
        if want is None:
            continue
        torch.testing.assert_close(got.cpu().double(), want, rtol=3e-4, atol=3e-5, msg=lambda m: f"{name} {what}: {m}")
    return out, lse, dq, dk, dv


@pytest.mark.parametrize("hd", WIDTHS)
@pytest.mark.parametrize("heads", [1, 2])
def test_wide_heads_against_fp64(hd, heads):
    g = torch.Generator().manual_seed(100 * hd + heads)
    E = heads * hd
    for i, (Tq, Tk) in enumerate(LENGTHS):
        B = 2 if Tk > 1 else 3
        kind = ("none", "random", "stretch")[i % 3] if Tk > 41 else ("none", "random")[i % 2]
        mask = _mask(kind, B, Tk, g)
        q = torch.randn(B, Tq, E, generator=g)
        k, v = torch.randn(B, Tk, E, generator=g), torch.randn(B, Tk, E, generator=g)
        dout = torch.randn(B, Tq, E, generator=g)
        scale = 1.0 / math.sqrt(hd)
        qr, kr, vr = (t.double().requires_grad_() for t in (q, k, v))
        _check(q.cuda(), k.cuda(), v.cuda(), mask, heads, scale, dout, qr, kr, vr, (B, Tq, Tk, heads, hd, kind))


@pytest.mark.parametrize("hd,heads", [(256, 2), (512, 1)])
def test_wide_heads_spectrum_length(hd, heads):
    """T = 1024 (the reference's spectrum length): 64 key chunks of online softmax, a masked stretch across chunk boundaries"""
    g = torch.Generator().manual_seed(hd)
    B, T, E = 2, 1024, heads * hd
    q, k, v, dout = (torch.randn(B, T, E, generator=g) for _ in range(4))
    mask = torch.rand(B, T, generator=g) > 0.3
    mask[:, 0] = True
    mask[0, 250:530] = False
    mask[1] = False                    # a fully padded sample
    qr, kr, vr = (t.double().requires_grad_() for t in (q, k, v))
    _check(q.cuda(), k.cuda(), v.cuda(), mask, heads, 1.0 / math.sqrt(hd), dout, qr, kr, vr, (T, hd, heads))


@pytest.mark.parametrize("hd,heads", [(256, 2), (384, 1), (144, 2)])
def test_packed_column_slices(hd, heads):
    """q | k | v as column slices of one (B, T, 3e) buffer (ld = 3e, the block's qkv); k | v of a (B, T, 2e) buffer against a
    separate query (ld = 2e, the pooling head's kv); gradients into slices of packed buffers too"""
    from multimodal_supernovae_amd import ops
    g = torch.Generator().manual_seed(hd * heads)
    B, T, E = 3, 200, heads * hd
    qkv = torch.randn(B, T, 3 * E, generator=g)
    dout = torch.randn(B, T, E, generator=g)
    mask = _mask("random", B, T, g)
    scale = 1.0 / math.sqrt(hd)
    qr, kr, vr = (qkv[..., i * E:(i + 1) * E].double().requires_grad_() for i in range(3))
    ref = _ref(qr, kr, vr, mask, heads, scale)
    ref.backward(dout.double())
    qc = qkv.cuda()
    mu8 = ops._mask_u8(mask.cuda())
    out, lse = ops.attention_fwd(qc[..., :E], qc[..., E:2 * E], qc[..., 2 * E:], mu8, heads, scale)
    torch.testing.assert_close(out.cpu().double(), ref.detach(), rtol=1e-4, atol=3e-5)
    d3 = torch.full_like(qc, float("nan"))
    ops.attention_bwd(qc[..., :E], qc[..., E:2 * E], qc[..., 2 * E:], mu8, heads, scale, out, lse, dout.cuda(),
                      d3[..., :E], d3[..., E:2 * E], d3[..., 2 * E:])
    torch.testing.assert_close(d3.cpu().double(), torch.cat([qr.grad, kr.grad, vr.grad], -1), rtol=3e-4, atol=3e-5)
    # k | v packed, a separate query of another length
    kv = torch.randn(B, T, 2 * E, generator=g)
    q = torch.randn(B, 33, E, generator=g)
    dout = torch.randn(B, 33, E, generator=g)
    qr, kr, vr = q.double().requires_grad_(), kv[..., :E].double().requires_grad_(), kv[..., E:].double().requires_grad_()
    kvc = kv.cuda()
    _check(q.cuda(), kvc[..., :E], kvc[..., E:], None, heads, scale, dout, qr, kr, vr, "kv packed")


@pytest.mark.parametrize("hd", [132, 256, 512])
@pytest.mark.parametrize("T", [1, 40, 220])
def test_shared_query(hd, T):
    """One query shared by the batch (q_bstride 0, Tq = 1, no mask: the pooling head); dq per sample"""
    g = torch.Generator().manual_seed(hd + T)
    B, heads = 5, 2
    E = heads * hd
    q = torch.randn(1, 1, E, generator=g)
    kv = torch.randn(B, T, 2 * E, generator=g)
    dout = torch.randn(B, 1, E, generator=g)
    scale = 1.0 / math.sqrt(hd)
    kr, vr = kv[..., :E].double().requires_grad_(), kv[..., E:].double().requires_grad_()
    qs = q.double().expand(B, 1, E).clone().requires_grad_()          # per-sample leaf: the reference's dq per sample
    kvc = kv.cuda()
    out, lse, dq, dk, dv = _check(q.cuda(), kvc[..., :E], kvc[..., E:], None, heads, scale, dout, qs, kr, vr, (hd, T),
                                  q_shared=True)
    torch.testing.assert_close(dq.cpu().double(), qs.grad, rtol=3e-4, atol=3e-5)


@pytest.mark.parametrize("hd,heads", [(130, 2), (257, 1), (130, 1)])
def test_odd_widths_are_padded_on_the_host(hd, heads):
    """Widths above 128 that are not a multiple of 4: ops pads them (130 -> 132, 257 -> 260) and the wide kernels take them; the
    C-ABI itself refuses such a width with rc 1"""
    from multimodal_supernovae_amd import _lib, ops
    g = torch.Generator().manual_seed(hd * 3 + heads)
    B, T, E = 2, 70, heads * hd
    q, k, v, dout = (torch.randn(B, T, E, generator=g) for _ in range(4))
    mask = _mask("stretch", B, T, g)
    qr, kr, vr = (t.double().requires_grad_() for t in (q, k, v))
    qc, kc, vc = q.cuda(), k.cuda(), v.cuda()
    out, lse, *_ = _check(qc, kc, vc, mask, heads, 1.0 / math.sqrt(hd), dout, qr, kr, vr, (hd, heads))
    mu8 = ops._mask_u8(mask.cuda())
    lse_c = torch.empty(B, heads, T, 2, device="cuda")
    rc = _lib.lib().msn_attention_fwd(ops.ptr(qc), E, T * E, ops.ptr(kc), E, T * E, ops.ptr(vc), E, T * E, ops.ptr(mu8), B, heads, T, T,
                                      hd, 0.1, ops.ptr(out), E, T * E, ops.ptr(lse_c), ops.stream_ptr())
    assert rc == 1, "the C-ABI must refuse a head wider than 128 that is not a multiple of 4"


def test_heads_wider_than_512_are_refused():
    from multimodal_supernovae_amd import _lib, ops
    B, T, hd = 1, 8, 516
    x = torch.zeros(B, T, hd, device="cuda")
    out = torch.empty_like(x)
    lse = torch.empty(B, 1, T, 2, device="cuda")
    rc = _lib.lib().msn_attention_fwd(ops.ptr(x), hd, T * hd, ops.ptr(x), hd, T * hd, ops.ptr(x), hd, T * hd, ops.ptr(None), B, 1, T, T, hd, 0.1,
                                      ops.ptr(out), hd, T * hd, ops.ptr(lse), ops.stream_ptr())
    assert rc == 1
    assert "516 > 512" in _lib.lib().msn_last_error().decode()
    delta = torch.empty(B, 1, T, device="cuda")
    rc = _lib.lib().msn_attention_bwd(ops.ptr(x), hd, T * hd, ops.ptr(x), hd, T * hd, ops.ptr(x), hd, T * hd, ops.ptr(None), B, 1, T, T, hd, 0.1,
                                      ops.ptr(out), hd, T * hd, ops.ptr(lse), ops.ptr(x), hd, T * hd, ops.ptr(delta),
                                      ops.ptr(out), hd, T * hd, ops.ptr(out), hd, T * hd, ops.ptr(out), hd, T * hd, ops.stream_ptr())
    assert rc == 1
    assert "516 > 512" in _lib.lib().msn_last_error().decode()
    with pytest.raises(_lib.MsnHipError):
        ops.attention_fwd(x, x, x, None, 1, 0.1)


def test_deterministic_and_identical_under_every_path_mode():
    """Two runs are bitwise equal (fixed-order sums, no atomics), and the three msn_set_attention_path modes reach the same
    kernels for these widths"""
    from multimodal_supernovae_amd import _lib, ops
    g = torch.Generator().manual_seed(5)
    B, T, heads, hd = 4, 220, 2, 256
    E = heads * hd
    q, k, v, dout = (torch.randn(B, T, E, generator=g).cuda() for _ in range(4))
    mu8 = ops._mask_u8(_mask("random", B, T, g).cuda())
    scale = 1.0 / math.sqrt(hd)
    runs = []
    try:
        for path in (0, 0, 1, 2):
            _lib.check(_lib.lib().msn_set_attention_path(path))
            out, lse = ops.attention_fwd(q, k, v, mu8, heads, scale)
            dq, dk, dv = (torch.full_like(t, float("nan")) for t in (q, k, v))
            ops.attention_bwd(q, k, v, mu8, heads, scale, out, lse, dout, dq, dk, dv)
            runs.append(torch.cat([out.flatten(), lse.flatten(), dq.flatten(), dk.flatten(), dv.flatten()]).cpu())
    finally:
        _lib.lib().msn_set_attention_path(0)
    assert not torch.isnan(runs[0]).any()
    for r in runs[1:]:
        assert torch.equal(r, runs[0])


def test_lse_layout_and_delta():
    """lse is (B, H, Tq, 2) = (row maximum of the scaled, filled scores, log of the sum of exponentials beside it); the backward
    writes delta = rowsum(dO * O) into the caller's buffer"""
    from multimodal_supernovae_amd import _lib, ops
    g = torch.Generator().manual_seed(11)
    B, Tq, Tk, heads, hd = 2, 50, 90, 2, 192
    E = heads * hd
    q, k, v = torch.randn(B, Tq, E, generator=g), torch.randn(B, Tk, E, generator=g), torch.randn(B, Tk, E, generator=g)
    dout = torch.randn(B, Tq, E, generator=g)
    mask = _mask("random", B, Tk, g)
    scale = 1.0 / math.sqrt(hd)
    qc, kc, vc, dc = q.cuda(), k.cuda(), v.cuda(), dout.cuda()
    mu8 = ops._mask_u8(mask.cuda())
    out, lse = ops.attention_fwd(qc, kc, vc, mu8, heads, scale)
    dot = torch.einsum("bihs,bjhs->bhij", q.double().view(B, Tq, heads, hd), k.double().view(B, Tk, heads, hd)) * scale
    dot = torch.where(mask[:, None, None, :], dot, torch.full_like(dot, -1e7))
    m = dot.max(-1)[0]
    torch.testing.assert_close(lse[..., 0].cpu().double(), m, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(lse[..., 1].cpu().double(), torch.log(torch.exp(dot - m[..., None]).sum(-1)), rtol=1e-5, atol=1e-5)
    delta = torch.full((B, heads, Tq), float("nan"), device="cuda")
    dq, dk, dv = torch.empty_like(qc), torch.empty_like(kc), torch.empty_like(vc)
    _lib.check(_lib.lib().msn_attention_bwd(ops.ptr(qc), E, Tq * E, ops.ptr(kc), E, Tk * E, ops.ptr(vc), E, Tk * E, ops.ptr(mu8), B, heads,
                                            Tq, Tk, hd, scale, ops.ptr(out), E, Tq * E, ops.ptr(lse), ops.ptr(dc), E, Tq * E,
                                            ops.ptr(delta), ops.ptr(dq), E, Tq * E, ops.ptr(dk), E, Tk * E, ops.ptr(dv), E, Tk * E,
                                            ops.stream_ptr()), "msn_attention_bwd")
    want = (dout.double() * out.cpu().double()).view(B, Tq, heads, hd).sum(-1).transpose(1, 2)
    torch.testing.assert_close(delta.cpu().double(), want, rtol=1e-5, atol=1e-5)
