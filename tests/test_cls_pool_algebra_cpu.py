"""The identities behind csrc/cls_pool.hip and functional._cls_pool_forward / _cls_pool_backward, in fp64 torch on the CPU: the
class-token attention of the ViT's last block with the key | value weights moved to the query's side equals the original
formulation (LayerNorm -> key | value Linear -> one-query softmax attention), value by value and gradient by gradient."""
import math

import pytest
import torch


def _inputs(B, T, e, heads, seed, q_gain=1.0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    return dict(x=r(B, T, e), g1=1 + 0.2 * r(e), b1=0.1 * r(e), wqkv=r(3 * e, e) / math.sqrt(e) * q_gain, bqkv=0.1 * r(3 * e),
                da=r(B, e), dx1=r(B, e))


def original(x, g1, b1, wqkv, bqkv, heads, eps=1e-6):
    """-> (h1, q, p (B, heads, T), a (B, e)) of the original formulation."""
    B, T, e = x.shape
    d = e // heads
    h1 = torch.nn.functional.layer_norm(x, (e,), g1, b1, eps)
    q2 = h1[:, 0] @ wqkv[:e].T + bqkv[:e]
    q = q2.view(B, heads, d)
    k = (h1 @ wqkv[e:2 * e].T + bqkv[e:2 * e]).view(B, T, heads, d)
    v = (h1 @ wqkv[2 * e:].T + bqkv[2 * e:]).view(B, T, heads, d)
    s = torch.einsum("bhi,bjhi->bhj", q, k) / math.sqrt(d)
    p = torch.softmax(s, dim=-1)
    a = torch.einsum("bhj,bjhi->bhi", p, v).reshape(B, e)
    return h1, q2, p, a


@pytest.mark.parametrize("B,T,e,heads", [(2, 1, 8, 1), (3, 5, 8, 2), (2, 9, 24, 3)])
def test_weights_move_to_the_query_side(B, T, e, heads):
    t = _inputs(B, T, e, heads, seed=T)
    leaves = {k: t[k].clone().requires_grad_() for k in ("x", "g1", "b1", "wqkv", "bqkv")}
    h1, q, p, a = original(heads=heads, **leaves)
    h1.retain_grad(), q.retain_grad()
    ((a * t["da"]).sum() + (leaves["x"][:, 0] * t["dx1"]).sum()).backward()
    d, scale = e // heads, 1 / math.sqrt(e // heads)
    wq, wk, wv = (leaves["wqkv"].detach()[i * e:(i + 1) * e] for i in range(3))
    bk, bv = leaves["bqkv"].detach()[e:2 * e], leaves["bqkv"].detach()[2 * e:]
    dh1_ref, dq_ref = h1.grad, q.grad
    h1, q, p, a = h1.detach(), q.detach(), p.detach(), a.detach()
    close = lambda u, v: torch.testing.assert_close(u, v, rtol=1e-10, atol=1e-11)
    # forward
    qh = q.view(B, heads, d)
    qt = torch.einsum("bhi,hic->bhc", qh, wk.view(heads, d, e))                    # Wk_h^T q
    c = torch.einsum("bhi,hi->bh", qh, bk.view(heads, d))
    s = scale * (torch.einsum("bhc,bjc->bhj", qt, h1) + c[..., None])
    close(torch.softmax(s, -1), p)
    m = torch.einsum("bhj,bjc->bhc", p, h1)
    close((torch.einsum("hic,bhc->bhi", wv.view(heads, d, e), m) + bv.view(heads, d)).reshape(B, e), a)
    # backward
    dah = t["da"].view(B, heads, d)
    dm = torch.einsum("bhi,hic->bhc", dah, wv.view(heads, d, e))
    close(torch.einsum("bhi,bhc->hic", dah, m).reshape(e, e), leaves["wqkv"].grad[2 * e:])
    close(dah.sum(0).reshape(e), leaves["bqkv"].grad[2 * e:])
    dp = torch.einsum("bhc,bjc->bhj", dm, h1)
    delta = torch.einsum("bhc,bhc->bh", dm, m)                                     # = sum_j p dp
    close(delta, (p * dp).sum(-1))
    ds = p * (dp - delta[..., None])
    dqt = scale * torch.einsum("bhj,bjc->bhc", ds, h1)
    dq = torch.einsum("hic,bhc->bhi", wk.view(heads, d, e), dqt).reshape(B, e)
    close(dq, dq_ref)
    close(torch.einsum("bhi,bhc->hic", qh, dqt).reshape(e, e), leaves["wqkv"].grad[e:2 * e])
    close(torch.zeros(e, dtype=torch.float64), leaves["bqkv"].grad[e:2 * e])        # dbk = scale sum_b (sum_j ds) q = 0
    assert float(ds.sum(-1).abs().max()) < 1e-12
    dh1 = torch.einsum("bhj,bhc->bjc", p, dm) + scale * torch.einsum("bhj,bhc->bjc", ds, qt)
    dh1[:, 0] += dq @ wq                                                           # the query branch: class rows only
    close(dh1, dh1_ref)
    # LayerNorm backward is linear in dh1: the query's part may be taken over the class rows alone and added (+ the skip)
    xl = leaves["x"].detach().clone().requires_grad_()
    gl, bl = (leaves[k].detach().clone().requires_grad_() for k in ("g1", "b1"))
    hl = torch.nn.functional.layer_norm(xl, (e,), gl, bl, 1e-6)
    part = dh1_ref.clone()
    part[:, 0] -= dq @ wq
    dx_a, dg_a, db_a = torch.autograd.grad(hl, (xl, gl, bl), part, retain_graph=True)
    only = torch.zeros_like(part)
    only[:, 0] = dq @ wq
    dx_b, dg_b, db_b = torch.autograd.grad(hl, (xl, gl, bl), only)
    skip = torch.zeros_like(dx_a)
    skip[:, 0] = t["dx1"]
    close(dx_a + dx_b + skip, leaves["x"].grad)
    close(dg_a + dg_b, leaves["g1"].grad)
    close(db_a + db_b, leaves["b1"].grad)


def test_diagonal_block_views():
    """functional._head_diag and the weight-gradient view pick the blocks the per-head products would write."""
    from multimodal_supernovae_amd import functional as F
    B, heads, d = 3, 4, 2
    e = heads * d
    full = torch.arange(B * heads * e, dtype=torch.float64).view(B * heads, e)
    got = F._head_diag(full, B, heads, d)
    for b in range(B):
        for h in range(heads):
            assert torch.equal(got[b, h], full[b * heads + h, h * d:(h + 1) * d])
    w = torch.arange(e * heads * e, dtype=torch.float64).view(e, heads * e)
    blocks = w.as_strided((heads, d, e), (d * heads * e + e, heads * e, 1))
    for h in range(heads):
        assert torch.equal(blocks[h], w[h * d:(h + 1) * d, h * e:(h + 1) * e])


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """Shape, alignment and pointer conditions are checked on the host: exercised here without a GPU."""
    import ctypes
    from multimodal_supernovae_amd import _lib
    lib = _lib.lib()
    ok = ctypes.c_void_p(4096)           # never dereferenced: every call below is refused by its checks
    odd = ctypes.c_void_p(4100)
    assert lib.msn_cls_pool_supported(65, 384, 6) == 1 and lib.msn_cls_pool_supported(256, 512, 8) == 1
    for T, e, heads in [(0, 384, 6), (257, 384, 6), (65, 516, 1), (65, 386, 1), (65, 384, 9), (65, 384, 5), (197, 768, 12)]:
        assert lib.msn_cls_pool_supported(T, e, heads) == 0, (T, e, heads)
    fwd = lambda x=ok, ldx=384, T=65, qt=ok, q=ok, bk=ok: lib.msn_cls_pool_fwd(x, ldx, 2, T, 384, 6, ok, ok, 1e-6, qt, q, 384, bk, 0.125,
                                                                               ok, ok, ok, ok, None)
    assert fwd(x=None) == 1 and b"empty operand" in lib.msn_last_error()
    assert fwd(T=300) == 1 and b"unsupported shape" in lib.msn_last_error()
    assert fwd(ldx=380) == 1 and fwd(x=odd) == 1 and b"16-byte aligned" in lib.msn_last_error()
    assert fwd(bk=None) == 1 and b"go together" in lib.msn_last_error()
    rc = lib.msn_cls_pool_dqt(ok, 384, 2, 65, 384, 6, ok, ok, ok, ok, ok, ok, None, 0.125, ok, ok, None)
    assert rc == 1 and b"empty operand" in lib.msn_last_error()
    bwd = lambda ws=ok, nb=1 << 20, dcls=ok, ldcls=384, lddx=384: lib.msn_cls_pool_bwd(
        ok, 384, 2, 65, 384, 6, ok, ok, ok, ok, ok, ok, ok, ok, 0.125, dcls, ldcls, ok, 384, ok, lddx, ok, ok, ws, nb, None)
    assert lib.msn_cls_pool_bwd_workspace_bytes(2, 384) == 2 * 2 * 384 * 4 and lib.msn_cls_pool_bwd_workspace_bytes(0, 384) == 0
    assert bwd(nb=100) == 1 and b"workspace too small" in lib.msn_last_error()
    assert bwd(ws=None) == 1
    assert bwd(ldcls=382) == 1 and bwd(dcls=odd) == 1 and b"class-row operand" in lib.msn_last_error()
    assert bwd(lddx=100) == 1 and b"16-byte aligned" in lib.msn_last_error()
