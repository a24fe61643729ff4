"""Class-token attention of the ViT's last block without keys | values (csrc/cls_pool.hip, functional._cls_pool_forward /
_cls_pool_backward) against the original formulation in fp64 on the CPU (LayerNorm -> key | value Linear -> one-query softmax
attention, autograd for the gradients).

Gate: maximum and RMS error of the new route <= 1.5 x the error of the route it replaces (the kernels functional._PreNormLastBlock
runs with CLS_POOL = False: msn_layernorm_fwd, msn_sgemm, msn_cls_attention_*, msn_wgrad_bias, msn_layernorm_bwd) on the same
inputs -- the project's convention for a re-ordered fp32 computation (tests/test_pgemm_gpu.py).  m = sum_j p h1[b, j] has no
counterpart in that route; its yardstick is the same sum formed in fp32 from that route's probabilities and LayerNorm output.
dqt is checked through dq = Wk_h dqt and dWk = sum_b q (x) dqt, both linear in it.  The key bias's gradient is exactly 0: the
absolute error of both routes is normalised by sum |ds| |q|.  Every case pools the errors of eight independent inputs of its shape
(_case): one draw of the small shapes has as few as 15 values of a quantity, each a few units in the last place off."""
import functools
import math

import pytest
import torch

from test_cls_pool_algebra_cpu import original

pytestmark = pytest.mark.gpu
EPS = 1e-6
GATE = 1.5

#        name               T    e   heads B  gain on the query
CASES = [("one_token", 1, 64, 1, 2, 1.0),             # p = 1 and ds = 0
         ("short", 5, 64, 1, 3, 1.0),
         ("16n_plus_1", 17, 128, 2, 3, 1.0),
         ("odd_length", 33, 128, 2, 1, 1.0),
         ("headline_rows", 65, 384, 6, 2, 1.0),
         ("peaked_softmax", 65, 384, 6, 2, 8.0)]


def _inputs(T, e, heads, B, gain, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    wqkv, bqkv = r(3 * e, e) / math.sqrt(e), 0.1 * r(3 * e)
    wqkv[:e] *= gain
    bqkv[:e] *= gain
    return dict(x=r(B, T, e), g1=1 + 0.2 * r(e), b1=0.1 * r(e), wqkv=wqkv, bqkv=bqkv, da=r(B, e), dx1=r(B, e))


def _reference(t, heads):
    """Every checked quantity of the original formulation, fp64 on the CPU."""
    d64 = {k: v.double() for k, v in t.items()}
    leaves = {k: d64[k].clone().requires_grad_() for k in ("x", "g1", "b1", "wqkv", "bqkv")}
    h1, q, p, a = original(heads=heads, eps=EPS, **leaves)
    q.retain_grad()
    ((a * d64["da"]).sum() + (leaves["x"][:, 0] * d64["dx1"]).sum()).backward()
    B, T, e = d64["x"].shape
    dw, db = leaves["wqkv"].grad, leaves["bqkv"].grad
    # the normaliser of the key bias's gradient: sum_b sum_j |ds| |q| per column
    dv = torch.einsum("bhi,bjhi->bhj", d64["da"].view(B, heads, -1),
                      (h1.detach() @ d64["wqkv"][2 * e:].T + d64["bqkv"][2 * e:]).view(B, T, heads, -1))
    ds = p.detach() * (dv - (p.detach() * dv).sum(-1, keepdim=True))
    dbk_scale = (ds.abs().sum(-1)[..., None] * q.detach().view(B, heads, -1).abs()).sum(0).reshape(e) / math.sqrt(e // heads)
    return dict(m=torch.einsum("bhj,bjc->bhc", p, h1).detach(), a=a.detach(), p=p.detach(), dx=leaves["x"].grad,
                dg1=leaves["g1"].grad, db1=leaves["b1"].grad, dq=q.grad, dWk=dw[e:2 * e], dWv=dw[2 * e:], dbv=db[2 * e:],
                dWq=dw[:e], dbq=db[:e], dbk=torch.zeros(e, dtype=torch.float64)), dbk_scale


def _new_route(c, heads):
    from multimodal_supernovae_amd import functional as F
    e = c["x"].shape[2]
    a2, pooled = F._cls_pool_forward(c["x"], heads, EPS, 1 / math.sqrt(e // heads), c["g1"], c["b1"], c["wqkv"], c["bqkv"])
    dx, dg1, db1, dw, db, (dm, dqt, dq) = F._cls_pool_backward(c["x"], heads, 1 / math.sqrt(e // heads), c["g1"], c["b1"], c["wqkv"],
                                                                pooled, c["da"], c["dx1"])
    return dict(m=pooled[6], a=a2, p=pooled[5], dx=dx, dg1=dg1, db1=db1, dq=dq, dWk=dw[e:2 * e], dWv=dw[2 * e:], dbv=db[2 * e:],
                dWq=dw[:e], dbq=db[:e], dbk=db[e:2 * e], dqt=dqt)


def _old_route(c, heads):
    """What _PreNormLastBlock runs between its input and the attention rows with CLS_POOL = False, launch for launch."""
    from multimodal_supernovae_amd import functional as F
    from multimodal_supernovae_amd import ops
    x, wqkv, bqkv = c["x"], c["wqkv"], c["bqkv"]
    B, T, e = x.shape
    scale = 1 / math.sqrt(e // heads)
    x2 = x.view(B * T, e)
    h1, m1, r1 = ops.layernorm_fwd(x2, c["g1"], c["b1"], EPS)
    kv = ops.sgemm(h1, wqkv[e:], ops.OP_N, ops.OP_T, bias=bqkv[e:])
    h1c = h1.view(B, T, e)[:, 0, :]
    q = ops.sgemm(h1c, wqkv[:e], ops.OP_N, ops.OP_T, bias=bqkv[:e])
    assert ops.cls_attention_supported(T, e // heads)
    a2, p = ops.cls_attention_fwd(q, kv, T, heads, scale)
    dq, dkv = ops.cls_attention_bwd(q, kv, T, heads, scale, a2, p, c["da"])

    def kv_backward(dwkv, dbkv):
        ops.wgrad_bias(dkv, h1, out=(dwkv, dbkv))
        return ops.sgemm(dkv, wqkv[e:], ops.OP_N, ops.OP_N)

    dx, dg1, db1, dw, db = F._cls_rows_backward_ln1(B, T, e, dq, h1c, kv_backward, wqkv, x2, m1, r1, c["g1"], c["dx1"])
    return dict(m=torch.bmm(p, h1.view(B, T, e)), a=a2, p=p, dx=dx, dg1=dg1, db1=db1, dq=dq, dWk=dw[e:2 * e], dWv=dw[2 * e:],
                dbv=db[2 * e:], dWq=dw[:e], dbq=db[:e], dbk=db[e:2 * e])


QUANTITIES = ("m", "a", "p", "dx", "dg1", "db1", "dq", "dWk", "dWv", "dbv", "dWq", "dbq", "dbk")
DRAWS = 8


@functools.lru_cache(maxsize=None)
def _case(name):
    """Per quantity the absolute errors against fp64 of (new route, old route), pooled over DRAWS independent inputs of the case's
    shape, and the new route's results of the first draw; computed once and shared, nothing changes them.  Pooled, because the
    errors are a few units in the last place and a single draw of the small shapes has as few as 15 values of a quantity: the
    ratio of two such maxima says nothing."""
    _, T, e, heads, B, gain = next(c for c in CASES if c[0] == name)
    new_err, old_err = {k: [] for k in QUANTITIES}, {k: [] for k in QUANTITIES}
    for draw in range(DRAWS):
        t = _inputs(T, e, heads, B, gain, seed=1000 * draw + T + e)
        ref, dbk_scale = _reference(t, heads)
        c = {k: v.cuda() for k, v in t.items()}
        new, old = _new_route(c, heads), _old_route(c, heads)
        for k in QUANTITIES:
            norm = dbk_scale.clamp_min(1e-300) if k == "dbk" else 1.0
            new_err[k].append(((new[k].detach().double().cpu().reshape(ref[k].shape) - ref[k]).abs() / norm).flatten())
            old_err[k].append(((old[k].detach().double().cpu().reshape(ref[k].shape) - ref[k]).abs() / norm).flatten())
        if draw == 0:
            first = {k: v.detach().cpu() for k, v in new.items()}
    return {k: (torch.cat(new_err[k]), torch.cat(old_err[k])) for k in QUANTITIES}, first


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_error_against_fp64_within_the_gate(name):
    errors, _ = _case(name)
    failed = []
    for k in QUANTITIES:
        n, o = errors[k]
        nmax, nrms, omax, orms = float(n.max()), float(n.square().mean().sqrt()), float(o.max()), float(o.square().mean().sqrt())
        print(f"{name:15s} {k:4s} max {nmax:.3e} / {omax:.3e} = {nmax / omax if omax else float('nan'):6.3f}   "
              f"rms {nrms:.3e} / {orms:.3e} = {nrms / orms if orms else float('nan'):6.3f}")
        if nmax > GATE * omax or nrms > GATE * orms:
            failed.append((k, nmax, omax, nrms, orms))
    assert not failed, failed


def test_key_bias_gradient_is_exactly_zero():
    assert all(float(_case(c[0])[0]["dbk"][0].max()) == 0.0 for c in CASES)


def test_one_token_has_unit_probability():
    new = _case("one_token")[1]
    assert torch.equal(new["p"], torch.ones_like(new["p"]))


def test_two_runs_are_bit_identical():
    _, T, e, heads, B, gain = CASES[4]
    c = {k: v.cuda() for k, v in _inputs(T, e, heads, B, gain, seed=5).items()}
    one, two = _new_route(c, heads), _new_route(c, heads)
    for k in one:
        assert torch.equal(one[k], two[k]), k


def _node(x, heads, params, dy, on):
    from multimodal_supernovae_amd import functional as F
    old = F.CLS_POOL
    F.CLS_POOL = on
    try:
        leaves = [x.clone().requires_grad_()] + [p.clone().requires_grad_() for p in params]
        out = F.pre_norm_last_block(leaves[0], heads, leaves[1:], eps=EPS)
        out.backward(dy)
        return [out.detach()] + [t.grad for t in leaves]
    finally:
        F.CLS_POOL = old


def test_past_the_support_bound_the_node_is_the_fallback_bit_for_bit():
    from multimodal_supernovae_amd import ops
    T, e, heads, B = 257, 64, 1, 2                       # one token past the bound
    assert ops.cls_pool_supported(256, e, heads) and not ops.cls_pool_supported(T, e, heads)
    assert not ops.cls_pool_supported(65, 768, 12) and not ops.cls_pool_supported(65, 516, 1)
    g = torch.Generator().manual_seed(9)
    r = lambda *s: torch.randn(*s, generator=g).cuda()
    params = [1 + 0.2 * r(e), 0.1 * r(e), r(3 * e, e) / 8, 0.1 * r(3 * e), r(e, e) / 8, 0.1 * r(e), 1 + 0.2 * r(e), 0.1 * r(e),
              r(4 * e, e) / 8, 0.1 * r(4 * e), r(e, 4 * e) / 16, 0.1 * r(e)]
    x, dy = r(B, T, e), r(B, e)
    for u, v in zip(_node(x, heads, params, dy, True), _node(x, heads, params, dy, False)):
        assert torch.equal(u, v)


def test_vit_s8_switch_on_against_switch_off():
    """Loss to 1e-5 and every parameter gradient to 1e-3 of its scale: the tolerance tests/test_headline_gpu.py sets between its
    two arithmetic routes of the same step."""
    from multimodal_supernovae_amd import encoders
    from multimodal_supernovae_amd import functional as F
    torch.manual_seed(4)
    model = encoders.vit_s8().cuda()
    img = torch.rand(6, 3, 64, 64, generator=torch.Generator().manual_seed(2)).cuda()
    res = {}
    old = F.CLS_POOL
    try:
        for on in (True, False):
            F.CLS_POOL = on
            model.zero_grad(set_to_none=True)
            loss = model(img).square().mean()
            loss.backward()
            res[on] = (float(loss.detach()), {k: p.grad.detach().clone() for k, p in model.named_parameters()})
    finally:
        F.CLS_POOL = old
    (l1, g1), (l0, g0) = res[True], res[False]
    assert abs(l1 - l0) <= 1e-5 * abs(l0), (l1, l0)
    worst = max((float((g1[k] - g0[k]).abs().max()) / (float(g0[k].abs().max()) + 1e-12), k) for k in g0)
    print("loss", l1, l0, "worst gradient difference", worst)
    assert worst[0] < 1e-3, worst
