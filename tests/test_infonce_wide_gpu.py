"""The contrastive losses and the retrieval ranks at embedding widths 288 - 1024 (multiples of 32: csrc/infonce_wide.hip) through
the C-ABI, against the oracle in fp64: softmax and sigmoid loss with their gradients, unequal row counts, row sharding emulated on
one GPU, strided and misaligned column views, ranks and AUC, determinism, and the width / workspace contract.
Tolerance: 1e-3 relative, as tests/test_infonce_gpu.py; ranks follow the margin rule of tests/infonce_refs.py (rank_rule)."""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
RTOL = 1e-3
CONTRACT = "256 < D <= 1024 with D a multiple of 32"


def _unit(n, d, seed):
    x = torch.randn(n, d, generator=torch.Generator().manual_seed(seed))
    return x / x.norm(dim=-1, keepdim=True)


def _run_hip(e1, e2, ls, lb):
    from multimodal_supernovae_amd.loss import clip_loss
    a, b = e1.cuda().requires_grad_(), e2.cuda().requires_grad_()
    s, c = ls.cuda().requires_grad_(), lb.cuda().requires_grad_()
    loss = clip_loss(a, b, s, c)
    loss.backward()
    return loss.detach().cpu(), a.grad.cpu(), b.grad.cpu(), s.grad.cpu(), c.grad.cpu()


def _run_oracle(e1, e2, ls, lb):
    from oracle.loss import clip_loss
    a, b = e1.double().requires_grad_(), e2.double().requires_grad_()
    s, c = ls.double().requires_grad_(), lb.double().requires_grad_()
    loss = clip_loss(a, b, s, c)
    loss.backward()
    return loss.detach(), a.grad, b.grad, s.grad, c.grad


def _compare(hip, ref):
    loss, d1, d2, ds, db = hip
    rl, r1, r2, rs, rb = ref
    assert abs(float(loss) - float(rl)) <= RTOL * abs(float(rl)) + 1e-6
    gscale = float(r1.abs().max())
    torch.testing.assert_close(d1.double(), r1, rtol=RTOL, atol=RTOL * gscale)
    torch.testing.assert_close(d2.double(), r2, rtol=RTOL, atol=RTOL * gscale)
    assert abs(float(ds) - float(rs)) <= RTOL * abs(float(rs)) + 1e-5
    assert abs(float(db)) <= 1e-4, "logit_bias is gradient-free under the softmax loss"


@pytest.mark.parametrize("n,d", [(1, 512), (33, 288), (129, 320), (256, 384), (1000, 512), (1024, 768), (4096, 1024)])
@pytest.mark.parametrize("log_scale,bias", [(math.log(10.0), -10.0), (math.log(31.0), 0.5)])
def test_against_oracle(n, d, log_scale, bias):
    e1, e2 = _unit(n, d, 100 + n), _unit(n, d, 200 + n)
    ls, lb = torch.tensor(log_scale), torch.tensor(bias)
    _compare(_run_hip(e1, e2, ls, lb), _run_oracle(e1, e2, ls, lb))


@pytest.mark.parametrize("d", [512, 1024])
@pytest.mark.parametrize("n1,n2", [(300, 170), (97, 640)])
def test_unequal_row_counts(d, n1, n2):
    e1, e2 = _unit(n1, d, 11 + d), _unit(n2, d, 12 + d)
    ls, lb = torch.tensor(math.log(19.5)), torch.tensor(-3.0)
    _compare(_run_hip(e1, e2, ls, lb), _run_oracle(e1, e2, ls, lb))


@pytest.mark.parametrize("d", [512, 1024])
@pytest.mark.parametrize("world", [2, 4, 8])
def test_row_sharded_kernels_sum_to_single_process(world, d):
    """`world` ranks emulated on one GPU, as tests/test_infonce_gpu.py does at D = 128."""
    from multimodal_supernovae_amd.loss import HipPairKernels as K
    from oracle.sharded import OraclePairKernels as O
    b = 96
    n = b * world
    e1, e2 = _unit(n, d, 31).cuda(), _unit(n, d, 32).cuda()
    ls, lb = torch.tensor(math.log(19.5)).cuda(), torch.tensor(-10.0).cuda()
    one = torch.tensor(1.0).cuda()
    lr, lc, total = K.forward(e1, e2, e1, e2, 0, ls, lb)
    g1, g2, gs, gb = K.backward(e1, e2, e1, e2, 0, ls, lb, lr, lc, one)
    parts = [K.forward(e1[r * b:(r + 1) * b], e2[r * b:(r + 1) * b], e1, e2, r * b, ls, lb) for r in range(world)]
    lr_all = torch.cat([p[0] for p in parts])
    lc_all = torch.cat([p[1] for p in parts])
    torch.testing.assert_close(lr_all, lr, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(lc_all, lc, rtol=1e-5, atol=1e-5)
    assert abs(float(sum(p[2] for p in parts)) - float(total)) < 1e-5
    ds_sum = 0.0
    for r in range(world):
        sl = slice(r * b, (r + 1) * b)
        d1, d2, ds, db = K.backward(e1[sl], e2[sl], e1, e2, r * b, ls, lb, lr_all, lc_all, one)
        torch.testing.assert_close(d1, g1[sl], rtol=1e-4, atol=1e-7)
        torch.testing.assert_close(d2, g2[sl], rtol=1e-4, atol=1e-7)
        o1, o2, os_, ob = O.backward(e1[sl], e2[sl], e1, e2, r * b, ls, lb, lr_all, lc_all, one)
        torch.testing.assert_close(d1, o1, rtol=RTOL, atol=1e-6)
        torch.testing.assert_close(d2, o2, rtol=RTOL, atol=1e-6)
        ds_sum += float(ds)
    assert abs(ds_sum - float(gs)) <= 1e-4 * abs(float(gs)) + 1e-6


def test_strided_and_misaligned_views():
    """Column slices of a packed (n, 3 * 512) buffer (the all-gather layout); the third block starts one float off 16 bytes.
    Row-strided views go straight into the C-ABI and must give the bits of contiguous copies."""
    from multimodal_supernovae_amd.loss import HipPairKernels as K
    d = 512
    wide = torch.cat([_unit(150, d, 1), _unit(150, d, 2), _unit(150, d + 1, 3)], dim=1).cuda()
    ls, lb = torch.tensor(2.5).cuda(), torch.tensor(-1.0).cuda()
    one = torch.tensor(1.0).cuda()
    for c1, c2 in ((0, d), (d, 2 * d + 1)):
        e1, e2 = wide[:, c1:c1 + d], wide[:, c2:c2 + d]
        f1, f2 = e1.contiguous(), e2.contiguous()
        lr, lc, a = K.forward(e1, e2, e1, e2, 0, ls, lb)
        lr2, lc2, b = K.forward(f1, f2, f1, f2, 0, ls, lb)
        assert float(a) == float(b) and torch.equal(lr, lr2) and torch.equal(lc, lc2)
        ga = K.backward(e1, e2, e1, e2, 0, ls, lb, lr, lc, one)
        gb = K.backward(f1, f2, f1, f2, 0, ls, lb, lr, lc, one)
        for x, y in zip(ga, gb):
            assert torch.equal(x, y)


@pytest.mark.parametrize("n,d", [(70, 288), (256, 512), (1024, 1024)])
def test_sigmoid_loss_against_oracle(n, d):
    from multimodal_supernovae_amd.loss import sigmoid_loss
    from oracle.loss import sigmoid_loss as ref_fn
    e1, e2 = _unit(n, d, 300 + n), _unit(n, d, 400 + n)
    ls, lb = torch.tensor(math.log(5.0)), torch.tensor(-3.0)
    a, b = e1.cuda().requires_grad_(), e2.cuda().requires_grad_()
    s, c = ls.cuda().requires_grad_(), lb.cuda().requires_grad_()
    loss = sigmoid_loss(a, b, s, c)
    loss.backward()
    ra, rb = e1.double().requires_grad_(), e2.double().requires_grad_()
    rs, rc = ls.double().requires_grad_(), lb.double().requires_grad_()
    ref = ref_fn(ra, rb, rs, rc)
    ref.backward()
    assert abs(float(loss.detach()) - float(ref.detach())) <= RTOL * abs(float(ref.detach()))
    for got, want in ((a.grad, ra.grad), (b.grad, rb.grad)):
        torch.testing.assert_close(got.cpu().double(), want, rtol=RTOL, atol=RTOL * float(want.abs().max()))
    assert abs(float(s.grad) - float(rs.grad)) <= RTOL * abs(float(rs.grad)) + 1e-6
    assert abs(float(c.grad) - float(rc.grad)) <= RTOL * abs(float(rc.grad)) + 1e-6


@pytest.mark.parametrize("d", [320, 512, 1024])
@pytest.mark.parametrize("n", [33, 1000, 4096])
def test_retrieval_ranks_against_oracle(n, d):
    from multimodal_supernovae_amd.utils import retrieval_ranks
    from infonce_refs import rank_rule
    from oracle.clip import roc_data
    g = torch.Generator().manual_seed(n + d)
    e1 = torch.randn(n, d, generator=g)
    e2 = e1 + 2.0 * torch.randn(n, d, generator=g)
    got = retrieval_ranks(e1.cuda(), e2.cuda()).cpu()
    _, _, ref = roc_data(e1.double(), e2.double())
    # equal wherever the fp64 margin of the partner's score exceeds the derived score bound; the rows left out are counted
    wrong, undecided, rows = rank_rule(got, e1, e2, normalised=True, ref=ref)
    assert wrong == 0 and undecided <= 0.01 * rows, (wrong, undecided)


@pytest.mark.parametrize("d", [288, 768])
def test_auc_against_oracle(d):
    from multimodal_supernovae_amd.utils import get_AUC
    from oracle.clip import auc
    g = torch.Generator().manual_seed(d)
    e1 = torch.randn(500, d, generator=g)
    e2 = e1 + 3.0 * torch.randn(500, d, generator=g)
    assert abs(get_AUC(e1.cuda(), e2.cuda()) - auc(e1.double(), e2.double())) < 1e-3


def test_deterministic_with_several_key_splits():
    from multimodal_supernovae_amd import _lib
    from multimodal_supernovae_amd.loss import HipPairKernels as K
    n, d = 1024, 512
    assert _lib.lib().msn_infonce_workspace_bytes(n, n, n, n, d) > 2 * n * d * 4      # the dQ slab: more than one split
    e1, e2 = _unit(n, d, 41).cuda(), _unit(n, d, 42).cuda()
    ls, lb, one = torch.tensor(math.log(19.5)).cuda(), torch.tensor(-10.0).cuda(), torch.tensor(1.0).cuda()
    f1, f2 = K.forward(e1, e2, e1, e2, 0, ls, lb), K.forward(e1, e2, e1, e2, 0, ls, lb)
    for x, y in zip(f1, f2):
        assert torch.equal(x, y)
    b1, b2 = (K.backward(e1, e2, e1, e2, 0, ls, lb, f1[0], f1[1], one) for _ in range(2))
    for x, y in zip(b1, b2):
        assert torch.equal(x, y)


def _entry_points(L, n, d, ws_bytes=None):
    """All five entry points at (n rows, width d) on single-process arguments; each returns (rc, last error text)."""
    dev = torch.device("cuda")
    e1, e2 = _unit(n, d, 1).to(dev), _unit(n, d, 2).to(dev)
    nb = L.msn_infonce_workspace_bytes(n, n, n, n, d) if ws_bytes is None else ws_bytes
    ws = torch.empty(max(nb, 16) // 4 + 1, dtype=torch.float32, device=dev)
    ls, lb, one = (torch.tensor(v, device=dev) for v in (1.0, 0.0, 1.0))
    lr, lc = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    loss, dsb = torch.empty((), device=dev), torch.empty(2, device=dev)
    g1, g2 = torch.empty(n, d, device=dev), torch.empty(n, d, device=dev)
    rank = torch.empty(n, dtype=torch.int32, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    from multimodal_supernovae_amd._lib import stream_ptr
    st = stream_ptr()
    calls = {
        "msn_infonce_fwd": lambda: L.msn_infonce_fwd(p(e1), d, n, p(e2), d, n, p(e1), d, n, p(e2), d, n, d, 0, p(ls), p(lb),
                                                     p(lr), p(lc), p(loss), p(ws), nb, st),
        "msn_infonce_bwd": lambda: L.msn_infonce_bwd(p(e1), d, n, p(e2), d, n, p(e1), d, n, p(e2), d, n, d, 0, p(ls), p(lb),
                                                     p(lr), p(lc), p(one), p(g1), d, p(g2), d, p(dsb), p(ws), nb, st),
        "msn_sigmoid_loss_fwd": lambda: L.msn_sigmoid_loss_fwd(p(e1), d, p(e2), d, n, p(e1), d, p(e2), d, n, d, 0, p(ls), p(lb),
                                                               p(loss), p(ws), nb, st),
        "msn_sigmoid_loss_bwd": lambda: L.msn_sigmoid_loss_bwd(p(e1), d, p(e2), d, n, p(e1), d, p(e2), d, n, d, 0, p(ls), p(lb),
                                                               p(one), p(g1), d, p(g2), d, p(dsb), p(ws), nb, st),
        "msn_retrieval_rank": lambda: L.msn_retrieval_rank(p(e1), d, p(e2), d, n, d, p(rank), p(ws), nb, st),
    }
    out = {}
    for name, call in calls.items():
        rc = call()
        out[name] = (rc, L.msn_last_error().decode() if rc else "")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("d", [260, 1000, 1056])
def test_unsupported_widths_are_refused_with_the_contract(d):
    from multimodal_supernovae_amd._lib import lib
    for name, (rc, msg) in _entry_points(lib(), 40, d).items():
        assert rc != 0, f"{name} accepted D={d}"
        assert f"D={d}" in msg and CONTRACT in msg, (name, msg)


def test_workspace_formula_covers_the_wide_path():
    from multimodal_supernovae_amd._lib import lib
    L = lib()
    n, d = 1000, 512
    nb = L.msn_infonce_workspace_bytes(n, n, n, n, d)
    for name, (rc, msg) in _entry_points(L, n, d, nb).items():
        assert rc == 0, (name, msg)
    for name, (rc, msg) in _entry_points(L, n, d, nb - 1).items():
        assert rc != 0 and "workspace" in msg, (name, msg)
