"""tests/attention_bf16_refs.py against itself, on the CPU: the emulation of the kernels' arithmetic stays inside every derived
bound (gate 1, no slack) and reproduces the exact expectations of the structured families, and every injected defect -- a key left
out or counted twice, a query left out of the dK/dV pass, two V rows swapped, a padding key left unmasked -- makes the comparison
the GPU tests run fail."""
import functools

import pytest
import torch

import attention_bf16_refs as R

B, H = 1, 2
LENGTHS = (1, 33, 197, 256)


@functools.lru_cache(maxsize=None)
def case(family, T):
    """Inputs, the fp64 references and the host-made operands of the backward (out = bf16(Oref), lse = fp32(lse_ref))."""
    inp = R.make_inputs(family, B, H, T)
    fref = R.forward_ref(inp["qkv"], B, T, H)
    out, lse = fref["out"].to(R.BF16), fref["lse"].to(R.F32)
    bref = R.backward_ref(inp["qkv"], out, inp["dout"], lse, B, T, H)
    return inp, fref, out, lse, bref


def run_forward(family, T, defect=None):
    inp, fref, _, _, _ = case(family, T)
    out, lse = R.emulate_forward(inp["qkv"], B, T, H, defect=defect)
    return R.forward_failures(family, inp, fref, out, lse, B, T, H)


def run_backward(family, T, defect=None):
    inp, _, out, lse, bref = case(family, T)
    dqkv = R.emulate_backward(inp["qkv"], out, inp["dout"], lse, B, T, H, defect=defect)
    return R.backward_failures(family, inp, bref, dqkv, B, T, H)


def positions(T):
    return sorted({0, T // 2, T - 1})


@pytest.mark.parametrize("T", LENGTHS)
@pytest.mark.parametrize("family", R.FAMILIES)
def test_emulation_passes_the_comparison(family, T):
    """Bounds (ratio <= 1), lse, and the exact expectations of the uniform and one-hot families."""
    bad, ratios = run_forward(family, T)
    assert not bad, (bad, ratios)
    bad, ratios = run_backward(family, T)
    assert not bad, (bad, ratios)


def test_references_against_autograd():
    """forward_ref / backward_ref are softmax attention and its gradient (autograd in fp64, the forward's own out and lse)."""
    T = 33
    inp = R.make_inputs("flat", B, H, T)
    x = inp["qkv"].double().requires_grad_()
    q, k, v = R.split_qkv(x, B, T, H)
    o = R.rows_of(torch.softmax(q @ k.transpose(-1, -2) * R.SCALE, -1) @ v)
    o.backward(inp["dout"].double())
    fref = R.forward_ref(inp["qkv"], B, T, H)
    torch.testing.assert_close(fref["out"], o.detach(), rtol=1e-12, atol=1e-12)
    bref = R.backward_ref(inp["qkv"], fref["out"], inp["dout"], fref["lse"], B, T, H)
    torch.testing.assert_close(bref["dqkv"], x.grad, rtol=1e-10, atol=1e-12)


def test_onehot_family_is_one_hot():
    """Every off-target probability is below e^-40, the permutation crosses tiles, and the expectations index as documented."""
    T = 197
    inp, fref, _, _, _ = case("onehot", T)
    q, k, v = (t.double() for t in R.split_qkv(inp["qkv"], B, T, H))
    p = torch.softmax(q @ k.transpose(-1, -2) * R.SCALE, -1)
    hit = torch.zeros_like(p).scatter(-1, inp["perm"][..., None], 1.0)
    assert float((p * (1 - hit)).max()) < 2.0 ** -57 and float((p * hit).sum(-1).min()) > 1 - 1e-12      # e^-40 = 2^-57.7
    for bh in inp["perm"].reshape(-1, T):
        assert sorted(bh.tolist()) == list(range(T))
        assert (bh[1:] // 16 != bh[:-1] // 16).all()
    want_o, want_dv = R.onehot_expect(inp, B, T, H)
    i, pi = 5, int(inp["perm"][0, 1, 5])
    assert torch.equal(want_o[i, 64:128], inp["qkv"][pi, 2 * 128 + 64:]) and torch.equal(want_dv[pi, 64:128], inp["dout"][i, 64:128])


# the structured family in which a defect cannot hide, and why the others may miss it:
#   a swap of V rows leaves the column sums of the uniform family unchanged; a doubled one-hot target still gives o / l = v
MATCHING = {"drop_key": ("uniform", "onehot"), "double_key": ("uniform",), "swap_v": ("onehot",), "unmask_pad": ("uniform",)}


@pytest.mark.parametrize("T", LENGTHS)
@pytest.mark.parametrize("kind", ["drop_key", "double_key", "swap_v"])
def test_forward_defects_are_caught(kind, T):
    for at in positions(T):
        for family in ("peaked",) + MATCHING[kind]:
            bad, ratios = run_forward(family, T, (kind, at))
            assert bad, (family, kind, at, ratios)


@pytest.mark.parametrize("T", [t for t in LENGTHS if t % R.BLOCK])
def test_unmasked_padding_key_is_caught(T):
    """A zero key past T scores 0 and takes the weight e^-lse.  The uniform family (lse = log T) always shows it.  In the peaked
    family lse is about 15 from 33 keys on: the weight is below 1e-6, less than the rounding the bounds allow, so no comparison
    can show it there; at T = 1 half of the queries score below 0 and it shows."""
    bad, ratios = run_forward("uniform", T, ("unmask_pad", None))
    assert bad, ratios
    if T == 1:
        bad, ratios = run_forward("peaked", T, ("unmask_pad", None))
        assert bad, ratios


@pytest.mark.parametrize("T", LENGTHS)
@pytest.mark.parametrize("kind,families", [("drop_key", ("peaked", "uniform")), ("double_key", ("peaked", "uniform")),
                                           ("drop_query", ("peaked", "uniform", "onehot")), ("swap_v", ("peaked", "onehot"))])
def test_backward_defects_are_caught(kind, families, T):
    """(With a single key P = 1 and dP = delta: dS and dQ are zero whatever the pass over keys does, so at T = 1 the key defects
    change nothing and the check is that the comparison still passes.)"""
    if T == 1 and kind in ("drop_key", "double_key"):
        for family in families:
            bad, ratios = run_backward(family, T, (kind, 0))
            assert not bad, (family, kind, ratios)
        return
    for at in positions(T):
        for family in families:
            bad, ratios = run_backward(family, T, (kind, at))
            assert bad, (family, kind, at, ratios)
