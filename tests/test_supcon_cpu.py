"""The label-aware contrastive loss without a GPU: loss.supcon_reference against torch.autograd of the formula written here from
per-row loops over the positive sets, against oracle/'s CLIP loss under distinct labels, and under relabelling of the unknown rows;
the fp32 emulation of the kernels' order (tests/supcon_refs.py) against every derived bound; every injected defect against the
comparison the GPU tests make; every refusal of the public functions; the constructor of LightCurveImageCLIP under loss="supcon"."""
import math
from itertools import combinations

import pytest
import torch

import infonce_refs as R
import supcon_refs as SR

F64 = torch.float64
TK = dict(n_out=16, emb=16, heads=2, depth=1, dropout=0.0, time_norm=20583.37, agg="mean")
SK = dict(n_out=16, emb=16, heads=2, depth=1, dropout=0.0, time_norm=17945.14, agg="mean")


# ------------------------------------------------------------------------------------------------------------ the reference
def _towers(m, n, d, seed):
    g = R.gen(seed)
    return [torch.nn.functional.normalize(torch.randn(n, d, generator=g, dtype=F64), dim=1) for _ in range(m)]


def _loops(embs, y, ls, lb):
    """the formula of the issue, row by row: the positives of row i are listed, never a mask"""
    n = embs[0].shape[0]
    pos = [[j for j in range(n) if j == i or (int(y[i]) >= 0 and int(y[j]) == int(y[i]))] for i in range(n)]
    total = 0.0
    for k, (a, b) in enumerate(combinations(range(len(embs)), 2)):
        s = ls if ls.dim() == 0 else ls[k]
        bias = lb if lb.dim() == 0 else lb[k]
        S = torch.exp(s) * (embs[b] @ embs[a].T) + bias
        for i in range(n):
            c = len(pos[i])
            total = total + (torch.logsumexp(S[i], 0) - sum(S[i, j] for j in pos[i]) / c) / (2 * n)
            total = total + (torch.logsumexp(S[:, i], 0) - sum(S[j, i] for j in pos[i]) / c) / (2 * n)
    return total


@pytest.mark.parametrize("pattern", SR.PATTERNS)
@pytest.mark.parametrize("m", [2, 3])
def test_reference_against_autograd_of_the_row_loops(m, pattern):
    from multimodal_supernovae_amd.loss import supcon_reference
    n, d = 41, 6
    embs = [e.requires_grad_(True) for e in _towers(m, n, d, 5 + m)]
    y = SR.make_labels(pattern, n, seed=m)
    pairs = m * (m - 1) // 2
    ls = (torch.tensor([1.1, 2.0, 2.7][:pairs], dtype=F64) if m == 3 else torch.tensor(2.3, dtype=F64)).requires_grad_(True)
    lb = (torch.tensor([0.3, -1.0, 0.0][:pairs], dtype=F64) if m == 3 else torch.tensor(-0.4, dtype=F64)).requires_grad_(True)
    want = _loops(embs, y, ls, lb)
    grads = torch.autograd.grad(want, [*embs, ls, lb])
    loss, dE, dls, dlb = supcon_reference([e.detach() for e in embs], y, ls.detach(), lb.detach())
    assert abs(float(loss - want.detach())) <= 1e-12
    for a, b in zip(dE, grads[:m]):
        assert float((a - b).abs().max()) <= 1e-12
    assert float((dls - grads[m]).abs().max()) <= 1e-12 and float((dlb - grads[m + 1]).abs().max()) <= 1e-12
    assert dls.shape == ls.shape and dlb.shape == lb.shape


@pytest.mark.parametrize("m", [2, 3])
def test_distinct_labels_give_the_clip_loss_of_the_oracle(m):
    from multimodal_supernovae_amd.loss import supcon_reference
    from oracle.loss import clip_loss_multimodal
    n, d = 37, 7
    embs = [e.requires_grad_(True) for e in _towers(m, n, d, 11)]
    ls = torch.tensor(2.1, dtype=F64, requires_grad=True)
    lb = torch.tensor(-0.7, dtype=F64, requires_grad=True)
    want = clip_loss_multimodal(embs, ls, lb)
    grads = torch.autograd.grad(want, [*embs, ls, lb])
    loss, dE, dls, dlb = supcon_reference([e.detach() for e in embs], SR.make_labels("distinct", n), ls.detach(), lb.detach())
    assert abs(float(loss - want.detach())) <= 1e-12
    for a, b in zip(dE + [dls, dlb], grads):
        assert float((a - b).abs().max()) <= 1e-12


def test_unknown_rows_are_singletons():
    from multimodal_supernovae_amd.loss import supcon_reference
    n = 60
    embs = _towers(2, n, 5, 3)
    y = SR.make_labels("unknown", n)
    assert int((y < 0).sum()) > 5 and int((y >= 0).sum()) > 5
    fresh = y.clone()
    fresh[y < 0] = 1000 + torch.arange(int((y < 0).sum()))
    a, b = supcon_reference(embs, y, 2.0, 0.1), supcon_reference(embs, fresh, 2.0, 0.1)
    assert float((a[0] - b[0]).abs()) == 0.0
    assert all(torch.equal(p, q) for p, q in zip(a[1] + [a[2], a[3]], b[1] + [b[2], b[3]]))
    # and float labels holding the same integers are the same labels
    c = supcon_reference(embs, y.to(torch.float32), 2.0, 0.1)
    assert torch.equal(a[0], c[0])


def test_label_patterns():
    n = 2100
    assert torch.equal(SR.make_labels("distinct", n), torch.arange(n))
    five = SR.make_labels("five", n)
    assert sorted(five.unique().tolist()) == [0, 1, 2, 3, 4]
    assert SR.make_labels("one", n).unique().numel() == 1
    unk = SR.make_labels("unknown", n)
    assert 0.25 < float((unk < 0).float().mean()) < 0.42 and int(unk.max()) == 4
    assert torch.equal(SR.make_labels("strided", n), torch.arange(n) % 37)
    sp = SR.make_labels("sparse", n)
    assert int(SR.positives(sp, 0, n).sum(1).max()) <= 4 and int(SR.positives(sp, 0, n).sum(1).min()) >= 2
    # P is symmetric and P_ij = 1 implies c_i == c_j
    for pat in SR.PATTERNS:
        P = SR.positives(SR.make_labels(pat, 300), 0, 300)
        c = P.sum(1)
        assert torch.equal(P, P.T) and bool((c >= 1).all())
        assert bool((c[:, None].expand_as(P)[P] == c[None, :].expand_as(P)[P]).all())


def test_every_pattern_meets_every_kind_of_case():
    for group in (SR.SMALL, SR.MULTI, SR.OFFSET):
        met = {p for n, _, p in SR.RUNS if n in group}
        assert met == set(SR.PATTERNS), (group, met)
    for n in SR.SMALL:
        assert R.CASES[n][1][0] == 1
    for n in SR.MULTI + SR.OFFSET:
        assert R.CASES[n][1][0] > 1
    for n in SR.OFFSET:
        assert R.CASES[n][0].q_offset > 0


# ------------------------------------------------------------------------------------------------------------ the emulation
def _bundle(name, family, pattern, g=None):
    case = R.CASES[name][0]
    inp = R.make_inputs(family, case)
    y = SR.labels_for(name, pattern)
    g = R.grad_out_of(name, family) if g is None else g
    args, fref, lses, bref = SR.refs(inp, case, y, g)
    return case, g, args, fref, lses, bref


def _emulated(args, fref, lses, g, fdefect=None, bdefect=None):
    fwd = SR.emulate_forward(*args, defect=fdefect)
    bwd = SR.emulate_backward(*args, *lses, fref["cnt"], g, defect=bdefect)
    return fwd, bwd


WORST = {}


@pytest.mark.parametrize("name,family,pattern", SR.RUNS + [SR.BIG])
def test_emulation_stays_inside_every_bound(name, family, pattern):
    case, g, args, fref, lses, bref = _bundle(name, family, pattern)
    assert R.plan_features(case) == R.CASES[name][1]
    fwd, bwd = _emulated(args, fref, lses, g)
    bad_f, r_f = SR.failures(fwd, fref)
    bad_b, r_b = SR.failures(bwd, bref)
    for k, v in {**r_f, **r_b}.items():
        WORST[k] = max(WORST.get(k, 0.0), v)
    print(f"\nRATIO emulation {family} {pattern} {name} " + " ".join(f"{k}={v:.3f}" for k, v in {**r_f, **r_b}.items()))
    print("WORST " + " ".join(f"{k}={v:.3f}" for k, v in WORST.items()))
    assert not bad_f + bad_b, (bad_f + bad_b, g)


# ------------------------------------------------------------------------------------------------------------ the defects
def _boundary_positive(case, y, pl):
    """a key that is a positive of some local row other than through the diagonal and sits at a tile, half-wave, wave or split
    boundary -> list of such keys (one per kind of boundary that has one)"""
    P = SR.positives(y, case.q_offset, case.b1)
    qi = case.q_offset + torch.arange(case.b1)
    P[torch.arange(case.b1), qi] = False
    has = P.any(0)
    kps = pl.keys_per_split
    k = torch.arange(case.n1)
    kinds = {"tile": (k % 32 == 31) | (k % 32 == 0), "half-wave": (k % 8 == 3) | (k % 8 == 4),
             "wave": (k % 128 == 31) | (k % 128 == 32) | (k % 128 == 95) | (k % 128 == 96),
             "split": ((k % kps == kps - 1) | (k % kps == 0)) & (k >= kps - 1)}
    out = {}
    for kind, where in kinds.items():
        hit = torch.nonzero(where & has).flatten()
        if hit.numel():
            out[kind] = int(hit[0])
    return out


DEFECT_CASES = [(n, p) for n in ("n300_d100", "sh2100_o1056") for p in ("sparse", "strided")]


@pytest.mark.parametrize("name,pattern", DEFECT_CASES)
def test_every_defect_is_caught(name, pattern):
    case, g, args, fref, lses, bref = _bundle(name, "flat", pattern, g=0.37)
    pl = R.plan(case.b1, case.b2, case.n1, case.n2, case.D)
    assert pl.ksplit > 1
    y = args[4]
    clean_f, clean_b = _emulated(args, fref, lses, g)
    assert not SR.failures(clean_f, fref)[0] and not SR.failures(clean_b, bref)[0]

    def caught(kind, at=None):
        fwd, bwd = _emulated(args, fref, lses, g, fdefect=(kind, at) if kind in SR.FORWARD_DEFECTS else None, bdefect=(kind, at))
        return SR.failures(fwd, fref)[0], SR.failures(bwd, bref)[0], fwd

    for kind in ("count_without_diagonal", "first_split_only", "one_over_c", "grad_out_ignored"):
        bf, bb, _ = caught(kind)
        assert bf or bb, kind
        if kind in ("count_without_diagonal", "first_split_only"):
            assert "cnt differs" in bf, kind
        if kind in ("one_over_c", "grad_out_ignored"):
            assert bb and not bf, kind
    if case.q_offset > 0:
        bf, bb, _ = caught("local_key_label")
        assert bf or bb, "local_key_label"
    ats = _boundary_positive(case, y, pl)
    assert set(ats) == {"tile", "half-wave", "wave", "split"}, ats
    for where, at in ats.items():
        for kind in ("positive_lost", "positive_doubled"):
            bf, _, fwd = caught(kind, at)
            # the exact count catches it alone
            assert not torch.equal(fwd["cnt"], fref["cnt"]), (kind, where, at)
            assert "cnt differs" in bf


@pytest.mark.parametrize("name", ["n300_d100", "sh2100_o1056"])
def test_negative_labels_matching_one_another_is_caught(name):
    """sparse and strided labels with a third of the rows unknown: the defect turns the unknown rows into one class"""
    for pattern in ("sparse", "strided"):
        case = R.CASES[name][0]
        inp = R.make_inputs("flat", case)
        y = SR.labels_for(name, pattern).clone()
        y[torch.arange(case.n1) % 3 == 1] = -1
        args, fref, lses, bref = SR.refs(inp, case, y, 0.37)
        fwd, bwd = _emulated(args, fref, lses, 0.37, fdefect=("negatives_match",), bdefect=("negatives_match",))
        assert "cnt differs" in SR.failures(fwd, fref)[0]
        assert SR.failures(bwd, bref)[0]
        fwd, bwd = _emulated(args, fref, lses, 0.37)
        assert not SR.failures(fwd, fref)[0] and not SR.failures(bwd, bref)[0]


# ------------------------------------------------------------------------------------------------------------ argument checks
def test_every_refusal_comes_before_a_launch():
    from multimodal_supernovae_amd import _lib
    from multimodal_supernovae_amd.loss import supcon_loss, supcon_loss_multimodal
    e = torch.randn(6, 8)
    y = torch.arange(6)
    with pytest.raises(_lib.MsnHipError, match=r"embeddings\[0\] must live on the GPU"):
        supcon_loss(e, e, y)
    with pytest.raises(_lib.MsnHipError, match="embeddings: D must be in 1..256"):
        supcon_loss(torch.randn(6, 257), torch.randn(6, 257), y)
    with pytest.raises(ValueError, match=r"labels must have shape \(6,\)"):
        supcon_loss(e, e, torch.arange(5))
    with pytest.raises(ValueError, match=r"labels must have shape \(6,\)"):
        supcon_loss(e, e, torch.zeros(6, 1, dtype=torch.long))
    with pytest.raises(ValueError, match="embeddings must have the same batch size"):
        supcon_loss(e, torch.randn(5, 8), y)
    with pytest.raises(ValueError, match="embeddings must have the same batch size"):
        supcon_loss_multimodal([e, e, torch.randn(7, 8)], y)
    with pytest.raises(ValueError, match="labels must hold integer values"):
        supcon_loss(e, e, torch.tensor([0.0, 1.0, 2.5, 1.0, 0.0, 3.0]))
    with pytest.raises(ValueError, match="labels must hold integer values"):
        supcon_loss(e, e, torch.tensor([0.0, 1.0, math.nan, 1.0, 0.0, 3.0]))
    with pytest.raises(TypeError, match="labels must have an integer or floating dtype"):
        supcon_loss(e, e, torch.zeros(6, dtype=torch.bool))
    with pytest.raises(ValueError, match="at least two modalities"):
        supcon_loss_multimodal([e], y)
    # N >= 2^31: views of one row, no memory behind them
    big = torch.zeros(1, 4).expand(2 ** 31, 4)
    with pytest.raises(_lib.MsnHipError, match=r"embeddings: N = 2147483648 rows; N must be below 2\^31"):
        supcon_loss(big, big, torch.zeros(1, dtype=torch.int32).expand(2 ** 31))
    # float labels holding integers pass the value check and meet the device check
    with pytest.raises(_lib.MsnHipError, match="must live on the GPU"):
        supcon_loss(e, e, torch.tensor([0.0, 1.0, -1.0, 1.0, 0.0, 3.0]))


def _clip(**kw):
    from multimodal_supernovae_amd.models_multimodal import LightCurveImageCLIP
    return LightCurveImageCLIP(enc_dim=32, nband=2, transformer_kwargs=TK, transformer_spectral_kwargs=SK,
                               combinations=["lightcurve", "spectral"], **kw)


def test_constructor_under_supcon():
    model = _clip(loss="supcon")
    assert model.loss == "supcon" and model.loss_kwargs == {}
    assert model.logit_scale.requires_grad and model.logit_bias.requires_grad
    assert list(model.state_dict()) == list(_clip(loss="softmax").state_dict())
    with pytest.raises(ValueError, match="align_uniform"):
        _clip(loss="supcon", loss_kwargs={"t": 2.0})
    with pytest.raises(ValueError, match=r"classification.*batch\[8\]"):
        model._loss([torch.zeros(4, 32), torch.zeros(4, 32)], None)
