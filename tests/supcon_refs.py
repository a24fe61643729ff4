"""Plain torch references for the label-aware contrastive kernels of csrc/supcon.hip (msn_supcon_fwd / _bwd): every output in fp64
from the fp32 operands as given, a per-element error bound derived from the kernels' rounding steps, an fp32 emulation of the
kernels' order with one switch per injected defect, and the label patterns.  Built on tests/infonce_refs.py (imported, not edited):
its plan mirror, input families (flat, hot, large, unnormalised), make_inputs, the score bound dS, the LSE, G, dQ, dscale and dbias
bound terms, U, MARGIN = 2 and TINY are reused as they stand.  Shared by tests/test_supcon_gpu.py (the kernels against these, on
the card) and tests/test_supcon_cpu.py (the emulation against the bounds and every defect against the comparison, on any machine).
Nothing here imports the package under test.

Interface (that of loss.HipSupConKernels): E1_loc, E2_loc (b, D) are this rank's rows q_offset .. of the gathered E1_all, E2_all
(n, D); labels_all (n) int; S = s E2 E1^T + bias.  Positives P_ij = [i == j] or (y_i == y_j and y_i >= 0), c_i = sum_j P_ij.
Direction 0 takes its queries from E2 (rows of S), direction 1 from E1 (columns of S); P is symmetric, so both use the same mask.
    loss share = 1/(2n) sum_{local i} [(lse_row_i - pm_row_i) + (lse_col_i - pm_col_i)],   pm_i = (1/c_i) sum_j P_ij S_ij
The backward is a launch of its own: it is given the fp32 log-sum-exps of every gathered row and the int32 counts of the local
rows, and its reference is the gradient those inputs define,
    G_ij = exp(S_ij - lse_q[i]) + exp(S_ij - lse_k[j]) - P_ij 2 / c_q[i],   dQ = g s / (2n) G K,
    dlogit_scale = g / (2n) sum_ij G_ij (S_ij - bias),   dbias = g / (2n) sum_ij G_ij          (direction 0, this rank's rows).

The bounds add three terms to those of infonce_refs (same conventions: u = 2^-24, MARGIN times a first-order worst case in fp64;
T = 32-key tiles one wave sweeps per key split, ks = key splits):
  cnt       an integer sum: exact, compared with torch.equal.
  pm        a lane adds S_ij over its positive keys in tile order (at most 16 T of them, and no more than c_i: adding nothing
            rounds nothing), then the two half-waves (1 add), the four waves in wave order (3), the key splits in split order
            (ks): NPADD_i = min(16 T, c_i) + 4 + ks additions on the longest path.  Every S_ij carries dS_ij.  The conversion of
            c_i to fp32 and the division round once each.
                dpm_i = (1/c_i) sum_P dS_ij + NPADD_i u (1/c_i) sum_P |S_ij| + 2 u |pm_i|
  loss      the row's term (lse_row - pm_row) + (lse_col - pm_col) is three more adds; then the strided per-thread sum and the
            block tree of the InfoNCE finish kernel:
                dloss = [sum_i (dlse_row_i + dlse_col_i + dpm_row_i + dpm_col_i)
                         + u (ceil(b / 1024) + 19) sum_i (|lse_row_i| + |lse_col_i| + |pm_row_i| + |pm_col_i|)] / 2n + 2 u |loss|
  G         tc = 2 / c_q rounds twice (conversion, division): 2 u tc; the two adds and the subtraction round: 2 u (a + c + P tc).
                dG_ij = a (dS_ij + u (2 |S_ij - lse_q| + 2)) + c (dS_ij + u (2 |S_ij - lse_k| + 2)) + 2 u (a + c + P_ij tc) + 2 u P_ij tc + TINY
  dQ, dscale, dbias   as in infonce_refs, from this G and dG.
MARGIN stays 2 (the project's choice, made before any card was involved).  A ratio above 1 on the card is a finding, not a
reason to raise it.

Largest error / bound ratios of the fp32 emulation below (tests/test_supcon_cpu.py, every case, family and label pattern; the
gate is 1):
    lse_row  lse_col  loss   dE1    dE2    dscale  dbias
    0.101    0.104    0.029  0.154  0.091  0.062   0.062
Largest ratios measured on an MI355X (tests/test_supcon_gpu.py, every case; the gate is 1; the counts equal in every case):
    pattern    lse_row lse_col    loss     dE1     dE2  dscale   dbias
    distinct     0.162   0.156   0.032   0.155   0.154   0.135   0.139
    five         0.133   0.127   0.029   0.123   0.123   0.120   0.120
    one          0.162   0.160   0.029   0.149   0.138   0.099   0.092
    unknown      0.117   0.125   0.022   0.135   0.124   0.114   0.116
    strided      0.142   0.159   0.026   0.152   0.131   0.101   0.105
    sparse       0.138   0.155   0.022   0.138   0.136   0.115   0.116
Every maximum sits at n <= 33 with D <= 12, where the few-ulp terms of the bound carry it, as for the InfoNCE kernels; the cases with
several key splits reach 0.065 (profiles/supcon_accuracy.txt)."""
import math

import torch

import infonce_refs as R

F32, F64 = R.F32, R.F64
U, MARGIN, TINY = R.U, R.MARGIN, R.TINY
QT, KT, NW = R.QT, R.KT, R.NW
FAMILIES = ("hot", "large", "flat", "unnormalised")
PATTERNS = ("distinct", "five", "one", "unknown", "strided", "sparse")


# ------------------------------------------------------------------------------------------------------------ label patterns
def make_labels(pattern, n, seed=0):
    """-> (n,) int64 labels on the CPU"""
    g = R.gen(7 + 13 * seed + 101 * PATTERNS.index(pattern) + n)
    i = torch.arange(n)
    if pattern == "distinct":
        return i.clone()
    if pattern == "five":
        return torch.randint(0, 5, (n,), generator=g)
    if pattern == "one":
        return torch.full((n,), 3)
    if pattern == "unknown":
        y = torch.randint(0, 5, (n,), generator=g)
        y[torch.rand(n, generator=g) < 1.0 / 3.0] = -1
        return y
    if pattern == "strided":
        return i % 37
    assert pattern == "sparse"
    return i % R.cdiv(n, 3)


def positives(labels_all, q_offset, b):
    """P (b, n) bool for the local rows q_offset .. q_offset + b - 1"""
    y = torch.as_tensor(labels_all).to(torch.int64)
    n = y.shape[0]
    yq = y[q_offset:q_offset + b]
    qi = q_offset + torch.arange(b, device=y.device)
    kj = torch.arange(n, device=y.device)
    return (qi[:, None] == kj[None, :]) | ((yq[:, None] == y[None, :]) & (yq >= 0)[:, None])


# ------------------------------------------------------------------------------------------------------------ fp64 references
def _tiles_per_wave(pl):
    return R.cdiv(pl.keys_per_split // KT, NW)


def forward_ref(e1_loc, e2_loc, e1_all, e2_all, labels_all, q_offset, log_scale, bias):
    """-> dict(lse_row, lse_col (b), cnt (b) int64, loss: this rank's share) with the bounds under "b_" + name, fp64."""
    e1l, e2l, e1a, e2a = R._f64(e1_loc, e2_loc, e1_all, e2_all)
    ls, bs = float(log_scale), float(bias)
    s = math.exp(ls)
    (b, D), n = e1l.shape, e1a.shape[0]
    pl = R.plan(b, b, n, n, D)
    c = R._counts(pl, D)
    lr, dlr, S0, dS0 = R._lse_side(e2l, e1a, s, ls, bs, c)
    lc, dlc, S1, dS1 = R._lse_side(e1l, e2a, s, ls, bs, c)
    P = positives(torch.as_tensor(labels_all).to(e1l.device), q_offset, b)
    Pf = P.to(F64)
    cnt = P.sum(1)
    cf = cnt.to(F64)
    npadd = cf.clamp(max=16.0 * _tiles_per_wave(pl)) + 4 + pl.ksplit

    def pmean(S, dS):
        pm = (Pf * S).sum(1) / cf
        return pm, (Pf * dS).sum(1) / cf + U * npadd * (Pf * S.abs()).sum(1) / cf + 2 * U * pm.abs()

    pm0, dpm0 = pmean(S0, dS0)
    pm1, dpm1 = pmean(S1, dS1)
    loss = (lr + lc - pm0 - pm1).sum() / (2 * n)
    mag = (lr.abs() + lc.abs() + pm0.abs() + pm1.abs()).sum()
    dloss = ((dlr + dlc + dpm0 + dpm1).sum() + U * (R.cdiv(b, 1024) + 19) * mag) / (2 * n) + 2 * U * loss.abs()
    return dict(lse_row=lr, lse_col=lc, cnt=cnt, loss=loss, b_lse_row=MARGIN * dlr, b_lse_col=MARGIN * dlc, b_loss=MARGIN * dloss)


def _side(Q, K, Pf, tcq, q_offset, s, ls, bias, lq_all, lk_all, c, dlq_all=None, dlk_all=None):
    S, dS = R._scores(Q, K, s, ls, bias, c.dacc)
    qi = q_offset + torch.arange(Q.shape[0], device=Q.device)
    lq, lk = lq_all[qi][:, None], lk_all[None, :K.shape[0]]
    a, cc = torch.exp(S - lq), torch.exp(S - lk)
    pt = Pf * tcq[:, None]
    G = a + cc - pt
    dG = a * (dS + U * (2 * (S - lq).abs() + 2)) + cc * (dS + U * (2 * (S - lk).abs() + 2)) + 2 * U * (a + cc + pt) + 2 * U * pt + TINY
    if dlq_all is not None:                # the LSE inputs are themselves off by at most dlq, dlk: first order in the exponentials
        dG = dG + a * dlq_all[qi][:, None] + cc * dlk_all[None, :K.shape[0]]
    return G, dG, S, dS


def backward_ref(e1_loc, e2_loc, e1_all, e2_all, labels_all, q_offset, log_scale, bias, lse_row_all, lse_col_all, cnt, grad_out,
                 d_lse_row=None, d_lse_col=None):
    """The gradient msn_supcon_bwd defines from its inputs (the fp32 log-sum-exps and the counts included)
    -> dict(dE1, dE2 (b, D), dscale, dbias) with the bounds under "b_" + name, fp64.
    d_lse_row, d_lse_col (n each, without MARGIN): for a launch that was fed LSEs which differ from the ones given here by at most
    these (the public functions hand the forward kernel's LSEs to the backward); each exponential of G moves by itself times the
    difference, to first order."""
    e1l, e2l, e1a, e2a, lr, lc = R._f64(e1_loc, e2_loc, e1_all, e2_all, lse_row_all, lse_col_all)
    ls, bs, g = float(log_scale), float(bias), float(grad_out)
    s = math.exp(ls)
    (b, D), n = e1l.shape, e1a.shape[0]
    c = R._counts(R.plan(b, b, n, n, D), D)
    gn = g / (2 * n)
    Pf = positives(torch.as_tensor(labels_all).to(e1l.device), q_offset, b).to(F64)
    tcq = 2.0 / torch.as_tensor(cnt).to(e1l.device).to(F64)
    dlr, dlc = (None, None) if d_lse_row is None else R._f64(d_lse_row, d_lse_col)
    G0, dG0, S0, dS0 = _side(e2l, e1a, Pf, tcq, q_offset, s, ls, bs, lr, lc, c, dlr, dlc)
    d2, bd2, ds, bsc, db, bb = R._products(G0, dG0, S0, dS0, e1a, gn * s, gn, ls, bs, c, True)
    G1, dG1, S1, dS1 = _side(e1l, e2a, Pf, tcq, q_offset, s, ls, bs, lc, lr, c, dlc, dlr)
    d1, bd1 = R._products(G1, dG1, S1, dS1, e2a, gn * s, gn, ls, bs, c, False)
    return dict(dE1=d1, dE2=d2, dscale=ds, dbias=db, b_dE1=bd1, b_dE2=bd2, b_dscale=bsc, b_dbias=bb)


def failures(got, ref):
    """the exact count apart, then infonce_refs.failures on the bounded outputs -> (list of failures, ratios)"""
    got = dict(got)
    bad = []
    if "cnt" in got:
        if not torch.equal(got.pop("cnt").detach().cpu().to(torch.int64), ref["cnt"].cpu().to(torch.int64)):
            bad.append("cnt differs")
    more, r = R.failures(got, ref)
    return bad + more, r


# ------------------------------------------------------------------------------------------------------------ the emulation
DEFECTS = ("count_without_diagonal", "negatives_match", "first_split_only", "positive_lost", "positive_doubled",
           "local_key_label", "one_over_c", "grad_out_ignored")
FORWARD_DEFECTS = DEFECTS[:6]


def _emulated_mask(y, q_offset, b, pl, kind, at):
    """-> (b, n) fp32 weight of every key in a local row's positive sum and count as the (defective) kernel sees it: 1 for a
    positive, 0 otherwise, 2 where `positive_doubled` counts key `at` twice"""
    n = y.shape[0]
    qi, kj = q_offset + torch.arange(b), torch.arange(n)
    yq = y[q_offset:q_offset + b]
    yk = y[(kj - q_offset) % n] if kind == "local_key_label" else y
    same = yq[:, None] == yk[None, :]
    if kind != "negatives_match":
        same = same & (yq >= 0)[:, None]
    P = (qi[:, None] == kj[None, :]) | same
    if kind == "first_split_only":
        P = P & (kj < pl.keys_per_split)[None, :]
    w = P.to(F32)
    if kind == "positive_lost":
        w[:, at] = 0.0
    if kind == "positive_doubled":
        w[:, at] = 2.0 * w[:, at]
    return w


def _emulate_psum(S, w, pl):
    """fp32 sum of w S over the positives in the kernel's order: per half-wave its tiles in turn, the two half-waves, the waves
    in wave order, the splits in split order -> (psum (nq) fp32, count (nq) int64)"""
    nq, nk = S.shape
    Sp = torch.cat([S, torch.zeros(nq, 1)], 1)                   # index -1 (past the split's end): never a positive
    wp = torch.cat([w, torch.zeros(nq, 1)], 1)
    total, count = torch.zeros(nq), torch.zeros(nq, dtype=torch.int64)
    for y in range(pl.ksplit):
        k_begin, k_end = y * pl.keys_per_split, min(nk, (y + 1) * pl.keys_per_split)
        halves = []
        for tiles in R._groups(pl, k_begin, k_end):
            ps, pc = torch.zeros(nq), torch.zeros(nq, dtype=torch.int64)
            for idx in tiles:
                ww = wp[:, idx]
                for r in range(idx.numel()):
                    ps = ps + torch.where(ww[:, r] > 0, ww[:, r] * Sp[:, idx[r]], torch.zeros(nq))
                pc = pc + ww.sum(1).to(torch.int64)
            halves.append((ps, pc))
        split_s, split_c = None, None
        for wv in range(NW):
            s2 = halves[2 * wv][0] + halves[2 * wv + 1][0]
            c2 = halves[2 * wv][1] + halves[2 * wv + 1][1]
            split_s = s2 if split_s is None else split_s + s2
            split_c = c2 if split_c is None else split_c + c2
        total, count = total + split_s, count + split_c
    return total, count


def emulate_forward(e1_loc, e2_loc, e1_all, e2_all, labels_all, q_offset, log_scale, bias, defect=None):
    """defect = (kind[, key index]) -> dict(lse_row, lse_col, cnt, loss) (fp32, cnt int64)"""
    kind, at = (tuple(defect) + (None,))[:2] if defect else (None, None)
    (b, D), n = e1_loc.shape, e1_all.shape[0]
    pl = R.plan(b, b, n, n, D)
    scale, bias = torch.exp(R._e32(log_scale)), R._e32(bias)
    S0, S1 = R._fscores(e2_loc, e1_all, scale, bias), R._fscores(e1_loc, e2_all, scale, bias)
    lr = R._emulate_lse(S0, pl, None, None, None)
    lc = R._emulate_lse(S1, pl, None, None, None)
    w = _emulated_mask(torch.as_tensor(labels_all).to(torch.int64), q_offset, b, pl, kind, at)
    ps0, cnt = _emulate_psum(S0, w, pl)
    ps1, _ = _emulate_psum(S1, w, pl)
    if kind == "count_without_diagonal":
        cnt = cnt - 1
    cf = cnt.to(F32)
    terms = (lr - ps0 / cf) + (lc - ps1 / cf)
    return dict(lse_row=lr, lse_col=lc, cnt=cnt, loss=terms.sum() / R._e32(2.0 * n))


def emulate_backward(e1_loc, e2_loc, e1_all, e2_all, labels_all, q_offset, log_scale, bias, lse_row_all, lse_col_all, cnt, grad_out,
                     defect=None):
    kind, at = (tuple(defect) + (None,))[:2] if defect else (None, None)
    (b, D), n = e1_loc.shape, e1_all.shape[0]
    pl = R.plan(b, b, n, n, D)
    scale, bias = torch.exp(R._e32(log_scale)), R._e32(bias)
    g = R._e32(1.0 if kind == "grad_out_ignored" else grad_out)
    gn = g / R._e32(2.0 * n)
    f = gn * scale
    w = _emulated_mask(torch.as_tensor(labels_all).to(torch.int64), q_offset, b, pl, kind, at)
    tc = R._e32(1.0 if kind == "one_over_c" else 2.0) / torch.as_tensor(cnt).to(F32)
    qi = q_offset + torch.arange(b)
    out = {}
    for dirn, (Q, K, lq_all, lk_all) in enumerate(((e2_loc, e1_all, lse_row_all, lse_col_all), (e1_loc, e2_all, lse_col_all, lse_row_all))):
        S = R._fscores(Q, K, scale, bias)
        lq, lk = lq_all.to(F32)[qi][:, None], lk_all.to(F32)[None, :n]
        G = torch.exp(S - lq) + torch.exp(S - lk)
        G = G - w * tc[:, None]
        dq, ds, db = R._emulate_products(G, S, K, pl, f, gn, bias, None)
        if dirn == 0:
            out.update(dE2=dq, dscale=ds, dbias=db)
        else:
            out.update(dE1=dq)
    return out


# ------------------------------------------------------------------------------------------------------------ the cases
SMALL = tuple(f"n{n}_d{d}" for n in (1, 5, 31, 32, 33) for d in (1, 5, 8, 12))
MULTI = ("n129_d64", "n300_d100", "n300_d130", "sh2100_o0")
OFFSET = ("sh2100_o1056", "sh2100_o2068")
CASE_NAMES = SMALL + MULTI + OFFSET                      # sh8187_o4000 runs once, apart (BIG)
BIG = ("sh8187_o4000", "hot", "five")
RUNS = [(name, fam, PATTERNS[(4 * ci + fi) % len(PATTERNS)]) for ci, name in enumerate(CASE_NAMES) for fi, fam in enumerate(FAMILIES)]


def labels_for(name, pattern):
    case = R.CASES[name][0]
    return make_labels(pattern, case.n1, seed=list(R.CASES).index(name))


def refs(inp, case, labels, grad_out, device="cpu"):
    """-> (launch operands on `device` (labels int64), forward reference, the fp32 LSEs of every gathered row, backward reference)"""
    e1a, e2a = inp["e1_all"].to(device), inp["e2_all"].to(device)
    y = labels.to(device)
    o = case.q_offset
    args = (e1a[o:o + case.b1], e2a[o:o + case.b2], e1a, e2a, y, o, inp["log_scale"], inp["bias"])
    fref = forward_ref(*args)
    if o == 0 and case.b1 == case.n1:
        lr, lc = fref["lse_row"], fref["lse_col"]
    else:
        lr, lc = R.lse_all_ref(e1a, e2a, inp["log_scale"], inp["bias"])
    lr, lc = lr.to(F32), lc.to(F32)
    bref = backward_ref(*args, lr, lc, fref["cnt"], grad_out)
    return args, fref, (lr, lc), bref
