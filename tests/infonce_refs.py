"""Plain torch references for the fused contrastive-loss kernels of csrc/infonce.hip and csrc/infonce_wide.hip (msn_infonce_fwd /
_bwd, msn_sigmoid_loss_fwd / _bwd, msn_retrieval_rank): every output in fp64 from the fp32 operands as given, a per-element error
bound derived from the kernels' rounding steps, a mirror of the key-split plan, an fp32 emulation of the kernels' arithmetic order
with one switch per injected defect, and the input families.  Shared by tests/test_infonce_pinned_gpu.py (the kernels against
these, on the card) and tests/test_infonce_refs_cpu.py (the emulation against the bounds and every defect against the comparison,
on any machine).  Nothing here imports the package under test.

Interface (that of loss.HipPairKernels): E1_loc (b1, D), E2_loc (b2, D) are this rank's rows q_offset .. of the gathered E1_all
(n1, D), E2_all (n2, D); S = s E2 E1^T + bias with s = exp(log_scale), n = min(n1, n2).  Direction 0 takes its queries from E2
(rows of S, keys E1), direction 1 from E1 (columns of S, keys E2).  The backward is a launch of its own: it is given the
log-sum-exps of every gathered row as fp32 inputs, and its reference is the gradient those inputs define,
    G_ij = [i < n] exp(S_ij - lse_q[i]) + [j < n] exp(S_ij - lse_k[j]) - 2 [i = j < n],     dQ = g s / (2 n) G K,
    dlogit_scale = g / (2 n) sum_ij G_ij (S_ij - bias),   dbias = g / (2 n) sum_ij G_ij      (direction 0, this rank's rows).
Sigmoid loss: Z = -s E2 E1^T + bias, z = +1 on the diagonal and -1 elsewhere, loss = sum softplus(z Z) / n^2,
G_ij = z sigmoid(z Z) and the same three products with g / n^2, dZ/dx = -s, dZ/dlog_scale = Z - bias.

The bounds.  u = 2^-24.  Every bound below is MARGIN times a first-order worst case: u times the matching sum of absolute terms,
evaluated in fp64.  With A_ij = sum_d |q_d k_d|, ls = log_scale, and the counts T (32-key tiles one wave sweeps per key split), ks
(key splits), kps (keys per split) taken from the plan:
  score     x_ij is an fp32 matrix-core sum of D products (D + 3 in the wide kernels, which add four partial sums): D u A_ij.
            s = __expf(ls) = exp2(ls log2e): the product rounds (|ls| u relative to s), the hardware exp2 adds 2 u.  S = x s + bias
            rounds once more whether or not the compiler fuses it.
                dS_ij = u ((D + |ls| + 3) s A_ij + |S_ij|)
  lse       every term of sum_j exp(S_ij - m) is a chain of __expf of non-positive arguments (its own, then one per rescale of the
            running sum: tile loop, half-waves, waves, splits).  The arguments of a chain add up to S_ij - M_i exactly in sign, so
            their roundings (the subtraction and the product with log2e) cost 2 u |S_ij - M_i| in all; each call adds 2 u (exp2,
            the product with the running sum), at most NEXP = T + 3 + ceil(ks / 8) calls.  The positive fp32 sums (16 registers -- 4
            in the wide kernels --, T tiles, 2 half-waves, 4 waves, ks splits) cost NADD u relative.  __logf costs 3 u |log L|, the
            final M + log L one u |lse|.
                dlse_i = sum_j P_ij (dS_ij + u (2 |S_ij - M_i| + 2 NEXP)) + u (NADD + 3 |lse_i - M_i| + |lse_i|)
  loss      the fp32 sum of lse_row + lse_col - 2 S_ii over the rank's rows (a strided per-thread sum, then a block tree):
                dloss = [sum_i (dlse_row_i + dlse_col_i + 2 dS_ii) + u (ceil(b / 1024) + 16) sum_i (|lse_row_i| + |lse_col_i| + 2 |S_ii|)] / 2n
                        + 2 u |loss|
  G         each of the two exponentials: its argument is off by dS_ij and by the roundings 2 u |S_ij - lse|, exp2 adds 2 u; the
            two adds and the -2 round: 2 u (a + c + 2 delta_ij).  A flushed exponential (argument below -87) is covered by the
            absolute floor TINY = 2^-100.
                dG_ij = a (dS_ij + u (2 |S_ij - lse_q| + 2)) + c (dS_ij + u (2 |S_ij - lse_k| + 2)) + 2 u (a + c + 2 delta_ij) + TINY
  dQ        the second product accumulates kps / 4 keys per wave (kps in the wide kernels), then 4 waves, then ks splits:
            NACC = kps / 4 + 4 + ks.  f = (g / 2n) s carries (|ls| + 6) u (division, __expf, two products).
                ddQ_id = |f| (sum_j dG_ij |K_jd| + NACC u sum_j |G_ij| |K_jd|) + (|ls| + 6) u |dQ_id|
  dscale    fp32 fma chains of 16 T terms per lane (4 T wide), a wave tree, four waves: NSC = 16 T + 10; the block sums are
            added in fp64 (nothing to model), the result is rounded to fp32 and scaled: 4 u.
                ddscale = |g| / 2n (sum_ij [dG_ij |S_ij - b| + |G_ij| (dS_ij + 2 u |S_ij - b|)] + NSC u sum_ij |G_ij| |S_ij - b|) + 4 u |dscale|
                ddbias  = |g| / 2n (sum_ij dG_ij + NSC u sum_ij |G_ij|) + 4 u |dbias|
  sigmoid   the loss is evaluated in fp64 on the fp32 Z: dloss = sum_ij sigmoid(z Z) dS_ij / n^2 + 2 u |loss|.  Backward:
            sg = 1 / (1 + __expf(-zz)) is off by sg (1 - sg) (dS + u (|zz| + 2)) from the exponential and 3 u sg from the add and the
            division; saturation to exactly 0 or 1 is inside the floor TINY.
  rank      a comparison of raw scores: ranks are held equal on every row whose fp64 margin min_j |x_ij - x_ii| exceeds
            dx_ij + dx_ii, dx_ij = MARGIN u (D + 3) A_ij.  Through utils.retrieval_ranks the rows are first normalised in fp32
            (sum of D squares, rsqrt, product: (D / 2 + 4) u relative per vector), which rank_score_bound(..., normalised=True) adds.
MARGIN = 2 covers what is not modelled: second-order terms, the unspecified order inside a matrix-core instruction, exponent and
logarithm instructions that are one ulp only on their documented range.  It was chosen before any card was involved: the fp32
emulation below (same tile, wave and split order, torch's fp32 exp and log) stays below 0.35 of every bound with MARGIN = 2 on every
case of tests/test_infonce_refs_cpu.py, and a worst case that is a sum of moduli is never reached by rounding errors of mixed sign.
A ratio above 1 on the card is a finding, not a reason to raise it.

Largest error / bound ratios measured on an MI355X (tests/test_infonce_pinned_gpu.py, every case; the gate is 1):
    family            lse_row  lse_col  loss   dE1    dE2    dscale  dbias
    flat              0.162    0.160    0.035  0.156  0.155  0.136   0.140
    hot               0.101    0.159    0.032  0.156  0.130  0.130   0.130
    hot, swapped      0.159    0.101    0.032  0.130  0.156  0.130   0.130
    large             0.138    0.155    0.024  0.140  0.133  0.120   0.120
    unnormalised      0.092    0.092    0.012  0.087  0.087  0.033   0.033
    sigmoid, large    -        -        0.034  0.037  0.041  0.004   0.013
    sigmoid, unnorm.  -        -        0.013  0.028  0.021  0.007   0.002
Every maximum of the softmax rows sits at n <= 33 with D <= 8, where the few-ulp terms of the bound carry it; the cases with
several key splits reach 0.085 (narrow) and 0.044 (wide), the emulation 0.28.  Ranks: equal on every row of the integer family."""
import math
from types import SimpleNamespace

import torch

F32, F64 = torch.float32, torch.float64
U = 2.0 ** -24               # unit roundoff of fp32
MARGIN = 2.0                 # everything not modelled (see the module docstring)
TINY = 2.0 ** -100           # absolute floor: flushed exponentials, saturated sigmoids
QT = KT = 32                 # queries per workgroup, keys per tile
NW = 4                       # waves per workgroup
NARROW_MAX_D = 256
FAMILIES = ("flat", "hot", "large", "unnormalised", "integer")


def gen(seed):
    return torch.Generator().manual_seed(seed)


def cdiv(a, b):
    return -(-a // b)


def row_of(r, h):
    """key row of a 32-key tile that accumulator register r of half-wave h holds"""
    return (r & 3) + 8 * (r >> 2) + 4 * h


# ------------------------------------------------------------------------------------------------------------ the plan
def plan(b1, b2, n1, n2, D):
    """make_plan of csrc/infonce_args.h -> ksplit, keys_per_split, qtiles, maxq, wide, workspace bytes."""
    wide = D > NARROW_MAX_D
    kstep = KT if wide else KT * NW
    maxq, maxk = max(b1, b2), max(n1, n2)
    qtiles = cdiv(maxq, QT)
    ks = max(1, 512 // (2 * qtiles))
    ks = min(ks, cdiv(maxk, kstep))
    ks = max(min(ks, 64), 1)
    kps = cdiv(cdiv(maxk, ks), kstep) * kstep
    ksplit = cdiv(maxk, kps)
    take = lambda nbytes: cdiv(nbytes, 256) * 256
    total = 3 * take(4 * 2 * ksplit * maxq) + take(4 * 2 * (0 if wide and ksplit == 1 else ksplit) * maxq * D) + take(8 * 2 * ksplit * qtiles)
    return SimpleNamespace(ksplit=ksplit, keys_per_split=kps, qtiles=qtiles, maxq=maxq, wide=wide, total=total, capped=ks == 64)


def _counts(pl, D):
    tiles = pl.keys_per_split // KT
    tw = tiles if pl.wide else cdiv(tiles, NW)
    per = 4 if pl.wide else 16
    return SimpleNamespace(dacc=D + (3 if pl.wide else 0), nexp=tw + 3 + cdiv(pl.ksplit, 8), nadd=per + tw + 2 + NW + pl.ksplit,
                           nacc=(pl.keys_per_split if pl.wide else pl.keys_per_split // NW) + NW + pl.ksplit, nsc=per * tw + 10)


# ------------------------------------------------------------------------------------------------------------ fp64 references
def _f64(*ts):
    return tuple(torch.as_tensor(t).to(F64) for t in ts)


def _scores(Q, K, s, ls, bias, dacc, sign=1.0):
    """S = sign s Q K^T + bias and its bound dS (without MARGIN), fp64"""
    x = Q @ K.T
    A = Q.abs() @ K.abs().T
    S = sign * x * s + bias
    return S, U * ((dacc + abs(ls) + 3) * s * A + S.abs())


def lse_all_ref(e1_all, e2_all, log_scale, bias, chunk=1024):
    """(lse_row of all n2 rows, lse_col of all n1 columns) in fp64, in row chunks (the n2 x n1 matrix is never held)."""
    e1, e2 = _f64(e1_all, e2_all)
    s, b = math.exp(float(log_scale)), float(bias)
    row = torch.cat([torch.logsumexp(e2[i:i + chunk] @ e1.T * s + b, 1) for i in range(0, e2.shape[0], chunk)])
    col = torch.cat([torch.logsumexp(e1[i:i + chunk] @ e2.T * s + b, 1) for i in range(0, e1.shape[0], chunk)])
    return row, col


def _lse_side(Q, K, s, ls, bias, c):
    S, dS = _scores(Q, K, s, ls, bias, c.dacc)
    mx = S.max(1).values
    lse = torch.logsumexp(S, 1)
    P = torch.exp(S - lse[:, None])
    dl = (P * (dS + U * (2 * (S - mx[:, None]).abs() + 2 * c.nexp))).sum(1) + U * (c.nadd + 3 * (lse - mx).abs() + lse.abs())
    return lse, dl, S, dS


def softmax_forward_ref(e1_loc, e2_loc, e1_all, e2_all, q_offset, log_scale, bias):
    """-> dict(lse_row (b2), lse_col (b1), loss: this rank's share) with the bounds under "b_" + name, fp64."""
    e1l, e2l, e1a, e2a = _f64(e1_loc, e2_loc, e1_all, e2_all)
    ls, b = float(log_scale), float(bias)
    s = math.exp(ls)
    (b1, D), b2, n1, n2 = e1l.shape, e2l.shape[0], e1a.shape[0], e2a.shape[0]
    n = min(n1, n2)
    c = _counts(plan(b1, b2, n1, n2, D), D)
    lr, dlr, S0, dS0 = _lse_side(e2l, e1a, s, ls, b, c)
    lc, dlc, _, _ = _lse_side(e1l, e2a, s, ls, b, c)
    nb = min(b1, b2)
    i = torch.arange(nb, device=e1l.device)
    ok = (q_offset + i) < n
    col = (q_offset + i).clamp(max=n1 - 1)
    dg, ddg = S0[i, col], dS0[i, col]
    okf = ok.to(F64)
    loss = ((lr[:nb] + lc[:nb] - 2 * dg) * okf).sum() / (2 * n)
    mag = ((lr[:nb].abs() + lc[:nb].abs() + 2 * dg.abs()) * okf).sum()
    dloss = (((dlr[:nb] + dlc[:nb] + 2 * ddg) * okf).sum() + U * (cdiv(max(b1, b2), 1024) + 16) * mag) / (2 * n) + 2 * U * loss.abs()
    return dict(lse_row=lr, lse_col=lc, loss=loss, b_lse_row=MARGIN * dlr, b_lse_col=MARGIN * dlc, b_loss=MARGIN * dloss)


def _softmax_side(Q, K, q_offset, n, s, ls, bias, lq_all, lk_all, c):
    S, dS = _scores(Q, K, s, ls, bias, c.dacc)
    qi = q_offset + torch.arange(Q.shape[0], device=Q.device)
    kj = torch.arange(K.shape[0], device=Q.device)
    q_in, k_in = qi < n, kj < n
    lq = lq_all[qi.clamp(max=lq_all.shape[0] - 1)][:, None]
    lk = lk_all[kj.clamp(max=lk_all.shape[0] - 1)][None, :]
    zero = torch.zeros_like(S)
    a = torch.where(q_in[:, None].expand_as(S), torch.exp(S - lq), zero)
    cc = torch.where(k_in[None, :].expand_as(S), torch.exp(S - lk), zero)
    delta = ((qi[:, None] == kj[None, :]) & q_in[:, None]).to(F64)
    G = a + cc - 2 * delta
    dG = a * (dS + U * (2 * (S - lq).abs() + 2)) + cc * (dS + U * (2 * (S - lk).abs() + 2)) + 2 * U * (a + cc + 2 * delta) + TINY
    return G, dG, S, dS


def _products(G, dG, S, dS, K, f, gn, ls, bias, c, scalars):
    """dQ = f G K and, for direction 0, (dscale, dbias) = gn (sum G (S - bias), sum G), with their bounds"""
    dQ = f * (G @ K)
    bQ = abs(f) * (dG @ K.abs() + U * c.nacc * (G.abs() @ K.abs())) + (abs(ls) + 6) * U * dQ.abs()
    if not scalars:
        return dQ, MARGIN * bQ
    X = S - bias
    ds, db = gn * (G * X).sum(), gn * G.sum()
    bs = abs(gn) * ((dG * X.abs() + G.abs() * (dS + 2 * U * X.abs())).sum() + U * c.nsc * (G.abs() * X.abs()).sum()) + 4 * U * ds.abs()
    bb = abs(gn) * (dG.sum() + U * c.nsc * G.abs().sum()) + 4 * U * db.abs()
    return dQ, MARGIN * bQ, ds, MARGIN * bs, db, MARGIN * bb


def softmax_backward_ref(e1_loc, e2_loc, e1_all, e2_all, q_offset, log_scale, bias, lse_row_all, lse_col_all, grad_out):
    """The gradient msn_infonce_bwd defines from its inputs (the fp32 log-sum-exps included)
    -> dict(dE1 (b1, D), dE2 (b2, D), dscale, dbias) with the bounds under "b_" + name, fp64."""
    e1l, e2l, e1a, e2a, lr, lc = _f64(e1_loc, e2_loc, e1_all, e2_all, lse_row_all, lse_col_all)
    ls, b, g = float(log_scale), float(bias), float(grad_out)
    s = math.exp(ls)
    (b1, D), b2, n1, n2 = e1l.shape, e2l.shape[0], e1a.shape[0], e2a.shape[0]
    n = min(n1, n2)
    c = _counts(plan(b1, b2, n1, n2, D), D)
    gn = g / (2 * n)
    G0, dG0, S0, dS0 = _softmax_side(e2l, e1a, q_offset, n, s, ls, b, lr, lc, c)
    d2, bd2, ds, bs, db, bb = _products(G0, dG0, S0, dS0, e1a, gn * s, gn, ls, b, c, True)
    G1, dG1, S1, dS1 = _softmax_side(e1l, e2a, q_offset, n, s, ls, b, lc, lr, c)
    d1, bd1 = _products(G1, dG1, S1, dS1, e2a, gn * s, gn, ls, b, c, False)
    return dict(dE1=d1, dE2=d2, dscale=ds, dbias=db, b_dE1=bd1, b_dE2=bd2, b_dscale=bs, b_dbias=bb)


def _sigmoid_side(Q, K, q_offset, s, ls, bias, c):
    Z, dZ = _scores(Q, K, s, ls, bias, c.dacc, sign=-1.0)
    qi = q_offset + torch.arange(Q.shape[0], device=Q.device)
    kj = torch.arange(K.shape[0], device=Q.device)
    z = torch.where(qi[:, None] == kj[None, :], 1.0, -1.0).to(F64)
    return Z, dZ, z


def sigmoid_forward_ref(e1_loc, e2_loc, e1_all, e2_all, q_offset, log_scale, bias):
    """-> dict(loss: this rank's share of mean softplus(z Z), b_loss)"""
    e2l, e1a = _f64(e2_loc, e1_all)
    ls, b = float(log_scale), float(bias)
    n, D = e1a.shape
    c = _counts(plan(e2l.shape[0], e2l.shape[0], n, n, D), D)
    Z, dZ, z = _sigmoid_side(e2l, e1a, q_offset, math.exp(ls), ls, b, c)
    u = z * Z
    loss = torch.nn.functional.softplus(u, threshold=200.0).sum() / n ** 2
    dloss = (torch.sigmoid(u) * dZ).sum() / n ** 2 + 2 * U * loss.abs()
    return dict(loss=loss, b_loss=MARGIN * dloss, Z=Z, z=z)


def sigmoid_backward_ref(e1_loc, e2_loc, e1_all, e2_all, q_offset, log_scale, bias, grad_out):
    e1l, e2l, e1a, e2a = _f64(e1_loc, e2_loc, e1_all, e2_all)
    ls, b, g = float(log_scale), float(bias), float(grad_out)
    s = math.exp(ls)
    n, D = e1a.shape
    c = _counts(plan(e1l.shape[0], e2l.shape[0], n, n, D), D)
    gn = g / n ** 2
    out = {}
    for name, Q, K, scalars in (("dE2", e2l, e1a, True), ("dE1", e1l, e2a, False)):
        Z, dZ, z = _sigmoid_side(Q, K, q_offset, s, ls, b, c)
        u = z * Z
        sg = torch.sigmoid(u)
        G = z * sg
        dG = sg * (1 - sg) * (dZ + U * (u.abs() + 2)) + 3 * U * sg + TINY
        res = _products(G, dG, Z, dZ, K, -gn * s, gn, ls, b, c, scalars)
        out[name], out["b_" + name] = res[0], res[1]
        if scalars:
            out["dscale"], out["b_dscale"], out["dbias"], out["b_dbias"] = res[2:]
    return out


def rank_ref(e1, e2):
    """rank[i] = #{j != i : <e2_i, e1_j> > <e2_i, e1_i>} in fp64 -> (ranks int64, x (n, n))"""
    a, q = _f64(e1, e2)
    x = q @ a.T
    d = x.diagonal()[:, None]
    return (x > d).sum(1), x


def rank_score_bound(e1, e2, normalised=False):
    """dx_ij of the module docstring for scores of e2 rows against e1 rows (fp64 operands as the reference uses them)"""
    a, q = _f64(e1, e2)
    D = a.shape[1]
    A = q.abs() @ a.abs().T
    return MARGIN * U * ((D + 3) + (2 * (D / 2 + 4) if normalised else 0)) * A


def rank_decided_rows(x, dx):
    """rows whose partner's score is further than the score bounds from every other score: there the rank is determined"""
    n = x.shape[0]
    d, dd = x.diagonal()[:, None], dx.diagonal()[:, None]
    gap = (x - d).abs() - (dx + dd)
    gap[torch.arange(n), torch.arange(n)] = math.inf
    return gap.min(1).values > 0


# ------------------------------------------------------------------------------------------------------------ the comparison
def worst_ratio(got, ref, bound):
    """max |got - ref| / bound; an exact element counts 0 whatever its bound, NaN and an error against a zero bound count inf."""
    got = torch.as_tensor(got).detach().to(F64).to(ref.device)
    err = (got - ref).abs()
    r = err / bound
    r = torch.where(err == 0, torch.zeros_like(r), r)
    r = torch.where(torch.isnan(r), torch.full_like(r, math.inf), r)
    return float(r.max())


def ratios(got, ref):
    """got: dict name -> tensor; ref: a *_ref dict -> dict name -> worst error / bound"""
    return {k: worst_ratio(v, ref[k], ref["b_" + k]) for k, v in got.items()}


def failures(got, ref):
    r = ratios(got, ref)
    return [f"{k} at {v:.3g} of its bound" for k, v in r.items() if not v <= 1.0], r


# ------------------------------------------------------------------------------------------------------------ input families
def _unit(n, d, g):
    x = torch.randn(n, d, generator=g, dtype=F64)
    return x / x.norm(dim=-1, keepdim=True)


def boundaries(pl, nk, q_glob):
    """the key indices at which a tile, wave or split begins or ends, and the query's own tile edges"""
    kps = pl.keys_per_split
    last = (cdiv(nk, kps) - 1) * kps
    own = q_glob // QT * QT
    cand = [0, 31, 32, 127, 128, kps - 1, kps, last, nk - 1, own, own + 31]
    return sorted({k for k in cand if 0 <= k < nk})


def _seed(family, case, swapped):
    return 7919 * case.n1 + 104729 * case.n2 + 31 * case.D + 1000003 * FAMILIES.index(family) + 17 * case.q_offset + int(swapped)


def make_case(b1, b2, n1, n2, D, q_offset=0):
    return SimpleNamespace(b1=b1, b2=b2, n1=n1, n2=n2, D=D, q_offset=q_offset)


def swap(case):
    return make_case(case.b2, case.b1, case.n2, case.n1, case.D, case.q_offset)


def _hot(case, g, swapped):
    """Keys E1: unit vectors (D = 1: distinct magnitudes, sign +-).  Local query i of E2 points along its designated key h(i),
    taken in turn from boundaries(); its length is found by bisection in fp64 so that the softmax weight of h(i) is 0.5."""
    pl = plan(case.b1, case.b2, case.n1, case.n2, case.D)
    n1, n2, D, s = case.n1, case.n2, case.D, 20.0
    K = _unit(n1, D, g)
    if D == 1:
        K = K * (0.5 + torch.rand(n1, 1, generator=g, dtype=F64))
    Qall = _unit(n2, D, g)
    hot = torch.full((case.b2,), -1, dtype=torch.long)
    if n1 >= 2:
        for i in range(case.b2):
            qg = case.q_offset + i
            cyc = [k for k in boundaries(pl, n1, qg) if k != qg] or [(qg + 1) % n1]
            hot[i] = cyc[i % len(cyc)]
        if D == 1:                                             # one dimension: only the two extreme keys can win a query
            ends = (int(K[:, 0].argmax()), int(K[:, 0].argmin()))
            for i in range(case.b2):
                hot[i] = ends[i % 2] if ends[i % 2] != case.q_offset + i else ends[1 - i % 2]
        V = K[hot] / K[hot].norm(dim=1, keepdim=True)
        C = V @ K.T                                            # (b2, n1)
        top = C[torch.arange(case.b2), hot][:, None]
        target = 0.5 if n1 > 2 else 0.6
        lo, hi = torch.zeros(case.b2, dtype=F64), torch.full((case.b2,), 1e4, dtype=F64)
        for _ in range(80):
            t = 0.5 * (lo + hi)
            w = 1.0 / torch.exp(s * t[:, None] * (C - top)).sum(1)
            up = w < target
            lo, hi = torch.where(up, t, lo), torch.where(up, hi, t)
        Qall[case.q_offset:case.q_offset + case.b2] = V * (0.5 * (lo + hi))[:, None]
    return K, Qall, math.log(s), 0.5, hot


def make_inputs(family, case, swapped=False):
    """-> dict(e1_all (n1, D), e2_all (n2, D), log_scale, bias: fp32 on the CPU[, hot: the designated key of each local query]).
    `swapped` builds the family for the other direction: the roles of the two modalities are exchanged, so the structured
    queries are rows of E1 and meet the kernels' direction 1."""
    assert family in FAMILIES
    if swapped:
        out = make_inputs(family, swap(case))
        out["e1_all"], out["e2_all"] = out["e2_all"], out["e1_all"]
        return out
    g = gen(_seed(family, case, swapped))
    n1, n2, D = case.n1, case.n2, case.D
    ex = {}
    if family == "flat":
        e1, e2 = _unit(n1, D, g), _unit(n2, D, g)
        ls, bias = math.log(10.0 + 21.0 * float(torch.rand((), generator=g))), (-10.0, 0.5)[(n1 + D) % 2]
    elif family == "hot":
        e1, e2, ls, bias, ex["hot"] = _hot(case, g, swapped)
    elif family == "large":
        e1, e2 = _unit(n1, D, g), _unit(n2, D, g)
        i = torch.arange(min(n1, n2))
        dup, anti = i[i % 4 == 0], i[i % 8 == 5]
        noise = _unit(min(n1, n2), D, g)
        near = e1[:min(n1, n2)] + 0.1 * noise
        near = near / near.norm(dim=1, keepdim=True)
        e2[dup], e2[anti] = near[dup], -near[anti]
        ls, bias = math.log(100.0), (10.0 if len(anti) == 0 or (n1 + D) % 2 else -10.0)
    elif family == "unnormalised":
        e1 = _unit(n1, D, g) * (0.1 + 2.9 * torch.rand(n1, 1, generator=g, dtype=F64))
        e2 = _unit(n2, D, g) * (0.1 + 2.9 * torch.rand(n2, 1, generator=g, dtype=F64))
        ls, bias = math.log(3.0), -1.0
    else:
        e1 = torch.randint(-2, 3, (n1, D), generator=g).to(F64)
        e2 = torch.randint(-2, 3, (n2, D), generator=g).to(F64)
        for i in range(0, n1 - 1, 7):                          # duplicated keys: exact ties with the partner
            e1[i + 1] = e1[i]
        ls, bias = 0.0, 0.0
    f = lambda v: torch.tensor(v, dtype=F32)
    return dict(e1_all=e1.to(F32).contiguous(), e2_all=e2.to(F32).contiguous(), log_scale=f(ls), bias=f(bias), **ex)


def local_rows(inp, case):
    o = case.q_offset
    return inp["e1_all"][o:o + case.b1], inp["e2_all"][o:o + case.b2]


def hot_weights(inp, case):
    """fp64 softmax weight of the designated key of every local query of E2"""
    e1, e2 = _f64(inp["e1_all"], local_rows(inp, case)[1])
    S = e2 @ e1.T * math.exp(float(inp["log_scale"])) + float(inp["bias"])
    P = torch.softmax(S, 1)
    return P[torch.arange(case.b2), inp["hot"]]


# ------------------------------------------------------------------------------------------------------------ the emulation
DEFECTS = ("skip_key", "double_key", "no_max_subtraction", "merge_without_rescale", "no_inf_guard", "local_positive",
           "n1_normaliser", "finite_lse_k", "no_minus_2_delta", "grad_out_ignored", "dscale_with_bias", "sigmoid_diag_sign",
           "rank_ge")
NEG = -math.inf


def _e32(x):
    return torch.as_tensor(x, dtype=F32)


def _fscores(Q, K, scale, bias, sign=1.0):
    return (Q.to(F32) @ K.to(F32).T) * (sign * scale) + bias


def _groups(pl, k_begin, k_end):
    """for every (wave, half-wave): the list of key-index vectors (one per tile it sweeps, -1 = past the split's end)"""
    out = []
    for w in range(NW):
        for h in range(2):
            tiles = []
            if pl.wide:
                for k0 in range(k_begin, k_end, KT):
                    tiles.append([k0 + row_of(4 * w + i, h) for i in range(4)])
            else:
                for k0 in range(k_begin + KT * w, k_end, KT * NW):
                    tiles.append([k0 + row_of(r, h) for r in range(16)])
            out.append([torch.tensor([k if k < k_end else -1 for k in t]) for t in tiles])
    return out


def _emulate_lse(S, pl, defect, at, qrows):
    """S (nq, nk) fp32 -> lse (nq) fp32 in the kernels' order: online (m, l) per half-wave over its tiles, half-waves, waves, splits
    folded eight at a time.  `qrows`: the rows (one query tile) a key defect applies to."""
    nq, nk = S.shape
    guard = defect != "no_inf_guard"
    Sp = torch.cat([S, torch.full((nq, 1), NEG)], 1)            # index -1 -> -inf
    pm, plv = [], []
    for y in range(pl.ksplit):
        k_begin, k_end = y * pl.keys_per_split, min(nk, (y + 1) * pl.keys_per_split)
        halves = []
        for tiles in _groups(pl, k_begin, k_end):
            m, l = torch.full((nq,), NEG), torch.zeros(nq)
            for idx in tiles:
                s = Sp[:, idx].clone()
                if defect == "skip_key" and at in idx.tolist():
                    s[qrows, idx.tolist().index(at)] = NEG
                mn = torch.maximum(m, s.max(1).values)
                if defect == "no_max_subtraction":
                    mn = torch.zeros(nq)
                add = torch.exp(s - mn[:, None]).sum(1)
                if defect == "double_key" and at in idx.tolist():
                    add[qrows] = add[qrows] + torch.exp(s[qrows, idx.tolist().index(at)] - mn[qrows])
                ln = l * torch.exp(m - mn) + add
                live = (mn > NEG) if guard else torch.ones(nq, dtype=torch.bool)
                l, m = torch.where(live, ln, l), torch.where(live, mn, m)
            halves.append((m, l))
        wm, wl = [], []
        for w in range(NW):
            (m, l), (m2, l2) = halves[2 * w], halves[2 * w + 1]
            mm = torch.maximum(m, m2)
            ll = l * torch.exp(m - mm) + l2 * torch.exp(m2 - mm)
            if guard:
                ll = torch.where(mm > NEG, ll, torch.zeros(nq))
            wm.append(mm)
            wl.append(ll)
        M = torch.stack(wm).max(0).values
        L = torch.zeros(nq)
        for w in range(NW):
            t = wl[w] * torch.exp(wm[w] - M)
            L = L + (torch.where(wm[w] > NEG, t, torch.zeros(nq)) if guard else t)
        pm.append(M)
        plv.append(L)
    M, L = torch.full((nq,), NEG), torch.zeros(nq)
    for s0 in range(0, pl.ksplit, 8):
        js = range(s0, min(s0 + 8, pl.ksplit))
        cm = M
        for j in js:
            cm = torch.maximum(cm, pm[j])
        if defect == "merge_without_rescale":
            Ln = L.clone()
            for j in js:
                Ln = Ln + plv[j]
        else:
            Ln = L * torch.exp(M - cm)
            if guard:
                Ln = torch.where(M > NEG, Ln, torch.zeros(nq))
            for j in js:
                t = plv[j] * torch.exp(pm[j] - cm)
                Ln = Ln + (torch.where(pm[j] > NEG, t, torch.zeros(nq)) if guard else t)
        live = (cm > NEG) if guard else torch.ones(nq, dtype=torch.bool)
        L, M = torch.where(live, Ln, L), torch.where(live, cm, M)
    return M + torch.log(L)


def _qrows(nq, qtile):
    return torch.arange(qtile * QT, min(nq, (qtile + 1) * QT))


def emulate_softmax_forward(e1_loc, e2_loc, e1_all, e2_all, q_offset, log_scale, bias, defect=None):
    """defect = (kind, key index, query tile) for the key defects of direction 0, (kind,) otherwise
    -> dict(lse_row, lse_col, loss) fp32"""
    kind, at, qtile = (tuple(defect) + (None, 0))[:3] if defect else (None, None, 0)
    (b1, D), b2, n1, n2 = e1_loc.shape, e2_loc.shape[0], e1_all.shape[0], e2_all.shape[0]
    pl = plan(b1, b2, n1, n2, D)
    scale, bias = torch.exp(_e32(log_scale)), _e32(bias)
    n = n1 if kind == "n1_normaliser" else min(n1, n2)
    S0, S1 = _fscores(e2_loc, e1_all, scale, bias), _fscores(e1_loc, e2_all, scale, bias)
    lr = _emulate_lse(S0, pl, kind, at, _qrows(b2, qtile))
    lc = _emulate_lse(S1, pl, kind if kind not in ("skip_key", "double_key") else None, None, None)
    nb = min(b1, b2)
    i = torch.arange(nb)
    ok = (q_offset + i) < n
    col = (i if kind == "local_positive" else q_offset + i).clamp(max=n1 - 1)
    terms = torch.where(ok, lr[:nb] + lc[:nb] - 2.0 * S0[i, col], torch.zeros(nb))
    return dict(lse_row=lr, lse_col=lc, loss=terms.sum() / _e32(2.0 * n))


def _emulate_products(G, S, K, pl, f, gn, bias, kind):
    """per key split: the fp32 slab G K and the fp32 block sums of G (S - bias) and G; slabs added in split order, block sums in fp64"""
    nq, nk = G.shape
    dq, ds, db = torch.zeros(nq, K.shape[1]), 0.0, 0.0
    X = S if kind == "dscale_with_bias" else S - bias
    for y in range(pl.ksplit):
        lo, hi = y * pl.keys_per_split, min(nk, (y + 1) * pl.keys_per_split)
        if lo >= hi:
            continue
        dq = dq + G[:, lo:hi] @ K[lo:hi].to(F32)
        for q0 in range(0, nq, QT):
            ds += float((G[q0:q0 + QT, lo:hi] * X[q0:q0 + QT, lo:hi]).sum())
            db += float(G[q0:q0 + QT, lo:hi].sum())
    return f * dq, gn * _e32(ds), gn * _e32(db)


def emulate_softmax_backward(e1_loc, e2_loc, e1_all, e2_all, q_offset, log_scale, bias, lse_row_all, lse_col_all, grad_out,
                             defect=None):
    kind, at, qtile = (tuple(defect) + (None, 0))[:3] if defect else (None, None, 0)
    (b1, D), b2, n1, n2 = e1_loc.shape, e2_loc.shape[0], e1_all.shape[0], e2_all.shape[0]
    pl = plan(b1, b2, n1, n2, D)
    scale, bias = torch.exp(_e32(log_scale)), _e32(bias)
    n = n1 if kind == "n1_normaliser" else min(n1, n2)
    g = _e32(1.0 if kind == "grad_out_ignored" else grad_out)
    gn = g / _e32(2.0 * n)
    f = gn * scale
    out = {}
    for dirn, (Q, K, lq_all, lk_all) in enumerate(((e2_loc, e1_all, lse_row_all, lse_col_all), (e1_loc, e2_all, lse_col_all, lse_row_all))):
        S = _fscores(Q, K, scale, bias)
        nq, nk = S.shape
        qi, kj = q_offset + torch.arange(nq), torch.arange(nk)
        q_in = qi < n
        k_in = torch.ones(nk, dtype=torch.bool) if kind == "finite_lse_k" else kj < n
        lq = lq_all.to(F32)[qi.clamp(max=lq_all.shape[0] - 1)][:, None]
        lk = lk_all.to(F32)[kj.clamp(max=lk_all.shape[0] - 1)][None, :]
        zero = torch.zeros_like(S)
        G = torch.where(q_in[:, None].expand_as(S), torch.exp(S - lq), zero)
        G = G + torch.where(k_in[None, :].expand_as(S), torch.exp(S - lk), zero)
        if kind != "no_minus_2_delta":
            pos = qi if kind != "local_positive" else torch.arange(nq)
            G = G - 2.0 * ((pos[:, None] == kj[None, :]) & q_in[:, None]).to(F32)
        if dirn == 0 and kind == "skip_key":
            G[_qrows(nq, qtile), at] = 0.0
        if dirn == 0 and kind == "double_key":
            G[_qrows(nq, qtile), at] *= 2.0
        dq, ds, db = _emulate_products(G, S, K, pl, f, gn, bias, kind)
        if dirn == 0:
            out.update(dE2=dq, dscale=ds, dbias=db)
        else:
            out.update(dE1=dq)
    return out


def emulate_sigmoid_forward(e1_loc, e2_loc, e1_all, e2_all, q_offset, log_scale, bias, defect=None):
    kind = defect[0] if defect else None
    scale, bias = torch.exp(_e32(log_scale)), _e32(bias)
    Z = _fscores(e2_loc, e1_all, scale, bias, sign=-1.0).to(F64)
    nq, nk = Z.shape
    diag = (q_offset + torch.arange(nq))[:, None] == torch.arange(nk)[None, :]
    u = torch.where(diag, -Z if kind == "sigmoid_diag_sign" else Z, -Z)
    soft = torch.where(u > 0, u + torch.log1p(torch.exp(-u.clamp(min=0))), torch.log1p(torch.exp(u.clamp(max=0))))
    return dict(loss=(soft.sum() / (float(nk) * float(nk))).to(F32))


def emulate_sigmoid_backward(e1_loc, e2_loc, e1_all, e2_all, q_offset, log_scale, bias, grad_out, defect=None):
    kind = defect[0] if defect else None
    (b1, D), b2, n = e1_loc.shape, e2_loc.shape[0], e1_all.shape[0]
    pl = plan(b1, b2, n, n, D)
    scale, bias = torch.exp(_e32(log_scale)), _e32(bias)
    g = _e32(1.0 if kind == "grad_out_ignored" else grad_out)
    gn = g / (_e32(float(n)) * _e32(float(n)))
    out = {}
    for dirn, (Q, K) in enumerate(((e2_loc, e1_all), (e1_loc, e2_all))):
        S = _fscores(Q, K, scale, bias, sign=-1.0)
        diag = (q_offset + torch.arange(S.shape[0]))[:, None] == torch.arange(S.shape[1])[None, :]
        z = torch.where(diag, -1.0 if kind == "sigmoid_diag_sign" else 1.0, -1.0).to(F32)
        sg = 1.0 / (1.0 + torch.exp(-(z * S)))
        dq, ds, db = _emulate_products(z * sg, S, K, pl, -gn * scale, gn, bias, kind)
        if dirn == 0:
            out.update(dE2=dq, dscale=ds, dbias=db)
        else:
            out.update(dE1=dq)
    return out


def emulate_rank(e1, e2, defect=None):
    x = e2.to(F32) @ e1.to(F32).T
    d = x.diagonal()[:, None]
    hit = (x >= d) if defect and defect[0] == "rank_ge" else (x > d)
    hit[torch.arange(x.shape[0]), torch.arange(x.shape[0])] = False
    return hit.sum(1)


# ------------------------------------------------------------------------------------------------------------ the cases
def _single(n1, n2, D):
    return make_case(n1, n2, n1, n2, D, 0)


# name -> (case, plan features the case claims to reach: ksplit, keys_per_split, keys in the last split of the longer key set)
CASES = {}
for _n in (1, 5, 31, 32, 33):
    for _d in (1, 5, 8, 12):
        CASES[f"n{_n}_d{_d}"] = (_single(_n, _n, _d), (1, 128, _n))
CASES.update({
    "n129_d64": (_single(129, 129, 64), (2, 128, 1)),
    "n300_d100": (_single(300, 300, 100), (3, 128, 44)),
    "n300_d130": (_single(300, 300, 130), (3, 128, 44)),
    "r70x45_d32": (_single(70, 45, 32), (1, 128, 70)),
    "r45x200_d32": (_single(45, 200, 32), (2, 128, 72)),
    "sh2100_o0": (make_case(32, 32, 2100, 2100, 128, 0), (17, 128, 52)),
    "sh2100_o1056": (make_case(32, 32, 2100, 2100, 128, 1056), (17, 128, 52)),
    "sh2100_o2068": (make_case(32, 32, 2100, 2100, 128, 2068), (17, 128, 52)),
    "sh8187_o4000": (make_case(40, 40, 8187, 8187, 64, 4000), (64, 128, 123)),
    "sh300_b40x24": (make_case(40, 24, 300, 300, 64, 130), (3, 128, 44)),
    "w33_d288": (_single(33, 33, 288), (2, 32, 1)),
    "w129_d320": (_single(129, 129, 320), (5, 32, 1)),
    "w300_d1024": (_single(300, 300, 1024), (10, 32, 12)),
    # the cap of 64 binds in make_plan (65 tiles), after which 64-key splits leave 33 of them: five trips of the folds
    "wsh2080_d512": (make_case(32, 32, 2080, 2080, 512, 1024), (33, 64, 32)),
    # 64 splits of one tile each at a wide width, the last one ragged
    "wsh2040_d512": (make_case(32, 32, 2040, 2040, 512, 2008), (64, 32, 24)),
})
SIGMOID_CASES = ("n33_d8", "n129_d64", "n300_d100", "sh2100_o1056", "w129_d320", "w300_d1024")
RANK_CASES = tuple((n, d) for n in (33, 300, 1000) for d in (8, 100, 512))
GRAD_OUTS = (1.0, 0.37, -2.5)


def plan_features(case):
    pl = plan(case.b1, case.b2, case.n1, case.n2, case.D)
    maxk = max(case.n1, case.n2)
    return (pl.ksplit, pl.keys_per_split, maxk - (pl.ksplit - 1) * pl.keys_per_split)


def grad_out_of(name, family):
    """1, 0.37 and -2.5 dealt over the (case, family) pairs"""
    return GRAD_OUTS[(list(CASES).index(name) + FAMILIES.index(family)) % 3]


def softmax_refs(inp, case, grad_out, device="cpu"):
    """-> (operands on `device`, forward reference, the fp32 log-sum-exps of every gathered row, backward reference)"""
    e1a, e2a = inp["e1_all"].to(device), inp["e2_all"].to(device)
    o = case.q_offset
    e1l, e2l = e1a[o:o + case.b1], e2a[o:o + case.b2]
    args = (e1l, e2l, e1a, e2a, o, inp["log_scale"], inp["bias"])
    fref = softmax_forward_ref(*args)
    if o == 0 and case.b1 == case.n1 and case.b2 == case.n2:
        lr, lc = fref["lse_row"], fref["lse_col"]
    else:
        lr, lc = lse_all_ref(e1a, e2a, inp["log_scale"], inp["bias"])
    lr, lc = lr.to(F32), lc.to(F32)
    bref = softmax_backward_ref(*args, lr, lc, grad_out)
    return args, fref, (lr, lc), bref


def rank_rule(got, e1, e2, normalised, ref=None):
    """the rank assertion: -> (rows whose rank is decided by the score bound and differs, rows left undecided, rows); `ref`: the
    fp64 ranks of another reference to hold `got` to instead of rank_ref's"""
    a, q = _f64(e1, e2)
    if normalised:
        a, q = a / a.norm(dim=-1, keepdim=True), q / q.norm(dim=-1, keepdim=True)
    own, x = rank_ref(a, q)
    ref = own if ref is None else torch.as_tensor(ref).to(own.device).to(torch.int64)
    decided = rank_decided_rows(x, rank_score_bound(a, q, normalised))
    got = torch.as_tensor(got).to(ref.device).to(torch.int64)
    return int(((got != ref) & decided).sum()), int((~decided).sum()), x.shape[0]
