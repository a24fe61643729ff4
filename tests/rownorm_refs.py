"""Plain torch references for the row kernels of csrc/rowops.hip (msn_layernorm_fwd / _bwd and their bf16 and plane forms,
msn_l2norm_fwd / _bwd, msn_time_embed_fwd / _bwd): every output in fp64 from the fp32 operands as given, a per-element error bound
derived from the kernels' rounding steps, mirrors of the launch rules, an fp32 emulation of the kernels' arithmetic order with one
switch per injected defect, and the input families.  Shared by tests/test_rownorm_pinned_gpu.py (the kernels against these, on the
card) and tests/test_rownorm_refs_cpu.py (the emulation against the bounds and every defect against the comparison, on any
machine).  Nothing here imports the package under test.

Launch rules (mirrored by ln_plan / te_plan).  A row of `cols` floats (a multiple of 4) is owned by LPR = 4 / 16 / 64 lanes of one
wave (up to 64 / 256 / 1024 columns); a lane holds nch = ceil(cols / 4 / LPR) <= 4 live 16-byte chunks.  A workgroup takes
RG = 256 / LPR rows per pass.  The forward runs min(ceil(rows / RG), 2048) workgroups, the backward min(ceil(rows / 4 RG), 512);
each backward workgroup publishes one slab of column partial sums, so slabs = the backward grid and a thread accumulates
rounds = ceil(rows / (slabs RG)) rows.

The bounds.  u = 2^-24.  Every bound is MARGIN times a first-order worst case: u times the matching sum of absolute terms,
evaluated in fp64, plus the propagated error of the quantities it is built from.  lg = log2(LPR).
  mean      per lane sum4 (a two-level tree), a sequential add over the nch chunks, lg shuffle steps: ks = 2 + nch + lg roundings
            on the longest path; inv_n = fl(1 / n) and the product with it round twice more.
                dmu = u (ks + 2) mean|x|
  variance  a = fl(x - mu^) carries u |a| and the shift dmu; sum_i a_i = 0, so the shift enters sum a^2 only as n dmu^2 -- second
            order, but on rows offset by 1000 sigma it is 6 u of the variance and is kept.  The squares: one product, three adds
            inside the chunk, the chain and the shuffles: kq = 4 + nch + lg; 2 u from a itself, two roundings for inv_n, one for
            + eps.  A square below the normal range may flush: the absolute floor FLOOR = 2^-126.
                dve = dmu^2 + u (kq + 6) (var + dmu^2 + eps) + FLOOR
  rstd      rsqrtf is allowed 2 ulp = RSQRT_U u = 4 u relative; dve enters through d rsqrt(v) / dv = -rstd^3 / 2.
                drstd = rstd^3 dve / 2 + 4 u rstd
            (on a constant row var = 0, ve = eps and dve ~ dmu^2 <= 1e-2 eps for |x| <= 100: the first order holds.)
  y         (x - mu^) rs^ gamma + beta: dmu enters multiplied by rstd |gamma|, drstd by |a gamma|; the subtraction and the two
            products round (3 u |xhat gamma|), the last add rounds (u |y|).
                dy = |gamma| (rstd dmu + |a| drstd + 3 u |xhat|) + u |y| + FLOOR
            On a constant row a = 0 and y = beta exactly in fp64; the bound left is |gamma| rstd dmu + u |beta|.
  backward  is a launch of its own: mean and rstd are fp32 INPUTS, and the reference is the gradient those inputs define,
            xhat = (x - mean) rstd, gd = gamma dy, m1 = mean(gd), m2 = mean(gd xhat), dx = rstd (gd - m1 - xhat m2) [+ add].
            xhat^ carries 2 u, gd^ u.  m1: k1 = 3 + nch + lg (own rounding, sum4, chain, shuffles) and 2 for inv_n; m2: the terms
            carry 4 u, three adds in dot4: k2 = 7 + nch + lg.
                dm1 = u (k1 + 2) mean|gd|          dm2 = u (k2 + 2) mean|gd xhat|
                ddx = rstd (3 u |gd| + 2 u |m1| + 4 u |xhat m2| + dm1 + |xhat| dm2) + u |dx| + FLOOR   (+ u |dx + add| with add)
  columns   dgamma = sum_r dy xhat, dbeta = sum_r dy, and the column sums of dx.  A term passes through the per-thread chain over
            the workgroup's row rounds, the RG-term sequential LDS sum, then sum_slabs_kernel: each of 16 groups adds its
            ceil(slabs / 16) slabs as four partial sums (ceil(./4) + 3 for the remainder that joins the first) and a two-level
            tree, and the sixteen groups are added one after the other:
                kcol = rounds + RG + ceil(ceil(slabs / 16) / 4) + 3 + 2 + 16
                ddgamma = u (3 + kcol) sum_r |dy xhat|    ddbeta = u kcol sum_r |dy|    dcolsum = sum_r ddx + u kcol sum_r |dx|
  l2norm    q = sum x^2 (kq as above), nrm = sqrtf(q) (correctly rounded; 1 u allowed), y = x / nrm and inv = 1 / nrm (u each):
                rho = u (kq / 2 + 2)      dy = (rho + u) |y| + FLOOR      dinv = (rho + u) |inv|
            A zero row gives 0 / 0 = NaN and inv = inf in the reference and in the kernel (no epsilon, as the model has none).
            Backward (y, inv are inputs): s = <y, dy> with ksd = 4 + nch + lg, dx = inv (dy - y s):
                dds = u ksd sum|y dy|     ddx = inv (|y| dds + 2 u |y s| + u |dy|) + u |dx| + FLOOR
  time      out = x w + bw + (c even ? sin : cos)(t omega[c / 2]) [+ band]: ang = fl(t omega) is off by u |t omega|, which enters
            the sine with slope <= 1; sinf / cosf are allowed 2 ulp of a value <= 1 = TRIG_U u = 4 u; the adds round.
                dout = u (|t omega| + 4 + |x w| + |x w + bw| + |x w + bw + trig| [+ |out|])
            Backward: one workgroup per sample; a thread adds chain = ceil(per_band / groups) tokens of a band (groups =
            256 / min(e, 256) row groups), the groups are added one after the other; the finish kernel sums the B samples as
            sum_slabs_kernel sums slabs (kfin = ceil(ceil(B / 16) / 4) + 3 + 2 + 16), and dbw adds the nband rows of dband:
                ddband = u (chain + groups + kfin) sum|dy|     ddbw = ddband summed + u nband sum|dy|
                ddw    = u (1 + nband chain + groups + kfin) sum|dy x|
The contract on magnitude is the one torch's fp32 layer_norm has: the squares of a row and their sum stay finite in fp32 (the huge
family sits at 1e15).
MARGIN = 2 covers what is not modelled: second-order terms and the choice between a fused and an unfused multiply-add, which the
compiler makes.  It was fixed before any card was involved, as in tests/infonce_refs.py: the fp32 emulation below (same lane,
chunk, shuffle, row-round, LDS and slab order; torch's fp32 rsqrt, sin and cos) reaches at most 0.49 of any bound on every case and
family of tests/test_rownorm_refs_cpu.py -- the time embedding at 9000 rad, whose bound is the one rounding of the angle that does
happen; LayerNorm's y reaches 0.44, the L2 backward 0.46, everything else stays below 0.4 -- and a worst case that is a sum of moduli is not reached by rounding errors of mixed sign.  A ratio above 1 on the card is a finding,
not a reason to raise it.

Largest error / bound ratios measured on an MI355X (tests/test_rownorm_pinned_gpu.py, every case; the gate is 1):
    layernorm         mean   rstd   y      dx     dx+add dgamma dbeta  colsum
    normal            0.162  0.127  0.443  0.238  0.258  0.045  0.037  0.033
    offset            0.145  0.092  0.143  0.172  0.160  0.047  0.038  0.027
    constant          0.138  0.032  0.138  0.156  0.165  exact  0.035  0.029
    wide              0.120  0.117  0.413  0.180  0.387  0.056  0.036  0.036
    tiny              0.088  0.034  0.251  0.136  0.167  0.042  0.036  0.031
    huge              0.083  0.082  0.369  0.176  0.000  0.044  0.037  0.033
    integer           0.091  0.123  0.099  0.148  0.279  0.043  exact  0.034
    normal, strided   0.117  0.108  0.427  0.244  -      0.045  0.037  -
    class-row view    0.037  0.072  0.402  0.153  -      0.030  0.022  -
    l2norm            y      inv    dx              time_embed      out    dw     dbw    dband
    normal            0.198  0.156  0.464           t = 0           0.293  0.042  0.037  0.037
    offset            0.145  0.133  0.164           |t| <= 100      0.434  0.042  0.029  0.036
    constant          0.156  0.119  0.147           |t| <= 9000     0.494  0.040  0.029  0.037
    wide              0.204  0.171  0.464
    tiny              0.147  0.115  0.399
    huge              0.166  0.130  0.406
    integer           0.110  0.106  0.247
The card and the emulation agree to the third digit on the maxima (y 0.443 at 1025 x 68, the time embedding 0.494 at 9000 rad, where
the rounding of the angle alone is half the bound).  The column sums sit near 0.04: their bound counts the longest chain of adds
(up to 100 at RG = 64), which roundings of mixed sign do not fill.  On the cases past the forward's cap (131137 x 64, 32785 x 68,
8197 x 260) no ratio exceeds 0.36 (LayerNorm) and 0.47 (L2); no launch left a NaN of the poisoned scratch in a result or wrote into a
gap of a strided output.
"""
import math
from types import SimpleNamespace

import torch

F32, F64 = torch.float32, torch.float64
U = 2.0 ** -24               # unit roundoff of fp32
MARGIN = 2.0                 # everything not modelled (see the module docstring)
FLOOR = 2.0 ** -126          # absolute floor: squares and products that flush
RSQRT_U = 4.0                # rsqrtf: 2 ulp, in units of u
TRIG_U = 4.0                 # sinf / cosf: 2 ulp of a value <= 1, in units of u
NCH = 4                      # 16-byte chunks per lane
LN_FAMILIES = ("normal", "offset", "constant", "wide", "tiny", "huge", "integer")
TE_REGIMES = ("zero", "hundred", "ninethousand")


def gen(seed):
    return torch.Generator().manual_seed(seed)


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------------------ the launch rules
def pick_lpr(cols):
    chunks = cols // 4
    return 4 if chunks <= 4 * NCH else 16 if chunks <= 16 * NCH else 64


def ln_grid(rows, lpr):
    return min(cdiv(rows, 256 // lpr), 2048)


def ln_bwd_grid(rows, lpr):
    return min(cdiv(rows, 4 * (256 // lpr)), 512)


def ln_plan(rows, cols):
    """-> lpr, rg (rows per workgroup pass), nch (live chunks per lane), lg, grid and passes of the forward (passes = loop
    iterations of the busiest thread), slabs and rounds of the backward, the backward's workspace bytes."""
    assert cols % 4 == 0 and 0 < cols <= 64 * NCH * 4 and rows > 0
    lpr = pick_lpr(cols)
    rg = 256 // lpr
    grid, slabs = ln_grid(rows, lpr), ln_bwd_grid(rows, lpr)
    return SimpleNamespace(lpr=lpr, rg=rg, nch=cdiv(cols // 4, lpr), lg=int(math.log2(lpr)), grid=grid, passes=cdiv(rows, grid * rg),
                           slabs=slabs, rounds=cdiv(rows, slabs * rg), ws_bytes=4 * 2 * cols * slabs,
                           padded=cdiv(cols // 4, lpr) * lpr * 4)


def _finish_depth(n):
    """sum_slabs_kernel / time_embed_bwd_finish_kernel over n partials: the longest chain of adds a term passes through"""
    return cdiv(cdiv(n, 16), 4) + 3 + 2 + 16


def finish_trips(n):
    """(4-way unrolled trips, single trips) of thread group 0 over n partials: `for (; b + 48 < n; b += 64)` then `for (; b < n; b += 16)`"""
    b, four, one = 0, 0, 0
    while b + 48 < n:
        four, b = four + 1, b + 64
    while b < n:
        one, b = one + 1, b + 16
    return four, one


def te_plan(B, T, e, nband):
    cpt = min(e, 256)
    groups = 256 // cpt
    per_band = T // nband
    total = B * T * e
    grid = min(cdiv(total, 256), 4096)
    return SimpleNamespace(cpt=cpt, groups=groups, per_band=per_band, col_passes=cdiv(e, cpt), chain=cdiv(per_band, groups),
                           idle_groups=max(0, groups - per_band), grid=grid, passes=cdiv(total, grid * 256), finish=finish_trips(B),
                           kfin=_finish_depth(B), ws_bytes=4 * B * e * (nband + 1))


# ------------------------------------------------------------------------------------------------------------ fp64 references
def _f64(*ts):
    return tuple(None if t is None else torch.as_tensor(t).to(F64) for t in ts)


def ln_forward_ref(x, gamma, beta, eps):
    """-> dict(mean (rows), rstd (rows), y (rows, cols)) with the bounds under "b_" + name, fp64, on x's device"""
    x, g, b = _f64(x, gamma, beta)
    rows, cols = x.shape
    p = ln_plan(rows, cols)
    mu = x.mean(1)
    a = x - mu[:, None]
    var = (a * a).mean(1)
    rstd = (var + eps).rsqrt()
    xh = a * rstd[:, None]
    y = xh * g + b
    dmu = U * (2 + p.nch + p.lg + 2) * x.abs().mean(1)
    dve = dmu ** 2 + U * (4 + p.nch + p.lg + 6) * (var + dmu ** 2 + eps) + FLOOR
    drs = 0.5 * rstd ** 3 * dve + RSQRT_U * U * rstd
    dy = g.abs() * (rstd[:, None] * dmu[:, None] + a.abs() * drs[:, None] + 3 * U * xh.abs()) + U * y.abs() + FLOOR
    return dict(mean=mu, rstd=rstd, y=y, b_mean=MARGIN * dmu + FLOOR, b_rstd=MARGIN * drs, b_y=MARGIN * dy)


def ln_backward_ref(dy, x, mean, rstd, gamma, add=None):
    """The gradient msn_layernorm_bwd defines from its inputs (the fp32 mean and rstd included)
    -> dict(dx (with `add` when given), dgamma, dbeta, colsum: the column sums of dx) with the bounds under "b_" + name."""
    dy, x, mean, rstd, g, add = _f64(dy, x, mean, rstd, gamma, add)
    rows, cols = x.shape
    p = ln_plan(rows, cols)
    rs = rstd[:, None]
    xh = (x - mean[:, None]) * rs
    gd = dy * g
    m1, m2 = gd.mean(1, keepdim=True), (gd * xh).mean(1, keepdim=True)
    dx = rs * (gd - m1 - xh * m2)
    dm1 = U * (3 + p.nch + p.lg + 2) * gd.abs().mean(1, keepdim=True)
    dm2 = U * (7 + p.nch + p.lg + 2) * (gd * xh).abs().mean(1, keepdim=True)
    ddx = rs * (3 * U * gd.abs() + 2 * U * m1.abs() + 4 * U * (xh * m2).abs() + dm1 + xh.abs() * dm2) + U * dx.abs() + FLOOR
    kcol = p.rounds + p.rg + _finish_depth(p.slabs)
    t = dy * xh
    out = dict(dx=dx, dgamma=t.sum(0), dbeta=dy.sum(0), colsum=dx.sum(0), b_dx=MARGIN * ddx, kcol=kcol,
               b_dgamma=MARGIN * U * (3 + kcol) * t.abs().sum(0) + FLOOR, b_dbeta=MARGIN * U * kcol * dy.abs().sum(0) + FLOOR,
               b_colsum=MARGIN * (ddx.sum(0) + U * kcol * dx.abs().sum(0)))
    return out if add is None else ln_add_ref(out, add)


def ln_add_ref(bref, add):
    """the reference of the same launch with the residual-branch gradient `add` fused in, from the one without: dx + add rounds once"""
    (add,) = _f64(add)
    dx = bref["dx"] + add.to(bref["dx"].device)
    b_dx = bref["b_dx"] + MARGIN * U * dx.abs()
    return dict(bref, dx=dx, b_dx=b_dx, colsum=dx.sum(0), b_colsum=b_dx.sum(0) + MARGIN * U * bref["kcol"] * dx.abs().sum(0))


def l2_forward_ref(x):
    """-> dict(y, inv) + bounds; a zero row is NaN / inf as x / x.norm() is"""
    (x,) = _f64(x)
    p = ln_plan(*x.shape)
    nrm = (x * x).sum(1).sqrt()
    y, inv = x / nrm[:, None], 1.0 / nrm
    rho = U * ((4 + p.nch + p.lg) / 2 + 2)
    return dict(y=y, inv=inv, b_y=MARGIN * ((rho + U) * y.abs() + FLOOR), b_inv=MARGIN * (rho + U) * inv.abs())


def l2_backward_ref(dy, y, inv):
    dy, y, inv = _f64(dy, y, inv)
    p = ln_plan(*y.shape)
    s = (y * dy).sum(1, keepdim=True)
    iv = inv[:, None]
    dx = iv * (dy - y * s)
    dds = U * (4 + p.nch + p.lg) * (y * dy).abs().sum(1, keepdim=True)
    ddx = iv.abs() * (y.abs() * dds + 2 * U * (y * s).abs() + U * dy.abs()) + U * dx.abs() + FLOOR
    return dict(dx=dx, b_dx=MARGIN * ddx)


def _band_rows(T, nband, device=None):
    return torch.arange(T, device=device) // (T // nband)


def te_forward_ref(x, t, w, bw, omega, band=None):
    """out[b,t,c] = x[b,t] w[c] + bw[c] + (c even ? sin : cos)(t[b,t] omega[c / 2]) + band[band(t)][c]  (the kernel's header)"""
    x, t, w, bw, om, band = _f64(x, t, w, bw, omega, band)
    e = w.numel()
    ang = t[:, :, None] * om.repeat_interleave(2)
    even = (torch.arange(e, device=x.device) % 2 == 0)
    trig = torch.where(even, torch.sin(ang), torch.cos(ang))
    lin = x[:, :, None] * w
    v1 = lin + bw
    v2 = v1 + trig
    out = v2
    d = ang.abs() + TRIG_U + lin.abs() + v1.abs() + v2.abs()
    if band is not None:
        out = v2 + band[_band_rows(x.shape[1], band.shape[0], x.device)][None]
        d = d + out.abs()
    return dict(out=out, b_out=MARGIN * U * d)


def te_backward_ref(dy, x, nband):
    """-> dict(dw (e), dbw (e), dband (nband, e)) + bounds"""
    dy, x = _f64(dy, x)
    B, T, e = dy.shape
    p = te_plan(B, T, e, nband)
    seg = dy.view(B, nband, T // nband, e)
    dband, aband = seg.sum((0, 2)), seg.abs().sum((0, 2))
    dx = dy * x[:, :, None]
    kb = p.chain + p.groups + p.kfin
    return dict(dw=dx.sum((0, 1)), dbw=dband.sum(0), dband=dband, b_dband=MARGIN * U * kb * aband + FLOOR,
                b_dbw=MARGIN * U * (kb + nband) * aband.sum(0) + FLOOR,
                b_dw=MARGIN * U * (1 + nband * p.chain + p.groups + p.kfin) * dx.abs().sum((0, 1)) + FLOOR)


# ------------------------------------------------------------------------------------------------------------ the comparison
def worst_ratio(got, ref, bound):
    """max |got - ref| / bound.  An element equal to its reference (infinities included) or NaN where the reference is NaN counts 0
    whatever its bound; a NaN against a number, and an error against a zero bound, count inf."""
    got = torch.as_tensor(got).detach().to(F64).to(ref.device)
    if got.numel() == 0:
        return 0.0
    same = (got == ref) | (torch.isnan(got) & torch.isnan(ref))
    r = (got - ref).abs() / bound
    r = torch.where(same, torch.zeros_like(r), r)
    r = torch.where(torch.isnan(r), torch.full_like(r, math.inf), r)
    return float(r.max())


def ratios(got, ref):
    return {k: worst_ratio(v, ref[k], ref["b_" + k]) for k, v in got.items()}


def failures(got, ref):
    r = ratios(got, ref)
    return [f"{k} at {v:.3g} of its bound" for k, v in r.items() if not v <= 1.0], r


# ------------------------------------------------------------------------------------------------------------ input families
def _seed(family, rows, cols):
    return 7919 * rows + 31 * cols + 1000003 * LN_FAMILIES.index(family)


def ln_inputs(family, rows, cols):
    """-> dict(x, dy, add (rows, cols), gamma, beta (cols)) fp32 on the CPU"""
    assert family in LN_FAMILIES
    g = gen(_seed(family, rows, cols))
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    gamma, beta = rn(cols) + 1, rn(cols)
    dy, add = rn(rows, cols), rn(rows, cols)
    if family == "normal":
        x = rn(rows, cols) * 2 + 0.5
    elif family == "offset":                                   # 100 and 1000 sigma away from zero, row by row
        off = torch.where(torch.arange(rows) % 2 == 0, 100.0, 1000.0).to(F64)
        x = rn(rows, cols) + off[:, None]
    elif family == "constant":                                 # every entry of a row equal and non-zero
        c = (0.5 + 99.5 * torch.rand(rows, generator=g, dtype=F64)) * torch.where(torch.rand(rows, generator=g) < 0.5, -1.0, 1.0)
        x = c[:, None].expand(rows, cols).clone()
    elif family == "wide":                                     # twelve octaves of magnitude, random signs
        x = torch.exp2(12 * torch.rand(rows, cols, generator=g, dtype=F64) - 6) * torch.where(torch.rand(rows, cols, generator=g) < 0.5, -1.0, 1.0)
    elif family == "tiny":
        x = rn(rows, cols) * 1e-15
    elif family == "huge":                                     # squares ~1e31, their sum over 1024 columns < 3.4e38
        x = rn(rows, cols) * 1e15
    else:                                                      # small integers: every sum is exact
        ri = lambda *s: torch.randint(-4, 5, s, generator=g).to(F64)
        x, dy, add = ri(rows, cols), ri(rows, cols), ri(rows, cols)
        gamma, beta = torch.ones(cols, dtype=F64), torch.zeros(cols, dtype=F64)
    f = lambda v: v.to(F32).contiguous()
    return dict(x=f(x), dy=f(dy), add=f(add), gamma=f(gamma), beta=f(beta))


def l2_inputs(family, rows, cols):
    """as ln_inputs; from three rows on, row 1 is a zero row between ordinary rows"""
    inp = ln_inputs(family, rows, cols)
    if family == "constant":
        inp["dy"] = inp["dy"] + 0.5
    if rows >= 3:
        inp["x"][1] = 0.0
    return dict(x=inp["x"], dy=inp["dy"])


def te_inputs(B, T, e, nband, regime, integer=False, norm=17945.14):
    assert regime in TE_REGIMES and e % 2 == 0 and T % nband == 0
    g = gen(131 * B + 17 * T + 7 * e + nband + 1009 * TE_REGIMES.index(regime))
    top = dict(zero=0.0, hundred=100.0, ninethousand=9000.0)[regime]
    t = (2 * torch.rand(B, T, generator=g) - 1) * top            # negative times included
    if integer:
        x = torch.randint(-4, 5, (B, T), generator=g).float()
        dy = torch.randint(-4, 5, (B, T, e), generator=g).float()
    else:
        x, dy = torch.randn(B, T, generator=g), torch.randn(B, T, e, generator=g)
    w, bw = torch.randn(e, generator=g), torch.randn(e, generator=g)
    band = torch.randn(nband, e, generator=g) if nband > 1 else None
    omega = torch.exp(torch.arange(0, e, 2).float() * (-math.log(norm) / e))
    return dict(x=x, t=t, w=w, bw=bw, omega=omega, band=band, dy=dy)


# ------------------------------------------------------------------------------------------------------------ the emulation
DEFECTS = ("one_pass_variance", "padding_in_variance", "padded_n", "eps_dropped", "m2_dropped", "add_ignored", "last_slab_dropped",
           "lds_group_dropped", "stride_as_cols", "band_edge_shifted", "l2_no_projection", "sincos_swapped", "omega_index")


def _e32(v):
    return torch.as_tensor(v, dtype=F32)


def _restride(t, defect):
    """stride_as_cols: row r is read at r * cols of the buffer the view lives in, not at r * ld"""
    if t is None or defect != "stride_as_cols":
        return t
    return t.as_strided(t.shape, (t.shape[1], 1), t.storage_offset())


def _lanes(x, lpr):
    """(rows, cols) -> (rows, NCH, lpr, 4): chunk lr + k lpr of the row in [:, k, lr], zeros past cols; live (NCH, lpr)"""
    rows, cols = x.shape
    pad = torch.zeros(rows, NCH * lpr * 4, dtype=F32)
    pad[:, :cols] = x
    live = (torch.arange(NCH * lpr) * 4 < cols).view(NCH, lpr)
    return pad.view(rows, NCH, lpr, 4), live


def _group_sum(s, lpr):
    """the xor butterfly over the lpr lanes of a row (every lane ends with the same bits)"""
    idx, o = torch.arange(lpr), lpr // 2
    while o:
        s = s + s[:, idx ^ o]
        o >>= 1
    return s[:, 0]


def _sum4(v):
    return (v[..., 0] + v[..., 1]) + (v[..., 2] + v[..., 3])


def _dot4(a, b):
    return ((a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]) + a[..., 3] * b[..., 3]


def _row_sum(v, lpr, f):
    """per lane: s = 0; s += f(chunk k) over the NCH chunks; then the butterfly"""
    s = torch.zeros(v.shape[0], lpr, dtype=F32)
    for k in range(NCH):
        s = s + f(k)
    return _group_sum(s, lpr)


def emulate_ln_forward(x, gamma, beta, eps, defect=None):
    x = _restride(x, defect).to(F32)
    rows, cols = x.shape
    p = ln_plan(rows, cols)
    v, live = _lanes(x, p.lpr)
    inv_n = _e32(1.0) / _e32(float(p.padded if defect == "padded_n" else cols))
    mu = _row_sum(v, p.lpr, lambda k: _sum4(v[:, k])) * inv_n
    one_pass = defect == "one_pass_variance"

    def squares(k):
        a = v[:, k] if one_pass else v[:, k] - mu[:, None, None]
        t = _dot4(a, a)
        return t if defect == "padding_in_variance" else torch.where(live[k], t, torch.zeros_like(t))
    var = _row_sum(v, p.lpr, squares) * inv_n
    if one_pass:
        var = var - mu * mu
    rs = torch.rsqrt(var + _e32(0.0 if defect == "eps_dropped" else eps))
    y = (x - mu[:, None]) * rs[:, None] * gamma.to(F32) + beta.to(F32)
    return dict(mean=mu, rstd=rs, y=y)


def _block_partials(c, p, defect):
    """column partial sums of one workgroup per slab: the per-thread chain over its row rounds, then the RG-term LDS sum"""
    rows, cols = c.shape
    pad = torch.zeros(p.rounds * p.slabs * p.rg, cols, dtype=F32)
    pad[:rows] = c
    pad = pad.view(p.rounds, p.slabs, p.rg, cols)
    acc = torch.zeros(p.slabs, p.rg, cols, dtype=F32)
    for j in range(p.rounds):
        acc = acc + pad[j]
    s = torch.zeros(p.slabs, cols, dtype=F32)
    for k in range(p.rg - (1 if defect == "lds_group_dropped" else 0)):
        s = s + acc[:, k]
    return s


def _sum_slabs(part, defect=None):
    """sum_slabs_kernel (and the finish kernel of time_embed): 16 groups, four partial sums each, added in a fixed order"""
    ns = part.shape[0] - (1 if defect == "last_slab_dropped" else 0)
    zero = torch.zeros(part.shape[1:], dtype=F32)
    t = zero
    for g in range(16):
        s0, s1, s2, s3 = zero, zero, zero, zero
        k = g
        while k + 48 < ns:
            s0, s1, s2, s3 = s0 + part[k], s1 + part[k + 16], s2 + part[k + 32], s3 + part[k + 48]
            k += 64
        while k < ns:
            s0 = s0 + part[k]
            k += 16
        t = t + ((s0 + s1) + (s2 + s3))
    return t


def emulate_ln_backward(dy, x, mean, rstd, gamma, add=None, defect=None):
    dy, x, add = (None if t is None else _restride(t, defect).to(F32) for t in (dy, x, add))
    rows, cols = x.shape
    p = ln_plan(rows, cols)
    gm, mean, rstd = gamma.to(F32), mean.to(F32), rstd.to(F32)
    xh = (x - mean[:, None]) * rstd[:, None]
    gd = dy * gm
    vg, _ = _lanes(gd, p.lpr)
    vx, _ = _lanes(xh, p.lpr)
    inv_n = _e32(1.0) / _e32(float(cols))
    m1 = _row_sum(vg, p.lpr, lambda k: _sum4(vg[:, k])) * inv_n
    m2 = _row_sum(vg, p.lpr, lambda k: _dot4(vg[:, k], vx[:, k])) * inv_n
    inner = gd - m1[:, None]
    if defect != "m2_dropped":
        inner = inner - xh * m2[:, None]
    dx = rstd[:, None] * inner
    if add is not None and defect != "add_ignored":
        dx = dx + add
    cols_of = lambda c: _sum_slabs(_block_partials(c, p, defect), defect)
    return dict(dx=dx, dgamma=cols_of(dy * xh), dbeta=cols_of(dy), colsum=cols_of(dx))


def emulate_l2_forward(x, defect=None):
    x = _restride(x, defect).to(F32)
    p = ln_plan(*x.shape)
    v, _ = _lanes(x, p.lpr)
    nrm = torch.sqrt(_row_sum(v, p.lpr, lambda k: _dot4(v[:, k], v[:, k])))
    return dict(y=x / nrm[:, None], inv=_e32(1.0) / nrm)


def emulate_l2_backward(dy, y, inv, defect=None):
    dy, y = _restride(dy, defect).to(F32), _restride(y, defect).to(F32)
    p = ln_plan(*y.shape)
    vy, _ = _lanes(y, p.lpr)
    vd, _ = _lanes(dy, p.lpr)
    s = _row_sum(vy, p.lpr, lambda k: _dot4(vy[:, k], vd[:, k]))
    inner = dy if defect == "l2_no_projection" else dy - y * s[:, None]
    return dict(dx=inv.to(F32)[:, None] * inner)


def _band_of(T, nband, defect):
    per = T // nband
    tok = torch.arange(T)
    if defect == "band_edge_shifted":                           # the last token of a band counted with the next one
        tok = tok + (tok % per == per - 1).long()
    return (tok // per).clamp(max=nband - 1)


def emulate_te_forward(x, t, w, bw, omega, band=None, defect=None):
    e = w.numel()
    c = torch.arange(e)
    om = omega[(c if defect == "omega_index" else c >> 1).clamp(max=e // 2 - 1)]
    ang = t.to(F32)[:, :, None] * om
    v = x.to(F32)[:, :, None] * w + bw
    first_sin = (c % 2 == 0) != (defect == "sincos_swapped")
    v = v + torch.where(first_sin, torch.sin(ang), torch.cos(ang))
    if band is not None:
        v = v + band[_band_of(x.shape[1], band.shape[0], defect)][None]
    return dict(out=v)


def emulate_te_backward(dy, x, nband, defect=None):
    dy, x = dy.to(F32), x.to(F32)
    B, T, e = dy.shape
    p = te_plan(B, T, e, nband)
    owner = _band_of(T, nband, defect)
    sx = torch.zeros(B, p.groups, e, dtype=F32)
    seg = []
    for k in range(nband):
        tok = torch.nonzero(owner == k).flatten()
        n = len(tok)
        d = torch.zeros(B, p.chain + 1, p.groups, e, dtype=F32)     # token i of the band -> chain step i // groups of group i % groups
        xx = torch.zeros(B, p.chain + 1, p.groups, dtype=F32)
        d.view(B, -1, e)[:, :n] = dy[:, tok]
        xx.view(B, -1)[:, :n] = x[:, tok]
        s = torch.zeros(B, p.groups, e, dtype=F32)
        for i in range(p.chain + 1):
            s = s + d[:, i]
            sx = sx + d[:, i] * xx[:, i, :, None]
        tot = torch.zeros(B, e, dtype=F32)
        for q in range(p.groups):
            tot = tot + s[:, q]
        seg.append(tot)
    sdx = torch.zeros(B, e, dtype=F32)
    for q in range(p.groups):
        sdx = sdx + sx[:, q]
    dband = torch.stack([_sum_slabs(s) for s in seg])
    return dict(dw=_sum_slabs(sdx), dbw=sequential_sum(dband), dband=dband)


def sequential_sum(rows):
    """fp32 sum of the rows of a matrix, one after the other from zero: how the finish kernel forms dbw from dband"""
    s = torch.zeros_like(rows[0])
    for r in rows:
        s = s + r
    return s


# ------------------------------------------------------------------------------------------------------------ the cases
def _rows_for_slabs(s, rg):
    return (s - 1) * 4 * rg + 1


def past_cap(rg):
    return 2048 * rg + rg + 1


# LayerNorm / L2: name -> (rows, cols, (lpr, forward passes, slabs, backward rounds)).  Per instantiation one main width with every
# row count of interest -- 1, RG - 1, RG + 1, the counts that make 15, 16, 17, 64 and 65 slabs, and the count past the forward's cap of
# 2048 workgroups -- and the other widths (dispatch edges, partly filled last chunks) at RG + 1 and at 17 slabs.
MAIN = {4: 64, 16: 68, 64: 260}
WIDTHS = {4: (4, 12, 60, 64), 16: (68, 200, 256), 64: (260, 384, 1020, 1024)}
LN_CASES = {}
for _lpr, _main in MAIN.items():
    _rg = 256 // _lpr
    for _rows in (1, _rg - 1, _rg + 1) + tuple(_rows_for_slabs(s, _rg) for s in (15, 16, 17, 64, 65)):
        LN_CASES[f"r{_rows}_c{_main}"] = (_rows, _main, (_lpr, 1, cdiv(_rows, 4 * _rg), 1 if _rows < _rg else 2 if _rows == _rg + 1 else 4))
    LN_CASES[f"r{past_cap(_rg)}_c{_main}"] = (past_cap(_rg), _main, (_lpr, 2, 512, 5))
    for _c in WIDTHS[_lpr]:
        if _c != _main:
            LN_CASES[f"r{_rg + 1}_c{_c}"] = (_rg + 1, _c, (_lpr, 1, 1, 2))
            LN_CASES[f"r{_rows_for_slabs(17, _rg)}_c{_c}"] = (_rows_for_slabs(17, _rg), _c, (_lpr, 1, 17, 4))
BIG_CASES = tuple(f"r{past_cap(256 // l)}_c{c}" for l, c in MAIN.items())
# every family at these (two or three widths per instantiation, RG + 1 rows: two workgroups, a ragged second one)
FAMILY_CASES = ("r65_c12", "r65_c60", "r65_c64", "r17_c68", "r17_c200", "r17_c256", "r5_c260", "r5_c1020", "r5_c1024")
# the bf16 and plane forms are tied to the fp32 kernel at the new edge widths, one row count past the forward's cap each
TIE_CASES = ((131137, 12), (32785, 68), (8197, 260), (8197, 1020))
EPS = (1e-5, 1e-6)


def ln_features(rows, cols):
    p = ln_plan(rows, cols)
    return (p.lpr, p.passes, p.slabs, p.rounds)


# time embedding: name -> (B, T, e, nband)
TE_CASES = {}
for _e in (2, 6, 64, 100, 256, 258, 384):
    for _nb in (1, 2, 3):
        TE_CASES[f"b3_t{_nb}_e{_e}_n{_nb}"] = (3, _nb, _e, _nb)              # a band of a single token
        TE_CASES[f"b5_t{6 * _nb}_e{_e}_n{_nb}"] = (5, 6 * _nb, _e, _nb)
for _b in (1, 15, 16, 17, 48, 49, 64, 65, 130):
    TE_CASES[f"b{_b}_t6_e64_n2"] = (_b, 6, 64, 2)
TE_CASES["b17_t242_e256_n2"] = (17, 242, 256, 2)                             # 1 053 184 elements > 4096 x 256: a second forward pass
TE_CASES["b2_t300_e64_n3"] = (2, 300, 64, 3)                                 # chains of 25 tokens per thread
TE_BIG = "b17_t242_e256_n2"
