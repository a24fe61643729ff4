"""Plain torch references for the bf16 attention kernels of csrc/attention_bf16.hip (msn_attention_bf16_fwd / _bwd): softmax
attention and its gradient in fp64 on the bf16 operands as given, per-element error bounds derived from the kernels' rounding
steps, an emulation of the kernels' arithmetic with switches that inject defects, and the input families.  Shared by
tests/test_attention_bf16_gpu.py (the kernels against these, on the card) and tests/test_attention_bf16_refs_cpu.py (the
emulation against the bounds, and every defect against the comparison, on any machine).

Nothing here imports the package under test.

Layout (that of the C ABI): qkv (B*T, 3E) bf16 with q | k | v side by side, E = 64 H, head h at columns 64 h .. 64 h + 63 of
its third; out / dout (B*T, E) bf16; lse (B, H, T) fp32, the natural-log sum-exp of the scaled scores.

The bounds.  The kernels round P (forward, dV) and dS (dQ, dK) to bf16 before the second product, keep the softmax sum
unrounded, accumulate in fp32 and round the result to bf16.  With u = 2^-8 (bf16) a rounded factor is off by at most u times
itself, so a product sum is off by at most u times the sum of the absolute products, and the stored result by u times itself:
    |O  - ref|[i,d] <= M u (sum_j P[i,j] |V[j,d]|   + |ref|)        |dQ - ref|[i,d] <= M u (sum_j |dS[i,j]| |K[j,d]| + |ref|) + C
    |dV - ref|[j,d] <= M u (sum_i P[i,j] |dO[i,d]|  + |ref|)        |dK - ref|[j,d] <= M u (sum_i |dS[i,j]| |Q[i,d]| + |ref|) + C
M = 1 + 2^-4 is the margin for the fp32 effects (fp32 accumulation of at most 256 + 64 exact bf16 products, one-ulp exp2 / log2,
the fp32 lse): each is at most 2^-15 relative to the same absolute sums.  C = 2^-18 sum P (|dP| + |delta|) scale |K or Q| covers
the cancellation inside dS = P (dP - delta) scale, whose two terms are fp32 sums of 64 products each."""
import math

import torch

U = 2.0 ** -8                # unit roundoff of bf16
MARGIN = 1.0 + 2.0 ** -4     # fp32 effects
CANCEL = 2.0 ** -18          # cancellation inside dS
HD = 64                      # head width
SCALE = 0.125
BLOCK = 32                   # keys per online-softmax step
LOG2E = 1.4426950408889634
LSE_TOL = dict(rtol=1e-4, atol=1e-4)
COLSUM_TOL = dict(rtol=1e-4, atol=1e-3)
FAMILIES = ("flat", "peaked", "uniform", "onehot")
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------------------ layout
def heads_of(x, B, T, H):
    """(B*T, H*64) -> (B, H, T, 64)"""
    return x.reshape(B, T, H, HD).permute(0, 2, 1, 3)


def rows_of(x):
    """(B, H, T, 64) -> (B*T, H*64)"""
    B, H, T, _ = x.shape
    return x.permute(0, 2, 1, 3).reshape(B * T, H * HD)


def split_qkv(qkv, B, T, H):
    E = H * HD
    return tuple(heads_of(qkv[:, i * E:(i + 1) * E], B, T, H) for i in range(3))


def pack_qkv(q, k, v):
    return torch.cat([rows_of(q), rows_of(k), rows_of(v)], dim=1).contiguous()


# ------------------------------------------------------------------------------------------------------------ fp64 references
def forward_ref(qkv, B, T, H, scale=SCALE):
    """-> dict(out (B*T, E), lse (B, H, T), bound (B*T, E)), all fp64."""
    q, k, v = (t.to(F64) for t in split_qkv(qkv, B, T, H))
    s = torch.einsum("bhid,bhjd->bhij", q, k) * scale
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse[..., None])
    o = p @ v
    bound = MARGIN * U * (p @ v.abs() + o.abs())
    return dict(out=rows_of(o), lse=lse, bound=rows_of(bound))


def backward_ref(qkv, out, dout, lse, B, T, H, scale=SCALE):
    """The gradient as msn_attention_bf16_bwd defines it: of (qkv, out, dout, lse) with the saved output (bf16) and lse (fp32)
    taken as inputs -> dict(dqkv (B*T, 3E), bound (B*T, 3E)), fp64."""
    q, k, v = (t.to(F64) for t in split_qkv(qkv, B, T, H))
    o, do = heads_of(out.to(F64), B, T, H), heads_of(dout.to(F64), B, T, H)
    s = torch.einsum("bhid,bhjd->bhij", q, k) * scale
    p = torch.exp(s - lse.to(F64)[..., None])
    delta = (do * o).sum(-1, keepdim=True)
    dp = do @ v.transpose(-1, -2)
    ds = p * (dp - delta) * scale
    dq, dk, dv = ds @ k, ds.transpose(-1, -2) @ q, p.transpose(-1, -2) @ do
    c = CANCEL * p * (dp.abs() + delta.abs()) * scale
    bq = MARGIN * U * (ds.abs() @ k.abs() + dq.abs()) + c @ k.abs()
    bk = MARGIN * U * (ds.abs().transpose(-1, -2) @ q.abs() + dk.abs()) + c.transpose(-1, -2) @ q.abs()
    bv = MARGIN * U * (p.transpose(-1, -2) @ do.abs() + dv.abs())
    return dict(dqkv=pack_qkv(dq, dk, dv), bound=pack_qkv(bq, bk, bv))


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound; an exact element counts 0 whatever its bound, NaN and an error against a zero bound count inf."""
    err = (got.detach().cpu().to(F64) - ref).abs()
    r = err / bound
    r = torch.where(err == 0, torch.zeros_like(r), r)
    r = torch.where(torch.isnan(r), torch.full_like(r, math.inf), r)
    return float(r.max())


def thirds(x):
    """(rows, 3E) -> its dq | dk | dv column blocks"""
    E = x.shape[1] // 3
    return x[:, :E], x[:, E:2 * E], x[:, 2 * E:]


def forward_ratios(out, fref):
    return {"O": worst_ratio(out, fref["out"], fref["bound"])}


def backward_ratios(dqkv, bref):
    got, ref, bound = thirds(dqkv), thirds(bref["dqkv"]), thirds(bref["bound"])
    return {n: worst_ratio(got[i], ref[i], bound[i]) for i, n in enumerate(("dQ", "dK", "dV"))}


def close(got, ref, rtol, atol):
    got = got.detach().cpu().to(F64)
    return bool(((got - ref).abs() <= atol + rtol * ref.abs()).all())        # NaN compares False


# ------------------------------------------------------------------------------------------------------------ input families
def _perm(T, c):
    """pi(i) = (a i + c) mod T with a ~ 0.618 T coprime to T: neighbouring queries aim at keys of different 16-token tiles,
    waves and 32-key blocks."""
    a = max(1, int(0.618 * T))
    while math.gcd(a, T) != 1:
        a += 1
    return (a * torch.arange(T) + c) % T


def _codes(T, g):
    """T distinct +-1 codes of width 64, any two at Hamming distance >= 10 (asserted)."""
    for _ in range(100):
        c = torch.randint(0, 2, (T, HD), generator=g).to(F64) * 2 - 1
        dot = c @ c.T - 2 * HD * torch.eye(T, dtype=F64)
        if T == 1 or float(dot.max()) <= HD - 20:
            return c
    raise AssertionError("no code set with the required distance")


def make_inputs(family, B, H, T, seed=0):
    """-> dict(qkv (B*T, 3E) bf16, dout (B*T, E) bf16[, perm (B, H, T): the key query i aims at]) on the CPU."""
    assert family in FAMILIES
    g = gen(1000003 * seed + 7919 * T + 31 * B + H + 101 * FAMILIES.index(family))
    shape = (B, H, T, HD)
    rn = lambda amp: torch.randn(shape, generator=g) * amp
    ex = {}
    if family in ("flat", "peaked"):
        amp = 0.8 if family == "flat" else 2.5
        q, k, v, do = rn(amp), rn(amp), rn(0.8), rn(1.0)
    elif family == "uniform":
        q, k, do = torch.zeros(shape), rn(1.0), rn(1.0)
        v = torch.randint(0, 2, shape, generator=g).float() * 2 - 1
        assert float(v.sum(2).abs().max()) <= 100         # M u |sum v| < 1/2: an integer step of the sum cannot hide
    else:
        odd = lambda: (torch.randint(0, 4, shape, generator=g) * 2 - 3).float()        # -3, -1, 1, 3
        v, do = odd(), odd()
        q, k, perm = torch.empty(shape), torch.empty(shape), torch.empty((B, H, T), dtype=torch.long)
        for b in range(B):
            for h in range(H):
                code = _codes(T, g).float()
                perm[b, h] = _perm(T, 7 + 5 * (b * H + h))
                k[b, h] = code
                q[b, h] = 16 * code[perm[b, h]]
        # off-target scores trail the target's by 16 * 0.125 * (64 - dot) >= 40: probabilities below e^-40
        ex["perm"] = perm
    return dict(qkv=pack_qkv(q, k, v).to(BF16), dout=rows_of(do).to(BF16).contiguous(), **ex)


def onehot_expect(inp, B, T, H):
    """-> (out (B*T, E), dv (B*T, E)) the one-hot family must give bit for bit: O[i] = v[pi(i)], dV[pi(i)] = dO[i]."""
    _, _, v = split_qkv(inp["qkv"], B, T, H)
    do = heads_of(inp["dout"], B, T, H)
    idx = inp["perm"][..., None].expand(B, H, T, HD)
    return rows_of(torch.gather(v, 2, idx)), rows_of(torch.zeros_like(do).scatter(2, idx, do))


def uniform_expect(inp, B, T, H):
    """-> sum_j v[j, d] per (sample, head) broadcast to the rows of out: T * O must be this integer to M u |sum v|."""
    _, _, v = split_qkv(inp["qkv"], B, T, H)
    return rows_of(v.to(F64).sum(2, keepdim=True).expand(B, H, T, HD))


def uniform_ok(out, inp, B, T, H):
    want = uniform_expect(inp, B, T, H)
    return bool(((T * out.detach().cpu().to(F64) - want).abs() <= MARGIN * U * want.abs()).all())


# ------------------------------------------------------------------------------------------------------------ the emulation
def _fma(a, b, c):
    """fp32 a * b + c with one rounding (the product of two fp32 is exact in fp64)"""
    return (a.to(F64) * b.to(F64) + c.to(F64)).to(F32)


def _rb(x):
    """round to bf16, keep as fp32"""
    return x.to(BF16).to(F32)


def _f32(x):
    return torch.tensor(x, dtype=F32)


def _pad(x, rows):
    return torch.cat([x, torch.zeros(rows - x.shape[0], x.shape[1], dtype=x.dtype)])


def _swap(vp, j):
    vp = vp.clone()
    vp[[j, j ^ 1]] = vp[[j ^ 1, j]]
    return vp


def emulate_forward(qkv, B, T, H, scale=SCALE, defect=None):
    """battn_fwd_kernel's arithmetic: fp32 scores, online softmax over 32-key blocks with the running maximum in the log2 domain,
    p = exp2(s scale log2e - m), l from the unrounded p, o from bf16(p) V rescaled when the maximum moves, bf16(o / l).
    defect = (kind, index): "drop_key" / "double_key" key `index` left out / counted twice, "swap_v" V rows index and index ^ 1
    swapped, "unmask_pad" the first zero padding key past T left unmasked.  -> (out (B*T, E) bf16, lse (B, H, T) fp32)"""
    kind, at = defect or (None, None)
    q, k, v = (t.to(F32) for t in split_qkv(qkv, B, T, H))
    Tp = (T + BLOCK - 1) // BLOCK * BLOCK
    sl = _f32(scale) * _f32(LOG2E)
    out, lse = torch.empty(B, H, T, HD, dtype=BF16), torch.empty(B, H, T, dtype=F32)
    for b in range(B):
        for h in range(H):
            kp, vp = _pad(k[b, h], Tp), _pad(v[b, h], Tp)
            if kind == "swap_v":
                vp = _swap(vp, at)
            live = torch.arange(Tp) < T
            if kind == "unmask_pad" and T < Tp:
                live[T] = True
            if kind == "drop_key":
                live[at] = False
            s = q[b, h] @ kp.T
            s[:, ~live] = -math.inf
            m, l, o = torch.full((T,), -math.inf), torch.zeros(T), torch.zeros(T, HD)
            for c0 in range(0, Tp, BLOCK):
                sb = s[:, c0:c0 + BLOCK]
                mn = torch.maximum(m, sb.max(1).values * sl)
                f = torch.exp2(m - mn)
                l, o, m = l * f, o * f[:, None], mn
                p = torch.exp2(_fma(sb, sl, -m[:, None]))
                pb = _rb(p)
                if kind == "double_key" and c0 <= at < c0 + BLOCK:
                    p, pb = p.clone(), pb.clone()
                    p[:, at - c0] *= 2
                    pb[:, at - c0] *= 2
                l = l + p.sum(1)
                o = o + pb @ vp[c0:c0 + BLOCK]
            out[b, h] = (o * (1.0 / l)[:, None]).to(BF16)
            lse[b, h] = (m + torch.log2(l)) * _f32(1.0 / LOG2E)
    return rows_of(out).contiguous(), lse


def emulate_backward(qkv, out, dout, lse, B, T, H, scale=SCALE, defect=None):
    """battn_bwd_dq_kernel / battn_bwd_dkv_kernel: P = exp2(s scale log2e - lse log2e), dS = P (dP scale - delta scale), both
    rounded to bf16 before the products, bf16 results.  defect: "drop_key" / "double_key" in the pass over keys (dQ),
    "drop_query" a query left out of the pass over queries (dK, dV), "swap_v" in dP = dO V^T.  -> dqkv (B*T, 3E) bf16"""
    kind, at = defect or (None, None)
    q, k, v = (t.to(F32) for t in split_qkv(qkv, B, T, H))
    o, do = heads_of(out.to(F32), B, T, H), heads_of(dout.to(F32), B, T, H)
    sc = _f32(scale)
    sl = sc * _f32(LOG2E)
    Tp = (T + BLOCK - 1) // BLOCK * BLOCK
    keys, queries = list(range(T)), list(range(T))
    if kind == "drop_key":
        keys.remove(at)
    if kind == "double_key":
        keys.append(at)
    if kind == "drop_query":
        queries.remove(at)
    res = [torch.empty(B, H, T, HD, dtype=BF16) for _ in range(3)]
    for b in range(B):
        for h in range(H):
            vv = _swap(_pad(v[b, h], Tp), at)[:T] if kind == "swap_v" else v[b, h]
            lse2 = lse[b, h].to(F32) * _f32(LOG2E)
            dls = (do[b, h] * o[b, h]).sum(1) * sc
            p = torch.exp2(_fma(q[b, h] @ k[b, h].T, sl, -lse2[:, None]))
            ds = p * _fma(do[b, h] @ vv.T, sc, -dls[:, None])
            pb, dsb = _rb(p), _rb(ds)
            res[0][b, h] = (dsb[:, keys] @ k[b, h][keys]).to(BF16)
            res[1][b, h] = (dsb[queries].T @ q[b, h][queries]).to(BF16)
            res[2][b, h] = (pb[queries].T @ do[b, h][queries]).to(BF16)
    return pack_qkv(*res)


# ------------------------------------------------------------------------------------------------------------ the comparison
def same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int16), b.view(torch.int16))


def forward_failures(family, inp, fref, out, lse, B, T, H):
    """What tests/test_attention_bf16_gpu.py asserts of a forward launch -> (list of failed checks, ratios)."""
    ratios = forward_ratios(out, fref)
    bad = [f"{n} at {r:.3g} of its bound" for n, r in ratios.items() if not r <= 1.0]
    if not close(lse, fref["lse"], **LSE_TOL):
        bad.append("lse")
    if family == "uniform" and not uniform_ok(out, inp, B, T, H):
        bad.append("T * O is not the integer column sum of v")
    if family == "onehot" and not same_bits(out, onehot_expect(inp, B, T, H)[0]):
        bad.append("O[i] != v[pi(i)] bit for bit")
    return bad, ratios


def backward_failures(family, inp, bref, dqkv, B, T, H):
    """The same for a backward launch.  The one-hot family is held to its exact expectations alone: its dQ and dK are sums of
    terms below e^-40 that fp32 flushes to zero, which the relative bounds do not model."""
    bad, ratios = [], {}
    if family == "onehot":
        dq, dk, dv = thirds(dqkv.detach().cpu())
        if not same_bits(dv.contiguous(), onehot_expect(inp, B, T, H)[1]):
            bad.append("dV[pi(i)] != dO[i] bit for bit")
        for n, t in (("dQ", dq), ("dK", dk)):
            if not float(t.to(F64).abs().max()) <= 1e-9:         # NaN fails
                bad.append(f"|{n}| > 1e-9")
    else:
        ratios = backward_ratios(dqkv, bref)
        bad = [f"{n} at {r:.3g} of its bound" for n, r in ratios.items() if not r <= 1.0]
    return bad, ratios
