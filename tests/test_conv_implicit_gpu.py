"""The implicit-GEMM convolutions of csrc/gemm.hip (msn_conv2d_fwd / _dgrad / _wgrad: the CONV = 1 and CONV = 2 branches of
sgemm_dma_kernel -- ConvGather, the zero page, the mirrored taps of dgrad, the multiply-shift pixel split of wgrad), launch by
launch at the C ABI, against F.conv2d and autograd in float64 on the CPU (glue_refs.conv2d_ref, itself tied to the verified
column references by tests/test_glue_refs_cpu.py).

Four kinds of test:
  a. every launch on integer-valued inputs ([-2, 2], bias in [-3, 3]: every sum is exact in float32 in any order, so the result
     must EQUAL the float64 reference), with both forward epilogues, with and without bias / dbias.  Each output sits between two
     guard bands of a sentinel that must survive, the workspace is full of NaN before every call (an exact result then proves
     that no split-K slab, tail slab or column-sum slot was read before it was written), the inputs must be left as they were
     and a second call must give the same bits;
  b. the same four comparisons under every forced tile width (ops.set_gemm_tile_n 0 / 64 / 128) and every finishing mode of the
     K-slab tail (ops.set_gemm_tail_split 1 / 2 / 0), so that the coverage of the three kernel instantiations does not depend on
     what the planner prefers; on random-normal inputs the two finishing modes of the slabbed launches are bit-identical
     and the unslabbed launch agrees with them within the bound of (c);
  c. random-normal inputs held to convmixer_refs.check_all (MARGIN x max(e32, FLOOR) of max|ref64|);
  d. functional.conv_cl on integers against float64 autograd of [relu](conv2d), pre-activations that are exactly 0 included,
     and which of ops.conv2d_fwd / conv2d_wgrad / conv2d_dgrad / col2im_tap it calls.

Geometries (B, H, W, C, Cout, kh, kw, sh, sw, ph, pw), with the launch each one gets by the planner at the time of writing (a
transcription of plan() run on the CPU, not observed on a card; (b) is what makes the coverage independent of it):

  geometry                               what it is                                            fwd        dgrad          wgrad
  (2, 6, 10, 64, 96, 3, 5, 1, 1, 0, 1)   kh != kw, ph != pw; valid padding in H: OH = 4 != H;  128x128    128x64,        128x64
                                         Cout = 96: 3 K-steps per tap in dgrad, a half-empty              120 rows
                                         last 128-column tile in fwd                                      (ragged M)
  (4, 6, 6, 96, 96, 3, 3, 1, 1, 0, 0)    padding 0 on both axes; C = 96: a 128-wide wgrad      128x128    128x128        128x128 (ragged
                                         tile straddles tap boundaries                                                   M = 96, N = 864)
  (2, 6, 6, 96, 64, 3, 3, 1, 1, 2, 2)    padding larger than (k-1)/2: OH = 8 > H; border       128x64     128x128,       64x128
                                         outputs made of padding and bias only                            72 rows
  (16, 5, 12, 64, 64, 2, 3, 1, 2, 1, 0)  even kh, sh != sw, ph != pw                           128x64     (strided)      64x128, 3 splits
  (16, 7, 9, 64, 64, 3, 3, 2, 3, 1, 1)   stride 3 in W: columns that no tap reaches            128x64     (strided)      64x128
  (32, 7, 9, 64, 128, 1, 1, 2, 2, 0, 0)  the ResNet downsample; odd sizes: the last window     128x64     (strided)      128x64, 5 splits
                                         sits on the border
  (8, 1, 64, 64, 128, 1, 5, 1, 1, 0, 0)  1-D series with valid padding (OW = 60)               128x64     128x64         128x64, 3 splits
  (2, 8, 8, 160, 128, 3, 3, 1, 1, 1, 1)  K = 1440; fwd: its one tile is cut into 6 K-slabs     128x128,   128x64         128x128
                                         of 256, so slabs begin inside a tap (tc0 = 96)        slabbed
  (2, 8, 8, 128, 160, 3, 3, 1, 1, 1, 1)  the mirror image: dgrad is the slabbed launch, also   128x64     128x128,       128x64
                                         starting mid-tap; fwd: a ragged last 64-column tile              slabbed
  (4, 8, 8, 256, 256, 3, 3, 1, 1, 1, 1)  fwd and dgrad: 4 tiles x 6 slabs each                 128x128,   128x128,       128x128, 2 splits
                                                                                               slabbed    slabbed
  (128, 8, 8, 64, 64, 3, 3, 1, 1, 1, 1)  wgrad over 8192 pixels                                128x64     128x64         64x128, 64 splits
                                                                                                                         (16-group reducer)
(strided: msn_conv2d_dgrad is stride-1 only; functional.conv_cl scatters through col2im_tap there, which (d) checks.)

Measured on an MI355X, as err / bound (e32), all relative to max|ref64|.  (c), the largest over its four geometries: y 1.087e-06 /
3.815e-06 (3.409e-07), dx 1.298e-06 / 3.815e-06 (3.017e-07), dw 4.527e-07 / 4.961e-06 (6.201e-07), db 1.407e-07 / 3.904e-06
(4.880e-07); the largest err of all is that dx, of (2, 6, 10, 64, 96, 3, 5, 1, 1, 0, 1), a third of its bound.  (b), random-normal:
the largest is dx of (4, 8, 8, 256, 256, 3, 3, 1, 1, 1, 1) without slabs, 1.820e-06 / 3.815e-06 (2.631e-07); the same tensor from
6 K-slabs per tile has 5.300e-07 (shorter sums).  Every integer comparison is exact, and the file runs in under 3 s.

A dgrad gather that takes H, W for the size of its source image (dY is OH x OW) computes the same numbers wherever OH == H and
OW == W -- every "same"-padding case -- and fails test_dgrad_equals_autograd_on_integers on the first three geometries and on
the 1-D series (more than 90 % of dx differs).
"""
import functools

import pytest
import torch

import convmixer_refs as R
import glue_refs as G

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64, F32 = torch.float64, torch.float32
EPI_NONE, EPI_RELU = 0, 1
SENTINEL = -12345.0
GUARD_ROWS = 128          # guard band = this many rows of the output (one whole row tile), a multiple of 4 floats
WS_GUARD = 1024           # floats behind the workspace that must stay NaN

GEOMS = G.IMPLICIT_GEOMS
SLABBED = [c for c in GEOMS if c[:5] in ((2, 8, 8, 160, 128), (2, 8, 8, 128, 160), (4, 8, 8, 256, 256))]
FORCED = SLABBED + GEOMS[:2]
NORMAL = [GEOMS[0], GEOMS[2], GEOMS[9], GEOMS[10]]


def _id(c):
    return "-".join(str(v) for v in c)


def _ops():
    from multimodal_supernovae_amd import ops
    return ops


def _L():
    from multimodal_supernovae_amd import _lib
    return _lib


def _dev(t):
    return t.to(DEV).contiguous()


def _stride1(case):
    return case[7] == 1 and case[8] == 1


# ---------------------------------------------------------------------------------------- inputs and references, once each
@functools.lru_cache(maxsize=None)
def _case(case, integers):
    """Inputs (CPU float32) and the references of one geometry; computed once, shared by every test, never written to.
    ref64 / ref32: y (no bias; the bias is added where a test uses one: exact at float64 on integers), dx, dw, db, all without
    ReLU.  ref32 (the yardstick of check_all) only for the random-normal inputs."""
    x, w, b, dy = G.conv_inputs(case, integers)
    stride, padding = case[7:9], case[9:11]
    ins = {"x": x, "w_tap": G.conv_w_tap(w), "w_tco": G.conv_w_tco(w), "b": b, "dy": dy, "w": w}
    bias = None if integers else b
    ref64 = dict(zip(("y", "dx", "dw", "db"), G.conv2d_ref(x, w, bias, stride, padding, dy, False, F64)))
    ref32 = None if integers else dict(zip(("y", "dx", "dw", "db"), G.conv2d_ref(x, w, bias, stride, padding, dy, False, F32)))
    return ins, ref64, ref32


@functools.lru_cache(maxsize=None)
def _device_inputs(case, integers):
    ins = _case(case, integers)[0]
    return {k: _dev(v) for k, v in ins.items()}


# ------------------------------------------------------------------------------------------------- one launch, watched
class _Guarded:
    """`shape` floats in the middle of a buffer of SENTINEL; the bands on both sides are a multiple of 4 floats (torch's
    allocations are 512-byte aligned, so the payload stays 16-byte aligned)."""

    def __init__(self, shape):
        n = 1
        for s in shape:
            n *= s
        self.band = max(GUARD_ROWS * shape[-1], 256)
        assert self.band % 4 == 0
        self.buf = torch.empty(n + 2 * self.band, dtype=F32, device=DEV)
        self.out = self.buf[self.band:self.band + n].view(shape)
        assert self.out.data_ptr() % 16 == 0

    def reset(self):
        self.buf.fill_(SENTINEL)

    def bands_intact(self):
        lo, hi = self.buf[:self.band], self.buf[self.buf.numel() - self.band:]
        return bool((lo == SENTINEL).all()) and bool((hi == SENTINEL).all())


def _launch(kind, case, integers=True, epi=EPI_NONE, bias=False, dbias=False):
    """One launch of `kind` ("fwd" | "dgrad" | "wgrad") through the C ABI on buffers this test owns, twice.  Checks the guard
    bands of every output and of the workspace, that the inputs are left alone and that both calls give the same bits; returns
    the outputs of the first call on the CPU."""
    L = _L()
    lib = L.lib()
    B, H, W, C, co, kh, kw, sh, sw, ph, pw = case
    assert lib.msn_conv2d_implicit_ok(*case), case
    oh, ow = G.conv_out(H, kh, sh, ph), G.conv_out(W, kw, sw, pw)
    t = _device_inputs(case, integers)
    taps = kh * kw
    if kind == "fwd":
        used = ["x", "w_tap"] + (["b"] if bias else [])
        outs = {"y": _Guarded((B * oh * ow, co))}
    elif kind == "dgrad":
        assert _stride1(case)
        used = ["dy", "w_tco"]
        outs = {"dx": _Guarded((B, H, W, C))}
    else:
        used = ["dy", "x"]
        outs = {"dw": _Guarded((co, taps * C))}
        if dbias:
            outs["db"] = _Guarded((co,))
    before = {k: t[k].clone() for k in used}
    nb = lib.msn_conv2d_workspace_bytes(*case)            # under the switches in force: the planner's own answer
    assert nb % 4 == 0
    ws = torch.empty(nb // 4 + WS_GUARD, dtype=F32, device=DEV)
    p, sp = L.ptr, L.stream_ptr()

    def call():
        ws.fill_(float("nan"))
        for o in outs.values():
            o.reset()
        if kind == "fwd":
            rc = lib.msn_conv2d_fwd(p(t["x"]), B, H, W, C, p(t["w_tap"]), co, kh, kw, sh, sw, ph, pw, p(t["b"] if bias else None),
                                    epi, p(outs["y"].out), p(ws), nb, sp)
        elif kind == "dgrad":
            rc = lib.msn_conv2d_dgrad(p(t["dy"]), B, H, W, C, p(t["w_tco"]), co, kh, kw, ph, pw, p(outs["dx"].out), p(ws), nb, sp)
        else:
            rc = lib.msn_conv2d_wgrad(p(t["dy"]), p(t["x"]), B, H, W, C, co, kh, kw, sh, sw, ph, pw, p(outs["dw"].out),
                                      p(outs["db"].out if dbias else None), p(ws), nb, sp)
        L.check(rc, "msn_conv2d_" + kind)
        torch.cuda.synchronize()
        tag = f"{kind}{case}"
        for k, o in outs.items():
            assert o.bands_intact(), f"{tag}: wrote outside {k}"
        assert bool(torch.isnan(ws[nb // 4:]).all()), f"{tag}: wrote behind its workspace"
        for k in used:
            assert G.same_bits(t[k], before[k]), f"{tag}: changed its input {k}"
        return {k: o.out.cpu().clone() for k, o in outs.items()}

    first, second = call(), call()
    for k in first:
        assert G.same_bits(first[k], second[k]), f"{kind}{case}: {k} differs between two calls"
    return first


def _exact(got, want64, what):
    want = want64.to(F32)
    assert got.shape == want.shape, (what, tuple(got.shape), tuple(want.shape))
    bad = got != want
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} of {bad.numel()} differ, first at flat index "
                                 f"{int(bad.flatten().nonzero()[0])}: {float(got[bad][0])} != {float(want[bad][0])}")
    assert torch.equal(got, want), what


def _check_fwd(case):
    """Both epilogues, with and without bias."""
    ins, ref, _ = _case(case, True)
    for bias in (False, True):
        pre = ref["y"] + ins["b"].double() if bias else ref["y"]
        assert bool((pre == 0).any()) and bool((pre < 0).any())          # ReLU meets exact zeros and has something to cut
        for epi in (EPI_NONE, EPI_RELU):
            y = _launch("fwd", case, epi=epi, bias=bias)["y"]
            _exact(y, torch.relu(pre) if epi == EPI_RELU else pre, f"fwd{case} epilogue {epi} bias {bias}")


def _check_dgrad(case):
    _exact(_launch("dgrad", case)["dx"], _case(case, True)[1]["dx"], f"dgrad{case}")


def _check_wgrad(case):
    """Without dbias, and with it: the CSUM kernel, whose column-sum slabs sit behind the split-K slabs of the product."""
    ins, ref, _ = _case(case, True)
    db = ins["dy"].double().sum(0)
    assert torch.equal(ref["db"], db)
    _exact(_launch("wgrad", case)["dw"], ref["dw"], f"wgrad{case}")
    got = _launch("wgrad", case, dbias=True)
    _exact(got["dw"], ref["dw"], f"wgrad + dbias{case}: dw")
    _exact(got["db"], db, f"wgrad + dbias{case}: db")


@pytest.fixture
def switches():
    """set(tile_n, tail_split); the process-wide switches go back to the planner's defaults whatever happens."""
    ops = _ops()

    def set_(bn, tail):
        ops.set_gemm_tile_n(bn)
        ops.set_gemm_tail_split(tail)
    try:
        yield set_
    finally:
        ops.set_gemm_tile_n(0)
        ops.set_gemm_tail_split(1)


# ------------------------------------------------------------------------------ a. each launch, exact on integers
@pytest.mark.parametrize("case", GEOMS, ids=_id)
def test_fwd_both_epilogues_equal_conv2d_on_integers(case):
    _check_fwd(case)


@pytest.mark.parametrize("case", [c for c in GEOMS if _stride1(c)], ids=_id)
def test_dgrad_equals_autograd_on_integers(case):
    _check_dgrad(case)


@pytest.mark.parametrize("case", GEOMS, ids=_id)
def test_wgrad_with_and_without_dbias_equals_autograd_on_integers(case):
    _check_wgrad(case)


# ------------------------------------------------- b. every instantiation and finishing mode, whatever the planner prefers
@pytest.mark.parametrize("tail", [1, 2, 0])
@pytest.mark.parametrize("tile_n", [0, 64, 128])
@pytest.mark.parametrize("case", FORCED, ids=_id)
def test_every_tile_width_and_tail_mode_exact_on_integers(case, tile_n, tail, switches):
    switches(tile_n, tail)
    _check_fwd(case)
    _check_dgrad(case)
    _check_wgrad(case)


@pytest.mark.parametrize("case", SLABBED, ids=_id)
def test_tail_modes_1_and_2_are_bit_identical_and_mode_0_is_within_the_bound(case, switches):
    """include/msn_hip.h promises "bit-identical: same order" for the in-kernel finish and the finishing launch."""
    ins, ref64, ref32 = _case(case, False)
    got = {}
    for tail in (1, 2, 0):
        switches(0, tail)
        got[tail] = {"y": _launch("fwd", case, integers=False, bias=True)["y"], "dx": _launch("dgrad", case, integers=False)["dx"]}
    for k in ("y", "dx"):
        assert G.same_bits(got[1][k], got[2][k]), f"{case}: {k} differs between the two ways of finishing a slabbed tile"
    for tail in (1, 0):
        R.check_all(f"conv{case} tail {tail}", got[tail], ref32, ref64, keys=("y", "dx"))
    for k in ("y", "dx"):                                   # slabbed against unslabbed, by the same yardstick
        assert R.scaled_err(got[0][k], got[1][k].double()) <= R.bound(ref32[k], ref64[k]), k


# ------------------------------------------------------------------- c. random-normal inputs, the project's own yardstick
@pytest.mark.parametrize("case", NORMAL, ids=_id)
def test_all_launches_random_normal_within_check_all(case):
    _, ref64, ref32 = _case(case, False)
    got = {"y": _launch("fwd", case, integers=False, bias=True)["y"], "dx": _launch("dgrad", case, integers=False)["dx"]}
    got.update(_launch("wgrad", case, integers=False, dbias=True))
    assert sorted(got) == ["db", "dw", "dx", "y"]
    R.check_all(f"conv{case}", got, ref32, ref64)


# --------------------------------------------------------------------------- d. the autograd wrapper and its dispatch
class _Spy:
    """Counts the calls of the four ops functions conv_cl chooses between; always puts the real ones back."""
    NAMES = ("conv2d_fwd", "conv2d_wgrad", "conv2d_dgrad", "col2im_tap")

    def __enter__(self):
        self.ops, self.real, self.calls = _ops(), {}, {n: 0 for n in self.NAMES}
        for n in self.NAMES:
            self.real[n] = getattr(self.ops, n)
            setattr(self.ops, n, self._wrap(n))
        return self.calls

    def _wrap(self, n):
        def f(*a, **kw):
            self.calls[n] += 1
            return self.real[n](*a, **kw)
        return f

    def __exit__(self, *exc):
        for n in self.NAMES:
            setattr(self.ops, n, self.real[n])


@functools.lru_cache(maxsize=None)
def _autograd_ref(case, relu, bias):
    ins = _case(case, True)[0]
    return G.conv2d_ref(ins["x"], ins["w"], ins["b"] if bias else None, case[7:9], case[9:11], ins["dy"], relu, F64)


def _conv_cl(case, relu, bias, x_grad=True):
    from multimodal_supernovae_amd import functional as F_
    ins = _case(case, True)[0]
    x, w, dy = ins["x"], ins["w"], ins["dy"]
    b = ins["b"] if bias else None
    want = _autograd_ref(case, relu, bias)
    xg = _dev(x).requires_grad_(x_grad)
    wg = _dev(w).requires_grad_()
    bg = _dev(b).requires_grad_() if bias else None
    with _Spy() as calls:
        y = F_.conv_cl(xg, wg, bg, case[7:9], case[9:11], relu=relu)
        y.backward(_dev(dy).view(y.shape))
        torch.cuda.synchronize()
    return (y.detach().cpu().reshape(-1, case[4]), xg.grad, wg.grad.cpu(), bg.grad.cpu() if bias else None), want, calls


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("case", GEOMS, ids=_id)
def test_conv_cl_equals_autograd_on_integers_and_takes_the_implicit_launches(case, relu, bias):
    B, H, W, C, co, kh, kw = case[:7]
    (y, dx, dw, db), (ry, rdx, rdw_tap, rdb), calls = _conv_cl(case, relu, bias)
    _exact(y, ry, f"conv_cl{case} y")
    if relu:
        assert bool((ry == 0).any()) and bool((ry > 0).any())
    _exact(dx.cpu(), rdx, f"conv_cl{case} x.grad")
    assert dw.shape == (co, C, kh, kw)
    _exact(dw.reshape(co, -1), G.relayout_ref(rdw_tap, co, C, kh * kw, 0), f"conv_cl{case} w.grad")
    if bias:
        _exact(db, rdb, f"conv_cl{case} b.grad")
    assert calls["conv2d_fwd"] == 1 and calls["conv2d_wgrad"] == 1, calls
    if _stride1(case):
        assert calls["conv2d_dgrad"] == 1 and calls["col2im_tap"] == 0, calls
    else:
        assert calls["conv2d_dgrad"] == 0 and calls["col2im_tap"] == 1, calls


@pytest.mark.parametrize("case", [GEOMS[0], GEOMS[5]], ids=_id)
def test_conv_cl_without_an_input_gradient_runs_neither_dgrad_path(case):
    B, H, W, C, co, kh, kw = case[:7]
    (y, dx, dw, db), (ry, _, rdw_tap, rdb), calls = _conv_cl(case, True, True, x_grad=False)
    assert dx is None
    assert calls == {"conv2d_fwd": 1, "conv2d_wgrad": 1, "conv2d_dgrad": 0, "col2im_tap": 0}, calls
    _exact(y, ry, f"conv_cl{case} y")
    _exact(dw.reshape(co, -1), G.relayout_ref(rdw_tap, co, C, kh * kw, 0), f"conv_cl{case} w.grad")
    _exact(db, rdb, f"conv_cl{case} b.grad")
