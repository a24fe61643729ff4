"""Weight averaging on the GPU (csrc/weight_avg.hip, optim.AveragedWeights, checkpoint.WeightAveraging): the kernel through the
C-ABI against fp64 and torch's AveragedModel, and the Trainer / GraphedTrainStep with the callback against hand loops.
Shapes: the tiny two-tower model and the 8-row batches of tests/test_grad_accum_gpu.py.

Bounds (derived, not measured).  One update avg' = fma(w, p - avg, avg) has two roundings: of the difference, at most
2 max(|avg|, |p|) large, then scaled by w <= 1, and of the result, at most max(|avg|, |p|) large: 2^-22 max(|avg|, |p|) per element
against fp64 arithmetic on the same fp32 inputs and the same fp32 w.  A sequence of n updates: n times that with the largest
snapshot entry, since neither recurrence amplifies an error (its factor is 1 - w <= 1); against torch's lerp, which has one
more rounding per update, n 2^-21 max|snapshot|."""
import copy
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu

EMA, SWA, SWAP = 0, 1, 2              # MSN_AVG_* of include/msn_hip.h
PASS = 4 * 256 * 4                    # elements one block covers per pass (kMtBlockElems of csrc/multi_tensor.h)
GUARD, SENTINEL = 8, -12345.0         # floats in front of and behind every tensor that no launch may touch
ALIGN = ["aligned", "avg", "p", "both"]          # which operand is a view one element into an aligned buffer


def _cap(n_tensors):
    """Blocks per tensor of a table of n_tensors (the cap of mt_grid_x, csrc/multi_tensor.h)."""
    return min(1024, max(32, 8192 // n_tensors))


def _sizes():
    sizes = [1, 3, 4, 5, 1023, 4096, 4097, 65537] + [1 + (7 * i) % 61 for i in range(247)]
    sizes.append(_cap(len(sizes) + 1) * PASS + PASS + 5)         # longer than (blocks per tensor) x (a pass): every block loops
    assert len(sizes) == 256 and _cap(256) == 32 and sizes[-1] == 135173 > 32 * PASS
    return sizes


class Arena:
    """Every tensor of a launch inside ONE device buffer: GUARD sentinels in front of and behind each, each start on a 16-byte
    boundary (or 4 bytes behind one: `misaligned`).  One copy up, one copy down."""

    def __init__(self, values, misaligned):
        self.offs, pos = [], 0
        for v in values:
            start = pos + GUARD + (1 if misaligned else 0)
            self.offs.append(start)
            pos = (start + v.numel() + GUARD + 3) // 4 * 4
        self.sizes = [v.numel() for v in values]
        host = torch.full((pos,), SENTINEL)
        self.guard = torch.ones(pos, dtype=torch.bool)
        for o, v in zip(self.offs, values):
            host[o:o + v.numel()] = v
            self.guard[o:o + v.numel()] = False
        self.host0 = host
        self.dev = host.cuda()
        assert self.dev.data_ptr() % 16 == 0
        self.views = [self.dev[o:o + n] for o, n in zip(self.offs, self.sizes)]
        assert all(v.data_ptr() % 16 == (4 if misaligned else 0) for v in self.views)

    def reset(self):
        self.dev.copy_(self.host0)

    def values(self):
        """(the tensors' values concatenated, guards intact?), after one copy down."""
        host = self.dev.cpu()
        return host[~self.guard], bool((host[self.guard] == SENTINEL).all())


def _random_values(sizes, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=g) * 10.0 ** ((i % 5) - 2) for i, n in enumerate(sizes)]


_ARENAS = {}


def _arenas(align):
    """(avg arena, p arena) of the 256-tensor launch for one alignment case, built once; the values are those of every case."""
    if align not in _ARENAS:
        sizes = _sizes()
        _ARENAS[align] = (Arena(_random_values(sizes, 1), align in ("avg", "both")), Arena(_random_values(sizes, 2), align in ("p", "both")))
    a, p = _ARENAS[align]
    a.reset()
    p.reset()
    return a, p


def _table(a, p):
    words = []
    for x, y in zip(a.views, p.views):
        words += [x.data_ptr(), y.data_ptr(), x.numel()]
    return torch.tensor(words, dtype=torch.int64).cuda(), len(a.views), max(a.sizes)


def _launch(table, n, max_n, mode, weight, state, expect=0):
    from multimodal_supernovae_amd._lib import lib, ptr, stream_ptr
    rc = lib().msn_weight_average(ptr(table) if table is not None else None, n, max_n, mode, weight,
                                  ptr(state) if state is not None else None, stream_ptr())
    assert rc == expect, (rc, lib().msn_last_error())
    return lib().msn_last_error()


def _state(n_averaged, active=1):
    return torch.tensor([n_averaged, active], dtype=torch.int64).cuda()


def _bits(t):
    return t.contiguous().view(torch.int32)


CASES = [(EMA, 1.0 - 0.9, 1), (EMA, 1.0 - 0.999, 1), (EMA, 1.0 - 0.9999, 7), (SWA, None, 1), (SWA, None, 2), (SWA, None, 1000),
         (SWA, None, 2 ** 24 + 1)]
_RESULTS = {}                         # (case index) -> {alignment: result bits}


@pytest.mark.parametrize("align", ALIGN)
def test_one_update_against_fp64(align):
    a, p = _arenas(align)
    table, n, max_n = _table(a, p)
    a0, p0 = a.host0[~a.guard].double(), p.host0[~p.guard].double()
    bound = 2.0 ** -22 * torch.maximum(a0.abs(), p0.abs())
    for ci, (mode, w, n_avg) in enumerate(CASES):
        a.reset()
        w32 = np.float32(w) if mode == EMA else np.float32(1.0 / (n_avg + 1))      # the fp32 weight both sides use
        assert mode == EMA or float(w32) == float(torch.tensor(1.0 / (n_avg + 1), dtype=torch.float64).float())
        state = _state(n_avg)
        _launch(table, n, max_n, mode, float(w32) if mode == EMA else 0.5, state)   # SWA ignores the argument
        got, intact = a.values()
        want = a0 + float(w32) * (p0 - a0)
        err = (got.double() - want).abs()
        worst = int(torch.argmax(err - bound))
        assert bool((err <= bound).all()), (ci, float(err[worst]), float(bound[worst]))
        assert intact and p.values()[1] and torch.equal(p.values()[0], p.host0[~p.guard])
        assert state.tolist() == [n_avg + 1, 1]
        _RESULTS.setdefault(ci, {})[align] = _bits(got)
        a.reset()
        _launch(table, n, max_n, mode, float(w32) if mode == EMA else 0.5, _state(n_avg))
        assert torch.equal(_bits(a.values()[0]), _bits(got)), ci                   # two runs give equal bits


def test_the_16_byte_path_and_the_scalar_path_give_the_same_bits():
    for align in ALIGN:                                     # (fills what a deselected case left out)
        if any(align not in _RESULTS.get(ci, {}) for ci in range(len(CASES))):
            test_one_update_against_fp64(align)
    for ci in range(len(CASES)):
        for align in ALIGN[1:]:
            assert torch.equal(_RESULTS[ci]["aligned"], _RESULTS[ci][align]), (ci, align)


def _plant(values):
    """Edge values into the largest tensor and a few small ones: NaNs with payloads, infinities, -0.0, denormals."""
    edge = torch.tensor([0x7FC00001, 0x7F800123, -0x00400000 & 0xFFFFFFFF, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001,
                         0x807FFFFF, 0x00400000, 0x00000000], dtype=torch.int64)
    edge = torch.where(edge >= 2 ** 31, edge - 2 ** 32, edge).to(torch.int32).view(torch.float32)
    for i in (4, 5, 6, 7, len(values) - 1):
        values[i][:edge.numel()] = edge
        values[i][-edge.numel():] = edge
    values[3][:5] = edge[:5]
    return values


@pytest.mark.parametrize("align", ["aligned", "both", "p"])
def test_first_update_copies_the_bits_and_swap_exchanges_them(align):
    sizes = _sizes()
    a = Arena(_random_values(sizes, 3), align == "both")
    p = Arena(_plant(_random_values(sizes, 4)), align in ("p", "both"))
    table, n, max_n = _table(a, p)
    p_bits, a_bits = _bits(p.host0[~p.guard]), _bits(a.host0[~a.guard])
    assert int(torch.isnan(p.host0).sum()) >= 15
    for mode in (EMA, SWA):
        a.reset()
        state = _state(0)
        _launch(table, n, max_n, mode, 0.25, state)
        got, intact = a.values()
        assert torch.equal(_bits(got), p_bits) and intact and state.tolist() == [1, 1]
    # swap: bit exact both ways, twice is the identity; state may be NULL and a given one is left alone
    a.reset()
    state = _state(5, 1)
    _launch(table, n, max_n, SWAP, 0.0, None)
    (ga, ia), (gp, ip) = a.values(), p.values()
    assert torch.equal(_bits(ga), p_bits) and torch.equal(_bits(gp), a_bits) and ia and ip
    _launch(table, n, max_n, SWAP, 7.0, state)              # the weight is not looked at in swap mode
    (ga, ia), (gp, ip) = a.values(), p.values()
    assert torch.equal(_bits(ga), a_bits) and torch.equal(_bits(gp), p_bits) and ia and ip and state.tolist() == [5, 1]


def test_active_word_and_device_count():
    a, p = _arenas("avg")
    table, n, max_n = _table(a, p)
    before = _bits(a.values()[0])
    for mode in (EMA, SWA):
        for n_avg in (0, 3):
            state = _state(n_avg, 0)
            _launch(table, n, max_n, mode, 0.1, state)      # active = 0: nothing changes
            got, intact = a.values()
            assert torch.equal(_bits(got), before) and intact and state.tolist() == [n_avg, 0]
    state = _state(4, 1)
    for _ in range(3):
        _launch(table, n, max_n, EMA, 0.1, state)
    assert state.tolist() == [7, 1]
    state = _state(0, 2 ** 40)                              # any non-zero word is "active"; the count goes up by one
    _launch(table, n, max_n, SWA, 0.0, state)
    _launch(table, n, max_n, SWA, 0.0, state)
    assert state.tolist() == [2, 2 ** 40] and a.values()[1]


@pytest.mark.parametrize("n_avg", [1, 2, 1000, 2 ** 24 + 1])
def test_swa_weight_is_the_double_quotient_rounded_once(n_avg):
    """avg = 0, p = 1: d = 1 and fma(w, 1, 0) = w, so the average holds the weight the device formed."""
    a, p = Arena([torch.zeros(9)], False), Arena([torch.ones(9)], True)
    table, n, max_n = _table(a, p)
    _launch(table, n, max_n, SWA, 0.75, _state(n_avg))
    got, intact = a.values()
    want = torch.from_numpy(np.full(9, np.float32(1.0 / (n_avg + 1)), dtype=np.float32))
    assert torch.equal(_bits(got), _bits(want)) and intact, (got.tolist(), float(want[0]))


def test_argument_checks_leave_the_buffers_untouched():
    a, p = _arenas("aligned")
    table, n, max_n = _table(a, p)
    state = _state(2, 1)
    cases = [((None, n, max_n, EMA, 0.1, state), "null table"), ((table, 0, max_n, EMA, 0.1, state), "1..65535"),
             ((table, 65536, max_n, SWA, 0.1, state), "1..65535"), ((table, -1, max_n, SWAP, 0.1, None), "1..65535"),
             ((table, n, -1, EMA, 0.1, state), "max_numel"), ((table, n, max_n, 3, 0.1, state), "mode must be"),
             ((table, n, max_n, -1, 0.1, state), "mode must be"), ((table, n, max_n, EMA, -0.01, state), "[0, 1]"),
             ((table, n, max_n, EMA, 1.5, state), "[0, 1]"), ((table, n, max_n, EMA, math.nan, state), "[0, 1]"),
             ((table, n, max_n, EMA, 0.1, None), "null state"), ((table, n, max_n, SWA, 0.1, None), "null state")]
    for args, msg in cases:
        text = _launch(*args, expect=1)
        assert msg.encode() in text, (msg, text)
    torch.cuda.synchronize()
    assert torch.equal(a.dev.cpu(), a.host0) and torch.equal(p.dev.cpu(), p.host0) and state.tolist() == [2, 1]


# --------------------------------------------------------------------------------------------------------------- sequences
SEQ_SIZES, SEQ_STEPS = [5, 1023, 4097, 12], 16


def _snapshots(steps=SEQ_STEPS, sizes=SEQ_SIZES, seed=11):
    g = torch.Generator().manual_seed(seed)
    return [[torch.randn(n, generator=g) * 10.0 ** (i - 1) for i, n in enumerate(sizes)] for _ in range(steps)]


def _torch_averaged(snaps, avg, decay):
    """torch's AveragedModel on the CPU fed the snapshots: get_ema_multi_avg_fn(decay), or the default SWA."""
    from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn
    holder = torch.nn.Module()
    holder.ps = torch.nn.ParameterList([torch.nn.Parameter(s.clone()) for s in snaps[0]])
    am = AveragedModel(holder, multi_avg_fn=get_ema_multi_avg_fn(decay)) if avg == "ema" else AveragedModel(holder)
    for snap in snaps:
        with torch.no_grad():
            for q, s in zip(holder.ps, snap):
                q.copy_(s)
        am.update_parameters(holder)
    return [q.detach().clone() for q in am.module.ps]


def _fed(snaps, avg, decay):
    """An AveragedWeights on mirror parameters fed the snapshots (on the CPU or the GPU) one by one."""
    from multimodal_supernovae_amd import optim
    mirror = [torch.nn.Parameter(s.detach().clone().cuda()) for s in snaps[0]]
    aw = optim.AveragedWeights(mirror, avg=avg, decay=decay)
    for snap in snaps:
        with torch.no_grad():
            for q, s in zip(mirror, snap):
                q.copy_(s)
        aw.update()
    return aw


def _check_sequence(got, snaps, avg, decay, against_torch=True):
    """`got` (one tensor per snapshot tensor) against the fp64 mean / recurrence and torch's AveragedModel."""
    steps = len(snaps)
    w32 = float(np.float32(1.0 - decay))
    for i, g in enumerate(got):
        col = torch.stack([s[i].detach().cpu().double().reshape(-1) for s in snaps])
        big = float(col.abs().max())
        if avg == "swa":
            want = col.mean(0)
        else:
            want = col[0].clone()
            for s in col[1:]:
                want = want + w32 * (s - want)
        err = float((g.detach().cpu().double().reshape(-1) - want).abs().max())
        assert err <= steps * 2.0 ** -22 * big, (avg, i, err, steps * 2.0 ** -22 * big)
    if against_torch:
        ref = _torch_averaged([[t.detach().cpu() for t in s] for s in snaps], avg, decay)
        for i, (g, r) in enumerate(zip(got, ref)):
            big = max(float(s[i].abs().max()) for s in snaps)
            err = float((g.detach().cpu().double() - r.double()).abs().max())
            assert err <= steps * 2.0 ** -21 * big, (avg, i, err, steps * 2.0 ** -21 * big)


@pytest.mark.parametrize("avg,decay", [("swa", 0.999), ("ema", 0.9), ("ema", 0.999)])
def test_sixteen_updates_against_fp64_and_torchs_averaged_model(avg, decay):
    snaps = _snapshots()
    aw = _fed(snaps, avg, decay)
    assert aw.n_averaged == SEQ_STEPS == aw.device_n_averaged() and aw.flat.numel() == 8 + 1024 + 4100 + 12
    _check_sequence(aw.averages, snaps, avg, decay)
    again = _fed(snaps, avg, decay)
    assert all(torch.equal(x, y) for x, y in zip(aw.averages, again.averages))


def test_averaged_weights_object():
    from multimodal_supernovae_amd import _lib, optim
    snaps = _snapshots(steps=3)
    aw = _fed(snaps, "ema", 0.9)
    live = [t.clone() for t in aw.tensors]
    avg = [a.clone() for a in aw.averages]
    sd = aw.averaged_state_dict()
    assert list(sd) == ["0", "1", "2", "3"] and all(torch.equal(sd[k], a) for k, a in zip(sd, avg))
    aw.swap()
    assert aw.swapped and all(torch.equal(t, a) for t, a in zip(aw.tensors, avg))
    assert all(torch.equal(b, l) for b, l in zip(aw.averages, live))
    assert all(torch.equal(aw.averaged_state_dict()[k], a) for k, a in zip(sd, avg))      # wherever the average lives now
    with pytest.raises(RuntimeError, match="swapped"):
        aw.update()
    aw.swap()
    assert not aw.swapped and all(torch.equal(t, l) for t, l in zip(aw.tensors, live))
    # the device word: off -> the launch is issued and changes nothing; written only when it changes
    aw.set_active(False)
    aw.update()
    assert aw.n_averaged == 3 == aw.device_n_averaged() and all(torch.equal(a, b) for a, b in zip(aw.averages, avg))
    aw.set_active(True)
    aw.update()
    assert aw.n_averaged == 4 == aw.device_n_averaged()
    # state dict: plain, and into another object
    state = aw.state_dict()
    assert state["n_averaged"] == 4 and state["avg"] == "ema" and state["swapped"] is False and state["decay"] == 0.9
    other = optim.AveragedWeights([torch.nn.Parameter(t.clone()) for t in aw.tensors], avg="ema", decay=0.9)
    other.load_state_dict(state)
    assert other.n_averaged == 4 == other.device_n_averaged()
    assert all(torch.equal(x, y) for x, y in zip(other.averages, aw.averages))
    aw.update()
    other.update()
    assert all(torch.equal(x, y) for x, y in zip(other.averages, aw.averages)) and other.device_n_averaged() == 5
    with pytest.raises(ValueError, match="avg='ema'"):
        optim.AveragedWeights([torch.nn.Parameter(t.clone()) for t in aw.tensors], avg="swa").load_state_dict(state)
    with pytest.raises(ValueError, match=r"missing here: \['3'\]"):
        optim.AveragedWeights([torch.nn.Parameter(t.clone()) for t in aw.tensors[:3]]).load_state_dict(state)
    # what the launch cannot take is refused by name
    with pytest.raises(_lib.MsnHipError, match="float32"):
        optim.AveragedWeights([torch.nn.Parameter(torch.zeros(4, dtype=torch.float64, device="cuda"))])
    with pytest.raises(_lib.MsnHipError, match="contiguous"):
        optim.AveragedWeights([torch.nn.Parameter(torch.zeros(4, 4, device="cuda").t()[1:])])
    moved = torch.nn.Parameter(torch.zeros(4, device="cuda"))
    aw2 = optim.AveragedWeights([moved], decay=0.5)
    aw2.update()
    moved.data = torch.ones(4, device="cuda")               # re-pointed, as SelfAttention.stacked_qkv does: the table follows
    aw2.update()
    assert torch.equal(aw2.averages[0], torch.full((4,), 0.5, device="cuda")) and aw2.n_averaged == 2


# ------------------------------------------------------------------------------------------------------------ the Trainer
def _G():
    import test_grad_accum_gpu as G
    return G


def _params(model):
    return [p.detach().clone() for p in model.parameters()]


def _callback(*a, **kw):
    from multimodal_supernovae_amd.checkpoint import WeightAveraging
    return WeightAveraging(*a, **kw)


def _snapper():
    """A callback that clones the parameters after every optimizer step / at every training-epoch end / around validation."""
    from multimodal_supernovae_amd.checkpoint import Callback

    class Snap(Callback):
        def __init__(self):
            self.steps, self.epochs, self.before_val, self.at_epoch_end = [], [], [], []

        def on_optimizer_step(self, trainer):
            self.steps.append(_params(trainer.model))

        def on_train_epoch_end(self, trainer):
            self.epochs.append(_params(trainer.model))

        def on_validation_start(self, trainer):                # first in the list: in front of the average's swap
            self.before_val.append(_G()._states(trainer.model, trainer.optimizer))

        def on_epoch_end(self, trainer):                       # behind the validation and the swap back
            self.at_epoch_end.append(_G()._states(trainer.model, trainer.optimizer))

    return Snap()


def _recomputed(model, snaps, avg, decay):
    """The average recomputed eagerly by a second AveragedWeights from parameter snapshots (trainable parameters only)."""
    keep = [i for i, p in enumerate(model.parameters()) if p.requires_grad]
    return _fed([[s[i] for i in keep] for s in snaps], avg, decay)


def test_eager_trainer_ema_equals_the_hand_loop_and_leaves_training_alone():
    from multimodal_supernovae_amd import optim
    from multimodal_supernovae_amd.trainer import Trainer
    G = _G()
    batches = G._batches(8, 3, device="cpu")
    base = G._model()
    hand, with_cb, without = copy.deepcopy(base), copy.deepcopy(base), copy.deepcopy(base)
    opt = hand.configure_optimizers()["optimizer"]
    aw = optim.AveragedWeights(hand, "ema", 0.9)
    snaps = []
    for _ in range(2):
        for i, batch in enumerate(batches):
            opt.zero_grad(set_to_none=True)
            loss = hand.training_step(tuple(t.cuda() if t is not None else None for t in batch), i)
            loss.backward()
            opt.step()
            aw.update()
            snaps.append(_params(hand))
    cb = _callback("ema", 0.9, validate_with_average=False, apply_at_end=False)
    tr = Trainer(max_epochs=2, callbacks=[cb]).fit(with_cb, batches)
    plain = Trainer(max_epochs=2).fit(without, batches)
    torch.cuda.synchronize()
    assert tr.global_step == 6 == cb.averager.n_averaged == cb.averager.device_n_averaged() and not cb.averager.swapped
    assert cb.averager.names == [k for k, p in with_cb.named_parameters() if p.requires_grad] == aw.names
    for k, x, y in zip(aw.names, cb.averager.averages, aw.averages):
        assert torch.equal(x, y), k
    keep = [i for i, p in enumerate(hand.parameters()) if p.requires_grad]
    _check_sequence(cb.averager.averages, [[s[i] for i in keep] for s in snaps], "ema", 0.9)       # fp64 and torch's AveragedModel
    G._bitwise(without, plain.optimizer, with_cb, tr.optimizer)          # parameters, moments, step counts: as without the callback
    G._bitwise(hand, opt, with_cb, tr.optimizer)


def _drive(model, batches, averager, k=1):
    from multimodal_supernovae_amd.trainer import GraphedTrainStep
    step = GraphedTrainStep(model, model.configure_optimizers()["optimizer"], warmup=3, accumulate_grad_batches=k,
                            weight_averaging=averager)
    snaps = []
    for i, b in enumerate(batches):
        step(b, i)
        torch.cuda.synchronize()
        snaps.append(_params(model))
    return step, snaps


@pytest.mark.parametrize("odd", [False, True])
def test_graph_replay_averages_inside_the_recorded_step(odd):
    from multimodal_supernovae_amd import optim
    G = _G()
    batches = G._batches(8, 8)
    if odd:
        batches[5] = tuple(t[:5] if t is not None else None for t in batches[5])       # another shape: the eager path, mid-run
    averaged, plain = G._model(), None
    plain = copy.deepcopy(averaged)
    aw = optim.AveragedWeights(averaged, "ema", 0.9)
    step, snaps = _drive(averaged, batches, aw)
    step_plain, _ = _drive(plain, batches, None)
    assert step.graph is not None and step.calls == 8 and step_plain.graph is not None
    assert aw.n_averaged == 8 == aw.device_n_averaged()
    ref = _recomputed(averaged, snaps, "ema", 0.9)
    for k, x, y in zip(aw.names, aw.averages, ref.averages):
        assert torch.equal(x, y), k
    for (k, p), q in zip(averaged.named_parameters(), plain.parameters()):
        assert torch.equal(p, q), k


@pytest.mark.parametrize("graphed", [False, True])
def test_gating_by_start_step_and_every_n_steps(graphed):
    from multimodal_supernovae_amd.trainer import Trainer
    G = _G()
    batches = G._batches(8, 7, device="cpu")
    model = G._model()
    snap, cb = _snapper(), _callback("ema", 0.9, start_step=2, every_n_steps=2, apply_at_end=False)
    tr = Trainer(max_epochs=1, graphed_steps=graphed, callbacks=[snap, cb]).fit(model, batches)
    torch.cuda.synchronize()
    assert tr.global_step == 7 == len(snap.steps) and (tr.graphed_step is not None and tr.graphed_step.graph is not None) == graphed
    assert cb.averager.n_averaged == 2 == cb.averager.device_n_averaged()
    ref = _recomputed(model, [snap.steps[3], snap.steps[5]], "ema", 0.9)              # after steps 4 and 6 only
    for k, x, y in zip(cb.averager.names, cb.averager.averages, ref.averages):
        assert torch.equal(x, y), k


@pytest.mark.parametrize("graphed", [False, True])
def test_accumulation_averages_at_window_boundaries_only(graphed):
    from multimodal_supernovae_amd.trainer import Trainer
    G = _G()
    batches = G._batches(8, 7, device="cpu")                              # windows 3 + 3 + 1
    model = G._model()
    snap, cb = _snapper(), _callback("swa", apply_at_end=False)
    tr = Trainer(max_epochs=1, graphed_steps=graphed, accumulate_grad_batches=3, callbacks=[snap, cb]).fit(model, batches)
    torch.cuda.synchronize()
    assert tr.global_step == 3 == cb.averager.n_averaged == cb.averager.device_n_averaged() == len(snap.steps)
    assert (tr.graphed_step is not None and tr.graphed_step.graph is not None) == graphed
    ref = _recomputed(model, snap.steps, "swa", 0.999)
    for k, x, y in zip(cb.averager.names, cb.averager.averages, ref.averages):
        assert torch.equal(x, y), k


def test_epoch_mode_is_classic_swa():
    from multimodal_supernovae_amd.trainer import Trainer
    G = _G()
    batches = G._batches(8, 2, device="cpu")
    model = G._model()
    snap, cb = _snapper(), _callback("swa", update_on="epoch", start_epoch=1, apply_at_end=False)
    tr = Trainer(max_epochs=4, callbacks=[snap, cb]).fit(model, batches)
    torch.cuda.synchronize()
    assert tr.global_step == 8 and cb.averager.n_averaged == 3 == cb.averager.device_n_averaged() and len(snap.epochs) == 4
    keep = [i for i, p in enumerate(model.parameters()) if p.requires_grad]
    _check_sequence(cb.averager.averages, [[s[i] for i in keep] for s in snap.epochs[1:]], "swa", 0.999, against_torch=False)


def test_validation_runs_on_the_average_and_fit_ends_holding_it(tmp_path):
    from multimodal_supernovae_amd import checkpoint as C
    from multimodal_supernovae_amd.trainer import Trainer
    G = _G()
    batches, val = G._batches(8, 3, device="cpu"), G._batches(8, 5, device="cpu")[3:]
    base = G._model()
    model = copy.deepcopy(base)
    snap, cb = _snapper(), _callback("ema", 0.9)
    tr = Trainer(max_epochs=2, callbacks=[snap, cb]).fit(model, batches, val)
    torch.cuda.synchronize()
    assert len(tr.history["val_loss"]) == 2 and len(snap.before_val) == 2 == len(snap.at_epoch_end)
    for (before, steps_b), (after, steps_a) in zip(snap.before_val, snap.at_epoch_end):       # parameters and RAdam's moments
        assert steps_b == steps_a and len(before) == len(after) and all(torch.equal(x, y) for x, y in zip(before, after))
    assert cb.averager.swapped and cb.averager.n_averaged == 6
    averaged = cb.averager.averaged_state_dict()
    for k, p in model.named_parameters():                                 # apply_at_end: the model holds the average
        assert torch.equal(p, averaged[k]), k
    second = copy.deepcopy(base)
    second.load_state_dict(model.state_dict())
    missing = second.load_state_dict(averaged, strict=False)
    assert not missing.unexpected_keys
    got = Trainer().validate(second, val)["val_loss"]
    assert got == tr.history["val_loss"][-1], (got, tr.history["val_loss"])
    assert tr.validate(model, val)["val_loss"] == got                     # the model holds the average already: no second swap
    # a checkpoint written now still carries the LIVE weights as state_dict, and the model keeps the average
    path = tr.save_checkpoint(str(tmp_path / "after.ckpt"))
    ckpt = C.load_checkpoint(path)
    live = snap.at_epoch_end[-1][0]
    for (k, _), want in zip(model.named_parameters(), live):
        assert torch.equal(ckpt["state_dict"][k], want.cpu()), k
    assert ckpt["callbacks"][cb.state_key]["average"]["swapped"] is False and cb.averager.swapped
    cb.restore_live(tr)
    assert not cb.averager.swapped
    for (k, p), want in zip(model.named_parameters(), live):
        assert torch.equal(p, want), k
    # a second fit of the same Trainer starts from the live weights (swapped back first) and goes on averaging
    cb.averager.swap()
    tr.max_epochs = 3
    tr.fit(model, batches, val)
    assert cb.averager.n_averaged == 15 and cb.averager.swapped


def test_checkpoint_carries_the_average_and_resume_continues_it(tmp_path):
    from multimodal_supernovae_amd import checkpoint as C
    from multimodal_supernovae_amd.trainer import Trainer
    G = _G()
    batches, val = G._batches(8, 3, device="cpu"), G._batches(8, 4, device="cpu")[3:]
    base = G._model()
    whole, first = copy.deepcopy(base), copy.deepcopy(base)
    cw = _callback("ema", 0.9, apply_at_end=False)
    tw = Trainer(max_epochs=4, callbacks=[cw]).fit(whole, batches, val)
    c1, mc = _callback("ema", 0.9, apply_at_end=False), C.ModelCheckpoint(str(tmp_path / "ckpt"))
    t1 = Trainer(max_epochs=2, callbacks=[c1, mc]).fit(first, batches, val)
    assert t1.global_step == 6 and os.path.exists(mc.best_model_path)
    raw = torch.load(mc.best_model_path, weights_only=True)
    assert raw["callbacks"]["WeightAveraging"]["average"]["n_averaged"] == 6
    torch.manual_seed(77)
    other = G._model()
    with torch.no_grad():
        for p in other.parameters():
            p.add_(0.01)
    c2 = _callback("ema", 0.9, apply_at_end=False)
    t2 = Trainer(max_epochs=4, callbacks=[c2]).fit(other, batches, val, ckpt_path=mc.best_model_path)
    torch.cuda.synchronize()
    assert tw.global_step == t2.global_step == 12 and cw.averager.n_averaged == c2.averager.n_averaged == 12
    assert c2.averager.device_n_averaged() == 12
    for k, x, y in zip(cw.averager.names, cw.averager.averages, c2.averager.averages):
        assert torch.equal(x, y), k
    G._bitwise(whole, tw.optimizer, other, t2.optimizer)
    assert tw.history == t2.history
    # load_average: the file's averaged weights into a fresh model -> the averaged model's parameters and validation loss
    fresh = G._model()
    assert C.WeightAveraging.load_average(fresh, mc.best_model_path) == 6
    want = c1.averager.averaged_state_dict()
    for k, p in fresh.named_parameters():
        assert torch.equal(p, want[k]), k
    assert Trainer().validate(fresh, val)["val_loss"] == t1.history["val_loss"][-1]


def test_frozen_backbone_averages_the_head_only():
    import test_supervised_gpu as S
    from multimodal_supernovae_amd import optim
    from multimodal_supernovae_amd.trainer import Trainer
    model = S._head("classification", seed=3, freeze_backbone=True, learning_rate=1e-2)
    batches = [S._batch(16, seed=s) for s in range(3)]
    cb = _callback("ema", 0.5, apply_at_end=False)
    Trainer(max_epochs=1, callbacks=[cb]).fit(model, batches)
    aw = cb.averager
    head = [(k, p) for k, p in model.named_parameters() if p.requires_grad]
    assert head and all(k.startswith("mlp.") for k, _ in head) and any(k.startswith("clip_model.") for k, _ in model.named_parameters())
    assert aw.names == [k for k, _ in head] and aw.n_averaged == 3
    assert aw.flat.numel() == sum((p.numel() + 3) // 4 * 4 for _, p in head) and aw.numel == sum(p.numel() for _, p in head)
    assert isinstance(optim.AveragedWeights(model.mlp), optim.AveragedWeights)


def _convmixer():
    from multimodal_supernovae_amd.models_multimodal import LightCurveImageCLIP
    torch.manual_seed(0)
    tk = dict(n_out=8, emb=16, heads=4, depth=2, dropout=0.0, time_norm=20583.37, agg="mean")
    ck = dict(dim=8, depth=2, channels=3, kernel_size=5, patch_size=4, n_out=8, dropout_prob=0.0)
    model = LightCurveImageCLIP(enc_dim=16, logit_scale=10.0, nband=2, transformer_kwargs=tk, conv_kwargs=ck,
                                combinations=["host_galaxy", "lightcurve"], loss="softmax", lr=1e-3)
    g = torch.Generator().manual_seed(1)
    batches = []
    for _ in range(3):
        batches.append((torch.rand(8, 3, 16, 16, generator=g), torch.randn(8, 12, generator=g), torch.rand(8, 12, generator=g) * 100,
                        torch.ones(8, 12, dtype=torch.bool), None, None, None, None, None))
    return model.cuda().train(), batches


def test_use_buffers_averages_batchnorm_statistics_and_not_the_counters():
    from multimodal_supernovae_amd.trainer import Trainer
    model, batches = _convmixer()
    snap, cb = _snapper(), _callback("swa", use_buffers=True, apply_at_end=False)
    stats = []
    snap.on_optimizer_step = lambda trainer: stats.append({k: b.detach().clone() for k, b in trainer.model.named_buffers()})
    Trainer(max_epochs=1, callbacks=[snap, cb]).fit(model, batches)
    aw = cb.averager
    floating = [k for k, b in model.named_buffers() if b.is_floating_point()]
    counters = [k for k, b in model.named_buffers() if not b.is_floating_point()]
    assert any("running_mean" in k for k in floating) and any("running_var" in k for k in floating)
    assert any("num_batches_tracked" in k for k in counters)
    assert set(floating) <= set(aw.names) and not set(counters) & set(aw.names) and aw.n_averaged == 3
    got = dict(zip(aw.names, aw.averages))
    for k in floating:
        col = torch.stack([s[k].double() for s in stats])
        err = float((got[k].double() - col.mean(0)).abs().max())
        assert err <= 3 * 2.0 ** -22 * float(col.abs().max()), (k, err)
    assert all(int(b) == 3 for k, b in model.named_buffers() if "num_batches_tracked" in k)


def test_update_bn_averages_the_batch_statistics_cumulatively():
    """The reference comes from the unchanged BatchNorm path: from reset statistics one training forward with the default
    momentum 0.1 leaves running_mean = 0.1 m and running_var = 0.9 + 0.1 v, which gives the batch's m and v back with ten
    times the rounding of a value of size max(1, |v|); update_bn must leave their plain means over the batches.  Bound:
    (10 x 2 + 3) roundings of 2^-24 on max(1, |statistic|) -- the recovery, and three cumulative updates."""
    from multimodal_supernovae_amd import optim
    model, batches = _convmixer()
    batches = [tuple(t.cuda() if t is not None else None for t in b) for b in batches]
    bns = {k: m for k, m in model.named_modules() if isinstance(m, torch.nn.BatchNorm2d)}
    assert len(bns) >= 3
    per_batch = []
    with torch.no_grad():
        for i, b in enumerate(batches):
            for m in bns.values():
                m.running_mean.zero_()
                m.running_var.fill_(1.0)
            model.training_step(b, i)
            per_batch.append({k: (m.running_mean.double() / 0.1, (m.running_var.double() - 0.9) / 0.1) for k, m in bns.items()})
    model.eval()
    optim.update_bn(batches, model)
    assert not model.training                                             # the mode is put back
    from multimodal_supernovae_amd import ops
    assert ops.BN_MOMENTUM is None
    for k, m in bns.items():
        assert int(m.num_batches_tracked) == 3
        for j, got in enumerate((m.running_mean, m.running_var)):
            want = torch.stack([pb[k][j] for pb in per_batch]).mean(0)
            tol = 23 * 2.0 ** -24 * torch.clamp(want.abs(), min=1.0)
            assert bool(((got.double() - want).abs() <= tol).all()), (k, j, float((got.double() - want).abs().max()))


# ---------------------------------------------------------------------------------------------------------- two ranks
def test_two_ranks_hold_identical_averages_and_resume_from_one_file():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "dist_check_weight_avg.py")], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0 and "DIST CHECK OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
