"""Device-drawn pretraining masks, the parts that need no GPU.  First the restatement, on the host, of the draws of csrc/
pretrain_masks.hip (include/msn_hip.h states them): the 64-bit mixer, the multiply-high range reduction and the ranking by (key,
position), in numpy uint64 (wrapping) and -- for the scalars the numpy forms are checked against -- in Python integers.  The masks
themselves come from the host functions' own formulas (models_pretraining.continuous_masks_from_starts / random_masks_from_order),
never from the kernel; tests/test_pretrain_masks_gpu.py imports the restatement from here.  Then the tests: the restatement keeps
the mask rules and draws uniformly, the refactored host functions are what they were, the new constructor arguments, and the
argument checks of msn_pretrain_masks* that return before a launch."""
import ctypes
import inspect
import random

import numpy as np
import pytest
import torch

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
F_LIST = (0.0, 0.15, 0.3, 0.5, 1.0)


def mix_int(seed, c):
    """Python integers: the mixer dropout's keep_scale applies to c * GOLDEN + seed (csrc/rowops.hip)."""
    x = (c * GOLDEN + seed) & M64
    x ^= x >> 33
    x = (x * 0xff51afd7ed558ccd) & M64
    x ^= x >> 33
    x = (x * 0xc4ceb9fe1a85ec53) & M64
    x ^= x >> 33
    return x


def mulhi_int(a, b):
    return (a * b) >> 64


def mix(seed, c):
    """The same on a numpy array of counters (uint64 arithmetic wraps)."""
    with np.errstate(over="ignore"):
        x = np.asarray(c).astype(np.uint64) * np.uint64(GOLDEN) + np.uint64(seed & M64)
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xff51afd7ed558ccd)
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xc4ceb9fe1a85ec53)
        x ^= x >> np.uint64(33)
    return x


def mulhi64(a, b):
    """(a * b) >> 64 for uint64 `a` and 0 <= b < 2^31 from 32-bit halves: no intermediate reaches 2^64."""
    a = np.asarray(a, dtype=np.uint64)
    b = np.asarray(b).astype(np.uint64)
    lo, hi = a & np.uint64(0xffffffff), a >> np.uint64(32)
    return ((hi * b + ((lo * b) >> np.uint64(32))) >> np.uint64(32)).astype(np.int64)


def hidden_counts(n, f):
    """floor((double)n * f), the one floating-point product of the kernel."""
    return np.floor(np.asarray(n).astype(np.float64) * float(f)).astype(np.int64)


def contiguous_starts(pad, nbands, f, seed):
    """(B, nbands) run starts of mode 0: band k + mulhi64(mix(seed, i nbands + k), n - h + 1)."""
    pad = np.asarray(pad, dtype=bool)
    B, T = pad.shape
    band = T // nbands
    n = pad[:, :band * nbands].reshape(B, nbands, band).sum(axis=2)
    h = hidden_counts(n, f)
    with np.errstate(over="ignore"):
        c = np.arange(B, dtype=np.uint64)[:, None] * np.uint64(nbands) + np.arange(nbands, dtype=np.uint64)[None, :]
    return band * np.arange(nbands, dtype=np.int64)[None, :] + mulhi64(mix(seed, c), n - h + 1)


def contiguous_masks(pad, nbands, f, seed):
    """(mask_in, mask_pred, starts) of mode 0 as torch tensors on the CPU, through the host helper's formulas."""
    from multimodal_supernovae_amd.models_pretraining import continuous_masks_from_starts
    pad = torch.as_tensor(np.asarray(pad, dtype=bool))
    starts = torch.from_numpy(contiguous_starts(pad.numpy(), nbands, f, seed))
    mask_in, mask_pred = continuous_masks_from_starts(pad, nbands, starts, f)
    return mask_in, mask_pred, starts


def random_order(pad, seed):
    """(B, T) rank of every observed position among its sample's observed positions in the order by (mix(seed, i T + j), j);
    T at the padded positions."""
    pad = np.asarray(pad, dtype=bool)
    B, T = pad.shape
    with np.errstate(over="ignore"):
        keys = mix(seed, np.arange(B, dtype=np.uint64)[:, None] * np.uint64(T) + np.arange(T, dtype=np.uint64)[None, :])
    order = np.full((B, T), T, dtype=np.int64)
    for i in range(B):
        idx = np.flatnonzero(pad[i])
        order[i, idx[np.lexsort((idx, keys[i, idx]))]] = np.arange(len(idx))      # by key, ties by position
    return order


def random_masks(pad, f, seed):
    """(mask_in, mask_pred) of mode 1 on the CPU: the ranking above through the host helper's formulas."""
    from multimodal_supernovae_amd.models_pretraining import random_masks_from_order
    pad = np.asarray(pad, dtype=bool)
    return random_masks_from_order(torch.from_numpy(pad), torch.from_numpy(random_order(pad, seed)), f)


def packed_pad(counts, band, tail=0, tail_observed=True):
    """Padding mask whose band k of sample i holds counts[i][k] observed points packed at the band's start (the reference's
    layout), followed by `tail` positions behind the last whole band."""
    counts = np.asarray(counts, dtype=np.int64)
    B, nbands = counts.shape
    pad = np.arange(band)[None, None, :] < counts[:, :, None]
    pad = pad.reshape(B, nbands * band)
    if tail:
        pad = np.concatenate([pad, np.full((B, tail), tail_observed, dtype=bool)], axis=1)
    return pad


def check_contiguous_invariants(pad, nbands, f, mask_in, mask_pred):
    """On whole bands: the two masks partition the padding mask; every band hides exactly floor(n f) points, in one run."""
    pad, mask_in, mask_pred = (np.asarray(a, dtype=bool) for a in (pad, mask_in, mask_pred))
    B, T = pad.shape
    band = T // nbands
    W = band * nbands
    assert ((mask_in | mask_pred) == pad)[:, :W].all() and not (mask_in & mask_pred)[:, :W].any()
    assert (mask_in[:, W:] == pad[:, W:]).all() and (mask_pred[:, W:] == pad[:, W:]).all()
    hid = mask_pred[:, :W].reshape(B, nbands, band)
    n = pad[:, :W].reshape(B, nbands, band).sum(axis=2)
    assert (hid.sum(axis=2) == hidden_counts(n, f)).all()
    rises = (hid[:, :, 1:] & ~hid[:, :, :-1]).sum(axis=2) + hid[:, :, 0]
    assert (rises <= 1).all()                                  # one run (none where h = 0)


def check_random_invariants(pad, f, mask_in, mask_pred):
    pad, mask_in, mask_pred = (np.asarray(a, dtype=bool) for a in (pad, mask_in, mask_pred))
    assert ((mask_in | mask_pred) == pad).all() and not (mask_in & mask_pred).any()
    assert (mask_pred.sum(axis=1) == hidden_counts(pad.sum(axis=1), f)).all()


# -------------------------------------------------------------------------------------------------------------------- the tests
SEED = 0x5EED0FDEADBEEF          # fixed: every statistic below is deterministic


def test_numpy_restatement_equals_python_integers():
    """The vectorised mixer and multiply-high against Python's integers, on edge values and -- through the host helpers -- on
    whole masks: the draws written out sample by sample in Python integers give the masks the numpy forms give."""
    from multimodal_supernovae_amd.models_pretraining import continuous_masks_from_starts, random_masks_from_order
    rng = np.random.default_rng(0)
    cs = [0, 1, 2 ** 31, 2 ** 63 + 12345, M64] + [int(v) for v in rng.integers(0, 2 ** 63, 50)]
    for seed in (0, 1, SEED, M64, 2 ** 63):
        got = mix(seed, np.array(cs, dtype=np.uint64))
        assert [int(g) for g in got] == [mix_int(seed, c) for c in cs]
        for b in (1, 2, 17, 4097, 2 ** 31 - 1):
            assert [int(v) for v in mulhi64(got, b)] == [mulhi_int(int(g), b) for g in got]
    assert mix_int(0, 0) == 0                        # every step of the mixer maps 0 to 0
    counts = rng.integers(0, 8, size=(40, 3))
    pad = packed_pad(counts, 7, tail=2)
    B, T, nbands, band = 40, 23, 3, 7
    for seed, f in ((SEED, 0.3), (M64 - 1, 0.5)):
        starts = [[band * k + mulhi_int(mix_int(seed, i * nbands + k), int(counts[i, k]) - int(counts[i, k] * f) + 1)
                   for k in range(nbands)] for i in range(B)]
        want = continuous_masks_from_starts(torch.from_numpy(pad), nbands, torch.tensor(starts), f)
        got = contiguous_masks(pad, nbands, f, seed)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and got[2].tolist() == starts
        order = np.full((B, T), T, dtype=np.int64)
        for i in range(B):
            obs = [j for j in range(T) if pad[i, j]]
            for rank, j in enumerate(sorted(obs, key=lambda j: (mix_int(seed, i * T + j), j))):
                order[i, j] = rank
        want = random_masks_from_order(torch.from_numpy(pad), torch.from_numpy(order), f)
        got = random_masks(pad, f, seed)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


@pytest.mark.parametrize("f", F_LIST)
def test_restated_contiguous_masks_keep_the_rules(f):
    """B = 4096 samples of 2 bands x 12 + a ragged tail position: partition, floor(n f) hidden per band, one run each."""
    rng = np.random.default_rng(1)
    counts = rng.integers(0, 13, size=(4096, 2))
    counts[0], counts[1], counts[2] = (0, 0), (12, 12), (1, 12)
    pad = packed_pad(counts, 12, tail=1)
    mask_in, mask_pred, starts = contiguous_masks(pad, 2, f, SEED)
    check_contiguous_invariants(pad, 2, f, mask_in, mask_pred)
    n, h = counts, hidden_counts(counts, f)
    lo = 12 * np.arange(2)[None, :]
    assert ((starts.numpy() >= lo) & (starts.numpy() <= lo + n - h)).all()


@pytest.mark.parametrize("f", F_LIST)
def test_restated_random_masks_keep_the_rules(f):
    rng = np.random.default_rng(2)
    pad = rng.random((4096, 20)) > 0.3
    pad[0], pad[1] = False, True
    mask_in, mask_pred = random_masks(pad, f, SEED)
    check_random_invariants(pad, f, mask_in, mask_pred)


def _pearson(observed, expected):
    return float(((observed - expected) ** 2 / expected).sum())


def test_contiguous_starts_are_uniform():
    """4096 samples of one band, n = 21, h = floor(21 * 0.25) = 5: Pearson's statistic over the 17 possible starts stays below
    the 0.999 quantile of chi-square with 16 degrees of freedom."""
    pad = np.ones((4096, 21), dtype=bool)
    _, mask_pred, drawn = contiguous_masks(pad, 1, 0.25, SEED)
    assert (mask_pred.sum(dim=1) == 5).all()
    starts = mask_pred.to(torch.uint8).argmax(dim=1).numpy()          # where the hidden run begins, read from the mask itself
    assert (starts == drawn[:, 0].numpy()).all() and starts.min() >= 0 and starts.max() <= 16
    stat = _pearson(np.bincount(starts, minlength=17).astype(np.float64), 4096 / 17)
    print(f"contiguous starts: Pearson statistic {stat:.2f} (bound 39.25)")
    assert stat <= 39.25


def test_random_subsets_are_uniform():
    """n = 20, h = 5, 4096 samples: the statistic of the per-position hidden counts (expected 1024 each) stays below the 0.999
    quantile of chi-square with 19 degrees of freedom."""
    pad = np.ones((4096, 20), dtype=bool)
    _, mask_pred = random_masks(pad, 0.25, SEED)
    counts = mask_pred.numpy().sum(axis=0).astype(np.float64)
    assert counts.sum() == 4096 * 5
    stat = _pearson(counts, 4096 * 5 / 20)
    print(f"random subsets: Pearson statistic {stat:.2f} (bound 43.82)")
    assert stat <= 43.82


def _old_get_continous_random_mask(padding_mask, nbands, f_mask=0.15):
    """The body of get_continous_random_mask before its formulas moved into continuous_masks_from_starts, kept verbatim."""
    pad = padding_mask.to(torch.bool)
    B, T = pad.shape
    band = T // nbands
    n_obs = pad[:, :band * nbands].reshape(B, nbands, band).sum(dim=2)
    n_hide = (n_obs.to(torch.float64) * float(f_mask)).floor().to(torch.int64)
    starts = torch.tensor([[random.randint(band * k, band * k + n - h) for k, (n, h) in enumerate(zip(ns, hs))]
                           for ns, hs in zip(n_obs.tolist(), n_hide.tolist())], dtype=torch.int64).reshape(B, nbands)
    pos = torch.arange(T, device=pad.device)[None, :].expand(B, T)
    which = torch.clamp(pos // band, max=nbands - 1)
    lo = torch.gather(starts.to(pad.device), 1, which)
    hi = lo + torch.gather(n_hide.to(pad.device), 1, which)
    inside = (pos >= lo) & (pos < hi) & (pos < band * nbands)
    mask_pred = pad & inside
    mask_pred[:, band * nbands:] = pad[:, band * nbands:]
    return pad & ~inside, mask_pred


def _old_get_random_mask(padding_mask, f_mask=0.15):
    """The body of get_random_mask before its last two lines moved into random_masks_from_order, kept verbatim."""
    pad = padding_mask.to(torch.bool)
    B, T = pad.shape
    n_obs = pad.sum(dim=1)
    n_hide = (n_obs.to(torch.float64) * float(f_mask)).floor().to(torch.int64)
    order = torch.full((B, T), T, dtype=torch.int64)
    pad_host = pad.cpu()
    for i, n in enumerate(n_obs.tolist()):
        ranks = torch.empty(n, dtype=torch.int64)
        ranks[torch.randperm(n)] = torch.arange(n)
        order[i, pad_host[i]] = ranks
    hidden = order.to(pad.device) < n_hide.to(pad.device)[:, None]
    return pad & ~hidden, pad & hidden


@pytest.mark.parametrize("f", F_LIST)
def test_refactored_random_host_function_reproduces_its_previous_output(f):
    from multimodal_supernovae_amd.models_pretraining import get_random_mask, random_masks_from_order
    assert inspect.signature(random_masks_from_order).parameters["f_mask"].default == 0.15
    pad = torch.from_numpy(np.random.default_rng(7).random((16, 23)) > 0.3)
    pad[0], pad[1] = False, True
    torch.manual_seed(1234)
    want = _old_get_random_mask(pad, f)
    state = torch.get_rng_state()
    torch.manual_seed(1234)
    got = get_random_mask(pad, f)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert torch.equal(torch.get_rng_state(), state)   # the same draws, in the same order


@pytest.mark.parametrize("T,nbands,f", [(24, 2, 0.3), (23, 2, 0.25), (12, 1, 0.15), (30, 3, 1.0), (9, 2, 0.0)])
def test_refactored_host_function_reproduces_its_previous_output(T, nbands, f):
    from multimodal_supernovae_amd.models_pretraining import get_continous_random_mask
    rng = np.random.default_rng(T)
    band = T // nbands
    pad = torch.from_numpy(packed_pad(rng.integers(0, band + 1, size=(16, nbands)), band, tail=T - band * nbands))
    random.seed(1234)
    want = _old_get_continous_random_mask(pad, nbands, f)
    state = random.getstate()
    random.seed(1234)
    got = get_continous_random_mask(pad, nbands, f)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert random.getstate() == state                  # the same draws, in the same order
    assert inspect.signature(get_continous_random_mask).parameters["f_mask"].default == 0.15


def test_constructor_arguments():
    from multimodal_supernovae_amd.models_pretraining import MaskedLightCurveEncoder, device_masks
    p = inspect.signature(MaskedLightCurveEncoder.__init__).parameters
    assert list(p)[:8] == ["self", "f_mask", "nband", "transformer_kwargs", "optimizer_kwargs", "lr_scheduler_kwargs", "lr", "optimizer"]
    assert (p["f_mask"].default, p["nband"].default, p["lr"].default, p["optimizer"].default) == (0.2, 1, 1e-3, "radam")
    assert p["mask_generator"].default == "reference" and p["mask_type"].default == "continuous"
    tk = dict(n_out=1, emb=8, heads=2, depth=1)
    m = MaskedLightCurveEncoder(transformer_kwargs=tk)
    assert (m.mask_generator, m.mask_type, m.last_mask_pred) == ("reference", "continuous", None)
    m = MaskedLightCurveEncoder(transformer_kwargs=tk, mask_generator="device", mask_type="random")
    assert (m.mask_generator, m.mask_type) == ("device", "random")
    with pytest.raises(ValueError, match="mask_generator"):
        MaskedLightCurveEncoder(transformer_kwargs=tk, mask_generator="gpu")
    with pytest.raises(ValueError, match="mask_type"):
        MaskedLightCurveEncoder(transformer_kwargs=tk, mask_type="contiguous")
    with pytest.raises(ValueError, match="mask_type"):
        device_masks(torch.ones(2, 4, dtype=torch.bool), 1, mask_type="block")
    d = inspect.signature(device_masks).parameters
    assert d["f_mask"].default == 0.15 and d["mask_type"].default == "continuous" and d["seed"].default is None
    assert all(d[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("x", "mask_type", "seed", "return_starts"))


def test_reference_generator_is_refused_by_the_graphed_step_without_a_gpu():
    from multimodal_supernovae_amd.models_pretraining import MaskedLightCurveEncoder
    from multimodal_supernovae_amd.trainer import GraphedTrainStep
    tk = dict(n_out=1, emb=8, heads=2, depth=1)
    with pytest.raises(RuntimeError, match='mask_generator="device"'):
        GraphedTrainStep(MaskedLightCurveEncoder(transformer_kwargs=tk), None)
    GraphedTrainStep(MaskedLightCurveEncoder(transformer_kwargs=tk, mask_generator="device"), None)


def test_argument_errors_return_before_a_launch():
    """T > 4096, nbands outside [1, T], f_mask outside [0, 1] (NaN included), an unknown mode, null pointers: MSN_ERR_SHAPE from
    both entry points; the pointers are never dereferenced, so this runs without a GPU."""
    from multimodal_supernovae_amd import _lib
    L = _lib.lib()
    fake = ctypes.c_void_p(4096)
    bad = [dict(T=4097), dict(nbands=0), dict(nbands=13), dict(f=1.5), dict(f=-0.1), dict(f=float("nan")), dict(mode=2),
           dict(pad=None), dict(mask_in=None), dict(B=0), dict(x=fake, x_masked=None)]
    for kw in bad:
        a = dict(pad=fake, x=None, B=4, T=12, nbands=2, f=0.15, mode=0, mask_in=fake, mask_pred=fake, x_masked=None, starts=None)
        a.update(kw)
        head = (a["pad"], a["x"], a["B"], a["T"], a["nbands"], a["f"], a["mode"])
        tail = (a["mask_in"], a["mask_pred"], a["x_masked"], a["starts"], None)
        assert L.msn_pretrain_masks(*head, 7, *tail) == 1, kw
        assert b"msn_pretrain_masks:" in L.msn_last_error()
        assert L.msn_pretrain_masks_dev(*head, fake, 7, *tail) == 1, kw
        assert b"msn_pretrain_masks_dev:" in L.msn_last_error()
    assert L.msn_pretrain_masks_dev(fake, None, 4, 12, 2, 0.15, 0, None, 7, fake, fake, None, None, None) == 1
    assert b"seed base" in L.msn_last_error()
    assert L.msn_pretrain_masks(fake, None, 4, 4097, 2, 0.15, 0, 7, fake, fake, None, None, None) == 1
    assert b"4097" in L.msn_last_error()


def test_device_masks_needs_the_gpu():
    """No quiet host fall-back: a padding mask on the CPU is an error that says so."""
    from multimodal_supernovae_amd import _lib
    from multimodal_supernovae_amd.models_pretraining import device_masks
    with pytest.raises(_lib.MsnHipError):
        device_masks(torch.ones(2, 4, dtype=torch.bool), 1, seed=3)
