"""Device-drawn pretraining masks on the card: msn_pretrain_masks* against the host restatement of its draws (tests/
test_pretrain_masks_cpu.py, fed through the host functions' formulas) bit for bit, MaskedLightCurveEncoder(mask_generator="device")
against masked_loss with the masks read back, and the step recorded and replayed by GraphedTrainStep / Trainer(graphed_steps=True)
with new masks at every replay."""
import functools

import numpy as np
import pytest
import torch

import test_pretrain_masks_cpu as R          # the host restatement of the kernel's draws lives there

pytestmark = pytest.mark.gpu

SEEDS = (0x5EED0FDEADBEEF, (1 << 64) - 3)          # the second: counters times the golden ratio wrap around it
SHAPES = [(7, 23, 2), (3, 200, 2), (5, 12, 1), (2, 1, 1), (2, 4096, 2)]
TK = dict(n_out=1, emb=16, heads=4, depth=2, dropout=0.0, time_norm=20583.37)


@functools.lru_cache(maxsize=None)
def _pad(B, T, nbands, scattered):
    """Row 0 has no observed point, row 1 is fully observed, row 2 (where there is one) holds a band with n = 1; the others are
    random: packed at the start of each band (the reference's layout) or, for the random-subset mode, scattered."""
    rng = np.random.default_rng(1000 * T + nbands)
    band = T // nbands
    if scattered:
        pad = rng.random((B, T)) > 0.3
        if B > 2:
            pad[2] = False
            pad[2, T // 2] = True                    # n_obs = 1
    else:
        counts = rng.integers(0, band + 1, size=(B, nbands))
        if B > 2:
            counts[2, 0] = 1
        pad = R.packed_pad(counts, band, tail=T - band * nbands)
    pad[0], pad[1] = False, True
    return pad


@functools.lru_cache(maxsize=None)
def _reference(B, T, nbands, mode, f, seed):
    """(pad, mask_in, mask_pred, starts | None) on the CPU, computed once per case and left unchanged."""
    pad = _pad(B, T, nbands, mode == "random")
    if mode == "continuous":
        mask_in, mask_pred, starts = R.contiguous_masks(pad, nbands, f, seed)
        return pad, mask_in, mask_pred, starts.to(torch.int32)
    return (pad, *R.random_masks(pad, f, seed), None)


@pytest.mark.parametrize("mode", ["continuous", "random"])
@pytest.mark.parametrize("B,T,nbands", SHAPES)
def test_kernel_equals_the_restatement(B, T, nbands, mode):
    from multimodal_supernovae_amd.models_pretraining import device_masks
    g = torch.Generator().manual_seed(T)
    for f in R.F_LIST:
        for seed in SEEDS:
            pad, want_in, want_pred, want_starts = _reference(B, T, nbands, mode, f, seed)
            x = torch.randn(B, T, generator=g)
            hidden = (want_pred & ~want_in).nonzero()        # (behind the last whole band mask_pred keeps shown points)
            if len(hidden):                          # a NaN under a hidden point must leave as 0: a select, not a product
                x[hidden[0, 0], hidden[0, 1]] = float("nan")
            x[0, 0] = float("inf")                   # row 0 is all padding
            out = device_masks(torch.from_numpy(pad).cuda(), nbands, f, x=x.cuda(), mask_type=mode, seed=seed,
                               return_starts=mode == "continuous")
            what = f"{(B, T, nbands)} {mode} f={f} seed={seed:#x}"
            assert out[0].dtype == out[1].dtype == torch.bool
            assert torch.equal(out[0].cpu(), want_in), what
            assert torch.equal(out[1].cpu(), want_pred), what
            want_x = torch.where(want_in, x, torch.zeros(()))
            assert torch.equal(out[2].cpu(), want_x), (what, (out[2].cpu() != want_x).nonzero()[:4])
            if mode == "continuous":
                assert out[3].dtype == torch.int32 and torch.equal(out[3].cpu(), want_starts), what
            # without x: the same masks, nothing else
            bare = device_masks(torch.from_numpy(pad).cuda(), nbands, f, mask_type=mode, seed=seed)
            assert len(bare) == 2 and torch.equal(bare[0], out[0]) and torch.equal(bare[1], out[1]), what


def test_more_samples_than_workgroups():
    """66000 samples of (T 5, 2 bands + a tail position): the launch has 65536 workgroups, so 464 of them take a second sample
    and reuse their LDS row."""
    from multimodal_supernovae_amd.models_pretraining import device_masks
    rng = np.random.default_rng(4)
    pad = R.packed_pad(rng.integers(0, 3, size=(66000, 2)), 2, tail=1)
    want_in, want_pred, want_starts = R.contiguous_masks(pad, 2, 0.5, 13)
    got = device_masks(torch.from_numpy(pad).cuda(), 2, 0.5, seed=13, return_starts=True)
    assert torch.equal(got[0].cpu(), want_in) and torch.equal(got[1].cpu(), want_pred)
    assert torch.equal(got[2].cpu(), want_starts.to(torch.int32))
    want_in, want_pred = R.random_masks(pad, 0.5, 13)
    got = device_masks(torch.from_numpy(pad).cuda(), 2, 0.5, seed=13, mask_type="random")
    assert torch.equal(got[0].cpu(), want_in) and torch.equal(got[1].cpu(), want_pred)


def test_other_mask_dtypes():
    """A byte and a float padding mask give the bool mask's result; 300 samples of (T 23, 2 bands) against the restatement."""
    from multimodal_supernovae_amd.models_pretraining import device_masks
    rng = np.random.default_rng(3)
    pad = R.packed_pad(rng.integers(0, 12, size=(300, 2)), 11, tail=1)
    want_in, want_pred, _ = R.contiguous_masks(pad, 2, 0.3, 11)
    for dtype in (torch.bool, torch.uint8, torch.float32):
        got = device_masks(torch.from_numpy(pad).to(dtype).cuda(), 2, 0.3, seed=11)
        assert torch.equal(got[0].cpu(), want_in) and torch.equal(got[1].cpu(), want_pred), dtype
    want_in, want_pred = R.random_masks(pad, 0.3, 11)
    got = device_masks(torch.from_numpy(pad).cuda(), 2, 0.3, seed=11, mask_type="random")
    assert torch.equal(got[0].cpu(), want_in) and torch.equal(got[1].cpu(), want_pred)


@pytest.mark.parametrize("mode", ["continuous", "random"])
def test_host_seed_and_device_seed_base_agree(mode):
    from multimodal_supernovae_amd import ops
    from multimodal_supernovae_amd.models_pretraining import device_masks
    pad = torch.from_numpy(_pad(7, 23, 2, mode == "random")).cuda()
    x = torch.randn(7, 23, device="cuda")
    kw = dict(x=x, mask_type=mode, return_starts=mode == "continuous")
    seen = []
    for base, offset in [(12345, 678), (-5, 100), (2 ** 63 - 1, 2 ** 63 + 7)]:      # the last two sums wrap 64 bits
        seed = ((base & R.M64) + offset) & R.M64
        token = ops.SeedToken(torch.tensor([base], dtype=torch.int64, device="cuda"), offset)
        a = device_masks(pad, 2, 0.3, seed=seed, **kw)
        b = device_masks(pad, 2, 0.3, seed=token, **kw)
        assert len(a) == len(b) and all(torch.equal(p, q) for p, q in zip(a, b)), (base, offset)
        want = _reference(7, 23, 2, mode, 0.3, seed)
        assert torch.equal(a[0].cpu(), want[1]) and torch.equal(a[1].cpu(), want[2])
        seen.append(a[1].cpu())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])     # other seeds, other masks


def test_argument_errors_raise_before_a_launch():
    from multimodal_supernovae_amd import _lib
    from multimodal_supernovae_amd.models_pretraining import device_masks
    ok = torch.ones(2, 12, dtype=torch.bool, device="cuda")
    for pad, nbands, f, word in [(torch.ones(2, 4097, dtype=torch.bool, device="cuda"), 2, 0.15, "4097"), (ok, 0, 0.15, "nbands"),
                                 (ok, 13, 0.15, "nbands"), (ok, 2, 1.5, "f_mask"), (ok, 2, -0.5, "f_mask")]:
        for mode in ("continuous", "random"):
            with pytest.raises(_lib.MsnHipError, match=r"code 1\).*" + word):      # MSN_ERR_SHAPE: returned in front of the launch
                device_masks(pad, nbands, f, mask_type=mode, seed=1)
    with pytest.raises(ValueError, match="return_starts"):
        device_masks(ok, 2, mask_type="random", return_starts=True, seed=1)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------- the model
def _batch(B=8, T=12, seed=5, nine=False):
    g = torch.Generator().manual_seed(seed)
    pad = torch.from_numpy(R.packed_pad(torch.randint(2, 7, (B, 2), generator=g).numpy(), T // 2))
    x, t = torch.randn(B, T, generator=g), torch.rand(B, T, generator=g) * 100
    if nine:
        return (None, x, t, pad, None, None, None, None, None)
    return (t, x, pad)


def _cuda(batch):
    return tuple(v.cuda() if v is not None else None for v in batch)


def _model(lr=3e-3, seed=0, **kw):
    from multimodal_supernovae_amd.models_pretraining import MaskedLightCurveEncoder
    torch.manual_seed(seed)
    kw.setdefault("mask_generator", "device")
    return MaskedLightCurveEncoder(f_mask=0.3, nband=2, transformer_kwargs=TK, lr=lr, **kw).cuda().train()


@pytest.mark.parametrize("mask_type", ["continuous", "random"])
def test_device_step_equals_masked_loss_with_the_masks_read_back(mask_type):
    m = _model(mask_type=mask_type)
    t, x, pad = _cuda(_batch())
    loss = m.training_step((t, x, pad), 0)
    loss.backward()
    mask_in, mask_pred = m.last_mask_in, m.last_mask_pred
    assert mask_in.dtype == mask_pred.dtype == torch.bool and int(mask_pred.sum()) > 0
    if mask_type == "continuous":
        R.check_contiguous_invariants(pad.cpu(), 2, 0.3, mask_in.cpu(), mask_pred.cpu())
    else:
        R.check_random_invariants(pad.cpu(), 0.3, mask_in.cpu(), mask_pred.cpu())
    grads = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}   # (the unused pooling projection has none)
    assert len(grads) >= 30 and bool(grads["last_layer.weight"].abs().sum() > 0), list(grads)
    m.zero_grad(set_to_none=True)
    ref = m.masked_loss(x, t, pad, mask_in, mask_pred)
    ref.backward()
    assert torch.equal(loss.detach(), ref.detach()), (float(loss), float(ref))
    assert {k for k, p in m.named_parameters() if p.grad is not None} == set(grads)
    for k, p in m.named_parameters():
        if p.grad is not None:
            assert torch.equal(grads[k], p.grad), k
    # the 9-tuple batch of the multimodal loaders reads the same fields; the validation step runs the same path
    torch.manual_seed(9)
    a = m.training_step((t, x, pad), 0).detach()
    torch.manual_seed(9)
    b = m.validation_step((None, x, t, pad, None, None, None, None, None), 0).detach()
    assert torch.equal(a, b) and "val_loss" in m.logged


def test_eager_device_runs_repeat_under_one_torch_seed():
    batch = _cuda(_batch())

    def run():
        m = _model(seed=3)
        opt = m.configure_optimizers()["optimizer"]
        torch.manual_seed(21)
        masks = []
        for _ in range(4):
            opt.zero_grad(set_to_none=True)
            m.training_step(batch, 0).backward()
            opt.step()
            masks.append(m.last_mask_pred.clone())
        return m, masks

    (a, ma), (b, mb) = run(), run()
    for (k, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        assert torch.equal(p, q), k
    assert all(torch.equal(p, q) for p, q in zip(ma, mb))
    assert len({tuple(v.flatten().tolist()) for v in ma}) > 1            # and the steps did not share one mask


# ---------------------------------------------------------------------------------------------------------------- replay
@pytest.mark.parametrize("nine", [False, True])
def test_replays_draw_new_masks_and_repeat_under_one_torch_seed(nine):
    from multimodal_supernovae_amd.trainer import GraphedTrainStep
    batch = _cuda(_batch(nine=nine))
    x, t, pad = (batch[1], batch[2], batch[3]) if nine else (batch[1], batch[0], batch[2])

    def run():
        m = _model(lr=0.0, seed=11)
        step = GraphedTrainStep(m, m.configure_optimizers()["optimizer"], warmup=2)
        losses, preds, ins = [], [], []
        for _ in range(7):
            loss = step(batch)
            torch.cuda.synchronize()
            losses.append(float(loss.detach()))
            preds.append(m.last_mask_pred.clone())
            ins.append(m.last_mask_in.clone())
        assert step.graph is not None
        return m, losses, preds, ins

    m, losses, preds, ins = run()
    assert len({tuple(p.flatten().tolist()) for p in preds[2:]}) >= 4, "the 5 replays must not share their masks"
    for loss, mask_in, mask_pred in zip(losses[2:], ins[2:], preds[2:]):
        R.check_contiguous_invariants(pad.cpu(), 2, 0.3, mask_in.cpu(), mask_pred.cpu())
        with torch.no_grad():                                            # lr = 0: the weights are the recorded step's
            eager = float(m.masked_loss(x, t, pad, mask_in, mask_pred))
        assert abs(loss - eager) <= 1e-5 * abs(eager), (loss, eager)
    _, losses_b, preds_b, ins_b = run()
    assert losses == losses_b
    assert all(torch.equal(p, q) for p, q in zip(preds + ins, preds_b + ins_b))


def _epochs(nine=False):
    batches = [_batch(seed=s, nine=nine) for s in range(6)]
    batches[-1] = tuple(v[:3] if v is not None else None for v in batches[-1])      # a short last batch: one eager step
    return batches


@pytest.mark.parametrize("k,nine", [(1, False), (2, True)])
def test_trainer_with_graphed_steps(k, nine):
    """Two epochs of 6 batches, the last one short, replayed (accumulate_grad_batches = 2: windows of two micro-batches): the
    run ends with one finite epoch loss per epoch and one finite loss per batch, and the step was recorded."""
    from multimodal_supernovae_amd.trainer import Trainer
    m = _model(seed=1)
    tr = Trainer(max_epochs=2, graphed_steps=True, accumulate_grad_batches=k).fit(m, _epochs(nine))
    torch.cuda.synchronize()
    assert tr.graphed_step.graph is not None
    hist = tr.history["train_loss"]
    assert len(hist) == 2 and all(np.isfinite(hist)), hist
    assert len(tr.step_losses) == 12 and all(bool(torch.isfinite(v)) for v in tr.step_losses)
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())
    # The same initial model on the same data, trained eagerly with its own mask draws, ends at the same loss level.  Bound: x is
    # standard normal and the untrained read-out is near 0, so a step's loss is a mean of ~9 squares of N(0, 1) draws (16 bands,
    # 6 in 10 of which hide one point: relative sd sqrt(2 / 9) = 0.47) and the mean over the 12 steps has a relative sd of 0.14
    # in either run, their ratio one of 0.19: a factor 3 is more than 5 sd.
    e = _model(seed=1)
    te = Trainer(max_epochs=2, accumulate_grad_batches=k).fit(e, _epochs(nine))
    assert len(te.history["train_loss"]) == len(hist) and len(te.step_losses) == 12
    mean_g = float(torch.stack([v.float() for v in tr.step_losses]).mean())
    mean_e = float(torch.stack([v.float() for v in te.step_losses]).mean())
    print(f"mean step loss: graphed {mean_g:.4f}, eager {mean_e:.4f}")
    assert 1 / 3 <= mean_g / mean_e <= 3.0, (mean_g, mean_e)


@pytest.mark.parametrize("k", [1, 2])
def test_last_masks_are_the_replayed_steps_after_eager_calls_in_between(k):
    """A short batch (one eager step) and a validation step rebind model.last_mask_*; the next replay must put the recording's
    tensors back: recorded shape, the mask rules, and the replayed loss reproduced by masked_loss with them."""
    from multimodal_supernovae_amd.trainer import GraphedTrainStep
    batch = _cuda(_batch())
    t, x, pad = batch
    short = tuple(v[:3] for v in batch)
    m = _model(lr=0.0, seed=11)
    step = GraphedTrainStep(m, m.configure_optimizers()["optimizer"], warmup=2, accumulate_grad_batches=k)
    for _ in range(4):
        step(batch)
    assert step.graph is not None
    torch.cuda.synchronize()
    recorded_in, recorded_pred = m.last_mask_in, m.last_mask_pred
    assert recorded_pred.shape == (8, 12)
    before = recorded_pred.clone()
    step(short, last_batch=True)                     # another shape: runs eagerly, as the last batch of an epoch does
    assert m.last_mask_pred.shape == (3, 12)
    m.validation_step(short, 0)
    assert m.last_mask_pred.shape == (3, 12) and m.last_mask_pred is not recorded_pred
    for _ in range(2):
        loss = step(batch)
        torch.cuda.synchronize()
        assert m.last_mask_pred is recorded_pred and m.last_mask_in is recorded_in
        mask_in, mask_pred = m.last_mask_in.clone(), m.last_mask_pred.clone()
        R.check_contiguous_invariants(pad.cpu(), 2, 0.3, mask_in.cpu(), mask_pred.cpu())
        with torch.no_grad():
            eager = float(m.masked_loss(x, t, pad, mask_in, mask_pred))
        assert abs(float(loss.detach()) - eager) <= 1e-5 * abs(eager), (float(loss.detach()), eager)
    assert not torch.equal(before, mask_pred)        # and the replays went on drawing


def test_reference_generator_with_random_subsets():
    """mask_generator="reference", mask_type="random": get_random_mask's draws (torch.randperm under the torch seed)."""
    from multimodal_supernovae_amd.models_pretraining import get_random_mask
    m = _model(mask_generator="reference", mask_type="random")
    t, x, pad = _cuda(_batch())
    torch.manual_seed(4)
    loss = m.training_step((t, x, pad), 0)
    torch.manual_seed(4)
    want_in, want_pred = get_random_mask(pad, f_mask=0.3)
    assert torch.equal(m.last_mask_in, want_in) and torch.equal(m.last_mask_pred, want_pred)
    R.check_random_invariants(pad.cpu(), 0.3, want_in.cpu(), want_pred.cpu())
    assert int(want_pred.sum()) > 0
    assert torch.equal(loss.detach(), m.masked_loss(x, t, pad, want_in, want_pred).detach())


def test_reference_generator_cannot_be_recorded():
    from multimodal_supernovae_amd.trainer import GraphedTrainStep, Trainer
    m = _model(mask_generator="reference")
    with pytest.raises(RuntimeError, match='mask_generator="device"'):
        GraphedTrainStep(m, m.configure_optimizers()["optimizer"], warmup=2)
    with pytest.raises(RuntimeError, match='mask_generator="device"'):
        Trainer(max_epochs=1, graphed_steps=True).fit(m, _epochs())
    # a model switched after construction is refused in front of the recording, not inside the capture
    m = _model()
    step = GraphedTrainStep(m, m.configure_optimizers()["optimizer"], warmup=1)
    batch = _cuda(_batch())
    step(batch)
    m.mask_generator = "reference"
    with pytest.raises(RuntimeError, match='mask_generator="device"'):
        step(batch)
    assert step.graph is None and not torch.cuda.is_current_stream_capturing()
    torch.cuda.synchronize()
