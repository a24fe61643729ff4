"""The Trainer with the optimizers named by `optimizer=` and with Lightning's lr_scheduler dict ("interval": "step" | "epoch",
"frequency"): against the same loop written by hand, bit for bit when eager, and under the graphed-against-eager bound of
tests/test_graph_gpu.py and tests/test_checkpoint_gpu.py (rtol 1e-5, atol 1e-7 on the parameters, 1e-5 relative on the losses)
when the step is replayed from a HIP graph.  Shapes: the tiny two-tower model of tests/test_grad_accum_gpu.py, 8 rows per batch,
2 epochs of 3 batches."""
import copy
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

TK = dict(n_out=8, emb=16, heads=4, depth=2, dropout=0.0, time_norm=20583.37, agg="mean")
SK = dict(n_out=8, emb=8, heads=2, depth=2, dropout=0.0, time_norm=17945.14, agg="mean")
COMBOS = ["lightcurve", "spectral"]
LR = 3e-3
EPOCHS, BATCHES = 2, 3


def warmup(step):
    """Linear warm-up over 4 optimizer steps: 1/4, 2/4, 3/4, 1, 1, ..."""
    return min(1.0, (step + 1) / 4.0)


def warmup_decay(step):
    """The same warm-up, then 10 % less per step: the lr changes in front of every step, replayed ones included."""
    return min((step + 1) / 4.0, 1.0 - 0.1 * (step - 3))


def _model(seed=0, optimizer="adamw"):
    from multimodal_supernovae_amd.models_multimodal import LightCurveImageCLIP
    torch.manual_seed(seed)
    return LightCurveImageCLIP(enc_dim=16, nband=2, transformer_kwargs=TK, transformer_spectral_kwargs=SK, combinations=COMBOS,
                               loss="softmax", lr=LR, optimizer_kwargs={"weight_decay": 1e-2}, optimizer=optimizer).cuda().train()


def _batches(n=8, steps=BATCHES):
    g = torch.Generator().manual_seed(5)
    out = []
    for _ in range(steps):
        mask = torch.ones(n, 12, dtype=torch.bool)
        mask[:, 9:] = torch.rand(n, 3, generator=g) > 0.5
        out.append((None, torch.randn(n, 12, generator=g), torch.rand(n, 12, generator=g) * 100, mask,
                    torch.randn(n, 10, generator=g), torch.rand(n, 10, generator=g) * 6000 + 3000,
                    torch.ones(n, 10, dtype=torch.bool), None, None))
    return out


def _scheduled(model, lr_scheduler, lrs=None):
    """model.configure_optimizers with "lr_scheduler": lr_scheduler(optimizer) added; `lrs` collects the lr every eager
    optimizer.step() runs with."""
    plain = model.configure_optimizers

    def configure():
        cfg = plain()
        cfg["lr_scheduler"] = lr_scheduler(cfg["optimizer"])
        if lrs is not None:
            cfg["optimizer"].register_step_pre_hook(lambda opt, args, kwargs: lrs.append(opt.param_groups[0]["lr"]))
        return cfg
    model.configure_optimizers = configure
    return model


def _by_step(fn, **more):
    return lambda opt: dict({"scheduler": torch.optim.lr_scheduler.LambdaLR(opt, fn), "interval": "step"}, **more)


def _hand_loop(model, batches, fn, epochs=EPOCHS, k=1):
    """zero_grad -> training_step -> backward -> optimizer.step() -> scheduler.step(), Lightning's order; with k > 1 torch's own
    AccumulateGrad adds (loss / k) over a window that closes at (i + 1) % k == 0 and on the last batch of the epoch."""
    opt = model.configure_optimizers()["optimizer"]
    sch = torch.optim.lr_scheduler.LambdaLR(opt, fn)
    lrs, losses = [], []
    opt.zero_grad(set_to_none=True)
    for _ in range(epochs):
        for i, batch in enumerate(batches):
            batch = tuple(t.cuda() if t is not None else None for t in batch)
            loss = model.training_step(batch, i)
            (loss if k == 1 else loss / k).backward()
            losses.append(loss.detach().clone())
            if (i + 1) % k == 0 or i == len(batches) - 1:
                lrs.append(opt.param_groups[0]["lr"])
                opt.step()
                sch.step()
                opt.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    return opt, sch, lrs, losses


def _states(model, opt):
    out, steps = [p.detach().clone() for p in model.parameters()], []
    for group in opt.param_groups:
        for p in group["params"]:
            st = opt.state.get(p, {})
            if len(st):
                out += [st["exp_avg"].clone(), st["exp_avg_sq"].clone()]
                steps.append(st["step"])
    return out, steps


def _bitwise(model_a, opt_a, model_b, opt_b):
    torch.cuda.synchronize()
    (ta, sa), (tb, sb) = _states(model_a, opt_a), _states(model_b, opt_b)
    assert len(ta) == len(tb) and len(sa) == len(sb) > 0
    assert all(type(s) is int for s in sa + sb) and sa == sb, (sa, sb)
    names = [k for k, _ in model_a.named_parameters()]
    for i, (x, y) in enumerate(zip(ta, tb)):
        assert torch.equal(x, y), (names[i] if i < len(names) else f"moment {i - len(names)}", float((x - y).abs().max()))


def test_eager_adamw_with_a_step_interval_warmup_is_the_loop_by_hand():
    from multimodal_supernovae_amd import optim
    from multimodal_supernovae_amd.trainer import Trainer
    batches = _batches()
    base = _model()
    hand, fitted = copy.deepcopy(base), copy.deepcopy(base)
    oh, sh, lrs_h, losses_h = _hand_loop(hand, batches, warmup)
    lrs = []
    tr = Trainer(max_epochs=EPOCHS).fit(_scheduled(fitted, _by_step(warmup), lrs), batches)
    assert type(tr.optimizer) is optim.AdamW and (tr.scheduler_interval, tr.scheduler_frequency) == ("step", 1)
    assert tr.global_step == 6 and tr.scheduler.last_epoch == sh.last_epoch == 6
    want = [LR * f for f in (0.25, 0.5, 0.75, 1.0, 1.0, 1.0)]
    assert lrs == lrs_h == want, (lrs, lrs_h, want)
    assert all(torch.equal(a, b) for a, b in zip(tr.step_losses, losses_h))
    _bitwise(hand, oh, fitted, tr.optimizer)
    assert all(s == 6 for s in _states(fitted, tr.optimizer)[1])


def test_accumulation_steps_the_scheduler_once_per_window():
    from multimodal_supernovae_amd.trainer import Trainer
    batches = _batches()
    base = _model()
    hand, fitted = copy.deepcopy(base), copy.deepcopy(base)
    oh, sh, lrs_h, losses_h = _hand_loop(hand, batches, warmup, k=2)          # windows 2 + 1 per epoch
    lrs = []
    tr = Trainer(max_epochs=EPOCHS, accumulate_grad_batches=2).fit(_scheduled(fitted, _by_step(warmup), lrs), batches)
    assert tr.global_step == 4 and len(tr.step_losses) == 6
    assert tr.scheduler.last_epoch == tr.global_step == sh.last_epoch, "the scheduler follows optimizer steps, not batches"
    assert lrs == lrs_h == [LR * f for f in (0.25, 0.5, 0.75, 1.0)]
    assert all(torch.equal(a, b) for a, b in zip(tr.step_losses, losses_h))
    _bitwise(hand, oh, fitted, tr.optimizer)


def test_an_epoch_interval_scheduler_is_stepped_after_the_epoch_only():
    from multimodal_supernovae_amd.trainer import Trainer
    lrs = []
    by_epoch = lambda opt: {"scheduler": torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5), "interval": "epoch"}   # noqa: E731
    tr = Trainer(max_epochs=EPOCHS).fit(_scheduled(_model(), by_epoch, lrs), _batches())
    assert (tr.scheduler_interval, tr.scheduler_frequency) == ("epoch", 1)
    assert tr.scheduler.last_epoch == 2 and tr.global_step == 6
    assert lrs == [LR] * 3 + [LR * 0.5] * 3, lrs                         # epoch 2 runs with the decayed lr
    assert tr.optimizer.param_groups[0]["lr"] == LR * 0.25
    # the bare scheduler (no dict) is the same thing
    lrs2 = []
    tr2 = Trainer(max_epochs=EPOCHS).fit(_scheduled(_model(), lambda opt: torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5), lrs2),
                                         _batches())
    assert lrs2 == lrs and tr2.scheduler.last_epoch == 2


def test_frequency_two_steps_the_scheduler_every_second_optimizer_step():
    from multimodal_supernovae_amd.trainer import Trainer
    lrs = []
    tr = Trainer(max_epochs=EPOCHS).fit(_scheduled(_model(), _by_step(warmup, frequency=2), lrs), _batches())
    assert tr.global_step == 6 and tr.scheduler.last_epoch == tr.global_step // 2 == 3
    assert lrs == [LR * f for f in (0.25, 0.25, 0.5, 0.5, 0.75, 0.75)], lrs


@pytest.mark.parametrize("schedule", [warmup, warmup_decay])
def test_graph_replayed_adamw_with_a_step_interval_scheduler_matches_eager(schedule):
    """Three eager warm-up calls, the capture, three replays.  With `warmup_decay` the lr changes in front of every replay:
    graph_pre_replay carries it into the device block the recorded launch reads."""
    from multimodal_supernovae_amd.trainer import Trainer
    batches = _batches()
    base = _model()
    eager, graphed = copy.deepcopy(base), copy.deepcopy(base)
    te = Trainer(max_epochs=EPOCHS).fit(_scheduled(eager, _by_step(schedule)), batches)
    tg = Trainer(max_epochs=EPOCHS, graphed_steps=True).fit(_scheduled(graphed, _by_step(schedule)), batches)
    torch.cuda.synchronize()
    assert tg.graphed_step.graph is not None and tg.global_step == te.global_step == 6
    assert tg.scheduler.last_epoch == te.scheduler.last_epoch == 6
    assert tg.optimizer.param_groups[0]["lr"] == te.optimizer.param_groups[0]["lr"] == LR * schedule(6)
    for x, y in zip(te.history["train_loss"], tg.history["train_loss"]):
        assert abs(x - y) <= 1e-5 * abs(x), (te.history, tg.history)
    for (k, p), (_, q) in zip(eager.named_parameters(), graphed.named_parameters()):
        torch.testing.assert_close(q, p, rtol=1e-5, atol=1e-7, msg=lambda m: f"{k}: {m}")
    assert _states(graphed, tg.optimizer)[1] == _states(eager, te.optimizer)[1] and set(_states(graphed, tg.optimizer)[1]) == {6}
    if schedule is warmup_decay:
        assert tg.optimizer._graph_hyper_seen[0][0] == LR * schedule(5), "the last replay did not run with the scheduler's lr"


def test_nesterov_sgd_fits_a_head_on_a_frozen_backbone():
    import test_supervised_gpu as S
    from multimodal_supernovae_amd import optim
    from multimodal_supernovae_amd.trainer import Trainer
    head = S._head("classification", seed=7, freeze_backbone=True, learning_rate=1e-2, optimizer="sgd",
                   optimizer_kwargs=dict(momentum=0.9, nesterov=True, weight_decay=1e-4))
    batches = [S._batch(8, seed=s) for s in range(BATCHES)]
    tr = Trainer(max_epochs=EPOCHS).fit(head, batches)
    torch.cuda.synchronize()
    before = S._head("classification", seed=7, freeze_backbone=True)
    assert type(tr.optimizer) is optim.SGD and tr.global_step == 6
    assert all(math.isfinite(float(x)) for x in tr.step_losses) and math.isfinite(tr.history["train_loss"][-1])
    for (k, p), (_, q) in zip(head.named_parameters(), before.named_parameters()):
        if k.startswith("mlp."):
            assert tr.optimizer.state[p]["momentum_buffer"].shape == p.shape
            assert bool(torch.isfinite(p).all()) and not torch.equal(p.cpu(), q.cpu()), k
        else:
            assert torch.equal(p.cpu(), q.cpu()) and len(tr.optimizer.state.get(p, {})) == 0, k


def test_resume_with_adamw_and_a_step_interval_scheduler_is_bitwise(tmp_path):
    """2 eager epochs, Trainer.save_checkpoint, a third epoch in a fresh model, optimizer and Trainer == 3 uninterrupted epochs."""
    from multimodal_supernovae_amd.trainer import Trainer
    batches = _batches()
    whole = _model(0)
    lrs_w = []
    tw = Trainer(max_epochs=3).fit(_scheduled(whole, _by_step(warmup_decay), lrs_w), batches)
    first = _model(0)
    t1 = Trainer(max_epochs=2).fit(_scheduled(first, _by_step(warmup_decay)), batches)
    path = str(tmp_path / "two_epochs.ckpt")
    t1.save_checkpoint(path)
    other = _model(7)
    lrs_o = []
    t2 = Trainer(max_epochs=3).fit(_scheduled(other, _by_step(warmup_decay), lrs_o), batches, ckpt_path=path)
    assert t2.global_step == tw.global_step == 9 and t2.scheduler.last_epoch == tw.scheduler.last_epoch == 9
    assert lrs_o == lrs_w[6:] and len(lrs_o) == 3, (lrs_w, lrs_o)
    assert t2.optimizer.param_groups[0]["lr"] == tw.optimizer.param_groups[0]["lr"]
    assert t2.history["train_loss"] == tw.history["train_loss"]
    _bitwise(whole, tw.optimizer, other, t2.optimizer)
