"""checkpoint.py without a GPU: the file layout, optimizer-state interop with torch.optim.RAdam, the bookkeeping of
ModelCheckpoint and EarlyStopping against a stub trainer, and the atomic write."""
import copy
import math
import os

import pytest
import torch
import torch.nn as nn

LAYOUT = {"epoch", "global_step", "pytorch-lightning_version", "state_dict", "optimizer_states", "lr_schedulers", "callbacks",
          "msn"}


class _Net(nn.Module):
    def __init__(self, seed=0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.a = nn.Parameter(torch.randn(5, 3, generator=g))
        self.b = nn.Parameter(torch.randn(7, generator=g))
        self.register_buffer("count", torch.tensor(3))

    def loss(self, i):
        g = torch.Generator().manual_seed(100 + i)
        return ((self.a * torch.randn(5, 3, generator=g)).sum() ** 2 + (self.b * torch.randn(7, generator=g)).sum() ** 2
                + (self.a ** 2).sum())


def _torch_radam(net):
    return torch.optim.RAdam(net.parameters(), lr=3e-3, weight_decay=1e-3)


def _steps(net, opt, first, last):
    for i in range(first, last):
        opt.zero_grad()
        net.loss(i).backward()
        opt.step()


def _state_steps(opt):
    return [st["step"] for st in opt.state.values()]


def test_file_layout_loads_weights_only_with_int_steps(tmp_path):
    from multimodal_supernovae_amd.checkpoint import load_checkpoint, save_checkpoint
    net = _Net()
    opt = _torch_radam(net)                                   # tensor steps, torch's extra group keys
    _steps(net, opt, 0, 3)
    sch = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
    path = tmp_path / "a.ckpt"
    save_checkpoint(path, net, opt, sch, extra={"epoch": 2, "global_step": 3, "callbacks": {"cb": {"n": 1}},
                                                "history": {"train_loss": [1.0, 0.5], "val_loss": []}})
    raw = torch.load(path, weights_only=True)                 # the form INTEGRATION.md shows
    assert set(raw) == LAYOUT and type(raw) is dict
    assert raw["epoch"] == 2 and raw["global_step"] == 3 and isinstance(raw["pytorch-lightning_version"], str)
    assert isinstance(raw["optimizer_states"], list) and isinstance(raw["lr_schedulers"], list) and raw["callbacks"] == {"cb": {"n": 1}}
    steps = [st["step"] for st in raw["optimizer_states"][0]["state"].values()]
    assert steps == [3, 3] and all(type(s) is int for s in steps)
    assert set(raw["state_dict"]) == {"a", "b", "count"}
    for k, v in net.state_dict().items():
        assert torch.equal(raw["state_dict"][k], v) and raw["state_dict"][k].device.type == "cpu"
    assert raw["msn"]["history"] == {"train_loss": [1.0, 0.5], "val_loss": []} and raw["msn"]["world_size"] == 1
    assert len(raw["msn"]["rng"]) == 1 and torch.equal(raw["msn"]["rng"][0]["torch_cpu"], torch.get_rng_state())
    ck = load_checkpoint(path)
    assert set(ck) == LAYOUT and ck["lr_schedulers"][0]["gamma"] == 0.5
    # a Lightning file: unknown keys are ignored, tensor steps become ints, absent keys are empty
    theirs = {"state_dict": net.state_dict(), "optimizer_states": [opt.state_dict()], "loops": {"fit_loop": {"x": 1}},
              "hparams_name": "kwargs", "epoch": 5, "global_step": 77, "pytorch-lightning_version": "2.1.3"}
    torch.save(theirs, tmp_path / "theirs.ckpt")
    ck = load_checkpoint(tmp_path / "theirs.ckpt")
    assert set(ck) == LAYOUT and ck["msn"] is None and ck["epoch"] == 5 and ck["lr_schedulers"] == [] and ck["callbacks"] == {}
    assert all(type(st["step"]) is int and st["step"] == 3 for st in ck["optimizer_states"][0]["state"].values())


def test_save_refuses_what_weights_only_cannot_load(tmp_path):
    from multimodal_supernovae_amd.checkpoint import save_checkpoint
    with pytest.raises(TypeError, match="cannot be stored"):
        save_checkpoint(tmp_path / "a.ckpt", _Net(), extra={"history": {"x": [object()]}})
    assert os.listdir(tmp_path) == []


def test_rng_states_round_trip(tmp_path):
    import random

    import numpy as np
    from multimodal_supernovae_amd.checkpoint import load_checkpoint, restore_rng, save_checkpoint
    torch.manual_seed(11)
    random.seed(12)
    np.random.seed(13)
    np.random.standard_normal(3)                              # leaves a cached gaussian in numpy's state
    save_checkpoint(tmp_path / "a.ckpt", _Net())
    want = (torch.rand(3), random.random(), np.random.standard_normal(2))
    torch.manual_seed(0)
    random.seed(0)
    np.random.seed(0)
    assert restore_rng(load_checkpoint(tmp_path / "a.ckpt"))
    got = (torch.rand(3), random.random(), np.random.standard_normal(2))
    assert torch.equal(got[0], want[0]) and got[1] == want[1] and (got[2] == want[2]).all()


def test_radam_state_round_trip_with_torch_radam_is_bitwise(tmp_path):
    """torch RAdam, 7 steps -> (deep copy) our RAdam -> file -> a fresh torch RAdam: its eighth step is the original's."""
    from multimodal_supernovae_amd.checkpoint import load_checkpoint, save_checkpoint
    from multimodal_supernovae_amd.optim import RAdam
    net = _Net()
    opt = _torch_radam(net)
    _steps(net, opt, 0, 7)
    assert all(torch.is_tensor(s) for s in _state_steps(opt))
    mid = copy.deepcopy(net)
    ours = RAdam(mid.parameters(), lr=3e-3, weight_decay=1e-3)          # constructed on CPU parameters
    ours.load_state_dict(copy.deepcopy(opt.state_dict()))
    assert _state_steps(ours) == [7, 7] and all(type(s) is int for s in _state_steps(ours))
    save_checkpoint(tmp_path / "o.ckpt", mid, ours)
    ck = load_checkpoint(tmp_path / "o.ckpt")
    fresh = _Net(seed=9)
    fresh.load_state_dict(ck["state_dict"], strict=True)
    opt2 = _torch_radam(fresh)
    opt2.load_state_dict(ck["optimizer_states"][0])
    _steps(net, opt, 7, 8)
    _steps(fresh, opt2, 7, 8)
    for (k, p), (_, q) in zip(net.named_parameters(), fresh.named_parameters()):
        print(k, "max |difference| after the eighth step", float((p - q).detach().abs().max()))
        assert torch.equal(p, q), k
    for p, q in zip(net.parameters(), fresh.parameters()):
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(opt.state[p][key], opt2.state[q][key])
        assert float(opt.state[p]["step"]) == float(opt2.state[q]["step"]) == 8.0


def test_our_load_state_dict_never_aliases_the_dict_it_is_given():
    from multimodal_supernovae_amd.optim import RAdam
    net = _Net()
    opt = _torch_radam(net)
    _steps(net, opt, 0, 2)
    live = opt.state_dict()                                   # references the live moment tensors of `opt`
    ours = RAdam(copy.deepcopy(net).parameters(), lr=3e-3)
    ours.load_state_dict(live)
    for p, q in zip(opt.param_groups[0]["params"], ours.param_groups[0]["params"]):
        for key in ("exp_avg", "exp_avg_sq"):
            assert ours.state[q][key].data_ptr() != opt.state[p][key].data_ptr()
            assert torch.equal(ours.state[q][key], opt.state[p][key])
    # our own state dict round-trips through our own load too, steps staying ints
    again = RAdam(copy.deepcopy(net).parameters(), lr=3e-3)
    again.load_state_dict(ours.state_dict())
    assert _state_steps(again) == [2, 2] and all(type(s) is int for s in _state_steps(again))


# ---------------------------------------------------------------------------------------------- callbacks
class _StubTrainer:
    """What a callback needs of a Trainer: 4 steps per epoch, monitored values from a fixed list, saves as small files."""

    def __init__(self, scores, name="val_loss"):
        self.scores, self.name = scores, name
        self.current_epoch, self.global_step, self.should_stop, self.is_global_zero = 0, 0, False, True
        self.saved = []

    def monitored(self, name):
        assert name == self.name, name
        return self.scores[self.current_epoch]

    def save_checkpoint(self, path):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            f.write(f"epoch {self.current_epoch}")
        self.saved.append(os.path.basename(path))

    def barrier(self):
        pass

    def run(self, callbacks, first=0):
        for epoch in range(first, len(self.scores)):
            if self.should_stop:
                return epoch
            self.current_epoch, self.global_step = epoch, 4 * (epoch + 1)
            for cb in callbacks:
                cb.on_epoch_end(self)
        return len(self.scores)


def _name(e):
    return f"epoch={e}-step={4 * (e + 1)}.ckpt"


SCORES = [0.5, 0.3, math.nan, 0.3, 0.7, 0.2]
# min, k = 2: {0, 1}; the NaN of epoch 2 ranks worst; epoch 3 (0.3) beats the worst kept (0.5) -> {1, 3}; 0.7 does not; epoch 5
#             (0.2) replaces the worst kept, 0.3 -- of the two equal ones the earlier, epoch 1 -> {3, 5}, best epoch 5
# max, k = 2: {0, 1}; NaN worst; epoch 3 (0.3) only EQUALS the worst kept (epoch 1) and does not replace it; epoch 4 (0.7)
#             does -> {0, 4}; 0.2 does not; best epoch 4
TOPK = {"min": ([3, 5], 5, 0.2), "max": ([0, 4], 4, 0.7)}


@pytest.mark.parametrize("mode", ["min", "max"])
@pytest.mark.parametrize("save_last", [False, True])
def test_model_checkpoint_keeps_the_k_best(tmp_path, mode, save_last):
    from multimodal_supernovae_amd.checkpoint import ModelCheckpoint
    cb = ModelCheckpoint(tmp_path, monitor="val_loss", mode=mode, save_top_k=2, save_last=save_last)
    _StubTrainer(SCORES).run([cb])
    keep, best, score = TOPK[mode]
    want = {_name(e) for e in keep} | ({"last.ckpt"} if save_last else set())
    assert set(os.listdir(tmp_path)) == want
    assert cb.best_model_path == str(tmp_path / _name(best)) and cb.best_model_score == score
    assert cb.best_k_models == {str(tmp_path / _name(e)): SCORES[e] for e in keep}
    assert cb.kth_best_model_path == str(tmp_path / _name(keep[0]))
    if save_last:
        last = tmp_path / "last.ckpt"
        assert cb.last_model_path == str(last) and last.is_file() and not last.is_symlink()
        assert last.read_text() == "epoch 5"                  # written at every epoch, also one that is not among the best
    else:
        assert cb.last_model_path == ""


def test_model_checkpoint_top_k_all_none_and_every_n_epochs(tmp_path):
    from multimodal_supernovae_amd.checkpoint import ModelCheckpoint
    every = ModelCheckpoint(tmp_path / "all", monitor="val_loss", save_top_k=-1)
    none = ModelCheckpoint(tmp_path / "none", monitor="val_loss", save_top_k=0, save_last=True)
    second = ModelCheckpoint(tmp_path / "second", every_n_epochs=2, save_top_k=-1)
    latest = ModelCheckpoint(tmp_path / "latest")            # monitor None: the latest file only
    nothing = ModelCheckpoint(tmp_path / "nothing", save_top_k=0)
    _StubTrainer(SCORES).run([every, none, second, latest, nothing])
    assert set(os.listdir(tmp_path / "all")) == {_name(e) for e in range(6)}
    assert every.best_model_path == str(tmp_path / "all" / _name(5))
    assert os.listdir(tmp_path / "none") == ["last.ckpt"] and none.best_model_path == ""
    assert set(os.listdir(tmp_path / "second")) == {_name(1), _name(3), _name(5)}
    assert os.listdir(tmp_path / "latest") == [_name(5)] and latest.best_model_path == str(tmp_path / "latest" / _name(5))
    assert not (tmp_path / "nothing").exists()
    with pytest.raises(ValueError):
        ModelCheckpoint(tmp_path, save_top_k=3)               # k > 1 needs a monitor, as Lightning says
    with pytest.raises(ValueError):
        ModelCheckpoint(tmp_path, monitor="val_loss", mode="smallest")


def test_model_checkpoint_name_template(tmp_path):
    from multimodal_supernovae_amd.checkpoint import ModelCheckpoint
    cb = ModelCheckpoint(tmp_path, filename="clip-{epoch:02d}-{val_loss:.3f}", monitor="val_loss")
    assert cb.format_checkpoint_name(3, 16, {"val_loss": 0.12345}) == str(tmp_path / "clip-epoch=03-val_loss=0.123.ckpt")
    assert ModelCheckpoint(tmp_path).format_checkpoint_name(0, 4) == str(tmp_path / "epoch=0-step=4.ckpt")
    tr = _StubTrainer([0.25, 0.125])
    tr.run([cb])
    assert tr.saved == ["clip-epoch=00-val_loss=0.250.ckpt", "clip-epoch=01-val_loss=0.125.ckpt"]
    assert os.listdir(tmp_path) == ["clip-epoch=01-val_loss=0.125.ckpt"]
    other = ModelCheckpoint(tmp_path / "o", filename="{step}_{AUC_val:.2f}")       # a logged name that is not the monitor
    _StubTrainer([0.5], name="AUC_val").run([other])
    assert os.listdir(tmp_path / "o") == ["step=4_AUC_val=0.50.ckpt"]


def test_model_checkpoint_state_dict_round_trip(tmp_path):
    from multimodal_supernovae_amd.checkpoint import ModelCheckpoint
    cb = ModelCheckpoint(tmp_path, monitor="val_loss", save_top_k=2, save_last=True)
    _StubTrainer(SCORES[:4]).run([cb])
    state = cb.state_dict()
    torch.save(state, tmp_path / "state.pt")
    state = torch.load(tmp_path / "state.pt", weights_only=True)
    os.remove(tmp_path / "state.pt")
    new = ModelCheckpoint(tmp_path, monitor="val_loss", save_top_k=2, save_last=True)
    assert new.state_key == cb.state_key != ModelCheckpoint(tmp_path, monitor="AUC_val", mode="max").state_key
    new.load_state_dict(state)
    for attr in ("best_model_path", "best_model_score", "best_k_models", "kth_best_model_path", "last_model_path"):
        assert getattr(new, attr) == getattr(cb, attr), attr
    tr = _StubTrainer(SCORES)                                 # goes on where the first run stopped: the same end as one run
    tr.run([new], first=4)
    assert set(os.listdir(tmp_path)) == {_name(3), _name(5), "last.ckpt"}


def test_early_stopping(tmp_path):
    from multimodal_supernovae_amd.checkpoint import EarlyStopping
    # patience: the third epoch in a row without improvement stops (epochs 3, 4, 5 after the best at epoch 2)
    tr = _StubTrainer([1.0, 0.9, 0.8, 0.8, 0.85, 0.9, 0.1, 0.0])
    cb = EarlyStopping("val_loss", patience=3)
    assert tr.run([cb]) == 6 and tr.should_stop and cb.wait_count == 3 and cb.stopped_epoch == 5 and cb.best_score == 0.8
    # an improvement resets the count
    tr = _StubTrainer([1.0, 1.0, 1.0, 0.9, 1.0, 1.0, 0.8])
    cb = EarlyStopping("val_loss", patience=3)
    assert tr.run([cb]) == 7 and not tr.should_stop and cb.wait_count == 0
    # min_delta: an improvement of no more than min_delta does not count
    tr = _StubTrainer([1.0, 0.95, 0.91, 0.5])
    cb = EarlyStopping("val_loss", patience=2, min_delta=0.1)
    assert tr.run([cb]) == 3 and tr.should_stop and cb.best_score == 1.0
    # mode max
    tr = _StubTrainer([0.5, 0.6, 0.55, 0.6, 0.7], name="AUC_val")
    cb = EarlyStopping("AUC_val", mode="max", patience=2)
    assert tr.run([cb]) == 4 and tr.should_stop and cb.best_score == 0.6 and cb.stopped_epoch == 3
    tr = _StubTrainer([0.5, 0.6, 0.65, 0.64, 0.7], name="AUC_val")
    assert tr.run([EarlyStopping("AUC_val", mode="max", patience=2)]) == 5 and not tr.should_stop
    # check_finite
    tr = _StubTrainer([1.0, math.nan, 0.5])
    assert tr.run([EarlyStopping("val_loss", patience=5)]) == 2 and tr.should_stop
    tr = _StubTrainer([1.0, math.inf, 0.5, 0.4])
    cb = EarlyStopping("val_loss", patience=5, check_finite=False)
    assert tr.run([cb]) == 4 and not tr.should_stop and cb.best_score == 0.4


def test_early_stopping_state_dict_round_trip(tmp_path):
    from multimodal_supernovae_amd.checkpoint import EarlyStopping
    scores = [1.0, 0.9, 0.95, 0.95, 0.95, 0.1]
    whole = EarlyStopping("val_loss", patience=3)
    assert _StubTrainer(scores).run([whole]) == 5
    first = EarlyStopping("val_loss", patience=3)
    _StubTrainer(scores[:3]).run([first])                     # interrupted with one epoch waited
    assert first.wait_count == 1
    torch.save(first.state_dict(), tmp_path / "s.pt")
    second = EarlyStopping("val_loss", patience=3)
    second.load_state_dict(torch.load(tmp_path / "s.pt", weights_only=True))
    assert second.wait_count == 1 and second.best_score == 0.9
    tr = _StubTrainer(scores)
    second.on_resume(tr)
    assert not tr.should_stop
    assert tr.run([second], first=3) == 5 and second.state_dict() == whole.state_dict()
    # resumed from the state of the stopping epoch: stops before it trains
    third = EarlyStopping("val_loss", patience=3)
    third.load_state_dict(whole.state_dict())
    tr = _StubTrainer(scores)
    third.on_resume(tr)
    assert tr.should_stop and tr.run([third], first=5) == 5


def test_atomic_write_keeps_the_previous_file(tmp_path, monkeypatch):
    from multimodal_supernovae_amd.checkpoint import save_checkpoint
    path = tmp_path / "a.ckpt"
    save_checkpoint(path, _Net(seed=1))
    before = path.read_bytes()

    def dying_save(obj, f, *args, **kwargs):
        f.write(b"half a checkpoint")
        f.flush()
        raise OSError("No space left on device")

    monkeypatch.setattr(torch, "save", dying_save)
    with pytest.raises(OSError, match="No space"):
        save_checkpoint(path, _Net(seed=2))
    with pytest.raises(OSError, match="No space"):
        save_checkpoint(tmp_path / "b.ckpt", _Net(seed=2))    # no earlier file: none appears
    monkeypatch.undo()
    assert path.read_bytes() == before
    assert os.listdir(tmp_path) == ["a.ckpt"]
    save_checkpoint(path, _Net(seed=2))                       # and a good write replaces it
    assert path.read_bytes() != before and os.listdir(tmp_path) == ["a.ckpt"]


# ------------------------------------------------------------------------------ the Trainer's side, on the CPU
class _Toy(nn.Module):
    """A module with the hooks the Trainer drives, on torch's own CPU ops: dropout (torch's CPU generator), a draw from
    Python's `random` and one from numpy per step, torch.optim.RAdam + StepLR."""

    def __init__(self, seed):
        super().__init__()
        torch.manual_seed(seed)
        self.net = nn.Sequential(nn.Linear(6, 8), nn.Dropout(0.25), nn.Linear(8, 1))
        self.bn = nn.BatchNorm1d(6)
        self.logged = {}

    def _loss(self, batch):
        x, y = batch
        return ((self.net(self.bn(x)).squeeze(1) - y) ** 2).mean()

    def training_step(self, batch, batch_idx):
        import random

        import numpy as np
        return self._loss(batch) * (1.0 + 0.01 * random.random() + 0.01 * float(np.random.rand()))

    def validation_step(self, batch, batch_idx):
        loss = self._loss(batch)
        self.logged["score"] = float(loss) * 2
        return loss

    def configure_optimizers(self):
        opt = torch.optim.RAdam(self.parameters(), lr=1e-2, weight_decay=1e-3)
        return {"optimizer": opt, "lr_scheduler": {"scheduler": torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)}}


def _toy_data():
    g = torch.Generator().manual_seed(3)
    ds = torch.utils.data.TensorDataset(torch.randn(32, 6, generator=g), torch.randn(32, generator=g))
    val = [(torch.randn(8, 6, generator=g), torch.randn(8, generator=g)), (torch.randn(5, 6, generator=g), torch.randn(5, generator=g))]
    return torch.utils.data.DataLoader(ds, batch_size=8, shuffle=True), val


def _toy_seed(seed):
    import random

    import numpy as np
    torch.manual_seed(seed)
    random.seed(seed + 1)
    np.random.seed(seed + 2)


def _toy_snap(model, tr):
    return ({k: v.clone() for k, v in model.state_dict().items()},
            [(float(st["step"]), st["exp_avg"].clone(), st["exp_avg_sq"].clone()) for st in tr.optimizer.state.values()],
            copy.deepcopy(tr.history), tr.optimizer.param_groups[0]["lr"], tr.global_step, tr.scheduler.last_epoch)


def _toy_equal(a, b):
    assert all(torch.equal(a[0][k], b[0][k]) for k in a[0]) and list(a[0]) == list(b[0])
    assert len(a[1]) == len(b[1]) > 0
    assert all(s == t and torch.equal(m, n) and torch.equal(v, w) for (s, m, v), (t, n, w) in zip(a[1], b[1]))
    assert a[2:] == b[2:], (a[2:], b[2:])


def test_trainer_resume_is_bitwise_on_the_cpu(tmp_path):
    """Trainer(callbacks=...), fit(ckpt_path=...) and the order of restoration with a toy module and torch's optimizer -- the
    GPU tests do the same with the package's models: one epoch + a resumed fit == three uninterrupted epochs, the shuffle
    order, dropout masks, `random` / numpy draws, BatchNorm buffers, scheduler and history included."""
    from multimodal_supernovae_amd.checkpoint import EarlyStopping, ModelCheckpoint
    from multimodal_supernovae_amd.trainer import Trainer
    cpu = torch.device("cpu")

    def whole():
        model = _Toy(0)
        _toy_seed(100)
        train, val = _toy_data()
        tr = Trainer(max_epochs=3, device=cpu).fit(model, train, val)
        return _toy_snap(model, tr)

    a = whole()
    _toy_equal(a, whole())                                    # precondition: the uninterrupted run twice
    assert a[4] == 12 and a[5] == 3 and len(a[2]["val_loss"]) == 3
    model = _Toy(0)
    _toy_seed(100)
    train, val = _toy_data()
    cb = ModelCheckpoint(tmp_path, monitor="score", filename="{epoch}-{score:.2f}", save_last=True)
    tr = Trainer(max_epochs=1, device=cpu, callbacks=[cb]).fit(model, train, val)
    assert tr.current_epoch == 0 and not tr.should_stop
    assert sorted(os.listdir(tmp_path)) == [os.path.basename(cb.best_model_path), "last.ckpt"]
    assert cb.best_model_score == model.logged["score"] and f"score={cb.best_model_score:.2f}" in cb.best_model_path
    raw = torch.load(tmp_path / "last.ckpt", weights_only=True)
    assert set(raw) == LAYOUT and raw["epoch"] == 0 and raw["global_step"] == 4 and raw["msn"]["history"] == tr.history
    assert list(raw["callbacks"]) == [cb.state_key] and raw["callbacks"][cb.state_key]["best_model_path"] == cb.best_model_path
    assert all(type(st["step"]) is int and st["step"] == 4 for st in raw["optimizer_states"][0]["state"].values())
    assert raw["lr_schedulers"][0]["last_epoch"] == 1
    other = _Toy(7)
    _toy_seed(999)
    cb2 = ModelCheckpoint(tmp_path, monitor="score", filename="{epoch}-{score:.2f}", save_last=True)
    tr2 = Trainer(max_epochs=3, device=cpu, callbacks=[cb2])
    tr2.fit(other, train, val, ckpt_path=tmp_path / "last.ckpt")
    _toy_equal(a, _toy_snap(other, tr2))
    assert tr2.current_epoch == 2 and len(cb2.best_k_models) == 1
    # Trainer.save_checkpoint after a fit, and a resume at the end of training: nothing more is trained
    tr2.save_checkpoint(tmp_path / "end" / "manual.ckpt")
    third = _Toy(5)
    tr3 = Trainer(max_epochs=3, device=cpu).fit(third, train, val, ckpt_path=tmp_path / "end" / "manual.ckpt")
    assert tr3.global_step == 12 and tr3.history == tr2.history
    assert all(torch.equal(v, other.state_dict()[k]) for k, v in third.state_dict().items())
    # a monitor nobody logged is an error, not a silent skip
    with pytest.raises(RuntimeError, match="AUC_val"):
        Trainer(max_epochs=1, device=cpu, callbacks=[EarlyStopping("AUC_val")]).fit(_Toy(0), train, val)
    # validate(): the best file's score again, history untouched
    before = copy.deepcopy(tr2.history)
    got = tr2.validate(_Toy(3), val, ckpt_path=tmp_path / "last.ckpt")
    assert got["val_loss"] == tr2.history["val_loss"][-1] and tr2.history == before


def test_rng_of_another_world_size_is_left_alone(tmp_path):
    from multimodal_supernovae_amd.checkpoint import load_checkpoint, restore_rng, save_checkpoint
    save_checkpoint(tmp_path / "a.ckpt", _Net())
    ck = load_checkpoint(tmp_path / "a.ckpt")
    ck["msn"]["world_size"], ck["msn"]["rng"] = 2, ck["msn"]["rng"] * 2
    torch.manual_seed(5)
    want = torch.get_rng_state()
    with pytest.warns(UserWarning, match="RNG"):
        assert not restore_rng(ck)
    assert torch.equal(torch.get_rng_state(), want)
