"""optim.Adam / AdamW / SGD, optim.build_optimizer, the models' `optimizer=` keyword and Trainer._scheduler_of without a GPU and
without the library: constructors, names, the lr_scheduler dict forms, and which parameters an optimizer is built over."""
import inspect

import pytest
import torch

TK = dict(n_out=8, emb=16, heads=2, depth=1, dropout=0.0, time_norm=1000.0, agg="mean")


def _params():
    return [torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2, 2))]


def _clip(**kw):
    from multimodal_supernovae_amd.models_multimodal import LightCurveImageCLIP
    return LightCurveImageCLIP(enc_dim=16, nband=2, transformer_kwargs=TK, transformer_spectral_kwargs=TK,
                               combinations=["lightcurve", "spectral"], loss="softmax", **kw)


def test_constructors_follow_torch():
    """Keywords and defaults of torch.optim.Adam / AdamW / SGD; torch.optim.Optimizer subclasses with torch's param_groups."""
    from multimodal_supernovae_amd import optim
    for ours, theirs in ((optim.Adam, torch.optim.Adam), (optim.AdamW, torch.optim.AdamW), (optim.SGD, torch.optim.SGD)):
        assert issubclass(ours, torch.optim.Optimizer)
        mine, ref = inspect.signature(ours.__init__).parameters, inspect.signature(theirs.__init__).parameters
        for name, p in mine.items():
            if p.kind in (p.POSITIONAL_OR_KEYWORD,) and name not in ("self", "params"):
                assert name in ref and ref[name].default == p.default, (ours.__name__, name, p.default)
        a, b = ours(_params()), theirs(_params())
        for key, value in a.defaults.items():
            assert b.defaults[key] == value, (ours.__name__, key)
        assert len(a.state) == 0
    assert optim.AdamW(_params()).defaults["weight_decay"] == 1e-2 and optim.Adam(_params()).defaults["weight_decay"] == 0.0
    sgd = optim.SGD(_params(), lr=0.1, momentum=0.9, nesterov=True, weight_decay=1e-4)
    assert sgd.param_groups[0]["nesterov"] is True and sgd.param_groups[0]["momentum"] == 0.9
    groups = optim.AdamW([dict(params=_params()[:1], lr=1e-2), dict(params=_params()[1:], betas=(0.8, 0.9))], lr=3e-4)
    assert [g["lr"] for g in groups.param_groups] == [1e-2, 3e-4] and groups.param_groups[1]["betas"] == (0.8, 0.9)


@pytest.mark.parametrize("name", ["Adam", "AdamW"])
@pytest.mark.parametrize("bad,word", [(dict(lr=-1e-3), "learning rate"), (dict(eps=-1.0), "epsilon"), (dict(betas=(1.0, 0.9)), "index 0"),
                                      (dict(betas=(0.9, 1.5)), "index 1"), (dict(weight_decay=-1.0), "weight_decay"),
                                      (dict(amsgrad=True), "amsgrad"), (dict(maximize=True), "maximize"),
                                      (dict(differentiable=True), "differentiable")])
def test_adam_constructor_validation(name, bad, word):
    from multimodal_supernovae_amd import optim
    with pytest.raises(ValueError, match=word):
        getattr(optim, name)(_params(), **bad)


@pytest.mark.parametrize("bad,word", [(dict(lr=-1e-3), "learning rate"), (dict(momentum=-0.1), "momentum"), (dict(weight_decay=-1.0), "weight_decay"),
                                      (dict(nesterov=True), "Nesterov"), (dict(nesterov=True, momentum=0.9, dampening=0.5), "Nesterov"),
                                      (dict(maximize=True), "maximize"), (dict(differentiable=True), "differentiable")])
def test_sgd_constructor_validation(bad, word):
    from multimodal_supernovae_amd import optim
    with pytest.raises(ValueError, match=word):
        optim.SGD(_params(), **bad)


def test_torch_only_keywords_are_accepted_and_ignored():
    from multimodal_supernovae_amd import optim
    for cls in (optim.Adam, optim.AdamW, optim.SGD):
        opt = cls(_params(), foreach=True, capturable=True, fused=True, maximize=False, differentiable=False)
        assert not {"foreach", "capturable", "fused"} & set(opt.defaults)
    optim.Adam(_params(), amsgrad=False)
    with pytest.raises(TypeError):
        optim.AdamW(_params(), no_such_keyword=1)


def test_build_optimizer_names():
    from multimodal_supernovae_amd import optim
    classes = {"radam": optim.RAdam, "adam": optim.Adam, "adamw": optim.AdamW, "sgd": optim.SGD}
    for name, cls in classes.items():
        for spelled in (name, name.upper(), name.capitalize()):
            opt = optim.build_optimizer(spelled, _params(), lr=2e-3)
            assert type(opt) is cls and opt.param_groups[0]["lr"] == 2e-3
    assert type(optim.build_optimizer("AdamW", _params(), 1e-3)) is optim.AdamW
    opt = optim.build_optimizer("sgd", _params(), lr=0.1, momentum=0.9, nesterov=True)
    assert opt.param_groups[0]["momentum"] == 0.9 and opt.param_groups[0]["nesterov"]
    with pytest.raises(ValueError) as err:
        optim.build_optimizer("lamb", _params(), lr=1e-3)
    for name in classes:
        assert name in str(err.value)
    assert "lamb" in str(err.value)


def test_step_on_cpu_parameters_is_an_error_not_a_fallback():
    from multimodal_supernovae_amd import _lib, optim
    for cls in (optim.Adam, optim.AdamW, optim.SGD):
        ps = _params()
        for p in ps:
            p.grad = torch.ones_like(p)
        with pytest.raises(_lib.MsnHipError):
            cls(ps).step()
        assert all(bool((p == 0).all()) for p in ps)


def test_scheduler_of_reads_interval_and_frequency():
    from multimodal_supernovae_amd.trainer import Trainer
    opt = torch.optim.SGD(_params(), lr=0.1)
    sch = torch.optim.lr_scheduler.StepLR(opt, step_size=1)
    of = Trainer._scheduler_of
    assert of({"optimizer": opt}) == (None, "epoch", 1)
    assert of({"optimizer": opt, "lr_scheduler": sch}) == (sch, "epoch", 1)
    assert of({"optimizer": opt, "lr_scheduler": {"scheduler": sch}}) == (sch, "epoch", 1)
    assert of({"optimizer": opt, "lr_scheduler": {"scheduler": sch, "interval": "step"}}) == (sch, "step", 1)
    assert of({"optimizer": opt, "lr_scheduler": {"scheduler": sch, "interval": "step", "frequency": 4}}) == (sch, "step", 4)
    # the form MaskedLightCurveEncoder returns: `monitor` is carried along by Lightning and unused by a StepLR
    assert of({"optimizer": opt, "lr_scheduler": {"scheduler": sch, "monitor": "val_loss", "interval": "epoch", "frequency": 1}}) == (sch, "epoch", 1)
    for bad in ({"interval": "batch"}, {"interval": "Step"}, {"interval": None}, {"frequency": 0}, {"frequency": -1}, {"frequency": 1.5},
                {"frequency": True}, {"frequency": "2"}):
        with pytest.raises(ValueError, match="interval|frequency"):
            of({"optimizer": opt, "lr_scheduler": dict({"scheduler": sch}, **bad)})
    plateau = torch.optim.lr_scheduler.ReduceLROnPlateau(opt)
    with pytest.raises(ValueError, match="ReduceLROnPlateau"):
        of({"optimizer": opt, "lr_scheduler": {"scheduler": plateau, "monitor": "val_loss"}})


def _ids(opt):
    return [id(p) for g in opt.param_groups for p in g["params"]]


def test_models_build_the_named_optimizer_over_the_same_parameters():
    """optimizer="adamw" on each of the three models: optim.AdamW over exactly what RAdam gets, with lr and optimizer_kwargs
    handed on; the default stays RAdam."""
    from multimodal_supernovae_amd import optim
    from multimodal_supernovae_amd.models_finetune import ClipMLP
    from multimodal_supernovae_amd.models_pretraining import MaskedLightCurveEncoder
    kw = {"weight_decay": 0.05}

    def pair(make):
        torch.manual_seed(0)
        model = make()
        assert model.optimizer == "radam"
        radam = model.configure_optimizers()["optimizer"]
        assert type(radam) is optim.RAdam
        model.optimizer = "adamw"
        adamw = model.configure_optimizers()["optimizer"]
        assert type(adamw) is optim.AdamW and _ids(adamw) == _ids(radam) and len(_ids(adamw)) > 0
        assert adamw.param_groups[0]["weight_decay"] == 0.05 and adamw.param_groups[0]["lr"] == radam.param_groups[0]["lr"]
        return model, adamw

    clip, opt = pair(lambda: _clip(lr=2e-4, optimizer_kwargs=kw))
    assert _ids(opt) == [id(p) for p in clip.parameters()] and opt.param_groups[0]["lr"] == 2e-4
    assert type(_clip(optimizer="AdamW", optimizer_kwargs=kw).configure_optimizers()["optimizer"]) is optim.AdamW

    head, opt = pair(lambda: ClipMLP(_clip(), classification=True, hidden_dim=8, learning_rate=3e-4, optimizer_kwargs=kw))
    skipped = {id(head.clip_model.logit_scale), id(head.clip_model.logit_bias)}
    assert _ids(opt) == [id(p) for p in head.mlp.parameters()] + [id(p) for p in head.clip_model.parameters() if id(p) not in skipped]
    frozen, opt = pair(lambda: ClipMLP(_clip(), classification=True, hidden_dim=8, freeze_backbone=True, learning_rate=3e-4,
                                       optimizer_kwargs=kw))
    assert _ids(opt) == [id(p) for p in frozen.mlp.parameters()]                    # the head only
    sgd = ClipMLP(_clip(), regression=True, hidden_dim=8, freeze_backbone=True, optimizer="sgd",
                  optimizer_kwargs=dict(momentum=0.9, nesterov=True)).configure_optimizers()["optimizer"]
    assert type(sgd) is optim.SGD and sgd.param_groups[0]["nesterov"] and sgd.param_groups[0]["lr"] == 1e-3

    tk = dict(n_out=1, emb=16, heads=2, depth=1, dropout=0.0)
    enc, opt = pair(lambda: MaskedLightCurveEncoder(transformer_kwargs=tk, optimizer_kwargs=kw, lr=5e-4,
                                                    lr_scheduler_kwargs={"step_size": 1, "gamma": 0.5}))
    assert _ids(opt) == [id(p) for p in enc.parameters()]
    cfg = enc.configure_optimizers()
    assert cfg["lr_scheduler"]["scheduler"].optimizer is cfg["optimizer"] and type(cfg["optimizer"]) is optim.AdamW

    with pytest.raises(ValueError, match="radam"):
        _clip(optimizer="lamb").configure_optimizers()


def test_model_state_dict_names_do_not_change_with_the_optimizer():
    assert list(_clip().state_dict()) == list(_clip(optimizer="adamw").state_dict())
