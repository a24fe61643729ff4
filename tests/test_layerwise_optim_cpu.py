"""optim.LAMB / LARS, optim.layerwise_param_groups, build_optimizer with a class and the models' `optimizer=` keyword with one,
without a GPU and without the library: constructors, names, param groups, and which parameters an optimizer is built over."""
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


def _ids(opt):
    return [id(p) for g in opt.param_groups for p in g["params"]]


def test_constructor_defaults_and_param_group_keys():
    from multimodal_supernovae_amd import optim
    lamb = optim.LAMB(_params())
    assert isinstance(lamb, torch.optim.Optimizer) and issubclass(optim.LAMB, optim._FusedStep)
    assert lamb.defaults == dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.0, bias_correction=True, always_adapt=False,
                                 trust_clip=False)
    assert set(lamb.param_groups[0]) >= set(lamb.defaults) | {"params"} and len(lamb.state) == 0
    sig = inspect.signature(optim.LAMB.__init__).parameters
    assert [k for k in sig][:9] == ["self", "params", "lr", "betas", "eps", "weight_decay", "bias_correction", "always_adapt", "trust_clip"]

    lars = optim.LARS(_params(), lr=0.1)
    assert isinstance(lars, torch.optim.Optimizer) and issubclass(optim.LARS, optim._FusedStep)
    assert lars.defaults == dict(lr=0.1, momentum=0.9, dampening=0.0, weight_decay=0.0, nesterov=False, trust_coefficient=1e-3, eps=1e-8)
    assert set(lars.param_groups[0]) >= set(lars.defaults) | {"params"} and len(lars.state) == 0
    with pytest.raises(TypeError):
        optim.LARS(_params())                                    # lr has no default, as in lightning-bolts
    groups = optim.LAMB([dict(params=_params()[:1], weight_decay=0.0), dict(params=_params()[1:], betas=(0.8, 0.9))], lr=3e-4,
                        weight_decay=0.01, trust_clip=True)
    assert [g["weight_decay"] for g in groups.param_groups] == [0.0, 0.01] and groups.param_groups[1]["betas"] == (0.8, 0.9)
    assert all(g["trust_clip"] is True and g["lr"] == 3e-4 for g in groups.param_groups)


@pytest.mark.parametrize("bad,word", [(dict(lr=-1e-3), "learning rate"), (dict(eps=-1.0), "epsilon"), (dict(betas=(1.0, 0.9)), "index 0"),
                                      (dict(betas=(0.9, 1.5)), "index 1"), (dict(betas=(-0.1, 0.9)), "index 0"),
                                      (dict(weight_decay=-1.0), "weight_decay"), (dict(maximize=True), "maximize"),
                                      (dict(differentiable=True), "differentiable")])
def test_lamb_constructor_validation(bad, word):
    from multimodal_supernovae_amd import optim
    with pytest.raises(ValueError, match=word):
        optim.LAMB(_params(), **bad)


@pytest.mark.parametrize("bad,word", [(dict(lr=-1e-3), "learning rate"), (dict(momentum=-0.1), "momentum"), (dict(weight_decay=-1.0), "weight_decay"),
                                      (dict(eps=-1e-8), "epsilon"), (dict(nesterov=True, momentum=0.0), "Nesterov"),
                                      (dict(nesterov=True, momentum=0.9, dampening=0.5), "Nesterov"),
                                      (dict(trust_coefficient=0.0), "trust_coefficient"), (dict(trust_coefficient=-1e-3), "trust_coefficient"),
                                      (dict(maximize=True), "maximize"), (dict(differentiable=True), "differentiable")])
def test_lars_constructor_validation(bad, word):
    from multimodal_supernovae_amd import optim
    with pytest.raises(ValueError, match=word):
        optim.LARS(_params(), **dict(dict(lr=0.1), **bad))


def test_torch_only_keywords_are_accepted_and_ignored():
    from multimodal_supernovae_amd import optim
    for make in (lambda **kw: optim.LAMB(_params(), **kw), lambda **kw: optim.LARS(_params(), lr=0.1, **kw)):
        opt = make(foreach=True, capturable=True, fused=True, maximize=False, differentiable=False)
        assert not {"foreach", "capturable", "fused", "maximize", "differentiable"} & set(opt.defaults)
        with pytest.raises(TypeError):
            make(no_such_keyword=1)


def test_build_optimizer_takes_lars_by_name_and_any_optimizer_class():
    from multimodal_supernovae_amd import optim
    assert optim.OPTIMIZERS["lars"] is optim.LARS and "lamb" not in optim.OPTIMIZERS
    for spelled in ("lars", "LARS", "Lars"):
        opt = optim.build_optimizer(spelled, _params(), lr=0.2, weight_decay=1e-4, nesterov=True)
        assert type(opt) is optim.LARS and opt.param_groups[0]["lr"] == 0.2 and opt.param_groups[0]["nesterov"]
    opt = optim.build_optimizer(optim.LAMB, _params(), lr=2e-3, weight_decay=0.01, trust_clip=True)
    assert type(opt) is optim.LAMB and opt.param_groups[0]["lr"] == 2e-3 and opt.param_groups[0]["trust_clip"]
    assert type(optim.build_optimizer(optim.LARS, _params(), 0.1)) is optim.LARS
    assert type(optim.build_optimizer(optim.AdamW, _params(), 1e-3)) is optim.AdamW
    for bad in (int, object, 3, None, "lambda"):
        with pytest.raises(ValueError, match="unknown optimizer") as err:
            optim.build_optimizer(bad, _params(), lr=1e-3)
        assert "lars" in str(err.value) and "radam" in str(err.value)


def test_models_build_lamb_from_the_class_over_the_same_parameters():
    """optimizer=optim.LAMB on each of the three models: optim.LAMB over exactly what RAdam gets, with lr and optimizer_kwargs
    handed on."""
    from multimodal_supernovae_amd import optim
    from multimodal_supernovae_amd.models_finetune import ClipMLP
    from multimodal_supernovae_amd.models_pretraining import MaskedLightCurveEncoder
    kw = {"weight_decay": 0.05}

    def pair(make):
        torch.manual_seed(0)
        model = make(optimizer=optim.LAMB)
        assert model.optimizer is optim.LAMB
        lamb = model.configure_optimizers()["optimizer"]
        model.optimizer = "radam"
        radam = model.configure_optimizers()["optimizer"]
        assert type(lamb) is optim.LAMB and type(radam) is optim.RAdam and _ids(lamb) == _ids(radam) and len(_ids(lamb)) > 0
        assert lamb.param_groups[0]["weight_decay"] == 0.05 and lamb.param_groups[0]["lr"] == radam.param_groups[0]["lr"]
        return model, lamb

    clip, opt = pair(lambda **o: _clip(lr=2e-4, optimizer_kwargs=kw, **o))
    assert _ids(opt) == [id(p) for p in clip.parameters()] and opt.param_groups[0]["lr"] == 2e-4
    head, opt = pair(lambda **o: ClipMLP(_clip(), classification=True, hidden_dim=8, freeze_backbone=True, learning_rate=3e-4,
                                         optimizer_kwargs=kw, **o))
    assert _ids(opt) == [id(p) for p in head.mlp.parameters()] and opt.param_groups[0]["lr"] == 3e-4
    tk = dict(n_out=1, emb=16, heads=2, depth=1, dropout=0.0)
    enc, opt = pair(lambda **o: MaskedLightCurveEncoder(transformer_kwargs=tk, optimizer_kwargs=kw, lr=5e-4,
                                                        lr_scheduler_kwargs={"step_size": 1, "gamma": 0.5}, **o))
    assert _ids(opt) == [id(p) for p in enc.parameters()]
    lars = _clip(lr=0.1, optimizer="lars", optimizer_kwargs=dict(weight_decay=1e-4)).configure_optimizers()["optimizer"]
    assert type(lars) is optim.LARS and lars.param_groups[0]["lr"] == 0.1
    assert list(_clip().state_dict()) == list(_clip(optimizer=optim.LAMB).state_dict())
    with pytest.raises(ValueError, match="radam"):
        _clip(optimizer=dict).configure_optimizers()


def test_layerwise_param_groups_split_by_ndim_and_skip_frozen_parameters():
    from multimodal_supernovae_amd import optim
    net = torch.nn.Sequential(torch.nn.Linear(4, 3), torch.nn.LayerNorm(3), torch.nn.Linear(3, 2), torch.nn.Conv1d(2, 2, 3))
    net.register_parameter("scale", torch.nn.Parameter(torch.zeros(())))
    net[2].weight.requires_grad_(False)
    net[1].bias.requires_grad_(False)
    groups = optim.layerwise_param_groups(net, 0.05)
    assert [set(g) for g in groups] == [{"params", "weight_decay"}] * 2
    assert [g["weight_decay"] for g in groups] == [0.0, 0.05]
    named = dict(net.named_parameters())
    assert [id(p) for p in groups[0]["params"]] == [id(named[k]) for k in ("scale", "0.bias", "1.weight", "2.bias", "3.bias")]
    assert [id(p) for p in groups[1]["params"]] == [id(named[k]) for k in ("0.weight", "3.weight")]
    again = optim.layerwise_param_groups(net.named_parameters(), 0.05)
    assert [[id(p) for p in g["params"]] for g in again] == [[id(p) for p in g["params"]] for g in groups]
    opt = optim.LAMB(groups, lr=1e-3)
    assert [g["weight_decay"] for g in opt.param_groups] == [0.0, 0.05]
    opt = optim.LARS(optim.layerwise_param_groups(net, 1e-4), lr=0.1)
    assert [len(g["params"]) for g in opt.param_groups] == [5, 2]


def test_step_on_cpu_parameters_is_an_error_not_a_fallback():
    from multimodal_supernovae_amd import _lib, optim
    for make in (lambda ps: optim.LAMB(ps, weight_decay=0.01), lambda ps: optim.LARS(ps, lr=0.1, weight_decay=1e-4)):
        ps = _params()
        for p in ps:
            p.grad = torch.ones_like(p)
        opt = make(ps)
        with pytest.raises(_lib.MsnHipError):
            opt.step()
        assert all(bool((p == 0).all()) for p in ps) and len(opt.state) == 0
        assert opt.trust_ratios() == []
