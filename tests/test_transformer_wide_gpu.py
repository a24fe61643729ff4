"""Towers whose attention heads are wider than 128 columns (emb 512 / 2 heads, 256 / 1, 1024 / 2; the pooling head's two heads
are emb / 2 wide) at module level against the CPU oracle in fp64 on the module's own state_dict: TransformerWithTimeEmbeddings
with every aggregation, a contrastive training step of LightCurveImageCLIP, and that step replayed as a HIP graph."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu
RTOL = 1e-3


def close(a, b, what):
    b = b.to(a.dtype)
    scale = float(b.abs().max()) + 1e-6
    torch.testing.assert_close(a, b, rtol=RTOL, atol=RTOL * scale * 0.1, msg=lambda m: f"{what}: {m}")


def _lc_inputs(B, T, nband, g, fully_padded):
    x = torch.randn(B, T, 1, generator=g)
    t = torch.sort(torch.rand(B, T // nband, generator=g) * 100, dim=1)[0].repeat(1, nband)
    mask = torch.zeros(B, T, dtype=torch.bool)
    for b in range(B):
        for k in range(nband):
            n = int(torch.randint(3, T // nband + 1, (1,), generator=g))
            mask[b, k * (T // nband):k * (T // nband) + n] = True
    if fully_padded:
        mask[-1] = False
    return x, t, mask


@pytest.mark.parametrize("emb,heads", [(512, 2), (256, 1), (1024, 2)])
@pytest.mark.parametrize("agg", ["mean", "max", "attn", "pretraining"])
@pytest.mark.parametrize("nband", [1, 2])
def test_wide_tower_against_oracle(emb, heads, agg, nband):
    from multimodal_supernovae_amd.transformer_utils import TransformerWithTimeEmbeddings
    from oracle import encoders as oenc
    g = torch.Generator().manual_seed(emb + heads + 7 * nband)
    torch.manual_seed(emb + heads)
    m = TransformerWithTimeEmbeddings(n_out=16, nband=nband, agg=agg, time_norm=1000.0, emb=emb, heads=heads, depth=2)
    P = {k: v.double().clone().requires_grad_() for k, v in m.state_dict().items()}
    B, T = 4, 36
    x, t, mask = _lc_inputs(B, T, nband, g, fully_padded=agg != "mean")     # (mean over no token: 0 / 0 in the reference too)
    ref = oenc.transformer_with_time_embeddings(P, "", x.double(), t.double(), mask, emb=emb, heads=heads, depth=2,
                                                time_norm=1000.0, nband=nband, agg=agg)
    cot = torch.randn(ref.shape, generator=g)
    (ref * cot.double()).sum().backward()
    m.cuda()
    y = m(x.cuda(), t.cuda(), mask.cuda())
    close(y.detach().cpu(), ref.detach(), "y")
    y.backward(cot.cuda())
    for k, p in m.named_parameters():
        if P[k].grad is None:                             # the projection under agg="pretraining"
            assert p.grad is None, k
            continue
        assert p.grad is not None, k
        close(p.grad.cpu(), P[k].grad, "grad " + k)


LC = dict(n_out=16, emb=512, heads=2, depth=2, dropout=0.0, time_norm=20583.37, agg="attn")
SP = dict(n_out=16, emb=256, heads=1, depth=2, dropout=0.0, time_norm=17945.14, agg="mean")
COMBOS = ["lightcurve", "spectral"]


def _model():
    from multimodal_supernovae_amd.models_multimodal import LightCurveImageCLIP
    torch.manual_seed(0)
    return LightCurveImageCLIP(enc_dim=32, nband=2, transformer_kwargs=LC, transformer_spectral_kwargs=SP, combinations=COMBOS,
                               loss="softmax", lr=1e-3)


def _batch(g, B=8, T=40, Ts=220):
    _, t, mask = _lc_inputs(B, T, 2, g, fully_padded=False)
    msp = torch.zeros(B, Ts, dtype=torch.bool)
    for b in range(B):
        msp[b, :int(torch.randint(20, Ts + 1, (1,), generator=g))] = True
    return (None, torch.randn(B, T, generator=g), t, mask, torch.randn(B, Ts, generator=g),
            torch.sort(torch.rand(B, Ts, generator=g) * 6000 + 3000, dim=1)[0], msp, None, None)


def test_clip_step_with_wide_towers_against_oracle():
    """512 / 2 light-curve tower with attention pooling (two 256-wide pooling heads) + 256 / 1 spectrum tower over 220 tokens:
    the loss and every parameter gradient of one training step against oracle.clip.training_loss in fp64"""
    from oracle import clip as oclip
    model = _model()
    cfg = {"combinations": COMBOS, "nband": 2, "transformer_kwargs": LC, "transformer_spectral_kwargs": SP}
    P = {k: v.double().clone().requires_grad_(v.is_floating_point()) for k, v in model.state_dict().items()}
    batch = _batch(torch.Generator().manual_seed(3))
    ref = oclip.training_loss(P, cfg, tuple(t.double() if t is not None and t.is_floating_point() else t for t in batch))
    ref.backward()
    model.cuda().train()
    loss = model.training_step(tuple(t.cuda() if t is not None else None for t in batch), 0)
    loss.backward()
    assert abs(float(loss.detach()) - float(ref.detach())) <= 1e-4 * abs(float(ref.detach())), (float(loss.detach()), float(ref.detach()))
    for k, p in model.named_parameters():
        if P[k].grad is None or k == "logit_bias":        # (the softmax loss does not depend on the bias: both gradients are rounding)
            continue
        assert p.grad is not None, k
        # relative Frobenius error per parameter: over B T = 1760 spectrum tokens x 1024 hidden units a few ReLU pre-activations lie
        # within fp32 rounding of zero and flip against fp64, each moving one row of a feed-forward weight's gradient by one token's
        # share -- about 1e-3 of the norm of a 1024 x 256 gradient per flip (seen: 1.4e-3 on ff.0.weight, one row off by 0.6 % of
        # its largest element); the attention itself is checked element-wise in tests/test_attention_wide_gpu.py and the towers in
        # test_wide_tower_against_oracle
        a, b = p.grad.cpu().double(), P[k].grad
        err = float((a - b).norm() / (b.norm() + 1e-30))
        assert err < 5e-3, (k, err)


def test_graphed_step_with_wide_towers_equals_eager_steps():
    from multimodal_supernovae_amd.trainer import GraphedTrainStep
    steps = 9                                           # several replays after the warm-up
    g = torch.Generator().manual_seed(5)
    batches = [tuple(t.cuda() if t is not None else None for t in _batch(g)) for _ in range(steps)]
    eager = _model().cuda().train()
    graphed = copy.deepcopy(eager)
    opt_e = eager.configure_optimizers()["optimizer"]
    losses_e = []
    for b in batches:
        opt_e.zero_grad(set_to_none=True)
        loss = eager.training_step(b, 0)
        loss.backward()
        opt_e.step()
        losses_e.append(float(loss.detach()))
    opt_g = graphed.configure_optimizers()["optimizer"]
    step = GraphedTrainStep(graphed, opt_g, warmup=3)
    losses_g = [float(step(b).detach()) for b in batches]
    assert step.graph is not None and step.calls == steps
    torch.cuda.synchronize()
    for a, b in zip(losses_e, losses_g):
        assert abs(a - b) <= 1e-5 * abs(a), (losses_e, losses_g)
    for (k, p), (_, q) in zip(eager.named_parameters(), graphed.named_parameters()):
        torch.testing.assert_close(q, p, rtol=1e-5, atol=1e-7, msg=lambda m: f"{k}: {m}")
