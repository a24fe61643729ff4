"""The benchmarked configuration itself (bench.py: ViT-S/8 image tower + the reference light-curve transformer,
symmetric InfoNCE, RAdam): one training step of the HIP path against the oracle on the same synthetic batch, and
size-independent properties at the full per-GPU batch of 1024."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _oracle_step(P, batch):
    import bench
    from oracle import clip as oclip
    from oracle import encoders as oenc
    from oracle import loss as oloss
    from oracle.build_defined import vision_transformer
    h = vision_transformer(P, "image_encoder.", batch[0], patch=8, heads=6, depth=12)
    e_img = oclip.l2_normalise(oenc.linear(P, "image_projection", h))
    h = oenc.transformer_with_time_embeddings(P, "lightcurve_encoder.", batch[1][..., None], batch[2], batch[3],
                                              emb=bench.LC["emb"], heads=bench.LC["heads"], depth=bench.LC["depth"],
                                              time_norm=bench.LC["time_norm"], nband=bench.NBAND, agg="mean")
    e_lc = oclip.l2_normalise(oenc.linear(P, "lightcurve_projection", h))
    return oloss.clip_loss_multimodal([e_img, e_lc], P["logit_scale"], P["logit_bias"]), e_img, e_lc


@pytest.fixture(params=["f32", "bf16x6"])
def gemm_precision(request):
    """Both arithmetic routes of the wide products: the native fp32 MFMA kernels and the fp32-grade plane kernels."""
    from multimodal_supernovae_amd import ops
    old = ops.GEMM_PRECISION
    ops.set_gemm_precision(request.param)
    yield request.param
    ops.GEMM_PRECISION = old


def test_headline_step_matches_oracle(gemm_precision):
    """fp32 tolerance of the north star: loss and embeddings within 1e-3 relative (observed ~1e-6); gradients of every
    parameter within 2e-3 of their own scale."""
    import bench
    model = bench.build_model("cpu", seed=3)
    P = {k: v.detach().clone().requires_grad_(v.is_floating_point()) for k, v in model.state_dict().items()}
    batch = bench.synthetic_batch(24, 99, "cpu")
    ref, e_img_ref, e_lc_ref = _oracle_step(P, batch)
    ref.backward()
    model.cuda()
    gb = tuple(t.cuda() if torch.is_tensor(t) else t for t in batch)
    embs = model(*gb)
    torch.testing.assert_close(embs[0].detach().cpu(), e_img_ref.detach(), rtol=1e-3, atol=1e-5)
    torch.testing.assert_close(embs[1].detach().cpu(), e_lc_ref.detach(), rtol=1e-3, atol=1e-5)
    loss = model.training_step(gb, 0)
    assert abs(float(loss.detach()) - float(ref.detach())) <= 1e-3 * abs(float(ref.detach()))
    loss.backward()
    worst = 0.0
    for k, p in model.named_parameters():
        if k == "logit_bias":      # analytically zero gradient
            continue
        g_ref = P[k].grad
        scale = float(g_ref.abs().max()) + 1e-12
        worst = max(worst, float((p.grad.cpu() - g_ref).abs().max()) / scale)
    assert worst < 2e-3, worst


def test_full_batch_properties(gemm_precision):
    """Per-GPU batch 1024 (the bench size): the symmetric InfoNCE is invariant under a common permutation of the pairs,
    embeddings are unit vectors, and a sample's embedding does not depend on the rest of the batch (LayerNorm
    towers): its value inside the 1024-batch equals its value in a 16-sample batch."""
    import bench
    model = bench.build_model("cuda", seed=5)
    batch = bench.synthetic_batch(1024, 7, "cuda")
    with torch.no_grad():
        e = model(*batch)
        loss = model._loss(e)
        perm = torch.randperm(1024, device="cuda")
        pb = tuple(t[perm] if torch.is_tensor(t) and t.dim() > 0 and t.shape[0] == 1024 else t for t in batch)
        ep = model(*pb)
        loss_p = model._loss(ep)
        small = tuple(t[:16] if torch.is_tensor(t) and t.dim() > 0 and t.shape[0] == 1024 else t for t in batch)
        es = model(*small)
    for t in e:
        torch.testing.assert_close(t.norm(dim=-1), torch.ones(1024, device="cuda"), rtol=0, atol=2e-6)
    assert abs(float(loss) - float(loss_p)) <= 2e-6 * abs(float(loss))
    for a, b in zip(e, ep):
        torch.testing.assert_close(a[perm], b, rtol=1e-5, atol=1e-6)
    for a, b in zip(e, es):
        torch.testing.assert_close(a[:16], b, rtol=1e-5, atol=2e-6)


def test_full_batch_plane_path_matches_fp32_path():
    """One training step at the bench size (1024 pairs: the persistent plane kernels walk several tiles per workgroup, cut tail
    tiles and chunk long reductions) under "bf16x6" against the same step under "f32": loss to 1e-5, every gradient to 1e-3
    of its scale (both routes are fp32 grade; they differ by summation order)."""
    import bench
    from multimodal_supernovae_amd import ops
    batch = bench.synthetic_batch(1024, 11, "cuda")
    out = {}
    for prec in ("f32", "bf16x6"):
        model = bench.build_model("cuda", seed=5)
        with ops.gemm_precision(prec):
            loss = model.training_step(batch, 0)
            loss.backward()
        out[prec] = (float(loss.detach()), {k: p.grad.detach().clone() for k, p in model.named_parameters()})
        del model
    l0, g0 = out["f32"]
    l1, g1 = out["bf16x6"]
    assert abs(l1 - l0) <= 1e-5 * abs(l0), (l0, l1)
    worst = max((float((g1[k] - g0[k]).abs().max()) / (float(g0[k].abs().max()) + 1e-12), k) for k in g0 if k != "logit_bias")
    assert worst[0] < 1e-3, worst


def test_plain_bench_run_and_its_dumped_outputs(tmp_path):
    """`bench.py --steps K --warmup W --dump-outputs DIR` without --full: one result line with the headline fields and none of
    what --full measures beside them; the last timed step's loss, parameters and gradients as float32 arrays within 64 MB, and
    the same arrays from a second run (the untimed steps that the warm-up adds by speed are undone before the timed ones)."""
    import json
    import subprocess
    import numpy as np
    dumps = []
    for i in range(2):
        d = tmp_path / f"run{i}"
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                            "--global-batch", "64", "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, r.stdout[-2000:]
        out = json.loads(lines[0])
        assert out["unit"] == "pairs/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
        assert out["steps"] == 3 and out["ms_per_step"] > 0
        assert abs(out["value"] - 64 / (out["ms_per_step"] * 1e-3)) <= 1e-6 * out["value"]
        assert not {"roofline", "cpu_baseline", "alt_arithmetic", "weak_scaling_256_per_gpu", "three_tower", "towers"} & set(out)
        files = sorted(os.listdir(d))
        assert "loss.npy" in files and "param.logit_scale.npy" in files and "grad.logit_scale.npy" in files
        arrays = {f: np.load(d / f) for f in files}
        assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
        assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrays.values())
        assert float(arrays["loss.npy"][0]) == pytest.approx(out["config"]["loss"], rel=1e-6)
        dumps.append(arrays)
    assert dumps[0].keys() == dumps[1].keys()
    for f, a in dumps[0].items():
        np.testing.assert_allclose(dumps[1][f], a, rtol=1e-4, atol=1e-5 * float(np.abs(a).max()) + 1e-12, err_msg=f)
