"""Contrastive losses with the reference's signatures (src/loss.py) on the fused HIP kernels.

    clip_loss(embs1, embs2, logit_scale, logit_bias)               -- ref src/loss.py:14-38
    clip_loss_multimodal(embeddings, logit_scales, logit_biases)   -- ref src/loss.py:41-65
    align_uniform_loss(embs1, embs2, alpha, t, lam), align_uniform_loss_multimodal(embeddings, alpha, t, lam)
                                                                   -- Wang & Isola 2020: no scale, no bias (below)
    supcon_loss(embs1, embs2, labels, logit_scale, logit_bias), supcon_loss_multimodal(embeddings, labels, ...)
                                                                   -- label-aware InfoNCE (SupCon / UniCL), csrc/supcon.hip (below)
    vicreg_loss(embs1, embs2, sim_coeff, std_coeff, cov_coeff, gamma, eps), vicreg_loss_multimodal(embeddings, ...)
                                                                   -- Bardes, Ponce, LeCun 2022: no negatives, csrc/vicreg.hip (below)
    barlow_twins_loss(embs1, embs2, lambd, eps), barlow_twins_loss_multimodal(embeddings, ...)
                                                                   -- Zbontar et al. 2021: the cross correlation of two towers driven to
                                                                      the identity, csrc/barlow.hip (below)

`logit_scale` is the LOG of the scale (the kernel exponentiates it, ref :22).  Tensors in,
0-dim tensor out, differentiable w.r.t. both embedding matrices, the scale and the bias.

Data parallel ("global negatives"): when torch.distributed is initialised with world_size > 1
and `global_negatives=True`, every rank passes its LOCAL rows; the embeddings (and afterwards the
per-row log-sum-exps, 2N floats) are all-gathered over RCCL, each rank evaluates only its own
rows / columns of the logit matrix, and the returned loss is the all-reduced global value.  The
gradient each rank gets for its local rows is already the full gradient of the global loss, so
parameter gradients must be SUMMED over ranks (see distributed.py), not averaged.
"""
from itertools import combinations as _pairs

import torch
import torch.distributed as dist

from . import _lib
from . import distributed as D
from ._lib import check, lib, ptr, stream_ptr


def _device_f32(*named):
    """Every pointer handed to the C-ABI must be float32 device memory with unit column stride: a host pointer would
    fault on the GPU (there is no CPU path to fall back to), so it is refused here."""
    for name, t in named:
        if t.device.type != "cuda":
            raise _lib.MsnHipError(f"{name} must live on the GPU (got {t.device}); the contrastive loss has no CPU path")
        if t.dtype != torch.float32:
            raise _lib.MsnHipError(f"{name} must be float32 (got {t.dtype})")
        if t.dim() == 2 and t.stride(1) != 1:
            raise _lib.MsnHipError(f"{name} must have contiguous columns (strides {t.stride()})")


class HipPairKernels:
    """The product compute backend: msn_infonce_fwd / msn_infonce_bwd through the C-ABI."""

    @staticmethod
    def forward(e1_loc, e2_loc, e1_all, e2_all, q_offset, log_scale, bias):
        _lib.require_gpu()
        _device_f32(("embs1", e1_loc), ("embs2", e2_loc), ("embs1 (gathered)", e1_all), ("embs2 (gathered)", e2_all),
                    ("logit_scale", log_scale), ("logit_bias", bias))
        if e1_loc.shape[1] != e2_loc.shape[1] or e1_all.shape[1] != e1_loc.shape[1] or e2_all.shape[1] != e1_loc.shape[1]:
            raise _lib.MsnHipError("both modalities must share the embedding width")
        b1, D = e1_loc.shape
        b2 = e2_loc.shape[0]
        n1, n2 = e1_all.shape[0], e2_all.shape[0]
        dev = e1_loc.device
        L = lib()
        nb = L.msn_infonce_workspace_bytes(b1, b2, n1, n2, D)
        ws = torch.empty(max(nb, 16) // 4 + 1, dtype=torch.float32, device=dev)
        lse_row = torch.empty(b2, dtype=torch.float32, device=dev)
        lse_col = torch.empty(b1, dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        check(L.msn_infonce_fwd(ptr(e1_loc), e1_loc.stride(0), b1, ptr(e2_loc), e2_loc.stride(0), b2,
                                ptr(e1_all), e1_all.stride(0), n1, ptr(e2_all), e2_all.stride(0), n2,
                                D, q_offset, ptr(log_scale), ptr(bias), ptr(lse_row), ptr(lse_col), ptr(loss),
                                ptr(ws), nb, stream_ptr()), "msn_infonce_fwd")
        return lse_row, lse_col, loss

    @staticmethod
    def backward(e1_loc, e2_loc, e1_all, e2_all, q_offset, log_scale, bias, lse_row_all, lse_col_all, grad_out):
        _device_f32(("embs1", e1_loc), ("embs2", e2_loc), ("embs1 (gathered)", e1_all), ("embs2 (gathered)", e2_all),
                    ("logit_scale", log_scale), ("logit_bias", bias), ("lse_row", lse_row_all), ("lse_col", lse_col_all),
                    ("grad_out", grad_out))
        if lse_row_all.numel() < e2_all.shape[0] or lse_col_all.numel() < e1_all.shape[0]:
            raise _lib.MsnHipError("backward needs the log-sum-exp of every gathered row")
        lse_row_all, lse_col_all = lse_row_all.contiguous(), lse_col_all.contiguous()
        b1, D = e1_loc.shape
        b2 = e2_loc.shape[0]
        n1, n2 = e1_all.shape[0], e2_all.shape[0]
        dev = e1_loc.device
        L = lib()
        nb = L.msn_infonce_workspace_bytes(b1, b2, n1, n2, D)
        ws = torch.empty(max(nb, 16) // 4 + 1, dtype=torch.float32, device=dev)
        d1 = torch.empty((b1, D), dtype=torch.float32, device=dev)
        d2 = torch.empty((b2, D), dtype=torch.float32, device=dev)
        dsb = torch.empty(2, dtype=torch.float32, device=dev)
        check(L.msn_infonce_bwd(ptr(e1_loc), e1_loc.stride(0), b1, ptr(e2_loc), e2_loc.stride(0), b2,
                                ptr(e1_all), e1_all.stride(0), n1, ptr(e2_all), e2_all.stride(0), n2,
                                D, q_offset, ptr(log_scale), ptr(bias), ptr(lse_row_all), ptr(lse_col_all),
                                ptr(grad_out), ptr(d1), D, ptr(d2), D, ptr(dsb), ptr(ws), nb, stream_ptr()),
              "msn_infonce_bwd")
        return d1, d2, dsb[0], dsb[1]


def _gather_rows(t, group):
    """All-gather equal-sized row blocks -> (world * b, ...) in rank order (no autograd)."""
    return D.all_gather_rows(t, group)


class _AllReduceSum(torch.autograd.Function):
    """Loss shares of the ranks summed into the global loss; the gradient of the global loss w.r.t. a rank's share is
    the incoming gradient itself (every rank differentiates the same global scalar)."""

    @staticmethod
    def forward(ctx, x, group):
        return D.all_reduce_sum(x.clone(), group, kind="loss_all_reduce")

    @staticmethod
    def backward(ctx, g):
        return g, None


def gather_embeddings(embs, group):
    """ONE all-gather for all modalities: the local (b, D) blocks are packed side by side into a (b, M*D) send buffer,
    gathered into (world * b, M*D), and handed back as M row-strided column views."""
    b = embs[0].shape[0]
    if any(e.shape[0] != b for e in embs):
        raise ValueError("global-negatives mode needs the same local batch for every modality")
    widths = [e.shape[1] for e in embs]
    pack = torch.cat([e.detach() for e in embs], dim=1) if len(embs) > 1 else embs[0].detach()
    everything = D.all_gather_rows(pack, group, kind="embedding_all_gather")
    out, off = [], 0
    for w in widths:
        out.append(everything[:, off:off + w])
        off += w
    return out


class _MultiPairLoss(torch.autograd.Function):
    """clip_loss_multimodal as ONE node: every modality pair i < j of one step, single process or row-sharded over
    `group`.  Sharded, the step costs three collectives whatever the number of pairs -- one all-gather of the packed
    (b, M*D) embeddings, one of the packed (2P, b) row / column log-sum-exps, one all-reduce of the scalar loss --
    and each rank evaluates only its own rows and columns of every pair's logit matrix."""

    @staticmethod
    def forward(ctx, scales, biases, kernels, group, sharded, *embs):
        m = len(embs)
        pairs = list(_pairs(range(m), 2))
        embs = [e.contiguous() for e in embs]
        scales = scales.detach().to(torch.float32)
        biases = biases.detach().to(torch.float32)
        if scales.dim() > 0 and scales.numel() < len(pairs) or biases.dim() > 0 and biases.numel() < len(pairs):
            raise ValueError(f"{len(pairs)} modality pairs need {len(pairs)} logit scales / biases (or one shared scalar)")
        s_k = [(scales if scales.dim() == 0 else scales[k]).reshape(()).contiguous() for k in range(len(pairs))]
        b_k = [(biases if biases.dim() == 0 else biases[k]).reshape(()).contiguous() for k in range(len(pairs))]
        if sharded:
            alls = gather_embeddings(embs, group)
            q_offset = dist.get_rank(group) * embs[0].shape[0]
        else:
            alls, q_offset = embs, 0
        lses, losses = [], []
        for k, (i, j) in enumerate(pairs):
            lse_row, lse_col, loss = kernels.forward(embs[i], embs[j], alls[i], alls[j], q_offset, s_k[k], b_k[k])
            lses += [lse_row, lse_col]
            losses.append(loss)
        total = losses[0] if len(losses) == 1 else torch.stack(losses).sum()
        if sharded:
            b = embs[0].shape[0]
            world = dist.get_world_size(group)
            pack = torch.stack(lses)                                                        # (2P, b)
            g = D.all_gather_rows(pack.view(1, 2 * len(pairs), b), group, kind="lse_all_gather")   # (world, 2P, b)
            lse_all = g.permute(1, 0, 2).reshape(2 * len(pairs), world * b)                 # row k: rank-ordered rows
            lses = [lse_all[r] for r in range(2 * len(pairs))]
            total = D.all_reduce_sum(total.clone(), group, kind="loss_all_reduce")
        ctx.kernels, ctx.q_offset, ctx.pairs, ctx.m = kernels, q_offset, pairs, m
        ctx.shapes = (scales.shape, biases.shape)
        ctx.save_for_backward(*embs, *alls, *s_k, *b_k, *lses)
        return total

    @staticmethod
    def backward(ctx, grad_out):
        m, pairs = ctx.m, ctx.pairs
        P = len(pairs)
        t = ctx.saved_tensors
        embs, alls = t[:m], t[m:2 * m]
        s_k, b_k, lses = t[2 * m:2 * m + P], t[2 * m + P:2 * m + 2 * P], t[2 * m + 2 * P:]
        g = grad_out.to(torch.float32).reshape(()).contiguous()
        d_emb = [None] * m
        d_s, d_b = [], []
        for k, (i, j) in enumerate(pairs):
            d1, d2, ds, db = ctx.kernels.backward(embs[i], embs[j], alls[i], alls[j], ctx.q_offset, s_k[k], b_k[k],
                                                  lses[2 * k], lses[2 * k + 1], g)
            d_emb[i] = d1 if d_emb[i] is None else d_emb[i].add_(d1)
            d_emb[j] = d2 if d_emb[j] is None else d_emb[j].add_(d2)
            d_s.append(ds)
            d_b.append(db)
        s_shape, b_shape = ctx.shapes
        if P == 1:
            gs, gb = d_s[0].reshape(s_shape), d_b[0].reshape(b_shape)
        else:
            gs, gb = torch.stack(d_s), torch.stack(d_b)
            gs = gs.sum() if len(s_shape) == 0 else gs
            gb = gb.sum() if len(b_shape) == 0 else gb
        return (gs, gb, None, None, None, *d_emb)


class _PairLoss(torch.autograd.Function):
    """One modality pair; single process or row-sharded over `group`."""

    @staticmethod
    def forward(ctx, e1, e2, log_scale, bias, kernels, group, sharded):
        e1 = e1.contiguous()
        e2 = e2.contiguous()
        log_scale = log_scale.detach().to(torch.float32).reshape(()).contiguous()
        bias = bias.detach().to(torch.float32).reshape(()).contiguous()
        if sharded:
            rank = dist.get_rank(group)
            e1_all, e2_all = gather_embeddings([e1, e2], group)
            q_offset = rank * e1.shape[0]
        else:
            e1_all, e2_all, q_offset = e1, e2, 0
        lse_row, lse_col, loss = kernels.forward(e1, e2, e1_all, e2_all, q_offset, log_scale, bias)
        if sharded:
            both = _gather_rows(torch.stack([lse_row, lse_col]).view(1, 2, -1), group)      # (world, 2, b)
            both = both.permute(1, 0, 2).reshape(2, -1)
            lse_row, lse_col = both[0], both[1]
            loss = D.all_reduce_sum(loss.clone(), group, kind="loss_all_reduce")
        ctx.kernels, ctx.q_offset = kernels, q_offset
        ctx.save_for_backward(e1, e2, e1_all, e2_all, log_scale, bias, lse_row, lse_col)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        e1, e2, e1_all, e2_all, log_scale, bias, lse_row, lse_col = ctx.saved_tensors
        g = grad_out.to(torch.float32).reshape(()).contiguous()
        d1, d2, dscale, dbias = ctx.kernels.backward(e1, e2, e1_all, e2_all, ctx.q_offset, log_scale, bias,
                                                     lse_row, lse_col, g)
        return d1, d2, dscale, dbias, None, None, None


def _is_sharded(global_negatives, group):
    if not (global_negatives and dist.is_available() and dist.is_initialized()):
        return False
    return dist.get_world_size(group) > 1 or global_negatives == "always"     # "always": also a one-rank group (tests)


def clip_loss(embs1, embs2, logit_scale=1.0, logit_bias=0.0, image_encoder=None, lightcurve_encoder=None,
              *, global_negatives=True, group=None, kernels=HipPairKernels):
    """Symmetric softmax InfoNCE of one modality pair (ref src/loss.py:14-38; the two encoder
    keyword arguments are accepted and ignored exactly as in the reference, :19-20)."""
    dev = embs1.device
    logit_scale = torch.as_tensor(logit_scale, dtype=torch.float32, device=dev)
    logit_bias = torch.as_tensor(logit_bias, dtype=torch.float32, device=dev)
    return _PairLoss.apply(embs1, embs2, logit_scale, logit_bias, kernels, group,
                           _is_sharded(global_negatives, group))


def clip_loss_multimodal(embeddings, logit_scales=1.0, logit_biases=0.0, *, global_negatives=True, group=None,
                         kernels=HipPairKernels):
    """Sum over modality pairs i < j (ref src/loss.py:41-65); a 0-dim scale / bias is shared by
    every pair (:49-52), a vector supplies one value per pair in (0,1),(0,2),(1,2)... order."""
    m = len(embeddings)
    if m < 2:
        raise ValueError("clip_loss_multimodal needs at least two modalities")
    dev = embeddings[0].device
    scales = torch.as_tensor(logit_scales, dtype=torch.float32, device=dev)
    biases = torch.as_tensor(logit_biases, dtype=torch.float32, device=dev)
    return _MultiPairLoss.apply(scales, biases, kernels, group, _is_sharded(global_negatives, group), *embeddings)


# ------------------------------------------------------------------------------------- sigmoid loss
class _SigmoidPair(torch.autograd.Function):
    """sigmoid_loss of one modality pair (ref src/loss.py:68-83) on msn_sigmoid_loss_fwd / _bwd."""

    @staticmethod
    def forward(ctx, e1, e2, log_scale, bias, group, sharded, gathered):
        _lib.require_gpu()
        e1, e2 = e1.contiguous(), e2.contiguous()
        if e1.shape != e2.shape:
            raise ValueError("sigmoid_loss needs the same number of rows in both modalities (labels are bs x bs)")
        log_scale = log_scale.detach().to(torch.float32).reshape(()).contiguous()
        bias = bias.detach().to(torch.float32).reshape(()).contiguous()
        if sharded:
            # `gathered`: this pair's columns of the step's ONE packed all-gather (sigmoid_loss_multimodal)
            e1_all, e2_all = gathered if gathered is not None else gather_embeddings([e1, e2], group)
            q_offset = dist.get_rank(group) * e1.shape[0]
        else:
            e1_all, e2_all, q_offset = e1, e2, 0
        _device_f32(("embs1", e1), ("embs2", e2), ("embs1 (gathered)", e1_all), ("embs2 (gathered)", e2_all),
                    ("logit_scale", log_scale), ("logit_bias", bias))
        b, D = e1.shape
        n = e1_all.shape[0]
        L = lib()
        nb = L.msn_infonce_workspace_bytes(b, b, n, n, D)
        ws = torch.empty(max(nb, 16) // 4 + 1, dtype=torch.float32, device=e1.device)
        loss = torch.empty((), dtype=torch.float32, device=e1.device)
        check(L.msn_sigmoid_loss_fwd(ptr(e1), e1.stride(0), ptr(e2), e2.stride(0), b, ptr(e1_all), e1_all.stride(0),
                                     ptr(e2_all), e2_all.stride(0), n, D, q_offset, ptr(log_scale), ptr(bias),
                                     ptr(loss), ptr(ws), nb, stream_ptr()), "msn_sigmoid_loss_fwd")
        ctx.q_offset = q_offset                      # the rank's SHARE of the loss: the caller sums the ranks once
        ctx.save_for_backward(e1, e2, e1_all, e2_all, log_scale, bias)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        e1, e2, e1_all, e2_all, log_scale, bias = ctx.saved_tensors
        g = grad_out.to(torch.float32).reshape(()).contiguous()
        b, D = e1.shape
        n = e1_all.shape[0]
        L = lib()
        nb = L.msn_infonce_workspace_bytes(b, b, n, n, D)
        ws = torch.empty(max(nb, 16) // 4 + 1, dtype=torch.float32, device=e1.device)
        d1, d2 = torch.empty_like(e1), torch.empty_like(e2)
        dsb = torch.empty(2, dtype=torch.float32, device=e1.device)
        check(L.msn_sigmoid_loss_bwd(ptr(e1), e1.stride(0), ptr(e2), e2.stride(0), b, ptr(e1_all), e1_all.stride(0),
                                     ptr(e2_all), e2_all.stride(0), n, D, ctx.q_offset, ptr(log_scale), ptr(bias),
                                     ptr(g), ptr(d1), D, ptr(d2), D, ptr(dsb), ptr(ws), nb, stream_ptr()),
              "msn_sigmoid_loss_bwd")
        return d1, d2, dsb[0], dsb[1], None, None, None


def sigmoid_loss(embs1, embs2, logit_scale=1.0, logit_bias=2.73, *, global_negatives=True, group=None):
    """Sigmoid-based CLIP loss with the reference's sign convention (ref src/loss.py:68-83); returns a
    float32 0-dim tensor (the reference returns float64: the fp64 evaluation happens inside the kernel)."""
    dev = embs1.device
    logit_scale = torch.as_tensor(logit_scale, dtype=torch.float32, device=dev)
    logit_bias = torch.as_tensor(logit_bias, dtype=torch.float32, device=dev)
    sharded = _is_sharded(global_negatives, group)
    share = _SigmoidPair.apply(embs1, embs2, logit_scale, logit_bias, group, sharded, None)
    return _AllReduceSum.apply(share, group) if sharded else share


def sigmoid_loss_multimodal(embeds, logit_scales=1.0, logit_biases=2.73, *, global_negatives=True, group=None):
    """Pairwise sum of sigmoid_loss (ref src/loss.py:86-107)."""
    m = len(embeds)
    if m < 2:
        raise ValueError("sigmoid_loss_multimodal needs at least two modalities")
    dev = embeds[0].device
    scales = torch.as_tensor(logit_scales, dtype=torch.float32, device=dev)
    biases = torch.as_tensor(logit_biases, dtype=torch.float32, device=dev)
    sharded = _is_sharded(global_negatives, group)
    alls = gather_embeddings([e.contiguous() for e in embeds], group) if sharded else None
    total = 0
    for k, (i, j) in enumerate(_pairs(range(m), 2)):
        s = scales if scales.dim() == 0 else scales[k]
        b = biases if biases.dim() == 0 else biases[k]
        total = total + _SigmoidPair.apply(embeds[i], embeds[j], s, b, group, sharded,
                                           (alls[i], alls[j]) if sharded else None)
    return _AllReduceSum.apply(total, group) if sharded else total


# --------------------------------------------------------------------------- alignment + uniformity (Wang & Isola 2020)
ALIGN_UNIFORM_MAX_D = 256


def _align_uniform_args(embs, alpha, t, lam):
    """The refusals of the C-ABI (msn_pair_field, msn_align_uniform_fwd / _bwd), made before anything is enqueued."""
    import math
    if alpha not in (1, 2):
        raise ValueError(f"align_uniform_loss: alpha must be 2 or 1 (got {alpha!r})")
    t, lam = float(t), float(lam)
    if not (t > 0 and math.isfinite(t)):
        raise ValueError(f"align_uniform_loss: t must be finite and positive (got {t})")
    if not (lam >= 0 and math.isfinite(lam)):
        raise ValueError(f"align_uniform_loss: lam must be finite and not negative (got {lam})")
    if len(embs) < 2:
        raise ValueError("align_uniform_loss_multimodal needs at least two modalities")
    _lib.require_gpu()
    _device_f32(*[(f"embeddings[{k}]", e) for k, e in enumerate(embs)])
    shape = tuple(embs[0].shape)
    if len(shape) != 2 or any(tuple(e.shape) != shape for e in embs):
        raise ValueError(f"align_uniform_loss: (N, D) partner sets of one shape needed (got {[tuple(e.shape) for e in embs]})")
    if shape[0] < 2:
        raise _lib.MsnHipError(f"align_uniform_loss: N must be at least 2 (got {shape[0]}): one row has no pair")
    if not 1 <= shape[1] <= ALIGN_UNIFORM_MAX_D:
        raise _lib.MsnHipError(f"align_uniform_loss: D must be in 1..{ALIGN_UNIFORM_MAX_D} (got {shape[1]}); wider embeddings are "
                               "not built")
    return int(alpha), t, lam


class _AlignUniform(torch.autograd.Function):
    """Every modality pair i < j of one step as ONE node.  The row field (r, F) of each tower against itself runs once
    (msn_pair_field); each pair adds its alignment term and lam / 2 (U_i + U_j), so a tower's uniformity and its field carry the
    weight (m - 1) lam / 2.  Nothing is read back: the scalars S and the incoming gradient stay on the device."""

    @staticmethod
    def forward(ctx, alpha, t, lam, *embs):
        from ._device_args import workspace
        from .embedding_metrics import pair_field
        m = len(embs)
        pairs = list(_pairs(range(m), 2))
        embs = [e.detach().contiguous() for e in embs]
        N, D = embs[0].shape
        dev = embs[0].device
        L = lib()
        fields = [pair_field(e, None, t, True) for e in embs]
        losses, comps, d2s = [], [], []
        for i, j in pairs:
            loss = torch.empty((), dtype=torch.float32, device=dev)
            comp = torch.empty(5, dtype=torch.float64, device=dev)
            d2 = torch.empty(N, dtype=torch.float64, device=dev)
            ws = workspace(L.msn_align_uniform_workspace_bytes(N), dev)
            check(L.msn_align_uniform_fwd(ptr(embs[i]), embs[i].stride(0), ptr(embs[j]), embs[j].stride(0), N, D,
                                          ptr(fields[i][0]), ptr(fields[j][0]), alpha, lam, ptr(loss), ptr(comp), ptr(d2),
                                          ptr(ws), ws.numel(), stream_ptr()), "msn_align_uniform_fwd")
            losses.append(loss)
            comps.append(comp)
            d2s.append(d2)
        ctx.m, ctx.pairs, ctx.args = m, pairs, (alpha, t, lam)
        ctx.save_for_backward(*embs, *[f[1] for f in fields], *comps, *d2s)
        ctx.mark_non_differentiable(*comps)
        total = losses[0] if len(losses) == 1 else torch.stack(losses).sum()
        return (total, *comps)

    @staticmethod
    def backward(ctx, grad_out, *_):
        m, pairs = ctx.m, ctx.pairs
        P = len(pairs)
        alpha, t, lam = ctx.args
        s = ctx.saved_tensors
        embs, Fs, comps, d2s = s[:m], s[m:2 * m], s[2 * m:2 * m + P], s[2 * m + P:]
        g = grad_out.to(torch.float32).reshape(()).contiguous()
        N, D = embs[0].shape
        L = lib()
        d_emb = [None] * m
        for k, (i, j) in enumerate(pairs):
            d1, d2 = torch.empty_like(embs[i]), torch.empty_like(embs[j])
            check(L.msn_align_uniform_bwd(ptr(embs[i]), embs[i].stride(0), ptr(embs[j]), embs[j].stride(0), N, D, ptr(Fs[i]),
                                          ptr(Fs[j]), ptr(d2s[k]), ptr(comps[k]), ptr(g), alpha, t, lam, ptr(d1), D, ptr(d2), D,
                                          stream_ptr()), "msn_align_uniform_bwd")
            d_emb[i] = d1 if d_emb[i] is None else d_emb[i].add_(d1)
            d_emb[j] = d2 if d_emb[j] is None else d_emb[j].add_(d2)
        return (None, None, None, *d_emb)


def align_uniform_loss_multimodal(embeddings, alpha=2, t=2.0, lam=1.0, *, global_negatives=True, group=None,
                                  return_components=False):
    """Alignment + uniformity (Wang & Isola 2020) summed over the modality pairs i < j, as clip_loss_multimodal sums:

        L(X, Y) = (1 / N) sum_i |x_i - y_i|^alpha + lam / 2 (U(X) + U(Y)),  U(X) = log mean_{i < j} exp(-t |x_i - x_j|^2)

    for unit-norm (N, D) partner sets, N >= 2, D <= 256, alpha 2 or 1, t > 0, lam >= 0; no logit scale, no bias.  float32
    0-dim tensor, differentiable w.r.t. every set; the gradient is the plain one (no projection onto the sphere: the
    normalisation that made the rows has its own backward).  return_components=True adds, per pair, the fp64 device block
    (align, U_x, U_y, S_x, S_y).
    Data parallel: each rank's own batch is one loss under the ordinary all-reduce of the gradients (global_negatives=False);
    uniformity over the rows gathered from every rank is not built and is refused."""
    embeddings = list(embeddings)
    alpha, t, lam = _align_uniform_args(embeddings, alpha, t, lam)
    if _is_sharded(global_negatives, group):
        raise NotImplementedError("align_uniform_loss: uniformity over the rows of every rank is not built; pass "
                                  "global_negatives=False (each rank's batch is its own loss; the gradients are all-reduced as usual)")
    out = _AlignUniform.apply(alpha, t, lam, *embeddings)
    return (out[0], list(out[1:])) if return_components else out[0]


def align_uniform_loss(e1, e2, alpha=2, t=2.0, lam=1.0, *, global_negatives=True, group=None):
    """align_uniform_loss_multimodal of one modality pair."""
    return align_uniform_loss_multimodal([e1, e2], alpha, t, lam, global_negatives=global_negatives, group=group)


def align_uniform_reference(embs, alpha=2, t=2.0, lam=1.0):
    """numpy longdouble restatement: (loss, [gradient per set]) of align_uniform_loss_multimodal, the uniformity through
    embedding_metrics.pair_field_reference (dU/dx_i = -2 t F_i / S, S = sum_i r_i / 2).  No GPU needed."""
    import numpy as np
    from .embedding_metrics import pair_field_reference
    if alpha not in (1, 2):
        raise ValueError(f"align_uniform_reference: alpha must be 2 or 1 (got {alpha!r})")
    X = [np.asarray(e, dtype=np.float32).astype(np.longdouble) for e in embs]
    m, (N, _) = len(X), X[0].shape
    if m < 2 or N < 2 or any(x.shape != X[0].shape for x in X):
        raise ValueError("align_uniform_reference: at least two (N, D) sets of one shape with N >= 2 needed")
    t, lam = np.longdouble(t), np.longdouble(lam)
    loss = np.longdouble(0)
    grads = [np.zeros(x.shape, dtype=np.longdouble) for x in X]
    for x, g in zip(X, grads):
        r, F = pair_field_reference(x, None, t, True)
        S = r.sum() / 2
        loss += (m - 1) * lam / 2 * np.log(S / (np.longdouble(N) * (N - 1) / 2))
        g -= (m - 1) * lam * t * F / S
    for i, j in _pairs(range(m), 2):
        diff = X[i] - X[j]
        d2 = (diff ** 2).sum(axis=1)
        if alpha == 2:
            loss += d2.sum() / N
            k = np.full(N, np.longdouble(2) / N)
        else:
            d = np.sqrt(d2)
            loss += d.sum() / N
            k = np.where(d > 0, 1 / (N * np.where(d > 0, d, 1)), 0)
        grads[i] += k[:, None] * diff
        grads[j] -= k[:, None] * diff
    return loss, grads


# --------------------------------------------------------------------------- VICReg (Bardes, Ponce, LeCun 2022)
VICREG_MAX_D = 256


def _vicreg_args(embs, sim_coeff, std_coeff, cov_coeff, gamma, eps):
    """The refusals of the C-ABI (msn_column_cov, msn_vicreg_fwd / _bwd), made before anything is enqueued."""
    import math
    coeffs = []
    for name, v in (("sim_coeff", sim_coeff), ("std_coeff", std_coeff), ("cov_coeff", cov_coeff)):
        v = float(v)
        if not (v >= 0 and math.isfinite(v)):
            raise ValueError(f"vicreg_loss: {name} must be finite and not negative (got {v})")
        coeffs.append(v)
    gamma, eps = float(gamma), float(eps)
    if not (gamma >= 0 and math.isfinite(gamma)):
        raise ValueError(f"vicreg_loss: gamma must be finite and not negative (got {gamma})")
    if not (eps > 0 and math.isfinite(eps)):
        raise ValueError(f"vicreg_loss: eps must be finite and positive (got {eps})")
    if len(embs) < 2:
        raise ValueError("vicreg_loss_multimodal needs at least two modalities")
    _lib.require_gpu()
    _device_f32(*[(f"embeddings[{k}]", e) for k, e in enumerate(embs)])
    shape = tuple(embs[0].shape)
    if len(shape) != 2 or any(tuple(e.shape) != shape for e in embs):
        raise ValueError(f"vicreg_loss: (N, D) partner sets of one shape needed (got {[tuple(e.shape) for e in embs]})")
    if shape[0] < 2:
        raise _lib.MsnHipError(f"vicreg_loss: N must be at least 2 (got {shape[0]}): one row has no variance")
    if not 1 <= shape[1] <= VICREG_MAX_D:
        raise _lib.MsnHipError(f"vicreg_loss: D must be in 1..{VICREG_MAX_D} (got {shape[1]}); wider embeddings are not built")
    return (*coeffs, gamma, eps)


class _VICReg(torch.autograd.Function):
    """Every modality pair i < j of one step as ONE node.  The means and the covariance of each tower run once (msn_column_cov);
    each pair adds its invariance term and the variance and covariance terms of its two towers, so a tower's two terms and its
    product (X - mean) M carry the weight m - 1.  Nothing is read back: the incoming gradient stays on the device."""

    @staticmethod
    def forward(ctx, sim_coeff, std_coeff, cov_coeff, gamma, eps, *embs):
        from ._device_args import workspace
        from .embedding_metrics import column_covariance
        m = len(embs)
        pairs = list(_pairs(range(m), 2))
        embs = [e.detach().contiguous() for e in embs]
        N, D = embs[0].shape
        dev = embs[0].device
        L = lib()
        stats = [column_covariance(e) for e in embs]
        losses, comps, Ms = [], [], []
        for i, j in pairs:
            loss = torch.empty((), dtype=torch.float32, device=dev)
            comp = torch.empty(5, dtype=torch.float64, device=dev)
            M = torch.empty((2, D, D), dtype=torch.float64, device=dev)
            ws = workspace(L.msn_vicreg_workspace_bytes(N, D), dev)
            check(L.msn_vicreg_fwd(ptr(embs[i]), embs[i].stride(0), ptr(embs[j]), embs[j].stride(0), N, D, ptr(stats[i][1]),
                                   ptr(stats[j][1]), sim_coeff, std_coeff, cov_coeff, gamma, eps, ptr(loss), ptr(comp), ptr(M[0]),
                                   ptr(M[1]), ptr(ws), ws.numel(), stream_ptr()), "msn_vicreg_fwd")
            losses.append(loss)
            comps.append(comp)
            Ms.append(M)
        ctx.m, ctx.pairs, ctx.sim_coeff = m, pairs, sim_coeff
        ctx.save_for_backward(*embs, *[s[0] for s in stats], *Ms)
        ctx.mark_non_differentiable(*comps)
        total = losses[0] if len(losses) == 1 else torch.stack(losses).sum()
        return (total, *comps)

    @staticmethod
    def backward(ctx, grad_out, *_):
        m, pairs = ctx.m, ctx.pairs
        s = ctx.saved_tensors
        embs, means, Ms = s[:m], s[m:2 * m], s[2 * m:]
        g = grad_out.to(torch.float32).reshape(()).contiguous()
        N, D = embs[0].shape
        L = lib()
        d_emb = [None] * m
        for k, (i, j) in enumerate(pairs):
            d1, d2 = torch.empty_like(embs[i]), torch.empty_like(embs[j])
            check(L.msn_vicreg_bwd(ptr(embs[i]), embs[i].stride(0), ptr(embs[j]), embs[j].stride(0), N, D, ptr(means[i]),
                                   ptr(means[j]), ptr(Ms[k][0]), ptr(Ms[k][1]), ptr(g), ctx.sim_coeff, ptr(d1), D, ptr(d2), D,
                                   stream_ptr()), "msn_vicreg_bwd")
            d_emb[i] = d1 if d_emb[i] is None else d_emb[i].add_(d1)
            d_emb[j] = d2 if d_emb[j] is None else d_emb[j].add_(d2)
        return (None, None, None, None, None, *d_emb)


def vicreg_loss_multimodal(embeddings, sim_coeff=25.0, std_coeff=25.0, cov_coeff=1.0, gamma=1.0, eps=1e-4, *,
                           global_negatives=True, group=None, return_components=False):
    """VICReg (Bardes, Ponce, LeCun 2022) summed over the modality pairs i < j, as align_uniform_loss_multimodal sums:

        L(X, Y) = sim_coeff inv + std_coeff (var(X) + var(Y)) + cov_coeff (cov(X) + cov(Y))
        inv = mean_ic (x_ic - y_ic)^2,  var(X) = mean_c max(0, gamma - sqrt(C_cc + eps)),  cov(X) = (1 / D) sum_{c != c'} C_cc'^2

    with C the covariance of the centred columns, C = Xc^T Xc / (N - 1), for (N, D) partner sets (not assumed unit-norm),
    N >= 2, D <= 256; no negatives, no logit scale, no bias.  float32 0-dim tensor, differentiable w.r.t. every set; the hinge
    is inactive at sqrt(C_cc + eps) == gamma.  return_components=True adds, per pair, the fp64 device block
    (inv, var_x, var_y, cov_x, cov_y).
    Data parallel: each rank's own batch is one loss under the ordinary all-reduce of the gradients (global_negatives=False);
    statistics over the rows of every rank are not built and are refused."""
    embeddings = list(embeddings)
    args = _vicreg_args(embeddings, sim_coeff, std_coeff, cov_coeff, gamma, eps)
    if _is_sharded(global_negatives, group):
        raise NotImplementedError("vicreg_loss: means and covariances over the rows of every rank are not built; pass "
                                  "global_negatives=False (each rank's batch is its own loss; the gradients are all-reduced as usual)")
    out = _VICReg.apply(*args, *embeddings)
    return (out[0], list(out[1:])) if return_components else out[0]


def vicreg_loss(e1, e2, sim_coeff=25.0, std_coeff=25.0, cov_coeff=1.0, gamma=1.0, eps=1e-4, *, global_negatives=True, group=None):
    """vicreg_loss_multimodal of one modality pair."""
    return vicreg_loss_multimodal([e1, e2], sim_coeff, std_coeff, cov_coeff, gamma, eps, global_negatives=global_negatives,
                                  group=group)


def vicreg_reference(embs, sim_coeff=25.0, std_coeff=25.0, cov_coeff=1.0, gamma=1.0, eps=1e-4, return_terms=False):
    """numpy longdouble restatement: (loss, [gradient per set]) of vicreg_loss_multimodal.  return_terms=True adds
    {"inv": {(i, j): .}, "var": [per set], "cov": [per set]}.  No GPU needed."""
    import numpy as np
    from .embedding_metrics import column_covariance_reference
    X = [np.asarray(e, dtype=np.float32).astype(np.longdouble) for e in embs]
    m = len(X)
    if m < 2 or X[0].ndim != 2 or X[0].shape[0] < 2 or any(x.shape != X[0].shape for x in X):
        raise ValueError("vicreg_reference: at least two (N, D) sets of one shape with N >= 2 needed")
    N, D = X[0].shape
    sim, std, covc, gamma, eps = (np.longdouble(v) for v in (sim_coeff, std_coeff, cov_coeff, gamma, eps))
    loss = np.longdouble(0)
    grads = [np.zeros(x.shape, dtype=np.longdouble) for x in X]
    terms = {"inv": {}, "var": [], "cov": []}
    for x, g in zip(X, grads):
        mean, C = column_covariance_reference(x)
        s = np.sqrt(np.diag(C) + eps)
        off = C - np.diag(np.diag(C))
        var, cov = np.maximum(gamma - s, 0).sum() / D, (off ** 2).sum() / D
        terms["var"].append(var)
        terms["cov"].append(cov)
        loss += (m - 1) * (std * var + covc * cov)
        M = 4 * covc / (D * np.longdouble(N - 1)) * off - np.diag(np.where(s < gamma, std / (D * np.longdouble(N - 1) * s), 0))
        g += (m - 1) * ((x - mean) @ M)
    for i, j in _pairs(range(m), 2):
        diff = X[i] - X[j]
        inv = (diff ** 2).sum() / (np.longdouble(N) * D)
        terms["inv"][(i, j)] = inv
        loss += sim * inv
        grads[i] += 2 * sim / (np.longdouble(N) * D) * diff
        grads[j] -= 2 * sim / (np.longdouble(N) * D) * diff
    return (loss, grads, terms) if return_terms else (loss, grads)


# --------------------------------------------------------------------------- Barlow Twins (Zbontar et al. 2021)
BARLOW_MAX_D = 256


def _barlow_args(embs, lambd, eps):
    """The refusals of the C-ABI (msn_cross_cov, msn_barlow_fwd / _bwd), made before anything is enqueued."""
    import math
    lambd, eps = float(lambd), float(eps)
    if not (lambd >= 0 and math.isfinite(lambd)):
        raise ValueError(f"barlow_twins_loss: lambd must be finite and not negative (got {lambd})")
    if not (eps > 0 and math.isfinite(eps)):
        raise ValueError(f"barlow_twins_loss: eps must be finite and positive (got {eps})")
    if len(embs) < 2:
        raise ValueError("barlow_twins_loss_multimodal needs at least two modalities")
    _lib.require_gpu()
    _device_f32(*[(f"embeddings[{k}]", e) for k, e in enumerate(embs)])
    shape = tuple(embs[0].shape)
    if len(shape) != 2 or any(tuple(e.shape) != shape for e in embs):
        raise ValueError(f"barlow_twins_loss: (N, D) partner sets of one shape needed (got {[tuple(e.shape) for e in embs]})")
    if shape[0] < 2:
        raise _lib.MsnHipError(f"barlow_twins_loss: N must be at least 2 (got {shape[0]}): one row has no variance")
    if not 1 <= shape[1] <= BARLOW_MAX_D:
        raise _lib.MsnHipError(f"barlow_twins_loss: D must be in 1..{BARLOW_MAX_D} (got {shape[1]}); wider embeddings are not built")
    return lambd, eps


class _BarlowTwins(torch.autograd.Function):
    """Every modality pair i < j of one step as ONE node.  Each pair runs its own statistics (msn_cross_cov: the means and
    variances of both towers and their cross covariance) and the D^2 assembly (msn_barlow_fwd) in forward; the means, M and d are
    saved, and each pair's backward launch adds into its two towers' gradients.  Nothing is read back: the incoming gradient
    stays on the device."""

    @staticmethod
    def forward(ctx, lambd, eps, *embs):
        from .embedding_metrics import _barlow_fwd, _cross_cov
        m = len(embs)
        pairs = list(_pairs(range(m), 2))
        embs = [e.detach().contiguous() for e in embs]
        N = embs[0].shape[0]
        losses, comps, saved = [], [], []
        for i, j in pairs:
            mx, my, vx, vy, cov = _cross_cov(embs[i], embs[j])
            loss, comp, _, M, d = _barlow_fwd(vx, vy, cov, N, lambd, eps)
            losses.append(loss)
            comps.append(comp)
            saved += [mx, my, M, d]
        ctx.m, ctx.pairs = m, pairs
        ctx.save_for_backward(*embs, *saved)
        ctx.mark_non_differentiable(*comps)
        total = losses[0] if len(losses) == 1 else torch.stack(losses).sum()
        return (total, *comps)

    @staticmethod
    def backward(ctx, grad_out, *_):
        m, pairs = ctx.m, ctx.pairs
        s = ctx.saved_tensors
        embs, saved = s[:m], s[m:]
        g = grad_out.to(torch.float32).reshape(()).contiguous()
        N, D = embs[0].shape
        L = lib()
        d_emb = [None] * m
        for k, (i, j) in enumerate(pairs):
            mx, my, M, d = saved[4 * k:4 * k + 4]
            d1, d2 = torch.empty_like(embs[i]), torch.empty_like(embs[j])
            check(L.msn_barlow_bwd(ptr(embs[i]), embs[i].stride(0), ptr(embs[j]), embs[j].stride(0), N, D, ptr(mx), ptr(my), ptr(M[0]),
                                   ptr(M[1]), ptr(d[0]), ptr(d[1]), ptr(g), ptr(d1), D, ptr(d2), D, stream_ptr()), "msn_barlow_bwd")
            d_emb[i] = d1 if d_emb[i] is None else d_emb[i].add_(d1)
            d_emb[j] = d2 if d_emb[j] is None else d_emb[j].add_(d2)
        return (None, None, *d_emb)


def barlow_twins_loss_multimodal(embeddings, lambd=5e-3, eps=1e-5, *, global_negatives=True, group=None, return_components=False):
    """Barlow Twins (Zbontar, Jing, Misra, LeCun, Deny 2021) summed over the modality pairs i < j:

        L(X, Y) = sum_a (c_aa - 1)^2 + lambd sum_{a != b} c_ab^2,    c = Xhat^T Yhat / N

    with Xhat, Yhat the columns standardised as BatchNorm1d(affine=False) does in training (biased variance, eps inside the
    root), for (N, D) partner sets (not assumed unit-norm), N >= 2, D <= 256; no negatives, no logit scale, no bias, no scale
    factor on the loss.  float32 0-dim tensor, differentiable w.r.t. every set.  return_components=True adds, per pair, the
    fp64 device block (on, off).
    Data parallel: each rank's own batch is one loss under the ordinary all-reduce of the gradients (global_negatives=False);
    statistics over the rows of every rank are not built and are refused."""
    embeddings = list(embeddings)
    args = _barlow_args(embeddings, lambd, eps)
    if _is_sharded(global_negatives, group):
        raise NotImplementedError("barlow_twins_loss: means and correlations over the rows of every rank are not built; pass "
                                  "global_negatives=False (each rank's batch is its own loss; the gradients are all-reduced as usual)")
    out = _BarlowTwins.apply(*args, *embeddings)
    return (out[0], list(out[1:])) if return_components else out[0]


def barlow_twins_loss(e1, e2, lambd=5e-3, eps=1e-5, *, global_negatives=True, group=None):
    """barlow_twins_loss_multimodal of one modality pair."""
    return barlow_twins_loss_multimodal([e1, e2], lambd, eps, global_negatives=global_negatives, group=group)


def barlow_twins_reference(embs, lambd=5e-3, eps=1e-5, return_terms=False):
    """numpy longdouble restatement: (loss, [gradient per set]) of barlow_twins_loss_multimodal.  return_terms=True adds
    {"on": {(i, j): .}, "off": {(i, j): .}, "corr": {(i, j): c}, "magnitude": [per set]}, the last being the sum over the set's
    pairs of |Yc A^T| + |Xc diag(d)|, the magnitudes of the two terms of its gradient (they nearly cancel where c is close to
    +-1, so an error is measured against them and not against their difference).  No GPU needed."""
    import numpy as np
    X = [np.asarray(e, dtype=np.float32).astype(np.longdouble) for e in embs]
    m = len(X)
    if m < 2 or X[0].ndim != 2 or X[0].shape[0] < 2 or any(x.shape != X[0].shape for x in X):
        raise ValueError("barlow_twins_reference: at least two (N, D) sets of one shape with N >= 2 needed")
    N, D = X[0].shape
    n, lam, eps = np.longdouble(N), np.longdouble(lambd), np.longdouble(eps)
    diag = np.eye(D, dtype=bool)
    loss = np.longdouble(0)
    grads = [np.zeros(x.shape, dtype=np.longdouble) for x in X]
    terms = {"on": {}, "off": {}, "corr": {}, "magnitude": [np.zeros(x.shape, dtype=np.longdouble) for x in X]}
    for i, j in _pairs(range(m), 2):
        xc, yc = X[i] - X[i].sum(axis=0) / n, X[j] - X[j].sum(axis=0) / n
        sx, sy = np.sqrt((xc * xc).sum(axis=0) / n + eps), np.sqrt((yc * yc).sum(axis=0) / n + eps)
        ss = np.outer(sx, sy)
        c = (xc.T @ yc) / n / ss
        on, off = ((np.diag(c) - 1) ** 2).sum(), (np.where(diag, 0, c) ** 2).sum()
        G = np.where(diag, 2 * (c - 1), 2 * lam * c)
        A = G / (n * ss)
        r, q = (G * c).sum(axis=1), (G * c).sum(axis=0)
        px, ox = yc @ A.T, xc * (-r / (n * sx * sx))
        py, oy = xc @ A, yc * (-q / (n * sy * sy))
        grads[i] += px + ox
        grads[j] += py + oy
        terms["magnitude"][i] += np.abs(px) + np.abs(ox)
        terms["magnitude"][j] += np.abs(py) + np.abs(oy)
        terms["on"][(i, j)], terms["off"][(i, j)], terms["corr"][(i, j)] = on, off, c
        loss += on + lam * off
    return (loss, grads, terms) if return_terms else (loss, grads)


# --------------------------------------------------------------------------- label-aware contrastive loss (SupCon / UniCL)
SUPCON_MAX_D = 256


class HipSupConKernels:
    """msn_supcon_fwd / msn_supcon_bwd through the C-ABI (the interface of HipPairKernels plus the gathered int32 labels and the
    counts of positives of the local rows)."""

    @staticmethod
    def _ws(e1_loc, e1_all):
        b, D = e1_loc.shape
        n = e1_all.shape[0]
        nb = lib().msn_supcon_workspace_bytes(b, b, n, n, D)
        return nb, torch.empty(max(nb, 16) // 4 + 1, dtype=torch.float32, device=e1_loc.device)

    @staticmethod
    def _check(e1_loc, e2_loc, e1_all, e2_all, labels_all):
        if labels_all.device != e1_loc.device or labels_all.dtype != torch.int32 or labels_all.dim() != 1 or labels_all.stride(0) != 1:
            raise _lib.MsnHipError("labels (gathered) must be contiguous int32 on the embeddings' device")
        D = e1_loc.shape[1]
        if e2_loc.shape[1] != D or e1_all.shape[1] != D or e2_all.shape[1] != D:
            raise _lib.MsnHipError("both modalities must share the embedding width")
        if e1_loc.shape[0] != e2_loc.shape[0] or e1_all.shape[0] != e2_all.shape[0]:
            raise _lib.MsnHipError("embs1 and embs2 must have the same number of rows (the label-aware loss needs b1 == b2, n1 == n2)")
        if labels_all.numel() != e1_all.shape[0]:
            raise _lib.MsnHipError(f"labels (gathered): {labels_all.numel()} labels for {e1_all.shape[0]} rows")

    @staticmethod
    def forward(e1_loc, e2_loc, e1_all, e2_all, labels_all, q_offset, log_scale, bias):
        _lib.require_gpu()
        _device_f32(("embs1", e1_loc), ("embs2", e2_loc), ("embs1 (gathered)", e1_all), ("embs2 (gathered)", e2_all),
                    ("logit_scale", log_scale), ("logit_bias", bias))
        HipSupConKernels._check(e1_loc, e2_loc, e1_all, e2_all, labels_all)
        b, D = e1_loc.shape
        n = e1_all.shape[0]
        dev = e1_loc.device
        nb, ws = HipSupConKernels._ws(e1_loc, e1_all)
        lse_row = torch.empty(b, dtype=torch.float32, device=dev)
        lse_col = torch.empty(b, dtype=torch.float32, device=dev)
        cnt = torch.empty(b, dtype=torch.int32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        check(lib().msn_supcon_fwd(ptr(e1_loc), e1_loc.stride(0), b, ptr(e2_loc), e2_loc.stride(0), b,
                                   ptr(e1_all), e1_all.stride(0), n, ptr(e2_all), e2_all.stride(0), n, D, q_offset,
                                   ptr(labels_all), ptr(log_scale), ptr(bias), ptr(lse_row), ptr(lse_col), ptr(cnt), ptr(loss),
                                   ptr(ws), nb, stream_ptr()), "msn_supcon_fwd")
        return lse_row, lse_col, cnt, loss

    @staticmethod
    def backward(e1_loc, e2_loc, e1_all, e2_all, labels_all, q_offset, log_scale, bias, lse_row_all, lse_col_all, cnt, grad_out):
        _lib.require_gpu()
        _device_f32(("embs1", e1_loc), ("embs2", e2_loc), ("embs1 (gathered)", e1_all), ("embs2 (gathered)", e2_all),
                    ("logit_scale", log_scale), ("logit_bias", bias), ("lse_row", lse_row_all), ("lse_col", lse_col_all),
                    ("grad_out", grad_out))
        HipSupConKernels._check(e1_loc, e2_loc, e1_all, e2_all, labels_all)
        b, D = e1_loc.shape
        n = e1_all.shape[0]
        if lse_row_all.numel() < n or lse_col_all.numel() < n:
            raise _lib.MsnHipError("backward needs the log-sum-exp of every gathered row")
        if cnt.device != e1_loc.device or cnt.dtype != torch.int32 or cnt.numel() != b:
            raise _lib.MsnHipError("cnt must hold one int32 count per local row on the embeddings' device")
        lse_row_all, lse_col_all, cnt = lse_row_all.contiguous(), lse_col_all.contiguous(), cnt.contiguous()
        dev = e1_loc.device
        nb, ws = HipSupConKernels._ws(e1_loc, e1_all)
        d1 = torch.empty((b, D), dtype=torch.float32, device=dev)
        d2 = torch.empty((b, D), dtype=torch.float32, device=dev)
        dsb = torch.empty(2, dtype=torch.float32, device=dev)
        check(lib().msn_supcon_bwd(ptr(e1_loc), e1_loc.stride(0), b, ptr(e2_loc), e2_loc.stride(0), b,
                                   ptr(e1_all), e1_all.stride(0), n, ptr(e2_all), e2_all.stride(0), n, D, q_offset,
                                   ptr(labels_all), ptr(log_scale), ptr(bias), ptr(lse_row_all), ptr(lse_col_all), ptr(cnt),
                                   ptr(grad_out), ptr(d1), D, ptr(d2), D, ptr(dsb), ptr(ws), nb, stream_ptr()),
              "msn_supcon_bwd")
        return d1, d2, dsb[0], dsb[1]


def _supcon_args(embs, labels, world=1):
    """The refusals of supcon_loss / supcon_loss_multimodal, made before anything is enqueued; each message names the argument.
    -> the labels as they go to the device conversion.  Shapes first, label values next, devices last, so that every refusal can
    be met without a GPU.  The value check of FLOATING labels reads the tensor and is skipped while a graph is being captured
    (integer labels are never read)."""
    if len(embs) < 2:
        raise ValueError("supcon_loss_multimodal: embeddings must hold at least two modalities")
    for k, e in enumerate(embs):
        if not torch.is_tensor(e) or e.dim() != 2:
            raise ValueError(f"supcon_loss: embeddings[{k}] must be a (b, D) tensor")
    b, D = embs[0].shape
    if any(e.shape[0] != b for e in embs):
        raise ValueError(f"supcon_loss: embeddings must have the same batch size in every modality (got {[e.shape[0] for e in embs]}); "
                         "a label belongs to one row of each")
    if any(e.shape[1] != D for e in embs):
        raise ValueError(f"supcon_loss: embeddings must share the width D (got {[e.shape[1] for e in embs]})")
    if not 1 <= D <= SUPCON_MAX_D:
        raise _lib.MsnHipError(f"supcon_loss: embeddings: D must be in 1..{SUPCON_MAX_D} (got {D}); wider embeddings are not built")
    if b < 1:
        raise ValueError("supcon_loss: embeddings must have at least one row")
    if b * world >= 2 ** 31:
        raise _lib.MsnHipError(f"supcon_loss: embeddings: N = {b * world} rows; N must be below 2^31")
    if not torch.is_tensor(labels):
        raise TypeError("supcon_loss: labels must be a tensor of b integers")
    if labels.dim() != 1 or labels.shape[0] != b:
        raise ValueError(f"supcon_loss: labels must have shape ({b},), one per row of the embeddings (got {tuple(labels.shape)})")
    if labels.dtype == torch.bool or labels.is_complex():
        raise TypeError(f"supcon_loss: labels must have an integer or floating dtype holding integers (got {labels.dtype})")
    if labels.is_floating_point():
        capturing = labels.is_cuda and torch.cuda.is_current_stream_capturing()
        if not capturing and not bool(((labels == labels.round()) & (labels.abs() < 2 ** 31)).all()):
            raise ValueError("supcon_loss: labels must hold integer values (a negative integer marks an unknown class)")
    for k, e in enumerate(embs):
        if e.device.type != "cuda":
            raise _lib.MsnHipError(f"supcon_loss: embeddings[{k}] must live on the GPU (got {e.device}); the loss has no CPU path")
        if e.dtype != torch.float32:
            raise _lib.MsnHipError(f"supcon_loss: embeddings[{k}] must be float32 (got {e.dtype})")
    if labels.device != embs[0].device:
        raise _lib.MsnHipError(f"supcon_loss: labels must live on the embeddings' device {embs[0].device} (got {labels.device})")
    return labels


class _SupConLoss(torch.autograd.Function):
    """supcon_loss_multimodal as ONE node, built like _MultiPairLoss: every modality pair i < j of one step with the same labels,
    single process or row-sharded over `group`.  Sharded, the labels travel in one extra all-gather; the embeddings, the
    log-sum-exps and the loss share travel exactly as in _MultiPairLoss, the counts stay local, and each rank ends with the
    complete dE of its own rows."""

    @staticmethod
    def forward(ctx, scales, biases, labels, kernels, group, sharded, *embs):
        m = len(embs)
        pairs = list(_pairs(range(m), 2))
        embs = [e.contiguous() for e in embs]
        scales = scales.detach().to(torch.float32)
        biases = biases.detach().to(torch.float32)
        if scales.dim() > 0 and scales.numel() < len(pairs) or biases.dim() > 0 and biases.numel() < len(pairs):
            raise ValueError(f"{len(pairs)} modality pairs need {len(pairs)} logit scales / biases (or one shared scalar)")
        s_k = [(scales if scales.dim() == 0 else scales[k]).reshape(()).contiguous() for k in range(len(pairs))]
        b_k = [(biases if biases.dim() == 0 else biases[k]).reshape(()).contiguous() for k in range(len(pairs))]
        labels = labels.detach().to(torch.int32).contiguous()          # on the device: nothing is read
        if sharded:
            alls = gather_embeddings(embs, group)
            labels_all = D.all_gather_rows(labels, group, kind="label_all_gather")
            q_offset = dist.get_rank(group) * embs[0].shape[0]
        else:
            alls, labels_all, q_offset = embs, labels, 0
        lses, cnts, losses = [], [], []
        for k, (i, j) in enumerate(pairs):
            lse_row, lse_col, cnt, loss = kernels.forward(embs[i], embs[j], alls[i], alls[j], labels_all, q_offset, s_k[k], b_k[k])
            lses += [lse_row, lse_col]
            cnts.append(cnt)
            losses.append(loss)
        total = losses[0] if len(losses) == 1 else torch.stack(losses).sum()
        if sharded:
            b = embs[0].shape[0]
            world = dist.get_world_size(group)
            pack = torch.stack(lses)                                                        # (2P, b)
            g = D.all_gather_rows(pack.view(1, 2 * len(pairs), b), group, kind="lse_all_gather")   # (world, 2P, b)
            lse_all = g.permute(1, 0, 2).reshape(2 * len(pairs), world * b)
            lses = [lse_all[r] for r in range(2 * len(pairs))]
            total = D.all_reduce_sum(total.clone(), group, kind="loss_all_reduce")
        ctx.kernels, ctx.q_offset, ctx.pairs, ctx.m = kernels, q_offset, pairs, m
        ctx.shapes = (scales.shape, biases.shape)
        ctx.save_for_backward(*embs, *alls, *s_k, *b_k, *lses, *cnts, labels_all)
        return total

    @staticmethod
    def backward(ctx, grad_out):
        m, pairs = ctx.m, ctx.pairs
        P = len(pairs)
        t = ctx.saved_tensors
        embs, alls = t[:m], t[m:2 * m]
        s_k, b_k = t[2 * m:2 * m + P], t[2 * m + P:2 * m + 2 * P]
        lses, cnts, labels_all = t[2 * m + 2 * P:2 * m + 4 * P], t[2 * m + 4 * P:2 * m + 5 * P], t[-1]
        g = grad_out.to(torch.float32).reshape(()).contiguous()
        d_emb = [None] * m
        d_s, d_b = [], []
        for k, (i, j) in enumerate(pairs):
            d1, d2, ds, db = ctx.kernels.backward(embs[i], embs[j], alls[i], alls[j], labels_all, ctx.q_offset, s_k[k], b_k[k],
                                                  lses[2 * k], lses[2 * k + 1], cnts[k], g)
            d_emb[i] = d1 if d_emb[i] is None else d_emb[i].add_(d1)
            d_emb[j] = d2 if d_emb[j] is None else d_emb[j].add_(d2)
            d_s.append(ds)
            d_b.append(db)
        s_shape, b_shape = ctx.shapes
        if P == 1:
            gs, gb = d_s[0].reshape(s_shape), d_b[0].reshape(b_shape)
        else:
            gs, gb = torch.stack(d_s), torch.stack(d_b)
            gs = gs.sum() if len(s_shape) == 0 else gs
            gb = gb.sum() if len(b_shape) == 0 else gb
        return (gs, gb, None, None, None, None, *d_emb)


def supcon_loss_multimodal(embeddings, labels, logit_scales=1.0, logit_biases=0.0, *, global_negatives=True, group=None,
                           kernels=HipSupConKernels):
    """Label-aware contrastive loss (SupCon, Khosla et al. 2020, in the cross-modal form of UniCL, Yang et al. 2022) summed over
    the modality pairs i < j with the same labels, as clip_loss_multimodal sums.  Per pair, with S = s E_j E_i^T + b:

        P_ij = [i == j] or (y_i == y_j and y_i >= 0),   c_i = sum_j P_ij
        loss = 1/(2N) sum_i [ LSE_j S_ij - (1/c_i) sum_j P_ij S_ij  +  LSE_j S_ji - (1/c_i) sum_j P_ji S_ji ]

    `labels`: (b,) integers (any integer dtype, or a floating dtype holding integers) on the embeddings' device, converted to int32
    there (the values must fit int32).  A negative label is "class unknown": the row is a singleton class whose only positive is its partner, so it trains as a
    plain InfoNCE row; with all labels distinct the loss is clip_loss.  `logit_scales` is the LOG of the scale.  float32 0-dim
    tensor, differentiable w.r.t. every embedding matrix, the scales and the biases; `labels` gets no gradient.  Every modality
    needs the same batch size, D <= 256, N < 2^31.  Data parallel with global_negatives: every rank passes its local rows and
    labels; the labels travel in one extra all-gather."""
    embeddings = list(embeddings)
    sharded = _is_sharded(global_negatives, group)
    labels = _supcon_args(embeddings, labels, dist.get_world_size(group) if sharded else 1)
    dev = embeddings[0].device
    scales = torch.as_tensor(logit_scales, dtype=torch.float32, device=dev)
    biases = torch.as_tensor(logit_biases, dtype=torch.float32, device=dev)
    return _SupConLoss.apply(scales, biases, labels, kernels, group, sharded, *embeddings)


def supcon_loss(embs1, embs2, labels, logit_scale=1.0, logit_bias=0.0, *, global_negatives=True, group=None,
                kernels=HipSupConKernels):
    """supcon_loss_multimodal of one modality pair: rows of S from embs2, columns from embs1, as clip_loss forms it."""
    return supcon_loss_multimodal([embs1, embs2], labels, logit_scale, logit_bias, global_negatives=global_negatives, group=group,
                                  kernels=kernels)


def supcon_reference(embs, labels, logit_scales=1.0, logit_biases=0.0):
    """torch fp64 restatement of supcon_loss_multimodal from log_softmax and a boolean mask, on any device:
    -> (loss, [dloss/dE per modality], dloss/dlogit_scales, dloss/dlogit_biases), the last two in the shape given (a scalar
    shared by every pair, or one value per pair)."""
    E = [torch.as_tensor(e).detach().to(torch.float64).requires_grad_(True) for e in embs]
    dev = E[0].device
    y = torch.as_tensor(labels).to(dev).to(torch.float64).round().to(torch.int64)
    ls = torch.as_tensor(logit_scales).detach().to(dev).to(torch.float64).requires_grad_(True)
    lb = torch.as_tensor(logit_biases).detach().to(dev).to(torch.float64).requires_grad_(True)
    N = E[0].shape[0]
    mask = (y[:, None] == y[None, :]) & (y >= 0)[:, None] | torch.eye(N, dtype=torch.bool, device=dev)
    w = mask.to(torch.float64) / mask.sum(1, keepdim=True)
    total = 0.0
    for k, (i, j) in enumerate(_pairs(range(len(E)), 2)):
        s = ls if ls.dim() == 0 else ls[k]
        b = lb if lb.dim() == 0 else lb[k]
        S = torch.exp(s) * (E[j] @ E[i].T) + b
        rows = -(w * torch.log_softmax(S, dim=1)).sum()
        cols = -(w * torch.log_softmax(S.T, dim=1)).sum()
        total = total + (rows + cols) / (2 * N)
    grads = torch.autograd.grad(total, [*E, ls, lb])
    return total.detach(), list(grads[:len(E)]), grads[-2], grads[-1]
