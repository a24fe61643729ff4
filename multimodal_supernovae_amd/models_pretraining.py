"""Masked-light-curve pretraining with the reference's surface, src/models_pretraining.py:
`get_random_mask`, `get_continous_random_mask` (masks as set operations on the device; the random draws are the
reference's -- one per sample / band, in its order -- so a seeded run hides the same points) and
`MaskedLightCurveEncoder` = TransformerWithTimeEmbeddings(agg="pretraining") + Linear(emb, 1), trained with an
MSE on the hidden points.  The transformer, the read-out GEMM and the masked MSE run on libmsn_hip.
`device_masks` draws the same kinds of mask in one launch on the padding mask's device (csrc/pretrain_masks.hip: its own counter-
based draws, the same mask rules and distribution); MaskedLightCurveEncoder(mask_generator="device") trains with them, keeps
nothing on the host and can be recorded by trainer.GraphedTrainStep."""
import random
from typing import Dict, Tuple

import torch
import torch.nn as nn

from . import functional as F_
from . import ops
from ._lib import check, lib, ptr, stream_ptr
from .transformer_utils import TransformerWithTimeEmbeddings


def _hidden_counts(observed_counts, f_mask):
    """floor(n_observed * f_mask) in double precision, as Python's int(n * f) gives it."""
    return (observed_counts.to(torch.float64) * float(f_mask)).floor().to(torch.int64)


def random_masks_from_order(padding_mask, order, f_mask=0.15):
    """get_random_mask's formulas for a given ranking: `order` (B, T) integers, the rank of every observed point among its
    sample's observed points (anything at the padded positions); the points ranked below floor(f_mask * n_observed) hide.
    Returns (mask, mask_pred) on the padding mask's device."""
    pad = padding_mask.to(torch.bool)
    n_hide = _hidden_counts(pad.sum(dim=1), f_mask)
    hidden = torch.as_tensor(order, dtype=torch.int64).to(pad.device) < n_hide.to(pad.device)[:, None]
    return pad & ~hidden, pad & hidden


def get_random_mask(padding_mask, f_mask=0.15):
    """Hide a random fraction of the observed points of every sample (ref src/models_pretraining.py:17-55).
    Returns (mask, mask_pred): `mask` = the padding mask without the hidden points, `mask_pred` = the hidden points.

    Set formulation: draw, per sample, one ranking of its observed points (ONE torch.randperm(n_observed) call per sample,
    in sample order -- the reference's draws, so a seeded run hides the same points), call the points ranked below
    n_hide = floor(f_mask * n_observed) "hidden", and build both outputs from the hidden set with two mask operations on
    the device the padding mask lives on (random_masks_from_order)."""
    pad = padding_mask.to(torch.bool)
    B, T = pad.shape
    n_obs = pad.sum(dim=1)
    order = torch.full((B, T), T, dtype=torch.int64)              # rank of every observed point in its sample's draw
    pad_host = pad.cpu()
    for i, n in enumerate(n_obs.tolist()):
        ranks = torch.empty(n, dtype=torch.int64)
        ranks[torch.randperm(n)] = torch.arange(n)                 # the j-th observed point has rank ranks[j]
        order[i, pad_host[i]] = ranks
    return random_masks_from_order(pad, order, f_mask)


def continuous_masks_from_starts(padding_mask, nbands, starts, f_mask=0.15):
    """get_continous_random_mask's formulas for given run starts: `starts` (B, nbands) integers, the first hidden position of
    every band (absolute, in [band k, band k + n - h]).  Returns (mask, mask_pred) on the padding mask's device."""
    pad = padding_mask.to(torch.bool)
    B, T = pad.shape
    band = T // nbands
    n_obs = pad[:, :band * nbands].reshape(B, nbands, band).sum(dim=2)
    n_hide = _hidden_counts(n_obs, f_mask)
    starts = torch.as_tensor(starts, dtype=torch.int64).reshape(B, nbands)
    pos = torch.arange(T, device=pad.device)[None, :].expand(B, T)
    which = torch.clamp(pos // band, max=nbands - 1)               # band of every position (a ragged tail joins the last band)
    lo = torch.gather(starts.to(pad.device), 1, which)
    hi = lo + torch.gather(n_hide.to(pad.device), 1, which)
    inside = (pos >= lo) & (pos < hi) & (pos < band * nbands)
    mask_pred = pad & inside
    mask_pred[:, band * nbands:] = pad[:, band * nbands:]          # positions beyond the last whole band are left as they are
    return pad & ~inside, mask_pred


def get_continous_random_mask(padding_mask, nbands, f_mask=0.15):
    """Hide one random CONTIGUOUS run of observed points per band (ref src/models_pretraining.py:58-98): in band k of
    sample i, with n observed points (packed at the start of the band) and h = floor(f_mask * n), the run starts at a
    uniformly drawn offset in [0, n - h] (ONE random.randint per (sample, band), sample-major: the reference's draws) and
    is h long.  Both outputs are then interval tests against the drawn starts (continuous_masks_from_starts), on the padding
    mask's device."""
    pad = padding_mask.to(torch.bool)
    B, T = pad.shape
    band = T // nbands
    n_obs = pad[:, :band * nbands].reshape(B, nbands, band).sum(dim=2)
    n_hide = _hidden_counts(n_obs, f_mask)
    starts = torch.tensor([[random.randint(band * k, band * k + n - h) for k, (n, h) in enumerate(zip(ns, hs))]
                           for ns, hs in zip(n_obs.tolist(), n_hide.tolist())], dtype=torch.int64).reshape(B, nbands)
    return continuous_masks_from_starts(pad, nbands, starts, f_mask)


_MASK_MODES = {"continuous": ops.MASK_CONTIGUOUS, "random": ops.MASK_RANDOM}


def device_masks(padding_mask, nbands, f_mask=0.15, *, x=None, mask_type="continuous", seed=None, return_starts=False):
    """The masks of get_continous_random_mask (mask_type="continuous") or get_random_mask ("random", `nbands` unused) drawn ON
    THE DEVICE in one launch: same rules and distribution, the kernel's own counter-based draws (msn_pretrain_masks in
    include/msn_hip.h states them).  Returns (mask_in, mask_pred[, x_masked][, starts]): bool views of the kernel's byte masks,
    x_masked = where(mask_in, x, 0) when `x` (B, T) is given, and with return_starts the (B, nbands) int32 run starts
    (continuous only).  `seed`: an int; None takes ops.new_seed() -- torch's CPU generator when eager (reproducible under
    torch.manual_seed), the recording's device-resident base under a graph capture, so every replay draws new masks.
    Nothing comes to the host and no allocation depends on data: legal inside a recorded step."""
    if mask_type not in _MASK_MODES:
        raise ValueError(f'mask_type must be "continuous" or "random" (got {mask_type!r})')
    if return_starts and mask_type != "continuous":
        raise ValueError('return_starts needs mask_type="continuous": a random subset has no run starts')
    if x is not None:
        x = x.float().contiguous()
    mask_in, mask_pred, x_masked, starts = ops.pretrain_masks(
        ops._mask_u8(padding_mask), nbands, f_mask, _MASK_MODES[mask_type], ops.new_seed() if seed is None else seed, x=x,
        want_starts=return_starts)
    out = (mask_in.view(torch.bool), mask_pred.view(torch.bool))
    if x is not None:
        out += (x_masked,)
    if return_starts:
        out += (starts,)
    return out


class _MaskedMSE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, select_u8):
        pred, target = pred.contiguous(), target.contiguous().float()
        stats = torch.empty(2, dtype=torch.float32, device=pred.device)
        check(lib().msn_masked_mse_fwd(ptr(ops._f32c(pred, "pred")), ptr(target), ptr(select_u8), pred.numel(), ptr(stats),
                                       stream_ptr()), "msn_masked_mse_fwd")
        ctx.sel = select_u8
        ctx.save_for_backward(pred, target, stats)
        return stats[0]

    @staticmethod
    def backward(ctx, g):
        pred, target, stats = ctx.saved_tensors
        d = torch.empty_like(pred)
        g = g.to(torch.float32).reshape(()).contiguous()
        check(lib().msn_masked_mse_bwd(ptr(pred), ptr(target), ptr(ctx.sel), pred.numel(), ptr(stats), ptr(g), ptr(d),
                                       stream_ptr()), "msn_masked_mse_bwd")
        return d, None, None


def masked_mse(pred, target, select):
    """mean((pred - target)^2) over the elements where `select` is true == nn.MSELoss()(pred[select], target[select])."""
    return _MaskedMSE.apply(pred, target, ops._mask_u8(select))


class MaskedLightCurveEncoder(nn.Module):
    """ref src/models_pretraining.py:101-259 (Lightning hooks as plain methods)."""

    def __init__(self, f_mask: float = 0.2, nband: int = 1, transformer_kwargs: Dict = None, optimizer_kwargs: Dict = None,
                 lr_scheduler_kwargs: Dict = None, lr: float = 1e-3, optimizer: str = "radam",
                 mask_generator: str = "reference", mask_type: str = "continuous"):
        """mask_generator: "reference" = the host draws of get_continous_random_mask / get_random_mask (Python's `random` /
        torch.randperm: what a seeded reference run hides); "device" = device_masks, one launch, nothing on the host -- the
        form trainer.GraphedTrainStep records.  mask_type: "continuous" (the reference's _step) | "random"."""
        super().__init__()
        if mask_generator not in ("reference", "device"):
            raise ValueError(f'mask_generator must be "reference" or "device" (got {mask_generator!r})')
        if mask_type not in _MASK_MODES:
            raise ValueError(f'mask_type must be "continuous" or "random" (got {mask_type!r})')
        self.mask_generator, self.mask_type = mask_generator, mask_type
        self.last_mask_in = self.last_mask_pred = None      # the last step's masks (static tensors under a graph replay)
        transformer_kwargs = dict(transformer_kwargs or {"n_out": 1, "emb": 128, "heads": 2, "depth": 4})
        self.nband, self.lr, self.f_mask = nband, lr, f_mask
        self.optimizer_kwargs = dict(optimizer_kwargs or {})
        self.optimizer = optimizer            # optim.build_optimizer's name ("radam", "adam", "adamw", "sgd", "lars") or an Optimizer class (optim.LAMB)
        self.lr_scheduler_kwargs = dict(lr_scheduler_kwargs or {})
        self.net = TransformerWithTimeEmbeddings(nband=nband, agg="pretraining", **transformer_kwargs)
        self.last_layer = nn.Linear(transformer_kwargs["emb"], 1)
        self.logged = {}

    def log(self, name, value, **kwargs):
        # detached: a logged loss must not keep its autograd graph alive into the next step
        self.logged[name] = value.detach() if torch.is_tensor(value) else value

    def forward(self, x, t, mask=None):
        h = self.net(x[..., None], t, mask)                                    # (B, T, emb), padded tokens zeroed
        return F_.linear(h, self.last_layer.weight, self.last_layer.bias).squeeze(2)

    def configure_optimizers(self):
        """RAdam + StepLR stepped once per epoch (ref src/models_pretraining.py:167-189); trainer.Trainer steps the
        scheduler it finds under "lr_scheduler" after every training epoch, as Lightning does."""
        from .optim import build_optimizer
        optimizer = build_optimizer(self.optimizer, self.parameters(), lr=self.lr, **self.optimizer_kwargs)
        out = {"optimizer": optimizer}
        if self.lr_scheduler_kwargs:
            out["lr_scheduler"] = {"scheduler": torch.optim.lr_scheduler.StepLR(optimizer, **self.lr_scheduler_kwargs),
                                   "monitor": "val_loss", "interval": "epoch", "frequency": 1}
        return out

    def masked_loss(self, x, t, padding_mask, mask_in, mask_pred):
        """MSE on the hidden points given explicit masks (what masked_pred + nn.MSELoss compute, ref :183-231)."""
        x_masked = x.clone()
        x_masked[~mask_in] = 0
        return masked_mse(self(x_masked, t, mask=padding_mask), x, mask_pred)

    def _step(self, batch, name):
        if len(batch) == 3:
            t, x, padding_mask = batch
        else:
            _, x, t, padding_mask, *_ = batch
        pad = padding_mask.to(x.device)
        if self.mask_generator == "device":
            # one launch draws both masks and the zeroed input where the padding mask lives: nothing comes to the host
            mask_in, mask_pred, x_masked = device_masks(pad, self.nband, self.f_mask, x=x, mask_type=self.mask_type)
            loss = masked_mse(self(x_masked, t, mask=pad), x, mask_pred)
        else:
            if self.mask_type == "continuous":
                # masks are built on the padding mask's device; only the per-band counts of observed points (B x nband integers)
                # come to the host, for the bounds of the random run starts
                mask_in, mask_pred = get_continous_random_mask(pad, self.nband, f_mask=self.f_mask)
            else:
                # the padding mask itself comes to the host: one torch.randperm per sample ranks its observed points there
                mask_in, mask_pred = get_random_mask(pad, f_mask=self.f_mask)
            loss = self.masked_loss(x, t, padding_mask, mask_in, mask_pred)
        self.last_mask_in, self.last_mask_pred = mask_in, mask_pred
        self.log(name, loss, on_epoch=True, on_step=False, prog_bar=True)
        return loss

    # what a recorded step leaves for the caller to read: trainer.GraphedTrainStep keeps the recording's tensors and puts them back
    # after every replay, so the attributes name the LAST step's masks whatever ran in between (an eager batch, a validation step)
    graph_static_attrs = ("last_mask_in", "last_mask_pred")

    def check_graph_capturable(self):
        """trainer.GraphedTrainStep asks before it records: the host draws synchronise (illegal under capture) and would
        freeze one mask into the graph."""
        if self.mask_generator != "device":
            raise RuntimeError('MaskedLightCurveEncoder(mask_generator="reference") draws its masks on the host and cannot be '
                               'recorded as a graph: construct it with mask_generator="device"')

    def training_step(self, batch, batch_idx):
        return self._step(batch, "train_loss")

    def validation_step(self, batch, batch_idx):
        return self._step(batch, "val_loss")
