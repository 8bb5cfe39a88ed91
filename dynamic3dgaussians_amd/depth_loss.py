"""The reference's masked depth-correlation loss on the HIP kernels of
csrc/gs_depth_loss.hip (C ABI include/gs_depth_loss.h): two forward launches
and one backward launch for every camera of a batch, nothing read back.

Drop-in for the depth term of the reference's dynamic training step
(dyn_train.py:256-265), per camera

    depth_pred = clamp(depth_pred.reshape(-1, 1)[mask], near, far)
    depth_pred = 1 / depth_pred
    depth_pred, gt = standardise(depth_pred), standardise(gt.reshape(-1, 1)[mask])
    loss       = 1 - pearson_corrcoef(gt, depth_pred)

which becomes, for all cameras of a rank at once,

    loss = depth_correlation_loss(depth, prior, mask=mask)            # sum over the cameras

with `depth` the [B, 1, H, W] plane GaussianRasterizerBatch returns and `prior`
the monocular prior in inverse-depth units.  `depth_correlation_loss_torch`
states the same loss in PyTorch operations in the reference's order, for any
device and dtype: the parity oracle, the benchmark's baseline and the CPU path
of tests that have no GPU.  The HIP path has no CPU fallback: host tensors
raise.

The plain masked depth L1 of the reference's train.py:223-228 needs nothing of
this: photometric_loss(depth, gt, mask=..., ssim_weight=0) with one channel
computes it.
"""
from __future__ import annotations

import functools
import math
from typing import Optional

import torch

from . import _args, _lib
from ._lib import GsplatError

NEAR, FAR = 1e-7, 50.0  # dyn_train.py:20
STATS = ("n", "mean_p", "mean_g", "Sxx", "Syy", "Sxy", "r", "valid")  # stats[b, 0:8]


_need = functools.partial(_args.need, op="depth-correlation loss needs", twin="depth_correlation_loss_torch runs")


def _struct(depth, target, mask, near, far, skip, losses, stats, ws):
    B, H, W = depth.shape
    p = _args.ptr
    return _lib.GsDepthLoss(B=B, H=H, W=W, depth=p(depth), target=p(target), mask=p(mask),
                            mask_batch_stride=H * W if mask is not None and mask.dim() == 3 else 0,
                            near=near, far=far, skip_degenerate=int(skip), losses=p(losses), stats=p(stats),
                            workspace=p(ws), workspace_bytes=ws.numel() if ws is not None else 0)


class _DepthCorrelationLoss(torch.autograd.Function):
    """(losses [B], stats [B, 8]) of depth, target [B, H, W]; the gradient reaches depth only."""

    @staticmethod
    def forward(ctx, depth, target, mask, near, far, skip):
        L = _lib.load()
        dev = depth.device
        depth, target = depth.detach(), target.detach()
        B, H, W = depth.shape
        losses = torch.empty(B, dtype=torch.float32, device=dev)
        stats = torch.empty(B, 8, dtype=torch.float32, device=dev)
        ws = torch.empty(L.gs_depth_loss_workspace_bytes(B, H, W), dtype=torch.uint8, device=dev)
        args = _struct(depth, target, mask, near, far, skip, losses, stats, ws)
        _lib.check(L.gs_depth_loss_forward(args, _lib.stream(dev)), "depth loss forward")
        ctx.save_for_backward(depth, target, mask, stats)  # the backward needs no workspace
        ctx.consts = (near, far, skip)
        ctx.mark_non_differentiable(stats)
        return losses, stats

    @staticmethod
    def backward(ctx, g_losses, _g_stats):
        depth, target, mask, stats = ctx.saved_tensors
        L = _lib.load()
        dev = depth.device
        up = g_losses.to(torch.float32).contiguous()  # [B], read on the device
        d_depth = torch.empty_like(depth)
        args = _struct(depth, target, mask, *ctx.consts, None, stats, None)
        _lib.check(L.gs_depth_loss_backward(args, up.data_ptr(), d_depth.data_ptr(), _lib.stream(dev)),
                   "depth loss backward")
        return d_depth, None, None, None, None, None


def _planes(depth, what="depth"):
    """[B, 1, H, W], [B, H, W] or [H, W] -> ([B, H, W] view, single)."""
    if not isinstance(depth, torch.Tensor) or depth.dim() not in (2, 3, 4) or (depth.dim() == 4 and depth.shape[1] != 1):
        raise GsplatError(f"{what} must be a [B, 1, H, W], [B, H, W] or [H, W] tensor")
    single = depth.dim() == 2
    B = 1 if single else depth.shape[0]
    return depth.reshape(B, depth.shape[-2], depth.shape[-1]), single


def depth_correlation_loss(depth: torch.Tensor, target: torch.Tensor, mask: Optional[torch.Tensor] = None,
                           near: float = NEAR, far: float = FAR, reduction: str = "sum",
                           skip_degenerate: bool = False, return_stats: bool = False):
    """1 - clamp(pearson(1 / clamp(depth, near, far), target), -1, 1) over the masked pixels, per
    camera plane of a batch [B, 1, H, W] (what GaussianRasterizerBatch returns), [B, H, W] or one
    plane [H, W]: the sum over the batch (reduction="sum") or the vector [B] (reduction="none";
    a scalar for one [H, W] plane).  `target` is the prior in inverse-depth units, in depth's
    layout; mask [H, W] or [B, H, W], non-zero = the pixel takes part (uint8 passes through, any
    other dtype is converted with != 0).  Contiguous float32 device tensors only.
    Differentiable in depth only; deterministic forward and backward.

    A camera with fewer than two masked pixels, a constant side or a non-finite moment is
    degenerate: its loss is NaN as in the reference, or 0 with an all-zero gradient plane under
    skip_degenerate=True; the other cameras are unaffected.  return_stats=True also returns the
    per-camera statistics [B, 8] = (n, mean p, mean g, Sxx, Syy, Sxy, unclamped r, valid)."""
    _args.check_reduction(reduction)
    d3, single = _planes(depth)
    _need(depth, "depth")
    _need(target, "target", depth.shape)
    if target.requires_grad:
        raise GsplatError("target gets no gradient from the depth-correlation loss (target.requires_grad is set)")
    B, H, W = d3.shape
    if min(B, H, W) < 1:
        raise GsplatError(f"depth must not be empty (got {tuple(depth.shape)})")
    mask = _args.mask_u8(mask, B, H, W)
    near, far = float(near), float(far)
    if not (math.isfinite(near) and math.isfinite(far) and 0.0 < near < far):
        raise GsplatError(f"near and far must be finite with 0 < near < far (got {near}, {far})")
    losses, stats = _DepthCorrelationLoss.apply(d3, target.reshape(B, H, W), mask, near, far, bool(skip_degenerate))
    out = _args.reduce_losses(losses, reduction, single)
    return (out, stats) if return_stats else out


def _pearson(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """The Pearson correlation coefficient by its definition: covariance over the product of the
    standard deviations, clamped to [-1, 1]."""
    dx, dy = x - x.mean(), y - y.mean()
    r = (dx * dy).sum() / (torch.sqrt((dx * dx).sum()) * torch.sqrt((dy * dy).sum()))
    return torch.clamp(r, -1.0, 1.0)


def depth_correlation_loss_torch(depth: torch.Tensor, target: torch.Tensor, mask: Optional[torch.Tensor] = None,
                                 near: float = NEAR, far: float = FAR, reduction: str = "sum",
                                 skip_degenerate: bool = False, return_stats: bool = False):
    """depth_correlation_loss in PyTorch operations, any device and dtype, camera by camera in the
    reference's order: boolean indexing, clamp, reciprocal, standardisation of both sides with
    the unbiased std, Pearson; autograd for the backward.

    A degenerate camera (n < 2, a constant side, a non-finite moment) is where the reference
    computes 0/0; whether that comes out as NaN or as noise depends there on how the mean of a
    constant rounds, so it is pinned here: NaN, with a NaN gradient where one would flow, or 0
    with a zero gradient under skip_degenerate=True."""
    _args.check_reduction(reduction)
    d3, single = _planes(depth)
    g3, _ = _planes(target, "target")
    B, H, W = d3.shape
    losses, stats = [], []
    for b in range(B):
        pred, gt = d3[b].reshape(-1, 1), g3[b].reshape(-1, 1)
        if mask is not None:
            sel = (mask if mask.dim() == 2 else mask[b]).flatten() != 0
            pred, gt = pred[sel], gt[sel]
        pred = 1 / torch.clamp(pred, min=near, max=far)
        n = pred.shape[0]
        dp = pred.detach() - pred.detach().mean() if n else pred.detach()
        dg = gt.detach() - gt.detach().mean() if n else gt.detach()
        sxx, syy, sxy = (dp * dp).sum(), (dg * dg).sum(), (dp * dg).sum()
        valid = n >= 2 and bool(pred.detach().max() > pred.detach().min()) and bool(gt.max() > gt.min()) \
            and bool(torch.isfinite(sxx) & torch.isfinite(syy) & torch.isfinite(sxy))
        if valid:
            pred_s = (pred - pred.mean()) / pred.std()
            gt_s = (gt - gt.mean()) / gt.std()
            loss = 1 - _pearson(gt_s, pred_s)
        elif skip_degenerate:
            loss = torch.where(torch.zeros_like(pred, dtype=torch.bool), pred, torch.zeros_like(pred)).sum()
        else:
            loss = pred.sum() * float("nan")
        losses.append(loss)
        if return_stats:
            zero = sxx.new_zeros(())
            r = sxy / torch.sqrt(sxx * syy) if valid else zero + float("nan")
            stats.append(torch.stack([zero + n, pred.detach().mean() if n else zero + float("nan"),
                                      gt.detach().mean() if n else zero + float("nan"), sxx, syy, sxy, r,
                                      zero + float(valid)]))
    losses = torch.stack(losses)
    out = _args.reduce_losses(losses, reduction, single)
    return (out, torch.stack(stats)) if return_stats else out
