"""The reference's quantile-trimmed (outlier-robust) squared losses and the batched exact
quantile under them, on the HIP kernels of csrc/gs_robust_loss.hip (C ABI
include/gs_robust_loss.h): a radix select on the residuals' bit patterns, no sort, nothing read
back, a deterministic backward.

Drop-ins for

    helpers.masked_mse_loss(pred, gt, mask, normalize, quantile)      # helpers.py:16-38
    ideaII.trimmed_mse_loss(pred, gt, quantile=0.9)                   # ideaII.py:378-384

which take a per-element squared residual, torch.quantile of it, and average the residuals
below that threshold:

    loss = masked_trimmed_mse_loss(pred, gt, mask=mask, quantile=0.9)   # sum over the cameras
    loss = trimmed_mse_loss(flow_a, flow_b, quantile=0.9)
    thr  = plane_quantile(x, 0.9)                                        # float64 [B]

The threshold of a plane of n values e and a quantile q is, with r = q (n - 1) in fp64,
lo = floor(r), hi = min(lo + 1, n - 1), w = r - lo and v_lo, v_hi the exact order statistics,

    thr = (double)v_lo + w ((double)v_hi - (double)v_lo)

held and compared in fp64: element i is kept iff (double)e[i] < thr.  A NaN element makes thr
NaN and nothing is kept.  The threshold and the kept set carry no gradient.

Every function has a `_torch` twin in PyTorch operations for any device and dtype: the parity
oracle, the benchmark's baseline and the CPU path.  The HIP path has no CPU fallback: host
tensors raise.  The twins add the residual's terms in index order and divide once, which is
how the kernels round.
"""
from __future__ import annotations

import functools
import math
from typing import Optional

import torch

from . import _args, _lib
from ._lib import GsplatError

STATS = ("thr", "kept", "kept_masked", "nan")  # stats[b, 0:4], float64
CHANNELS, ROWS, VALUES = 0, 1, 2  # include/gs_robust_loss.h


_need = functools.partial(_args.need, op="robust losses need", twin="the _torch twins run")


def _check_q(q) -> float:
    q = float(q)
    if not (math.isfinite(q) and 0.0 <= q <= 1.0):
        raise GsplatError(f"quantile must be in [0, 1] (got {q})")
    return q


def _check_over(quantile_over: str):
    if quantile_over not in ("all", "masked"):
        raise ValueError(f"quantile_over must be 'all' or 'masked' (got {quantile_over!r})")


def _check_int32(B: int, N: int):
    if B * N > 2 ** 31 - 1:
        raise GsplatError(f"{B} planes of {N} elements do not fit int32")


def _struct(cfg, pred, gt, mask, losses, stats, ws):
    layout, B, R, N, q, select, over_masked, normalize, width, skip = cfg
    p = _args.ptr
    return _lib.GsRobustLoss(B=B, R=R, N=N, layout=layout, pred=p(pred), gt=p(gt), mask=p(mask),
                             mask_batch_stride=N if mask is not None and mask.dim() == 2 else 0, quantile=q,
                             select=int(select), over_masked=int(over_masked), normalize=int(normalize),
                             norm_width=width, skip_degenerate=int(skip), losses=p(losses), stats=p(stats),
                             workspace=p(ws), workspace_bytes=ws.numel() if ws is not None else 0)


def _forward(cfg, pred, gt, mask):
    L = _lib.load()
    layout, B, _, N = cfg[:4]
    dev = pred.device
    losses = torch.empty(B, dtype=torch.float32, device=dev)
    stats = torch.empty(B, 4, dtype=torch.float64, device=dev)
    ws = torch.empty(L.gs_robust_loss_workspace_bytes(B, N, layout), dtype=torch.uint8, device=dev)
    _lib.check(L.gs_robust_loss_forward(_struct(cfg, pred, gt, mask, losses, stats, ws), _lib.stream(dev)),
               "robust loss forward")
    return losses, stats


class _RobustLoss(torch.autograd.Function):
    """(losses [B], stats [B, 4]) of pred, gt in the layout cfg names; the gradient reaches pred only."""

    @staticmethod
    def forward(ctx, pred, gt, mask, cfg):
        pred, gt = pred.detach(), gt.detach()
        losses, stats = _forward(cfg, pred, gt, mask)
        ctx.save_for_backward(pred, gt, mask, stats)  # the statistics, not the residual plane
        ctx.cfg = cfg
        ctx.mark_non_differentiable(stats)
        return losses, stats

    @staticmethod
    def backward(ctx, g_losses, _g_stats):
        pred, gt, mask, stats = ctx.saved_tensors
        L = _lib.load()
        dev = pred.device
        up = g_losses.to(torch.float32).contiguous()  # [B], read on the device
        d_pred = torch.empty_like(pred)
        args = _struct(ctx.cfg, pred, gt, mask, None, stats, None)
        _lib.check(L.gs_robust_loss_backward(args, up.data_ptr(), d_pred.data_ptr(), _lib.stream(dev)),
                   "robust loss backward")
        return d_pred, None, None, None


def plane_quantile(x: torch.Tensor, q: float) -> torch.Tensor:
    """The float64 thresholds [B] of the planes x [B, N] (a scalar for one plane [N]) at the
    quantile q in [0, 1]: the module's definition of thr, with exact order statistics from a radix
    select.  Values must be >= 0 or NaN (a NaN, or a negative value, makes its plane's threshold
    NaN; the other planes are unaffected).  Contiguous float32 device tensors; N up to int32."""
    if not isinstance(x, torch.Tensor) or x.dim() not in (1, 2):
        raise GsplatError("x must be a [B, N] or [N] tensor")
    _need(x, "x")
    q = _check_q(q)
    x2 = x.detach().reshape(1, -1) if x.dim() == 1 else x.detach()
    B, N = x2.shape
    if min(B, N) < 1:
        raise GsplatError(f"x must not be empty (got {tuple(x.shape)})")
    _check_int32(B, N)
    _, stats = _forward((VALUES, B, 1, N, q, True, False, False, 0, False), x2, None, None)
    return stats[0, 0] if x.dim() == 1 else stats[:, 0]


def _mask_bytes(mask, B, H, W):
    mask = _args.mask_u8(mask, B, H, W)
    if mask is None:
        return None
    return mask.reshape(-1) if mask.dim() == 2 else mask.reshape(B, -1)


def _images(pred, what="pred"):
    """[B, C, H, W] or [C, H, W] -> ([B, C, H, W] view, single)."""
    if not isinstance(pred, torch.Tensor) or pred.dim() not in (3, 4):
        raise GsplatError(f"{what} must be a [B, C, H, W] or [C, H, W] tensor")
    return (pred[None], True) if pred.dim() == 3 else (pred, False)


def masked_trimmed_mse_loss(pred: torch.Tensor, gt: torch.Tensor, mask: Optional[torch.Tensor] = None,
                            quantile: float = 1.0, normalize: bool = False, quantile_over: str = "all",
                            reduction: str = "sum", return_stats: bool = False, skip_degenerate: bool = False):
    """The reference's masked_mse_loss for every camera of a batch [B, C, H, W] (or one [C, H, W]):
    e = mean_c (pred - gt)^2 per pixel, one threshold per camera at `quantile`, and over the kept
    pixels (e < thr; every pixel at quantile >= 1, the reference's special case)

        normalize=False   sum kept m e / (number of kept pixels)
        normalize=True    sum kept m e / (W sum kept m + 1e-8)           (helpers.py:30-36)

    mask [H, W] or [B, H, W] at gt's size, non-zero = the pixel takes part (uint8 passes through,
    any other dtype is converted with != 0).  quantile_over="masked" takes the quantile over the
    masked pixels only and keeps only those; "all" is the reference.  The sum over the cameras
    (reduction="sum") or the vector [B] ("none"; a scalar for one [C, H, W]).  Contiguous float32
    device tensors only.  Differentiable in pred only; deterministic forward and backward.

    A camera with no kept pixel gives NaN with normalize=False (0 with a zero gradient under
    skip_degenerate=True) and 0 with normalize=True; the other cameras are unaffected.
    return_stats=True also returns [B, 4] float64 = (thr, kept count, sum kept m, NaN count)."""
    _args.check_reduction(reduction)
    _check_over(quantile_over)
    p4, single = _images(pred)
    _need(pred, "pred")
    _need(gt, "gt", pred.shape)
    if gt.requires_grad:
        raise GsplatError("gt gets no gradient from the robust losses (gt.requires_grad is set)")
    q = _check_q(quantile)
    B, C, H, W = p4.shape
    if min(B, C, H, W) < 1:
        raise GsplatError(f"pred must not be empty (got {tuple(pred.shape)})")
    _check_int32(B, H * W)
    mask = _mask_bytes(mask, B, H, W)
    cfg = (CHANNELS, B, C, H * W, q, q < 1.0, quantile_over == "masked" and mask is not None, bool(normalize), W,
           bool(skip_degenerate))
    losses, stats = _RobustLoss.apply(p4.reshape(B, C, H * W), gt.reshape(B, C, H * W), mask, cfg)
    out = _args.reduce_losses(losses, reduction, single)
    return (out, stats) if return_stats else out


def trimmed_mse_loss(pred: torch.Tensor, gt: torch.Tensor, quantile: float = 0.9) -> torch.Tensor:
    """The reference's trimmed_mse_loss: e = the mean of (pred - gt)^2 over the last axis, one
    threshold at `quantile` over all prod(shape[:-1]) rows, the mean of the rows with e < thr.  No
    special case at quantile = 1: the largest row is dropped, as in the reference.  Contiguous
    float32 device tensors; differentiable in pred only."""
    if not isinstance(pred, torch.Tensor) or pred.dim() < 1:
        raise GsplatError("pred must be a tensor with at least one axis")
    _need(pred, "pred")
    _need(gt, "gt", pred.shape)
    if gt.requires_grad:
        raise GsplatError("gt gets no gradient from the robust losses (gt.requires_grad is set)")
    q = _check_q(quantile)
    R = pred.shape[-1]
    N = pred.numel() // R if R else 0
    if min(R, N) < 1:
        raise GsplatError(f"pred must not be empty (got {tuple(pred.shape)})")
    _check_int32(1, N)
    cfg = (ROWS, 1, R, N, q, True, False, False, 0, False)
    losses, _ = _RobustLoss.apply(pred.reshape(1, N, R), gt.reshape(1, N, R), None, cfg)
    return losses[0]


# ------------------------------------------------------------ the PyTorch twins

def _residual_torch(pred, gt, dim):
    """The mean of (pred - gt)^2 along `dim`: the terms added in index order, divided once (by a
    tensor: a division by a Python number becomes a multiplication by its reciprocal on a device,
    which rounds differently when the length is no power of two)."""
    sq = (pred - gt) ** 2
    s = sq.select(dim, 0)
    for c in range(1, sq.shape[dim]):
        s = s + sq.select(dim, c)
    return s / torch.full((), float(sq.shape[dim]), dtype=s.dtype, device=s.device)


def _threshold_torch(e: torch.Tensor, q: float) -> torch.Tensor:
    """thr (0-dim float64) of the 1-D values e: a sort in e's dtype, the lerp in fp64."""
    n = e.numel()
    nan = torch.full((), float("nan"), dtype=torch.float64, device=e.device)
    if n == 0:
        return nan
    v = torch.sort(e.detach()).values
    r = q * (n - 1)
    lo = math.floor(r)
    hi = min(lo + 1, n - 1)
    w = r - lo
    v_lo, v_hi = v[lo].double(), v[hi].double()
    return torch.where(torch.isnan(v[-1]), nan, v_lo + w * (v_hi - v_lo))  # a NaN sorts last


def plane_quantile_torch(x: torch.Tensor, q: float) -> torch.Tensor:
    """plane_quantile in PyTorch operations, any device and dtype."""
    q = _check_q(q)
    if x.dim() == 1:
        return _threshold_torch(x, q)
    return torch.stack([_threshold_torch(row, q) for row in x])


def masked_trimmed_mse_loss_torch(pred: torch.Tensor, gt: torch.Tensor, mask: Optional[torch.Tensor] = None,
                                  quantile: float = 1.0, normalize: bool = False, quantile_over: str = "all",
                                  reduction: str = "sum", return_stats: bool = False, skip_degenerate: bool = False):
    """masked_trimmed_mse_loss in PyTorch operations, any device and dtype, camera by camera in the
    reference's order: the residual, the threshold, boolean indexing of (e * mask) by the kept
    set, the mean or the normalised sum; autograd for the backward."""
    _args.check_reduction(reduction)
    _check_over(quantile_over)
    q = _check_q(quantile)
    p4, single = _images(pred)
    g4, _ = _images(gt, "gt")
    B, _, H, W = p4.shape
    losses, stats = [], []
    for b in range(B):
        e = _residual_torch(p4[b], g4[b], 0)  # [H, W]
        mb = torch.ones_like(e, dtype=torch.bool) if mask is None else (mask if mask.dim() == 2 else mask[b]) != 0
        part = mb if quantile_over == "masked" else torch.ones_like(mb)
        if q < 1.0:
            thr = _threshold_torch(e[part], q)
            kept = part & (e.detach().double() < thr)
        else:
            thr = torch.full((), float("inf"), dtype=torch.float64, device=e.device)
            kept = part
        sel = (e * mb.to(e.dtype))[kept]
        cnt, cm = kept.sum(), (kept & mb).sum()
        if normalize:
            loss = sel.sum() / (W * cm.to(e.dtype) + 1e-8)
        elif skip_degenerate and int(cnt) == 0:
            loss = sel.sum()
        else:
            loss = sel.mean()
        losses.append(loss)
        if return_stats:
            stats.append(torch.stack([thr, cnt.double(), cm.double(), (torch.isnan(e.detach()) & part).sum().double()]))
    losses = torch.stack(losses)
    out = _args.reduce_losses(losses, reduction, single)
    return (out, torch.stack(stats)) if return_stats else out


def trimmed_mse_loss_torch(pred: torch.Tensor, gt: torch.Tensor, quantile: float = 0.9) -> torch.Tensor:
    """trimmed_mse_loss in PyTorch operations, any device and dtype."""
    q = _check_q(quantile)
    e = _residual_torch(pred, gt, -1)
    thr = _threshold_torch(e.flatten(), q)
    return e[e.detach().double() < thr].mean()
