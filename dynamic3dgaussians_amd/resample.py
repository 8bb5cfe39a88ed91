"""Bilinear resample between a render and a prior of another size, on the HIP
kernels of csrc/gs_resample.hip (C ABI include/gs_resample.h): one forward
launch, and one table launch plus one gather launch for the backward.  No
atomics: the backward is deterministic, unlike F.interpolate's on a device.

Drop-in for the reference's

    feature_map = F.interpolate(feature_map.unsqueeze(0), size=(gt_h, gt_w), mode='bilinear',
                                align_corners=True).squeeze(0)            # revise_train.py:101
    depth_pred  = F.interpolate(depth_pred.unsqueeze(0), size=(288, 512), mode='bilinear',
                                align_corners=False)                      # dyn_double.py:303

which become, for every camera and channel of a rank at once,

    feature_map = bilinear_resize(feature_map, (gt_h, gt_w), align_corners=True)
    depth_pred  = bilinear_resize(depth_pred, (288, 512))

The depth term at the prior's size is the composition

    depth_correlation_loss(bilinear_resize(depth, (h, w), align_corners=False), prior_hw, mask=mask_hw)

with `depth` the [B, 1, H, W] plane of GaussianRasterizerBatch; it fits
TimestepDriver's depth_loss(depth, cams) closure as it is.

`bilinear_resize_torch` states the same arithmetic in PyTorch operations for
any device and dtype: the parity oracle, the benchmark's baseline and the CPU
path of tests that have no GPU.  The HIP path has no CPU fallback: host
tensors raise.

The axis rule (include/gs_resample.h), per axis with input size I, output size
O and output index o, in fp32:

    align_corners:      scale = (I - 1) / (O - 1) if O > 1 else 0;  src = scale * o
    half-pixel centres: scale = I / O;  src = max(0, fmaf(scale, o + 0.5, -0.5))
    i0 = min(int(src), I - 1);  i1 = min(i0 + 1, I - 1);  l1 = src - i0;  l0 = 1 - l1
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from . import _args, _lib
from ._lib import GsplatError

MAX_SIZE = 32768  # per axis, include/gs_resample.h


@functools.lru_cache(maxsize=64)
def axis_tables(I: int, O: int, align_corners: bool, dtype: str = "float32"):  # noqa: E741
    """(i0 [O] int64, i1 [O] int64, l0 [O], l1 [O], first [I + 1] int64) of one axis by the rule
    above, as numpy arrays (shared: do not modify).  The fused multiply-add is reproduced as a
    float64 product and sum rounded once to fp32: the product of an fp32 scale and o + 0.5 is
    exact in float64, and where the sum is not (a product below 0.5) the result clamps to 0
    anyway.  first[i] is the smallest o with i0[o] >= i (O where there is none).
    dtype="float64" evaluates the same rule in float64 throughout (what F.interpolate does for
    float64 tensors): for comparisons with float64 references, never what the kernels compute."""
    if not (1 <= I <= MAX_SIZE and 1 <= O <= MAX_SIZE):
        raise GsplatError(f"sizes must be in [1, {MAX_SIZE}] (got {I} -> {O})")
    ft = {"float32": np.float32, "float64": np.float64}[dtype]
    o = np.arange(O, dtype=np.float64)
    if align_corners:
        scale = ft(I - 1) / ft(O - 1) if O > 1 else ft(0.0)
        src = (np.float64(scale) * o).astype(ft)
    else:
        scale = ft(I) / ft(O)
        src = np.maximum(ft(0.0), (np.float64(scale) * (o + 0.5) - 0.5).astype(ft))
    i0 = np.minimum(src.astype(np.int64), I - 1)
    i1 = np.minimum(i0 + 1, I - 1)
    l1 = src - i0.astype(ft)
    l0 = ft(1.0) - l1
    first = np.searchsorted(i0, np.arange(I + 1), side="left").astype(np.int64)
    assert l1.dtype == ft and l0.dtype == ft
    for a in (i0, i1, l0, l1, first):
        a.setflags(write=False)
    return i0, i1, l0, l1, first


def _size(size):
    try:
        h, w = (int(s) for s in size)
    except (TypeError, ValueError):
        raise GsplatError(f"size must be (h, w) (got {size!r})") from None
    if not (1 <= h <= MAX_SIZE and 1 <= w <= MAX_SIZE):
        raise GsplatError(f"size must be in [1, {MAX_SIZE}] per axis (got {(h, w)})")
    return h, w


def _planes(x):
    """[B, Ch, H, W], [Ch, H, W] or [H, W] -> the [B, Ch, H, W] view."""
    if not isinstance(x, torch.Tensor) or x.dim() not in (2, 3, 4):
        raise GsplatError("x must be a [B, Ch, H, W], [Ch, H, W] or [H, W] tensor")
    if min(x.shape) < 1:
        raise GsplatError(f"x must not be empty (got {tuple(x.shape)})")
    if not (x.shape[-2] <= MAX_SIZE and x.shape[-1] <= MAX_SIZE):
        raise GsplatError(f"H and W must be in [1, {MAX_SIZE}] (got {tuple(x.shape[-2:])})")
    lead = (1,) * (4 - x.dim()) + tuple(x.shape[:-2])
    return x.reshape(*lead, x.shape[-2], x.shape[-1])


def _struct(B, Ch, H, W, h, w, align, x=None, y=None, ws=None):
    p = _args.ptr
    return _lib.GsResample(B=B, Ch=Ch, H=H, W=W, h=h, w=w, align_corners=int(align), x=p(x), y=p(y),
                           workspace=p(ws), workspace_bytes=ws.numel() if ws is not None else 0)


class _BilinearResize(torch.autograd.Function):
    """y [B, Ch, h, w] of x [B, Ch, H, W]."""

    @staticmethod
    def forward(ctx, x, h, w, align):
        L = _lib.load()
        x = x.detach()
        B, Ch, H, W = x.shape
        y = torch.empty(B, Ch, h, w, dtype=torch.float32, device=x.device)
        _lib.check(L.gs_resample_forward(_struct(B, Ch, H, W, h, w, align, x=x, y=y), _lib.stream(x.device)),
                   "resample forward")
        ctx.geometry = (B, Ch, H, W, h, w, align)  # the backward needs neither x nor y
        return y

    @staticmethod
    def backward(ctx, d_y):
        L = _lib.load()
        B, Ch, H, W, h, w, align = ctx.geometry
        dev = d_y.device
        d_y = d_y.to(torch.float32).contiguous()
        d_x = torch.empty(B, Ch, H, W, dtype=torch.float32, device=dev)
        ws = torch.empty(L.gs_resample_workspace_bytes(H, W), dtype=torch.uint8, device=dev)
        _lib.check(L.gs_resample_backward(_struct(B, Ch, H, W, h, w, align, ws=ws), d_y.data_ptr(), d_x.data_ptr(),
                                          _lib.stream(dev)), "resample backward")
        return d_x, None, None, None


def bilinear_resize(x: torch.Tensor, size, align_corners: bool = False) -> torch.Tensor:
    """x [B, Ch, H, W], [Ch, H, W] or [H, W] resampled bilinearly to size = (h, w), every plane on
    its own, in x's layout: F.interpolate(x, size=size, mode='bilinear', align_corners=...) by the
    axis rule of this module.  Contiguous float32 device tensors only.  Differentiable in x;
    forward and backward are deterministic.  Equal sizes give a bit-exact copy."""
    h, w = _size(size)
    x4 = _planes(x)
    _args.need(x, "x", op="resample needs", twin="bilinear_resize_torch runs")
    y = _BilinearResize.apply(x4, h, w, bool(align_corners))
    return y.reshape(*x.shape[:-2], h, w)


def bilinear_resize_torch(x: torch.Tensor, size, align_corners: bool = False,
                          axis_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """bilinear_resize in PyTorch operations, any device and dtype: the axis tables of the rule
    (axis_tables), the four taps gathered by indexing, the blend
    l0y * (l0x * a + l1x * b) + l1y * (l0x * c + l1x * d) in x's dtype with the fp32 weights
    converted to it, and autograd for the backward.  axis_dtype=torch.float64 evaluates the axis
    rule in float64 instead (F.interpolate's weights for float64 tensors), for comparisons with
    a float64 reference; the kernels' weights are the fp32 ones."""
    h, w = _size(size)
    x4 = _planes(x)
    H, W = x4.shape[-2:]
    t = lambda a, dt: torch.from_numpy(a.copy()).to(device=x.device, dtype=dt)  # noqa: E731
    if axis_dtype not in (torch.float32, torch.float64):
        raise GsplatError(f"axis_dtype must be torch.float32 or torch.float64 (got {axis_dtype})")
    ft = "float32" if axis_dtype == torch.float32 else "float64"
    y0, y1, l0y, l1y, _ = axis_tables(H, h, bool(align_corners), ft)
    x0, x1, l0x, l1x, _ = axis_tables(W, w, bool(align_corners), ft)
    y0, y1, x0, x1 = (t(a, torch.long) for a in (y0, y1, x0, x1))
    l0y, l1y = (t(a, x.dtype)[:, None] for a in (l0y, l1y))
    l0x, l1x = (t(a, x.dtype) for a in (l0x, l1x))
    top, bot = x4[:, :, y0], x4[:, :, y1]
    y = l0y * (l0x * top[..., x0] + l1x * top[..., x1]) + l1y * (l0x * bot[..., x0] + l1x * bot[..., x1])
    return y.reshape(*x.shape[:-2], h, w)
