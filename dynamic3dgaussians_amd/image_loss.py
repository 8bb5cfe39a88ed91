"""The reference's photometric loss (L1 + SSIM) on the HIP kernels of
csrc/gs_loss.hip (C ABI include/gs_loss.h): one forward and one backward
launch for every camera and channel of a batch.

Drop-in for the per-camera image loss of the reference's training step
(train.py:161-183; l1_loss_v1 helpers.py:110-111; calc_ssim
external.py:90-133):

    im   = exp(cam_m[id])[:, None, None] * im + cam_c[id][:, None, None]
    loss = 0.8 * l1_loss_v1(im * mask, gt * mask) + 0.2 * (1 - calc_ssim(im * mask, gt * mask))

becomes, for all cameras of a rank at once,

    loss = photometric_image_loss(im, gt, cam_m=params['cam_m'], cam_c=params['cam_c'],
                                  cam_ids=ids, mask=mask)            # sum over the cameras

which is the `TimestepDriver(image_loss=...)` form.  `photometric_loss` is the
autograd function underneath (gain / offset per image and channel);
`photometric_loss_torch` states the same loss in PyTorch operations for any
device and dtype: the parity oracle, the benchmark's baseline and the CPU
path of tests that have no GPU.  The HIP path has no CPU fallback: host
tensors raise.
"""
from __future__ import annotations

import functools
import math
from typing import Optional

import torch

from . import _args, _lib
from ._lib import GsplatError

WINDOW, SIGMA = 11, 1.5
C1, C2 = 0.01 ** 2, 0.03 ** 2


_need = functools.partial(_args.need, op="photometric loss needs", twin="photometric_loss_torch runs")


def _struct(image, target, mask, gain, offset, l1_weight, ssim_weight, losses, ws):
    B, Ch, H, W = image.shape
    p = _args.ptr
    return _lib.GsPhotoLoss(B=B, Ch=Ch, H=H, W=W, image=p(image), target=p(target), mask=p(mask), gain=p(gain),
                            offset=p(offset),
                            mask_batch_stride=H * W if mask is not None and mask.dim() == 3 else 0,
                            l1_weight=l1_weight, ssim_weight=ssim_weight, losses=p(losses), workspace=p(ws),
                            workspace_bytes=ws.numel())


class _PhotometricLoss(torch.autograd.Function):
    """losses [B] of image, target [B, Ch, H, W]; gradients to image, gain, offset."""

    @staticmethod
    def forward(ctx, image, target, mask, gain, offset, l1_weight, ssim_weight):
        L = _lib.load()
        dev = image.device
        image, target = image.detach(), target.detach()
        mask = mask.detach() if mask is not None else None
        gain = gain.detach() if gain is not None else None
        offset = offset.detach() if offset is not None else None
        B, Ch, H, W = image.shape
        losses = torch.empty(B, dtype=torch.float32, device=dev)
        # the derivative maps the backward convolves live here (torch's caching allocator)
        ws = torch.empty(L.gs_photo_loss_workspace_bytes(B, Ch, H, W), dtype=torch.uint8, device=dev)
        args = _struct(image, target, mask, gain, offset, l1_weight, ssim_weight, losses, ws)
        _lib.check(L.gs_photo_loss_forward(args, _lib.stream(dev)), "photometric loss forward")
        ctx.save_for_backward(image, target, mask, gain, offset, ws)
        ctx.weights = (l1_weight, ssim_weight)
        return losses

    @staticmethod
    def backward(ctx, g_losses):
        image, target, mask, gain, offset, ws = ctx.saved_tensors
        L = _lib.load()
        dev = image.device
        up = g_losses.to(torch.float32).contiguous()  # [B], read on the device
        d_image = torch.empty_like(image)
        need_corr = gain is not None and (ctx.needs_input_grad[3] or ctx.needs_input_grad[4])
        d_gain = torch.empty_like(gain) if need_corr else None
        d_offset = torch.empty_like(offset) if need_corr else None
        args = _struct(image, target, mask, gain, offset, *ctx.weights, up, ws)  # losses: unused by the backward
        _lib.check(L.gs_photo_loss_backward(args, up.data_ptr(), d_image.data_ptr(),
                                            d_gain.data_ptr() if need_corr else None,
                                            d_offset.data_ptr() if need_corr else None, _lib.stream(dev)),
                   "photometric loss backward")
        return d_image, None, None, d_gain, d_offset, None, None


def photometric_loss(image: torch.Tensor, target: torch.Tensor, mask: Optional[torch.Tensor] = None,
                     gain: Optional[torch.Tensor] = None, offset: Optional[torch.Tensor] = None,
                     l1_weight: float = 0.8, ssim_weight: float = 0.2, reduction: str = "sum") -> torch.Tensor:
    """l1_weight * L1 + ssim_weight * (1 - SSIM) of x = (gain * image + offset) * mask against
    y = target * mask, per image of a batch [B, Ch, H, W] (or one image [Ch, H, W]): the sum over
    the batch (reduction="sum", the TimestepDriver.image_loss contract) or the vector [B]
    (reduction="none").  gain / offset [B, Ch] ([Ch] for one image) and mask [H, W] or [B, H, W]
    are optional.  Contiguous float32 device tensors only (a mask of another dtype is converted).
    Differentiable in image, gain and offset; deterministic forward and backward."""
    _args.check_reduction(reduction)
    if not isinstance(image, torch.Tensor) or image.dim() not in (3, 4):
        raise GsplatError("image must be a [B, Ch, H, W] or [Ch, H, W] tensor")
    single = image.dim() == 3
    _need(image, "image")
    _need(target, "target", image.shape)
    if target.requires_grad:
        raise GsplatError("target gets no gradient from the photometric loss (target.requires_grad is set)")
    if single:
        image, target = image[None], target[None]
    B, Ch, H, W = image.shape
    if min(B, Ch, H, W) < 1:
        raise GsplatError(f"image must not be empty (got {tuple(image.shape)})")
    mask = _args.mask_f32(mask, B, H, W)
    if (gain is None) != (offset is None):  # the kernel takes both or neither
        other = offset if gain is None else gain
        if gain is None:
            gain = torch.ones_like(other)
        else:
            offset = torch.zeros_like(other)
    if gain is not None:
        shape = (Ch,) if single else (B, Ch)
        _need(gain, "gain", shape)
        _need(offset, "offset", shape)
        gain, offset = gain.reshape(B, Ch), offset.reshape(B, Ch)
    if not math.isfinite(l1_weight) or not math.isfinite(ssim_weight):
        raise GsplatError("l1_weight and ssim_weight must be finite")
    losses = _PhotometricLoss.apply(image, target, mask, gain, offset, float(l1_weight), float(ssim_weight))
    return _args.reduce_losses(losses, reduction, single)


def photometric_image_loss(im, target, *, cam_m: Optional[torch.Tensor] = None,
                           cam_c: Optional[torch.Tensor] = None, cam_ids=None,
                           mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The `TimestepDriver.image_loss` form: the SUM over the rank's cameras of the reference's
    0.8 L1 + 0.2 (1 - SSIM) (train.py:183).  cam_m / cam_c [n_cams, 3] are the reference's
    per-camera colour correction (train.py:161): gain = exp(cam_m[cam_ids]) and offset =
    cam_c[cam_ids] stay torch operations, so autograd reaches the two parameters.  With feature
    channels, im and target are (images, feature maps) pairs as for l1_image_loss; the two terms
    are added and the correction applies to the images only."""
    if isinstance(im, (tuple, list)):
        if not isinstance(target, (tuple, list)) or len(target) != len(im):
            raise GsplatError("a tuple of renders needs a tuple of targets of the same length")
        total = photometric_image_loss(im[0], target[0], cam_m=cam_m, cam_c=cam_c, cam_ids=cam_ids, mask=mask)
        for a, b in zip(im[1:], target[1:]):
            total = total + photometric_loss(a, b, mask=mask)
        return total
    gain = offset = None
    if cam_m is not None or cam_c is not None:
        if cam_m is None or cam_c is None:
            raise GsplatError("cam_m and cam_c come together")
        if cam_ids is None:
            cam_ids = torch.arange(im.shape[0], device=im.device)
        elif not isinstance(cam_ids, torch.Tensor):
            cam_ids = torch.as_tensor(list(cam_ids), dtype=torch.long, device=im.device)
        gain = torch.exp(cam_m[cam_ids]).contiguous()
        offset = cam_c[cam_ids].contiguous()
    return photometric_loss(im, target, mask=mask, gain=gain, offset=offset)


def _window_2d(like: torch.Tensor) -> torch.Tensor:
    """The 11 x 11 window as the reference builds it: fp32 taps, normalised and multiplied out
    in fp32, then converted to the image's dtype."""
    taps = torch.tensor([math.exp(-(i - WINDOW // 2) ** 2 / float(2 * SIGMA ** 2)) for i in range(WINDOW)],
                        dtype=torch.float32)
    taps = (taps / taps.sum()).unsqueeze(1)
    return taps.mm(taps.t()).to(device=like.device, dtype=like.dtype)


def photometric_loss_torch(image: torch.Tensor, target: torch.Tensor, mask: Optional[torch.Tensor] = None,
                           gain: Optional[torch.Tensor] = None, offset: Optional[torch.Tensor] = None,
                           l1_weight: float = 0.8, ssim_weight: float = 0.2, reduction: str = "sum") -> torch.Tensor:
    """photometric_loss in PyTorch operations, any device and dtype: five zero-padded depthwise
    convolutions per call and autograd for the backward, as the reference computes it."""
    _args.check_reduction(reduction)
    single = image.dim() == 3
    if single:
        image, target = image[None], target[None]
        gain = gain[None] if gain is not None else None
        offset = offset[None] if offset is not None else None
    Ch = image.shape[1]
    x = image
    if gain is not None:
        x = gain[:, :, None, None] * x
    if offset is not None:
        x = x + offset[:, :, None, None]
    y = target
    if mask is not None:
        m = mask.to(x.dtype)
        m = m[None, None] if m.dim() == 2 else m[:, None]
        x, y = x * m, y * m
    l1 = torch.abs(x - y).mean(dim=(1, 2, 3))

    win = _window_2d(x).expand(Ch, 1, WINDOW, WINDOW).contiguous()
    blur = lambda t: torch.nn.functional.conv2d(t, win, padding=WINDOW // 2, groups=Ch)  # noqa: E731
    mu1, mu2 = blur(x), blur(y)
    mu1_sq, mu2_sq, mu12 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s1 = blur(x * x) - mu1_sq
    s2 = blur(y * y) - mu2_sq
    s12 = blur(x * y) - mu12
    ssim_map = ((2 * mu12 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2))
    losses = l1_weight * l1 + ssim_weight * (1 - ssim_map.mean(dim=(1, 2, 3)))
    return _args.reduce_losses(losses, reduction, single)
