"""The reference's "speedup" feature decoder fused with its L1 distillation loss,
on the matrix-core kernels of csrc/gs_feature_decoder.hip (C ABI and
arithmetic: include/gs_feature_decoder.h).

The reference renders half the prior's channels and lifts them with a learned
1x1 convolution before the L1 against the prior:

    feature_map = cnn_decoder(feature_map)               # revise_train.py:50-53, 102-103, 126
    Ll1_feature = l1_loss(feature_map, gt_feature_map)   # utils/loss_utils.py:17-18

which becomes, for every camera of a rank at once and without ever creating the
decoded [B, C_out, h, w] map,

    dec  = FeatureDecoder(32, 64).cuda()
    loss = dec.loss(feature_maps, gt_feature_maps)        # sum over the cameras

`decode_features` is the plain decode (inference, or in front of another loss),
`decoded_l1_loss` the fused loss; both are differentiable in x, weight and bias
and deterministic.  The reference checkout does not contain models/networks.py
(CNN_decoder); the layer is taken to be the upstream one,
nn.Conv2d(in_dim, out_dim, kernel_size=1) with bias.

`decode_features_torch` and `decoded_l1_loss_torch` state the same arithmetic in
PyTorch operations for any device and dtype: the parity oracle, the benchmark's
baseline and the CPU path.  The HIP path has no CPU fallback: host tensors raise.

    y[b,c,p] = bias[c] + sum_f weight[c,f] x[b,f,p]
    loss[b]  = sum_{c,p} m[p] |y - target| / (C_out h w)
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _args, _lib
from ._lib import GsplatError

MAX_F_IN, MAX_C_OUT, MAX_WEIGHTS = _lib.FD_MAX_F_IN, _lib.FD_MAX_C_OUT, _lib.FD_MAX_WEIGHTS


def _weight2d(weight):
    if not isinstance(weight, torch.Tensor):
        raise GsplatError("weight must be a tensor")
    if weight.dim() == 4 and weight.shape[2:] == (1, 1):
        return weight.reshape(weight.shape[0], weight.shape[1])
    if weight.dim() != 2:
        raise GsplatError(f"weight must be [C_out, F_in] or [C_out, F_in, 1, 1] (got {tuple(weight.shape)})")
    return weight


def _shapes(x, weight, bias, target=None, mask=None):
    """The [B, F_in, h, w] view of x, the 2-D weight, and the checks both paths share."""
    if not isinstance(x, torch.Tensor) or x.dim() not in (3, 4):
        raise GsplatError("x must be a [B, F_in, h, w] or [F_in, h, w] tensor")
    w2 = _weight2d(weight)
    x4 = x.reshape(1, *x.shape) if x.dim() == 3 else x
    if min(x4.shape) < 1 or min(w2.shape) < 1:
        raise GsplatError(f"x and weight must not be empty (got {tuple(x.shape)}, {tuple(weight.shape)})")
    B, F_in, h, w = x4.shape
    C_out = w2.shape[0]
    if w2.shape[1] != F_in:
        raise GsplatError(f"weight [C_out, F_in] must match x's {F_in} channels (got {tuple(weight.shape)})")
    if bias is not None and (not isinstance(bias, torch.Tensor) or tuple(bias.shape) != (C_out,)):
        raise GsplatError(f"bias must be [C_out] = [{C_out}]")
    t4 = m = None
    if target is not None:
        if not isinstance(target, torch.Tensor) or target.dim() != x.dim():
            raise GsplatError("target must be a tensor with x's number of dimensions")
        t4 = target.reshape(1, *target.shape) if target.dim() == 3 else target
        if tuple(t4.shape) != (B, C_out, h, w):
            raise GsplatError(f"target must be [B, C_out, h, w] = {(B, C_out, h, w)} (got {tuple(target.shape)})")
        if target.requires_grad:
            raise GsplatError("target must not require a gradient: the loss is differentiable in x, weight and bias")
    if mask is not None:
        if not isinstance(mask, torch.Tensor) or tuple(mask.shape) not in ((h, w), (B, h, w)):
            raise GsplatError(f"mask must be [h, w] or [B, h, w] (got {tuple(getattr(mask, 'shape', ()))})")
        m = mask
    return x4, w2, t4, m


def _reduce(loss, reduction):
    _args.check_reduction(reduction, GsplatError)
    return loss.sum() if reduction == "sum" else loss


def decode_features_torch(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """decode_features in PyTorch operations (einsum), any device and dtype."""
    x4, w2, _, _ = _shapes(x, weight, bias)
    y = torch.einsum("cf,bfhw->bchw", w2, x4)
    if bias is not None:
        y = y + bias[None, :, None, None]
    return y.reshape(*x.shape[:-3], w2.shape[0], *x.shape[-2:])


def decoded_l1_loss_torch(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], target: torch.Tensor,
                          mask: Optional[torch.Tensor] = None, reduction: str = "sum") -> torch.Tensor:
    """decoded_l1_loss in PyTorch operations, any device and dtype: per camera the mean over all
    C_out * h * w elements of m * |decode(x) - target| (l1_loss of y * m against target * m for
    m >= 0)."""
    x4, w2, t4, m = _shapes(x, weight, bias, target, mask)
    y = decode_features_torch(x4, w2, bias)
    a = (y - t4).abs()
    if m is not None:
        a = a * (m[:, None] if m.dim() == 3 else m)
    return _reduce(a.mean(dim=(1, 2, 3)), reduction)


def _device_checks(**tensors):
    for name, t in tensors.items():
        if t is not None:
            _args.need(t, name, op="feature decoder needs", twin="decode_features_torch / decoded_l1_loss_torch run")


def _limits(F_in, C_out):
    if not (1 <= F_in <= MAX_F_IN and 1 <= C_out <= MAX_C_OUT and F_in * C_out <= MAX_WEIGHTS):
        raise GsplatError(f"the HIP feature decoder takes F_in <= {MAX_F_IN}, C_out <= {MAX_C_OUT} and "
                          f"F_in * C_out <= {MAX_WEIGHTS} (got {F_in} -> {C_out}); decode_features_torch / "
                          "decoded_l1_loss_torch take any size")


def _struct(x4, C_out, ws, **ptrs):
    B, F_in, h, w = x4.shape
    p = {k: _args.ptr(v) for k, v in ptrs.items()}
    return _lib.GsFeatureDecoder(B=B, F_in=F_in, C_out=C_out, h=h, w=w, x=x4.data_ptr(), workspace=ws.data_ptr(),
                                 workspace_bytes=ws.numel(), **p)


def _workspace(L, x4, C_out, which):
    B, F_in, h, w = x4.shape
    n = L.gs_feature_decoder_workspace_bytes(B, F_in, C_out, h, w, which)
    return torch.empty(max(n, 16), dtype=torch.uint8, device=x4.device)


class _Decode(torch.autograd.Function):
    """y [B, C_out, h, w] of x [B, F_in, h, w]."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        L = _lib.load()
        x, weight = x.detach(), weight.detach()
        bias = bias.detach() if bias is not None else None
        C_out = weight.shape[0]
        y = torch.empty(x.shape[0], C_out, *x.shape[2:], dtype=torch.float32, device=x.device)
        ws = _workspace(L, x, C_out, _lib.FD_PASS_DECODE)
        _lib.check(L.gs_feature_decoder_forward(_struct(x, C_out, ws, weight=weight, bias=bias, y=y),
                                                _lib.stream(x.device)), "feature decoder forward")
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    def backward(ctx, d_y):
        L = _lib.load()
        x, weight = ctx.saved_tensors
        C_out = weight.shape[0]
        d_y = d_y.to(torch.float32).contiguous()
        d_x = torch.empty_like(x)
        d_w = torch.empty_like(weight)
        d_b = torch.empty(C_out, dtype=torch.float32, device=x.device) if ctx.has_bias else None
        ws = _workspace(L, x, C_out, _lib.FD_PASS_BACKWARD)
        _lib.check(L.gs_feature_decoder_backward(_struct(x, C_out, ws, weight=weight, d_y=d_y, d_x=d_x, d_weight=d_w,
                                                         d_bias=d_b), _lib.stream(x.device)),
                   "feature decoder backward")
        return d_x, d_w, d_b


class _DecodedL1(torch.autograd.Function):
    """loss [B] of x [B, F_in, h, w] against target [B, C_out, h, w]."""

    @staticmethod
    def forward(ctx, x, weight, bias, target, mask):
        L = _lib.load()
        x, weight = x.detach(), weight.detach()
        bias = bias.detach() if bias is not None else None
        C_out = weight.shape[0]
        loss = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
        ws = _workspace(L, x, C_out, _lib.FD_PASS_LOSS)
        per_cam = int(mask is not None and mask.dim() == 3)
        _lib.check(L.gs_feature_decoder_loss_forward(
            _loss_struct(x, C_out, ws, weight, bias, target, mask, per_cam, loss=loss), _lib.stream(x.device)),
            "feature decoder loss forward")
        ctx.save_for_backward(x, weight, bias, target, mask)
        return loss

    @staticmethod
    def backward(ctx, up):
        L = _lib.load()
        x, weight, bias, target, mask = ctx.saved_tensors
        C_out = weight.shape[0]
        up = up.to(torch.float32).contiguous()
        d_x = torch.empty_like(x)
        d_w = torch.empty_like(weight)
        d_b = torch.empty(C_out, dtype=torch.float32, device=x.device) if bias is not None else None
        ws = _workspace(L, x, C_out, _lib.FD_PASS_LOSS_BACKWARD)
        per_cam = int(mask is not None and mask.dim() == 3)
        _lib.check(L.gs_feature_decoder_loss_backward(
            _loss_struct(x, C_out, ws, weight, bias, target, mask, per_cam, up=up, d_x=d_x, d_weight=d_w, d_bias=d_b),
            _lib.stream(x.device)), "feature decoder loss backward")
        return d_x, d_w, d_b, None, None


def _loss_struct(x, C_out, ws, weight, bias, target, mask, per_cam, **out):
    s = _struct(x, C_out, ws, weight=weight, bias=bias, target=target, mask=mask, **out)
    s.mask_per_camera = per_cam
    return s


def decode_features(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The 1x1 decoder y = weight x + bias per pixel: x [B, F_in, h, w] (or one map [F_in, h, w]),
    weight [C_out, F_in] or the conv's [C_out, F_in, 1, 1], bias [C_out] or None -> [B, C_out, h, w]
    ([C_out, h, w]).  Contiguous float32 device tensors only; differentiable in x, weight and
    bias; forward and backward are deterministic."""
    x4, w2, _, _ = _shapes(x, weight, bias)
    _device_checks(x=x, weight=weight, bias=bias)
    _limits(x4.shape[1], w2.shape[0])
    y = _Decode.apply(x4, w2, bias)
    return y.reshape(*x.shape[:-3], w2.shape[0], *x.shape[-2:])


def decoded_l1_loss(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], target: torch.Tensor,
                    mask: Optional[torch.Tensor] = None, reduction: str = "sum") -> torch.Tensor:
    """l1_loss(decode_features(x, weight, bias) * mask, target * mask) per camera, without the
    decoded map: target [B, C_out, h, w] ([C_out, h, w]), mask [h, w] or [B, h, w] float weights
    >= 0.  reduction="sum": the sum over the cameras (the TimestepDriver.image_loss convention);
    "none": [B].  Contiguous float32 device tensors only; differentiable in x, weight and bias;
    deterministic."""
    _args.check_reduction(reduction, GsplatError)
    x4, w2, t4, m = _shapes(x, weight, bias, target, mask)
    _device_checks(x=x, weight=weight, bias=bias, target=target, mask=mask)
    _limits(x4.shape[1], w2.shape[0])
    return _reduce(_DecodedL1.apply(x4, w2, bias, t4, m), reduction)


def as_weight_bias(decoder):
    """(weight, bias) of a FeatureDecoder or of a (weight, bias) pair."""
    if isinstance(decoder, FeatureDecoder):
        return decoder.conv.weight, decoder.conv.bias
    if isinstance(decoder, (tuple, list)) and len(decoder) == 2:
        return decoder[0], decoder[1]
    raise GsplatError("decoder must be a FeatureDecoder or a (weight, bias) pair")


class FeatureDecoder(torch.nn.Module):
    """The reference's CNN_decoder(in_dim, out_dim) as the upstream layer: one
    nn.Conv2d(in_dim, out_dim, kernel_size=1) with bias, torch's initialisation, state_dict keys
    conv.weight / conv.bias.  forward is decode_features, .loss the fused decoded_l1_loss."""

    def __init__(self, in_dim: int, out_dim: int):
        super().__init__()
        self.conv = torch.nn.Conv2d(in_dim, out_dim, kernel_size=1)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return decode_features(x, self.conv.weight, self.conv.bias)

    def loss(self, x: torch.Tensor, target: torch.Tensor, mask: Optional[torch.Tensor] = None,
             reduction: str = "sum") -> torch.Tensor:
        return decoded_l1_loss(x, self.conv.weight, self.conv.bias, target, mask=mask, reduction=reduction)
