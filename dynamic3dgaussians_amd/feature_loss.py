"""The reference's feature-distillation loss: the rendered semantic channels
resampled to the size of a per-view 2-D feature prior (bilinear,
align_corners=True), then the photometric loss against the prior.  Two HIP
stages, resample.bilinear_resize and image_loss.photometric_loss; nothing in
PyTorch operations in between.

    feature_map = F.interpolate(feature_map.unsqueeze(0), size=(gt_h, gt_w), mode='bilinear',
                                align_corners=True).squeeze(0)
    Ll1_feature = l1_loss(feature_map, gt_feature_map)                   # revise_train.py:101-104

becomes, for every camera of a rank at once,

    loss = feature_distillation_loss(feature_maps, gt_feature_maps)       # sum over the cameras

and sanity_feature.py:487's 0.8 * L1 + 0.2 * (1 - SSIM) is the same call with
l1_weight=0.8, ssim_weight=0.2.  `distillation_image_loss` is the
`TimestepDriver(image_loss=...)` form for the (colour, features) render.
"""
from __future__ import annotations

from typing import Optional

import torch

from ._lib import GsplatError
from .feature_decoder import as_weight_bias, decode_features, decoded_l1_loss
from .image_loss import photometric_image_loss, photometric_loss
from .resample import bilinear_resize


def feature_distillation_loss(feat: torch.Tensor, target: torch.Tensor, mask: Optional[torch.Tensor] = None,
                              l1_weight: float = 1.0, ssim_weight: float = 0.0, align_corners: bool = True,
                              reduction: str = "sum") -> torch.Tensor:
    """photometric_loss(bilinear_resize(feat, target.shape[-2:], align_corners), target, ...): feat
    [B, F, H, W] (or one map [F, H, W]) against the prior target [B, F, h, w] ([F, h, w]); mask
    [h, w] or [B, h, w] at the prior's size.  The defaults are revise_train.py's plain L1 with
    weight 1.  Contiguous float32 device tensors only; differentiable in feat; deterministic."""
    if not isinstance(feat, torch.Tensor) or not isinstance(target, torch.Tensor):
        raise GsplatError("feat and target must be tensors")
    if feat.dim() not in (3, 4) or target.dim() != feat.dim() or feat.shape[:-2] != target.shape[:-2]:
        raise GsplatError(f"feat [B, F, H, W] and target [B, F, h, w] must agree in all but the last two "
                          f"dimensions (got {tuple(feat.shape)}, {tuple(target.shape)})")
    resized = bilinear_resize(feat, target.shape[-2:], align_corners=align_corners)
    return photometric_loss(resized, target, mask=mask, l1_weight=l1_weight, ssim_weight=ssim_weight,
                            reduction=reduction)


def decoded_distillation_loss(feat: torch.Tensor, target: torch.Tensor, decoder, mask: Optional[torch.Tensor] = None,
                              l1_weight: float = 1.0, ssim_weight: float = 0.0, align_corners: bool = True,
                              reduction: str = "sum") -> torch.Tensor:
    """feature_distillation_loss in the reference's "speedup" mode (revise_train.py:50-53, 102-103):
    feat [B, F, H, W] (or [F, H, W]) is resized to the prior's size and lifted to the C_out channels
    of target [B, C_out, h, w] by the 1x1 decoder, a FeatureDecoder or a (weight [C_out, F], bias)
    pair, before the loss.  With ssim_weight == 0 that is l1_weight * decoded_l1_loss (fused, no
    decoded map), else photometric_loss of decode_features.  Differentiable in feat and in the
    decoder's parameters; deterministic.  (feature_distillation_loss keeps its parameter list, so
    the decoder has a function of its own.)"""
    if not isinstance(feat, torch.Tensor) or not isinstance(target, torch.Tensor):
        raise GsplatError("feat and target must be tensors")
    weight, bias = as_weight_bias(decoder)
    if not isinstance(weight, torch.Tensor) or weight.dim() not in (2, 4):
        raise GsplatError("the decoder's weight must be [C_out, F] or [C_out, F, 1, 1]")
    C_out, F_in = weight.shape[:2]
    if (feat.dim() not in (3, 4) or target.dim() != feat.dim() or feat.shape[:-3] != target.shape[:-3]
            or feat.shape[-3] != F_in or target.shape[-3] != C_out):
        raise GsplatError(f"with a {F_in} -> {C_out} decoder feat must be [B, {F_in}, H, W] and target "
                          f"[B, {C_out}, h, w] (got {tuple(feat.shape)}, {tuple(target.shape)})")
    resized = bilinear_resize(feat, target.shape[-2:], align_corners=align_corners)
    if ssim_weight == 0:
        return l1_weight * decoded_l1_loss(resized, weight, bias, target, mask=mask, reduction=reduction)
    return photometric_loss(decode_features(resized, weight, bias), target, mask=mask, l1_weight=l1_weight,
                            ssim_weight=ssim_weight, reduction=reduction)


def distillation_image_loss(im, target, *, feature_weight: float = 1.0, l1_weight: float = 1.0,
                            ssim_weight: float = 0.0, align_corners: bool = True,
                            feature_mask: Optional[torch.Tensor] = None, decoder=None,
                            **photometric_kwargs) -> torch.Tensor:
    """The `TimestepDriver.image_loss` form for the (colour, features) render: im = (images
    [C, 3, H, W], feature maps [C, F, H, W]), target = (images [C, 3, H, W], prior features
    [C, F, h, w]).  The SUM over the rank's cameras of photometric_image_loss on the colour part
    (photometric_kwargs: cam_m, cam_c, cam_ids, mask) plus feature_weight times
    feature_distillation_loss on the features (l1_weight, ssim_weight, align_corners; feature_mask
    at the prior's size).  decoder=None: as before; with a decoder the feature term is
    decoded_distillation_loss and the prior has the decoder's C_out channels."""
    if not isinstance(im, (tuple, list)) or not isinstance(target, (tuple, list)) or len(im) != 2 or len(target) != 2:
        raise GsplatError("distillation_image_loss needs im = (images, feature maps) and "
                          "target = (images, prior features)")
    colour = photometric_image_loss(im[0], target[0], **photometric_kwargs)
    if decoder is None:
        feature = feature_distillation_loss(im[1], target[1], mask=feature_mask, l1_weight=l1_weight,
                                            ssim_weight=ssim_weight, align_corners=align_corners)
    else:
        feature = decoded_distillation_loss(im[1], target[1], decoder, mask=feature_mask, l1_weight=l1_weight,
                                            ssim_weight=ssim_weight, align_corners=align_corners)
    return colour + feature_weight * feature
