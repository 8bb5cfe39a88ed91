"""The reference's quality reports on the HIP kernels of csrc/gs_metrics.hip
(C ABI include/gs_metrics.h): masked PSNR, masked SSIM and mask IoU for every
camera of a batch in one launch each, forward only.

What the reference computes in PyTorch and where:

    calc_psnr(im, gt)                     external.py:85-87   -> psnr_plain(image_metrics(im, gt))
    compute_psnr(pred, gt, mask)          metrics.py:14-43    -> psnr_clamped(image_metrics(pred, gt, mask))
    mPSNR().update(...) / .compute()      metrics.py:82-129   -> MaskedPSNR
    mSSIM().update(...) / .compute()      metrics.py:334-424  -> MaskedSSIM (image_metrics(...).ssim)
    compute_pose_errors(preds, targets)   metrics.py:46-79    -> pose_errors (host numpy fp64, like the reference)
    mask_iou(a, b)                        metrics.py:222-250  -> iou(a, b)  (threshold 0.9)
    mIOU().update(...) / .compute()       metrics.py:295-331  -> MeanIoU
    MaskIoU().update(...) / .compute()    metrics.py:523-552  -> MaskIoU    (threshold 0)

Images are channels-first here ([B, Ch, H, W]; the reference's metrics.py takes
[B, H, W, Ch]).  `image_metrics` returns the four per-image sums the kernel
writes; the PSNRs and the L1 are derived from them on the device, without a
readback.  The accumulators keep device tensors in `update` and read back in
`compute` only.  `evaluate_cameras` scores one forward-only batch render;
`evaluate_sequence` loops it over timesteps and reads back once.

`image_metrics_torch` and `mask_iou_torch` state the same quantities in PyTorch
operations for any device and dtype: the parity oracle (fp64 on the CPU), the
benchmark's baseline and the CPU path of tests that have no GPU.  The HIP path
has no CPU fallback: host tensors raise.

The masked SSIM is not the training SSIM of image_loss.py: its windows are
"valid" (the map is (H - 10) x (W - 10)), each pass of its blur is rescaled by
11 / (unmasked taps) -- the tap count, not the unmasked weight: the reference's
choice, kept -- the mask is propagated between the passes and the variances
are clamped.  Its constants (window 11, sigma 1.5, k1 0.01, k2 0.03) are the
documented defaults of torchmetrics' StructuralSimilarityIndexMeasure, which
the reference inherits them from.

    PCK().update(...) / .compute()        metrics.py:489-520  -> PCK        (plain torch; the 2-D tracks
                                                                             come from tracking.track_points)

    unproject_image(...) / mMDE()         metrics.py:131-213, 254-292 -> MeanDepthError (the z-buffer and the
                                                                             abs-rel score are depth_geometry's
                                                                             point_depth_maps / depth_abs_rel)

Out of scope: LPIPS (mLPIPS needs network weights that do not ship with this
package) and the image file unproject_image saves of its estimated depth map
(save_depth_map; point_depth_maps returns the map).
"""
from __future__ import annotations

import functools
import math
from typing import Callable, Iterable, NamedTuple, Optional, Tuple

import torch

from . import _args, _lib
from ._lib import GsplatError

WINDOW, SIGMA = 11, 1.5
C1, C2 = 0.01 ** 2, 0.03 ** 2


_need = functools.partial(_args.need, op="metrics need", twin="image_metrics_torch / mask_iou_torch run")


class ImageMetrics(NamedTuple):
    """Per-image sums of one image_metrics call ([B] tensors; 0-dim for a single image)."""
    sse: torch.Tensor       # sum over Ch, H, W of ((pred - target) * mask)^2
    sae: torch.Tensor       # sum over Ch, H, W of |(pred - target) * mask|
    mask_sum: torch.Tensor  # sum over H, W of mask (H * W without one)
    ssim: torch.Tensor      # mean of the masked-SSIM map (0 with ssim=False)
    shape: Tuple[int, int, int]  # (Ch, H, W)


def _check_pair(pred, target, mask, need):
    """Shapes of a [B, Ch, H, W] / [Ch, H, W] pair and its mask; -> (pred, target, mask, single)."""
    if not isinstance(pred, torch.Tensor) or pred.dim() not in (3, 4):
        raise GsplatError("pred must be a [B, Ch, H, W] or [Ch, H, W] tensor")
    single = pred.dim() == 3
    if need:
        _need(pred, "pred")
        _need(target, "target", pred.shape)
    elif not isinstance(target, torch.Tensor) or target.shape != pred.shape:
        raise GsplatError(f"target must have shape {tuple(pred.shape)}")
    if single:
        pred, target = pred[None], target[None]
    B, Ch, H, W = pred.shape
    if min(B, Ch, H, W) < 1:
        raise GsplatError(f"pred must not be empty (got {tuple(pred.shape)})")
    if need:
        mask = _args.mask_f32(mask, B, H, W)
    elif mask is not None:
        _args.check_mask(mask, B, H, W, need_device=False)
    return pred, target, mask, single


def image_metrics(pred: torch.Tensor, target: torch.Tensor, mask: Optional[torch.Tensor] = None, *,
                  ssim: bool = True) -> ImageMetrics:
    """sse, sae, mask_sum and the masked SSIM of pred against target, per image of a batch
    [B, Ch, H, W] (or one image [Ch, H, W]); mask [H, W] or [B, H, W] is optional.  Contiguous
    float32 device tensors only (a mask of another dtype is converted).  ssim=False skips the
    window passes (any H, W; ssim is 0); ssim=True needs H, W >= 11.  Forward only: no gradient
    reaches the inputs.  Asynchronous; two calls on the same inputs give the same bits."""
    pred, target, mask, single = _check_pair(pred, target, mask, need=True)
    B, Ch, H, W = pred.shape
    if ssim and (H < WINDOW or W < WINDOW):
        raise GsplatError(f"the masked SSIM needs H, W >= {WINDOW} (got {H} x {W}): no window fits; "
                          "ssim=False gives the sums alone")
    L = _lib.load()
    dev = pred.device
    pred, target = pred.detach(), target.detach()
    out = torch.empty(B, 4, dtype=torch.float32, device=dev)
    ws = torch.empty(L.gs_image_metrics_workspace_bytes(B, Ch, H, W), dtype=torch.uint8, device=dev)
    args = _lib.GsImageMetrics(B=B, Ch=Ch, H=H, W=W, pred=pred.data_ptr(), target=target.data_ptr(),
                               mask=mask.data_ptr() if mask is not None else None,
                               mask_batch_stride=H * W if mask is not None and mask.dim() == 3 else 0,
                               want_ssim=1 if ssim else 0, out=out.data_ptr(), workspace=ws.data_ptr(),
                               workspace_bytes=ws.numel())
    _lib.check(L.gs_image_metrics(args, _lib.stream(dev)), "image metrics")
    cols = out[0] if single else out.t()
    return ImageMetrics(cols[0], cols[1], cols[2], cols[3], (Ch, H, W))


def _window_1d(like: torch.Tensor) -> torch.Tensor:
    """metrics.py:366-376: the normalised 1-D Gaussian in the image's dtype."""
    hw = WINDOW // 2
    f_i = ((torch.arange(WINDOW, device=like.device, dtype=like.dtype) - hw) / SIGMA) ** 2
    filt = torch.exp(-0.5 * f_i)
    return filt / torch.sum(filt)


def _masked_blur_pass(z, m, f):
    """One pass of metrics.py:379-390, channels first: z [B, Ch, H, W], m [B, 1, H, W], f [kh, kw]."""
    ch = z.shape[1]
    f = f[None, None].expand(ch, -1, -1, -1)
    z_ = torch.nn.functional.conv2d(z * m, f, groups=ch)  # "valid"
    m_ = torch.nn.functional.conv2d(m, torch.ones_like(f[:1]))
    out = torch.where(m_ != 0, z_ * torch.ones_like(f).sum() / (m_ * ch), torch.zeros((), dtype=z.dtype, device=z.device))
    return out, (m_ != 0).to(z.dtype)


def _masked_ssim_torch(pred, target, m):
    filt = _window_1d(pred)

    def blur(z):  # along the rows, then down the columns (metrics.py:392-394)
        return _masked_blur_pass(*_masked_blur_pass(z, m, filt[None, :]), filt[:, None])[0]

    mu0, mu1 = blur(pred), blur(target)
    mu00, mu11, mu01 = mu0 * mu0, mu1 * mu1, mu0 * mu1
    sigma00 = (blur(pred ** 2) - mu00).clamp(min=0.0)
    sigma11 = (blur(target ** 2) - mu11).clamp(min=0.0)
    sigma01 = blur(pred * target) - mu01
    sigma01 = torch.sign(sigma01) * torch.minimum(torch.sqrt(sigma00 * sigma11), torch.abs(sigma01))
    numer = (2 * mu01 + C1) * (2 * sigma01 + C2)
    denom = (mu00 + mu11 + C1) * (sigma00 + sigma11 + C2)
    return (numer / denom).mean(dim=(1, 2, 3))


def image_metrics_torch(pred: torch.Tensor, target: torch.Tensor, mask: Optional[torch.Tensor] = None, *,
                        ssim: bool = True) -> ImageMetrics:
    """image_metrics in PyTorch operations, any device and dtype, as the reference computes
    them: the sums of metrics.py:120-123 and mSSIM.update (metrics.py:363-420; ten masked
    depthwise convolutions and ten mask-count convolutions per call)."""
    pred, target, mask, single = _check_pair(pred, target, mask, need=False)
    B, Ch, H, W = pred.shape
    if ssim and (H < WINDOW or W < WINDOW):
        raise GsplatError(f"the masked SSIM needs H, W >= {WINDOW} (got {H} x {W}): no window fits")
    if mask is None:
        m = torch.ones(B, 1, H, W, dtype=pred.dtype, device=pred.device)
    else:
        m = mask.to(pred.dtype)
        m = m[None, None].expand(B, 1, H, W) if m.dim() == 2 else m[:, None]
    d = (pred - target) * m
    sse = torch.pow(d, 2).sum(dim=(1, 2, 3))
    sae = torch.abs(d).sum(dim=(1, 2, 3))
    mask_sum = m.sum(dim=(1, 2, 3))
    s = _masked_ssim_torch(pred, target, m) if ssim else torch.zeros_like(sse)
    if single:
        sse, sae, mask_sum, s = sse[0], sae[0], mask_sum[0], s[0]
    return ImageMetrics(sse, sae, mask_sum, s, (Ch, H, W))


# ---- derived on the device, without readback (fp64: one log of a sum's ratio)

def psnr_masked(m: ImageMetrics) -> torch.Tensor:
    """-10 log10(sse / (mask_sum Ch)): one mPSNR update (metrics.py:120-129)."""
    return -10.0 * torch.log(m.sse.double() / (m.mask_sum.double() * m.shape[0])) / math.log(10.0)


def psnr_clamped(m: ImageMetrics) -> torch.Tensor:
    """compute_psnr (metrics.py:31-43): psnr_masked with mask_sum.clamp(min=1)."""
    return -10.0 * torch.log(m.sse.double() / m.mask_sum.double().clamp(min=1.0) / m.shape[0]) / math.log(10.0)


def psnr_plain(m: ImageMetrics) -> torch.Tensor:
    """calc_psnr (external.py:85-87) of an unmasked call: 20 log10(1 / sqrt(mse))."""
    ch, h, w = m.shape
    return 20.0 * torch.log10(1.0 / torch.sqrt(m.sse.double() / (ch * h * w)))


def l1(m: ImageMetrics) -> torch.Tensor:
    """Mean absolute error over Ch, H, W (l1_loss_v1, helpers.py:110-111, of the masked pair)."""
    ch, h, w = m.shape
    return m.sae.double() / (ch * h * w)


# ---- mask IoU

def _check_masks(pred_mask, target_mask, need):
    if not isinstance(pred_mask, torch.Tensor) or pred_mask.dim() not in (2, 3):
        raise GsplatError("pred_mask must be a [B, H, W] or [H, W] tensor")
    if need:
        _need(pred_mask, "pred_mask")
        _need(target_mask, "target_mask", pred_mask.shape)
    elif not isinstance(target_mask, torch.Tensor) or target_mask.shape != pred_mask.shape:
        raise GsplatError(f"target_mask must have shape {tuple(pred_mask.shape)}")
    if pred_mask.numel() == 0:
        raise GsplatError(f"pred_mask must not be empty (got {tuple(pred_mask.shape)})")


def mask_iou(pred_mask: torch.Tensor, target_mask: torch.Tensor,
             threshold: float = 0.9) -> Tuple[torch.Tensor, torch.Tensor]:
    """(intersection, union) pixel counts of (pred_mask > threshold) and (target_mask >
    threshold), per image of [B, H, W] (or one [H, W] pair): int64 device tensors, exact.
    threshold 0.9 is the reference's mask_iou (metrics.py:234-235), 0 its MaskIoU for {0, 1}
    masks.  Contiguous float32 device tensors only."""
    _check_masks(pred_mask, target_mask, need=True)
    threshold = float(threshold)
    if math.isnan(threshold):
        raise GsplatError("threshold must not be NaN")
    single = pred_mask.dim() == 2
    B = 1 if single else pred_mask.shape[0]
    n = pred_mask.numel() // B
    L = _lib.load()
    dev = pred_mask.device
    out = torch.empty(B, 2, dtype=torch.int64, device=dev)
    _lib.check(L.gs_mask_iou(B, n, pred_mask.detach().data_ptr(), target_mask.detach().data_ptr(), threshold,
                             out.data_ptr(), _lib.stream(dev)), "mask IoU")
    return (out[0, 0], out[0, 1]) if single else (out[:, 0], out[:, 1])


def mask_iou_torch(pred_mask: torch.Tensor, target_mask: torch.Tensor,
                   threshold: float = 0.9) -> Tuple[torch.Tensor, torch.Tensor]:
    """mask_iou in PyTorch operations (metrics.py:234-243), any device and dtype."""
    _check_masks(pred_mask, target_mask, need=False)
    a, b = pred_mask > threshold, target_mask > threshold
    dims = (-2, -1)
    return torch.logical_and(a, b).sum(dim=dims), torch.logical_or(a, b).sum(dim=dims)


def iou_ratio(intersection: torch.Tensor, union: torch.Tensor) -> torch.Tensor:
    """intersection / union, 1 where the union is empty (metrics.py:245-247); fp64, on the counts' device."""
    u = union.double()
    return torch.where(union == 0, torch.ones_like(u), intersection.double() / u.clamp(min=1.0))


def iou(pred_mask: torch.Tensor, target_mask: torch.Tensor, threshold: float = 0.9, *,
        counts: Callable = mask_iou) -> torch.Tensor:
    """The reference's mask_iou value per image: intersection over union, 1 for two empty masks."""
    return iou_ratio(*counts(pred_mask, target_mask, threshold))


def pose_errors(preds, targets) -> Tuple[float, float, float]:
    """The reference's compute_pose_errors (metrics.py:46-79) for two sequences
    of N >= 2 camera-to-world poses ([N, 4, 4] tensors or arrays, e.g.
    camera.PoseRefiner.poses() against the true poses): (ate, rpe_t,
    rpe_r_deg) -- the mean distance of the camera centres; and, over the N - 1
    consecutive pairs, with rel_i = pose_i^-1 pose_{i+1} and the error
    target_rel_i^-1 pred_rel_i, the mean norm of its translation and the mean
    angle of its rotation in degrees.  Host numpy in fp64 throughout: the
    reference insists on numpy for the arccos near 1, where small angles live
    (a reporting function of tiny inputs; it reads device tensors back)."""
    import numpy as np

    def host(x):
        if isinstance(x, torch.Tensor):
            x = x.detach().cpu().numpy()
        x = np.asarray(x, dtype=np.float64)
        if x.ndim != 3 or x.shape[1:] != (4, 4):
            raise ValueError(f"poses must be [N, 4, 4], got {x.shape}")
        return x

    p, t = host(preds), host(targets)
    if p.shape != t.shape or p.shape[0] < 2:
        raise ValueError(f"preds and targets must be the same N >= 2 poses, got {p.shape} and {t.shape}")
    ate = float(np.linalg.norm(p[:, :3, 3] - t[:, :3, 3], axis=-1).mean())
    rel_p = np.linalg.inv(p[:-1]) @ p[1:]
    rel_t = np.linalg.inv(t[:-1]) @ t[1:]
    err = np.linalg.inv(rel_t) @ rel_p
    rpe_t = float(np.linalg.norm(err[:, :3, 3], axis=-1).mean())
    cos = np.clip((np.trace(err[:, :3, :3], axis1=-2, axis2=-1) - 1.0) / 2.0, -1.0, 1.0)
    rpe_r = float(np.arccos(cos).mean()) / np.pi * 180.0
    return ate, rpe_t, rpe_r


# ---- accumulators: device tensors in update(), the only readback in compute()

class _Accumulator:
    def __len__(self) -> int:
        return len(self._entries)

    def result(self) -> torch.Tensor:  # a 0-dim fp64 tensor on the entries' device
        raise NotImplementedError

    def compute(self) -> float:
        """The reduced value as a Python float: the accumulator's only readback."""
        if not self._entries:
            raise GsplatError(f"{type(self).__name__}.compute() before any update()")
        return float(self.result())


class MaskedPSNR(_Accumulator):
    """The reference's mPSNR (metrics.py:82-129): every update is one entry, the squared error
    and the mask count times Ch summed over the update's images; compute() is the
    mean over the entries of -10 log10(sse / total).  `update_images` files every image of a
    call as its own entry (a loop of per-image updates in one launch).  `metrics`: image_metrics
    (HIP, device tensors) or image_metrics_torch."""

    def __init__(self, metrics: Callable = image_metrics):
        self.metrics = metrics
        self._entries = []  # (sse, total) pairs, each [n] fp64

    def update(self, pred, target, mask=None) -> None:
        m = self.metrics(pred, target, mask, ssim=False)
        self._entries.append((m.sse.double().sum().reshape(1), (m.mask_sum.double().sum() * m.shape[0]).reshape(1)))

    def update_images(self, m: ImageMetrics) -> None:
        self._entries.append((m.sse.double().reshape(-1), m.mask_sum.double().reshape(-1) * m.shape[0]))

    def result(self) -> torch.Tensor:
        sse = torch.cat([e[0] for e in self._entries])
        total = torch.cat([e[1] for e in self._entries])
        return -10.0 * torch.log(sse / total).mean() / math.log(10.0)


class MaskedSSIM(_Accumulator):
    """The reference's mSSIM (metrics.py:334-424): the mean over all images of all updates."""

    def __init__(self, metrics: Callable = image_metrics):
        self.metrics = metrics
        self._entries = []  # [n] fp64 per update

    def update(self, pred, target, mask=None) -> None:
        self.update_images(self.metrics(pred, target, mask, ssim=True))

    def update_images(self, m: ImageMetrics) -> None:
        self._entries.append(m.ssim.double().reshape(-1))

    def result(self) -> torch.Tensor:
        return torch.cat(self._entries).mean()


class MaskIoU(_Accumulator):
    """The reference's MaskIoU (metrics.py:523-552) for {0, 1} masks (any value > 0 counts, as
    .to(torch.bool) of a non-negative mask): every update is one entry, intersection and union
    summed over the update's images; compute() is the mean over the entries of
    intersection / union.clamp(min=1e-8) -- a mean of per-update ratios, and 0 (not 1) for an
    update whose union is empty: the reference's final line, kept."""

    def __init__(self, counts: Callable = mask_iou):
        self.counts = counts
        self._entries = []  # (intersection, union) pairs, each [1] fp64

    def update(self, pred_mask, target_mask) -> None:
        i, u = self.counts(pred_mask, target_mask, 0.0)
        self._entries.append((i.double().sum().reshape(1), u.double().sum().reshape(1)))

    def result(self) -> torch.Tensor:
        i = torch.cat([e[0] for e in self._entries])
        u = torch.cat([e[1] for e in self._entries])
        return (i / u.clamp(min=1e-8)).mean()


class MeanIoU(_Accumulator):
    """The reference's mIOU (metrics.py:295-331): the mean of mask_iou values (threshold 0.9,
    1 for two empty masks), one per image of every update."""

    def __init__(self, counts: Callable = mask_iou, threshold: float = 0.9):
        self.counts, self.threshold = counts, threshold
        self._entries = []  # [n] fp64 per update

    def update(self, pred_mask, target_mask) -> None:
        self._entries.append(iou_ratio(*self.counts(pred_mask, target_mask, self.threshold)).reshape(-1))

    def result(self) -> torch.Tensor:
        return torch.cat(self._entries).mean()


class PCK(_Accumulator):
    """The reference's PCK (metrics.py:489-520), the share of correct keypoints: every update
    is one entry, the count of predictions preds [N, 2] strictly nearer than `threshold` (in
    pixels) to their targets [N, 2] and N; compute() is the mean over the entries of
    correct / max(total, 1e-8) -- a mean of per-update ratios, and 0 for an empty update: the
    reference's final line, kept.  `visible` ([N] bool, optional; no reference analogue, its
    callers index the visible points first): the update counts the visible targets only, as
    preds[visible] / targets[visible] would, without the host synchronisation of a boolean
    index.  Plain torch on the tensors' device (tracking.track_points produces the
    predictions); nothing is read back before compute()."""

    def __init__(self):
        self._entries = []  # (correct, total) pairs, each [1] fp64

    def update(self, preds: torch.Tensor, targets: torch.Tensor, threshold: float,
               visible: Optional[torch.Tensor] = None) -> None:
        if preds.shape != targets.shape or preds.dim() != 2:
            raise GsplatError(f"preds and targets must both be [N, D] (got {tuple(preds.shape)} and "
                              f"{tuple(targets.shape)})")
        ok = torch.linalg.norm(preds - targets, dim=-1) < threshold
        if visible is None:
            total = torch.full((1,), float(preds.shape[0]), dtype=torch.float64, device=preds.device)
        else:
            if visible.shape != ok.shape:
                raise GsplatError(f"visible must have shape {tuple(ok.shape)} (got {tuple(visible.shape)})")
            vis = visible.to(device=ok.device, dtype=torch.bool)
            ok = ok & vis
            total = vis.sum().double().reshape(1)
        self._entries.append((ok.sum().double().reshape(1), total))

    def result(self) -> torch.Tensor:
        correct = torch.cat([e[0] for e in self._entries])
        total = torch.cat([e[1] for e in self._entries])
        return (correct / total.clamp(min=1e-8)).mean()


class MeanDepthError(_Accumulator):
    """The reference's mMDE (metrics.py:254-292): the mean over images of unproject_image's
    absolute relative depth error.  update(points, w2c, K, depth_gt, exclude) projects the
    cloud points [P, 3] (or [B, P, 3], one per camera) into the cameras w2c [B, 4, 4],
    K [B, 3, 3], keeps the nearest point per pixel and scores the map against depth_gt
    [B, H, W] where it is finite, depth_gt > 0 and exclude != 1 (exclude [H, W] or [B, H, W],
    optional): one entry per image, as a loop of the reference's per-image updates.  compute()
    is the mean of the entries (NaN if an image had no valid pixel, as the reference's).
    `maps` / `score`: depth_geometry's point_depth_maps / depth_abs_rel (HIP, device tensors)
    or their _torch twins.  Nothing is read back before compute()."""

    def __init__(self, maps: Optional[Callable] = None, score: Optional[Callable] = None):
        from . import depth_geometry
        self.maps = maps if maps is not None else depth_geometry.point_depth_maps
        self.score = score if score is not None else depth_geometry.depth_abs_rel
        self._entries = []  # [n] fp64 per update

    def update(self, points, w2c, K, depth_gt, exclude=None) -> None:
        est = self.maps(points, w2c, K, depth_gt.shape[-2:])
        self.update_images(self.score(est, depth_gt, exclude))

    def update_images(self, scores: torch.Tensor) -> None:
        self._entries.append(scores.double().reshape(-1))

    def result(self) -> torch.Tensor:
        return torch.cat(self._entries).mean()


# ---- a forward-only batch render, scored

def evaluate_cameras(rendervar: dict, settings_all, targets: torch.Tensor, masks: Optional[torch.Tensor] = None, *,
                     seg: Optional[torch.Tensor] = None, seg_targets: Optional[torch.Tensor] = None,
                     clip: bool = True, depth_gt: Optional[torch.Tensor] = None,
                     depth_exclude: Optional[torch.Tensor] = None) -> dict:
    """Render the cameras `settings_all` (a list of GaussianRasterizationSettings, or a
    GaussianRasterizerBatch built from one, reused over calls) from `rendervar`
    (timesteps.params2rendervar) in one forward-only batch launch and score the images against
    `targets` [C, 3, H, W] under `masks` ([H, W] or [C, H, W], optional) with one image_metrics
    call.  The render is clipped to [0, 1] first (clip=True), as the reference's loops do
    (im.clip(0, 1)) before they score or save it.  With `seg` and `seg_targets` ([C, H, W] soft
    masks, e.g. a rendered segmentation channel and its ground truth) one mask_iou call at 0.9.

    Returns per-camera device tensors, nothing read back: image (the scored render), metrics
    (the ImageMetrics), sse, sae, mask_sum, ssim, l1, psnr (calc_psnr; over the masked pair
    when masks are given), psnr_masked (the mPSNR update, with masks), and intersection, union,
    iou with seg.  With `depth_gt` [C, H, W] (and `depth_exclude`, [H, W] or [C, H, W],
    optional) also mde: the mMDE score of the cloud rendervar["means3D"] in each camera of the
    settings (depth_geometry.point_depth_maps and depth_abs_rel).  Runs under torch.no_grad():
    the parameters get no .grad."""
    from .rasterizer import GaussianRasterizerBatch
    with torch.no_grad():
        ras = settings_all if isinstance(settings_all, GaussianRasterizerBatch) else \
            GaussianRasterizerBatch(list(settings_all))
        rv = {k: v.detach() for k, v in rendervar.items()}
        if "semantic_feature" in rv:
            im = ras(**rv, label=None)[0]
        else:
            im = ras(**rv)[0]
        if clip:
            im = im.clamp(0.0, 1.0)
        im = im.contiguous()
        m = image_metrics(im, targets, masks)
        out = {"image": im, "metrics": m, "sse": m.sse, "sae": m.sae, "mask_sum": m.mask_sum, "ssim": m.ssim,
               "l1": l1(m), "psnr": psnr_plain(m)}
        if masks is not None:
            out["psnr_masked"] = psnr_masked(m)
        if (seg is None) != (seg_targets is None):
            raise GsplatError("seg and seg_targets come together")
        if seg is not None:
            i, u = mask_iou(seg, seg_targets, 0.9)
            out.update(intersection=i, union=u, iou=iou_ratio(i, u))
        if depth_gt is None and depth_exclude is not None:
            raise GsplatError("depth_exclude comes with depth_gt")
        if depth_gt is not None:
            from . import depth_geometry as dg
            w2c, K, hw = dg.cameras_of_settings(ras.settings_list)
            est = dg.point_depth_maps(rv["means3D"].contiguous(), w2c, K, hw)
            out["mde"] = dg.depth_abs_rel(est, depth_gt, depth_exclude)
        return out


def evaluate_sequence(params_per_timestep: Iterable[dict], settings_all, targets_fn: Callable[[int], torch.Tensor],
                      masks_fn: Optional[Callable[[int], Optional[torch.Tensor]]] = None) -> dict:
    """evaluate_cameras over the timesteps of a trained sequence: `params_per_timestep` yields
    the Dynamic3DGaussians parameters of timestep t (timesteps.params2rendervar's input),
    targets_fn(t) its images [C, 3, H, W], masks_fn(t) its masks or None.  Every camera image
    is one entry of the accumulators, as in the reference's per-image loops.  One readback at
    the end.  Returns the means the reference reports: psnr (calc_psnr, external.py:85-87),
    l1, mssim (mSSIM.compute) and, when every timestep had masks, mpsnr (mPSNR.compute);
    images is the number of images scored."""
    from .rasterizer import GaussianRasterizerBatch
    from .timesteps import params2rendervar
    ras = settings_all if isinstance(settings_all, GaussianRasterizerBatch) else \
        GaussianRasterizerBatch(list(settings_all))
    mpsnr, mssim = MaskedPSNR(), MaskedSSIM()
    psnr, l1s, masked = [], [], True
    for t, params in enumerate(params_per_timestep):
        with torch.no_grad():
            rv = params2rendervar({k: v.detach() for k, v in params.items()})
        mk = masks_fn(t) if masks_fn is not None else None
        r = evaluate_cameras(rv, ras, targets_fn(t), mk)
        masked = masked and mk is not None
        mssim.update_images(r["metrics"])
        mpsnr.update_images(r["metrics"])
        psnr.append(r["psnr"].reshape(-1))
        l1s.append(r["l1"].reshape(-1))
    if not psnr:
        raise GsplatError("evaluate_sequence: no timestep")
    vals = [torch.cat(psnr).mean(), torch.cat(l1s).mean(), mssim.result()] + ([mpsnr.result()] if masked else [])
    host = torch.stack(vals).tolist()  # the one readback
    out = dict(zip(("psnr", "l1", "mssim", "mpsnr"), host))
    out["images"] = sum(int(p.numel()) for p in psnr)
    return out
