#!/usr/bin/env python3
"""Generate tests/golden/eval_metrics.npz from the REFERENCE's own Python code
(run where the reference checkout exists; the fixture -- data only -- is
committed, the reference never travels).

The reference's metrics.py (compute_psnr :14-43, mPSNR :82-129, mask_iou
:222-250, mIOU :295-331, mSSIM :334-424, MaskIoU :523-552) imports
torchmetrics, which is not installed here.  It is imported under a stand-in
`torchmetrics` in sys.modules, the way make_golden.py stands in for Open3D:
Metric, PeakSignalNoiseRatio, StructuralSimilarityIndexMeasure and
dim_zero_cat below are a few lines of our own that keep the constructor
arguments the reference's subclasses pass and set

    kernel_size = 11, sigma = 1.5, k1 = 0.01, k2 = 0.03

UNPINNED CONSTANTS: those four are the documented defaults of torchmetrics'
StructuralSimilarityIndexMeasure; they cannot be read from a torchmetrics
installation here, so they are stated, not imported.  All arithmetic that is
recorded is the reference's own (its update / compute bodies).

torch.set_default_dtype(torch.float64) is set before the import, so the
reference's own filter (built with torch.arange under the default dtype) and
every sum are fp64.  The inputs are stored as the fp32 values they were drawn
as, channels first; the reference gets them as fp64 [B, H, W, Ch].

The reference's PSNR code hard-codes three channels (compute_psnr divides by
3.0, mPSNR counts masks.sum() * 3), so those records exist for the
three-channel cases only.  mPSNR.update prints masks.shape before it
replaces a missing mask, so it is always given one (ones where the case has
none).  mask_iou and MaskIoU sum in .float(): their recorded values carry
fp32 rounding.

Cases (all seeded), B x Ch x H x W:
  one_window     1 x 3 x 11 x 11   no mask: one output pixel
  empty_windows  2 x 3 x 13 x 29   80 % random binary [B, H, W] mask, columns 0..11 zeroed:
                                   windows with no unmasked tap in the first pass, map == 1 exactly
  ragged_masked  2 x 3 x 45 x 77   80 % mask, a 20 x 30 hole in image 1 only: several tiles, ragged
                                   last ones, halos across tile edges, masks that differ per image
  flat           1 x 3 x 37 x 53   rows 0..17 zero in both, the rest 0.7 against 0.7 + 0.01 noise:
                                   the E[z^2] - mu^2 cancellation and the variance clamps
  features       1 x 32 x 21 x 40  amplitude 10, no mask
and soft segmentation masks `iou.*` 3 x 45 x 77 (image 2 below every threshold: an empty union).

Usage: python tests/golden/make_golden_metrics.py --reference <reference checkout>
"""
from __future__ import annotations

import argparse
import contextlib
import io
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

CASES = ("one_window", "empty_windows", "ragged_masked", "flat", "features")
SHAPES = {"one_window": (1, 3, 11, 11), "empty_windows": (2, 3, 13, 29), "ragged_masked": (2, 3, 45, 77),
          "flat": (1, 3, 37, 53), "features": (1, 32, 21, 40)}
SEEDS = {"one_window": 21, "empty_windows": 22, "ragged_masked": 23, "flat": 24, "features": 25}


# ---- the stand-in torchmetrics: a few lines of our own

class Metric:
    def __init__(self, **kwargs):
        assert not kwargs, kwargs
        self.device = torch.device("cpu")

    def add_state(self, name, default, dist_reduce_fx=None):
        setattr(self, name, list(default) if isinstance(default, list) else default)


class PeakSignalNoiseRatio(Metric):
    def __init__(self, data_range=None, base=10.0, dim=None, reduction="elementwise_mean", **kwargs):
        super().__init__(**kwargs)
        self.data_range, self.base, self.dim, self.reduction = data_range, base, dim, reduction


class StructuralSimilarityIndexMeasure(Metric):
    def __init__(self, reduction="elementwise_mean", data_range=None, return_full_image=False, **kwargs):
        super().__init__(**kwargs)
        # the documented defaults (module docstring: unpinned constants)
        self.kernel_size, self.sigma, self.k1, self.k2 = 11, 1.5, 0.01, 0.03
        self.data_range, self.reduction, self.return_full_image = data_range, reduction, return_full_image
        self.add_state("similarity", default=[], dist_reduce_fx="cat")


def dim_zero_cat(x):
    """A list of tensors joined along dimension 0, 0-dim entries as one element each."""
    x = x if isinstance(x, (list, tuple)) else [x]
    return torch.cat([y.reshape(1) if y.dim() == 0 else y for y in x], dim=0)


def _stand_in_modules():
    mods = {n: types.ModuleType(n) for n in (
        "torchmetrics", "torchmetrics.functional", "torchmetrics.functional.image",
        "torchmetrics.functional.image.lpips", "torchmetrics.image", "torchmetrics.metric",
        "torchmetrics.utilities", "torchmetrics.utilities.imports")}
    mods["torchmetrics.functional.image.lpips"]._NoTrainLpips = None
    mods["torchmetrics.image"].PeakSignalNoiseRatio = PeakSignalNoiseRatio
    mods["torchmetrics.image"].StructuralSimilarityIndexMeasure = StructuralSimilarityIndexMeasure
    mods["torchmetrics.metric"].Metric = Metric
    mods["torchmetrics.utilities"].dim_zero_cat = dim_zero_cat
    mods["torchmetrics.utilities.imports"]._TORCHVISION_AVAILABLE = False
    return mods


def load_reference_metrics(reference):
    from tests.golden.make_golden import _load_module
    saved = {}
    for n, m in _stand_in_modules().items():
        saved[n] = sys.modules.get(n)
        sys.modules[n] = m
    try:
        return _load_module("ref_metrics", os.path.join(reference, "metrics.py"))
    finally:
        for n, m in saved.items():
            if m is None:
                sys.modules.pop(n, None)
            else:
                sys.modules[n] = m


# ---- inputs

def _smooth(gen, b, ch, h, w):
    """A low-frequency pattern plus a little noise, in [0, 1] roughly."""
    yy, xx = torch.meshgrid(torch.linspace(0, 1, h, dtype=torch.float32), torch.linspace(0, 1, w, dtype=torch.float32),
                            indexing="ij")
    f = torch.rand(b, ch, 4, generator=gen, dtype=torch.float32) * 6.0
    f = f[..., None, None]
    base = 0.5 + 0.25 * torch.sin(f[:, :, 0] * xx + f[:, :, 1]) * torch.cos(f[:, :, 2] * yy + f[:, :, 3])
    return (base + 0.05 * torch.randn(b, ch, h, w, generator=gen, dtype=torch.float32)).float()


def case_inputs(name):
    """fp32 pred, target [B, Ch, H, W] and the uint8 mask [B, H, W] (None without one)."""
    gen = torch.Generator().manual_seed(SEEDS[name])
    b, ch, h, w = SHAPES[name]
    mask = None
    if name in ("one_window", "empty_windows", "ragged_masked"):
        pred = _smooth(gen, b, ch, h, w).clamp(0, 1)
        target = (0.5 * _smooth(gen, b, ch, h, w) + 0.5 * pred).clamp(0, 1)
        if name != "one_window":
            mask = (torch.rand(b, h, w, generator=gen, dtype=torch.float32) < 0.8).to(torch.uint8)
        if name == "empty_windows":
            mask[:, :, :12] = 0
        if name == "ragged_masked":
            mask[1, 10:30, 25:55] = 0
    elif name == "flat":
        pred = torch.full((b, ch, h, w), 0.7, dtype=torch.float32)
        target = (0.7 + 0.01 * torch.randn(b, ch, h, w, generator=gen, dtype=torch.float32)).float()
        pred[:, :, :18] = 0.0
        target[:, :, :18] = 0.0
    else:
        pred = (10.0 * torch.randn(b, ch, h, w, generator=gen, dtype=torch.float32)).float()
        target = (pred + 5.0 * torch.randn(b, ch, h, w, generator=gen, dtype=torch.float32)).float()
    return pred.contiguous(), target.contiguous(), mask


def iou_inputs():
    """Soft masks [3, 45, 77] fp32 in [0, 1]: two overlapping blobs with noise; image 2 of both
    stays below 0.85 (an empty union at 0.9)."""
    gen = torch.Generator().manual_seed(31)
    h, w = 45, 77
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")

    def blob(cy, cx, r):
        return torch.sigmoid((r - torch.sqrt((yy - cy) ** 2 + (xx - cx) ** 2)) * 0.8)

    pred = torch.stack([blob(20, 30, 12), blob(25, 50, 15), 0.85 * blob(22, 38, 10)])
    target = torch.stack([blob(22, 34, 12), blob(20, 44, 9), 0.85 * blob(10, 10, 6)])
    pred = (pred + 0.05 * torch.rand(3, h, w, generator=gen, dtype=torch.float32)).clamp(0, 1)
    target = (target + 0.05 * torch.rand(3, h, w, generator=gen, dtype=torch.float32)).clamp(0, 1)
    pred[2].clamp_(max=0.85)
    target[2].clamp_(max=0.85)
    return pred.float().contiguous(), target.float().contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference (metrics.py, external.py)")
    a = ap.parse_args()
    torch.set_default_dtype(torch.float64)  # before the import: the reference's filter is fp64
    from tests.golden.make_golden import _load_with_placeholders
    R = load_reference_metrics(a.reference)
    ex = _load_with_placeholders("ref_external_metrics", os.path.join(a.reference, "external.py"))
    out = {}
    quiet = io.StringIO()  # the reference's update bodies print shapes
    for name in CASES:
        pred, target, mask = case_inputs(name)
        b, ch, h, w = pred.shape
        p, t = pred.double().permute(0, 2, 3, 1), target.double().permute(0, 2, 3, 1)  # [B, H, W, Ch]
        m = mask.double() if mask is not None else None
        out[f"{name}.pred"], out[f"{name}.target"] = pred.numpy(), target.numpy()
        if mask is not None:
            out[f"{name}.mask"] = mask.numpy()
        with contextlib.redirect_stdout(quiet):
            ssim = R.mSSIM()
            ssim.update(p, t, m)
            assert ssim.kernel_size == 11 and ssim.sigma == 1.5 and ssim.data_range == 1.0
            out[f"{name}.ssim"] = ssim.similarity[0].numpy()
            out[f"{name}.ssim_compute"] = ssim.compute().numpy()
            out[f"{name}.calc_psnr"] = ex.calc_psnr(pred.double(), target.double())[:, 0].numpy()
            if ch == 3:
                ones = torch.ones(b, h, w)
                whole = R.mPSNR()  # one update of the whole batch
                whole.update(p, t, m if m is not None else ones)
                out[f"{name}.mpsnr_sse"] = torch.stack(whole.sum_squared_error).numpy()
                out[f"{name}.mpsnr_total"] = torch.stack(whole.total).numpy()
                out[f"{name}.mpsnr_compute"] = whole.compute().numpy()
                each = R.mPSNR()  # one update per image
                for i in range(b):
                    each.update(p[i:i + 1], t[i:i + 1], (m if m is not None else ones)[i:i + 1])
                out[f"{name}.mpsnr_compute_per_image"] = each.compute().numpy()
                out[f"{name}.compute_psnr"] = np.array(
                    [R.compute_psnr(p[i], t[i], m[i] if m is not None else None) for i in range(b)], np.float64)
        assert out[f"{name}.ssim"].dtype == np.float64
        print(f"{name}: ssim {out[name + '.ssim']} calc_psnr {out[name + '.calc_psnr']}")
    sp, st = iou_inputs()
    out["iou.pred"], out["iou.target"] = sp.numpy(), st.numpy()
    with contextlib.redirect_stdout(quiet):
        vals = [R.mask_iou(sp[i].double(), st[i].double()) for i in range(3)]
        out["iou.mask_iou"] = np.array([float(v) for v in vals], np.float64)
        miou = R.mIOU()
        for i in range(3):
            miou.update(sp[i].double(), st[i].double())
        out["iou.miou_compute"] = miou.compute().numpy().astype(np.float64)
        hard_p, hard_t = (sp > 0.5).double(), (st > 0.5).double()  # {0, 1} masks for MaskIoU
        mi = R.MaskIoU()
        for i in range(3):
            mi.update(hard_p[i], hard_t[i])
        out["iou.maskiou_intersection"] = torch.stack(mi.intersection).numpy().astype(np.float64)
        out["iou.maskiou_union"] = torch.stack(mi.union).numpy().astype(np.float64)
        out["iou.maskiou_compute"] = mi.compute().numpy().astype(np.float64)
    print("mask_iou", out["iou.mask_iou"], "mIOU", out["iou.miou_compute"], "MaskIoU", out["iou.maskiou_intersection"],
          out["iou.maskiou_union"], out["iou.maskiou_compute"])
    path = os.path.join(HERE, "eval_metrics.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
