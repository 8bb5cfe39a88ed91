#!/usr/bin/env python3
"""Generate tests/golden/photometric_loss.npz from the REFERENCE's own Python
code (run where the reference checkout exists; the fixture -- data only -- is
committed, the reference never travels).

The reference's per-camera photometric loss, train.py:161-183:

    im   = exp(cam_m)[:, None, None] * im + cam_c[:, None, None]
    loss = 0.8 * l1_loss_v1(im * mask, gt * mask) + 0.2 * (1 - calc_ssim(im * mask, gt * mask))

with l1_loss_v1 from helpers.py (:110-111) and calc_ssim from external.py
(:90-133), loaded as make_golden.py loads them (an empty placeholder module
for Open3D while they import).  Everything runs in fp64 on the CPU; the
inputs are stored as the fp32 values they were drawn as, so the fp64 run and
a later fp32 run start from the same numbers.  Recorded per case: image,
target, mask (uint8), cam_m, cam_c, the loss and its autograd gradients with
respect to the image, cam_m and cam_c.

Cases (all seeded):
  small     3 x 9 x 7     smooth; the image is smaller than the window
  masked    3 x 37 x 53   smooth, a random 80 % mask, a colour correction
  flat      3 x 37 x 53   top half exactly 0 in both, bottom half 0.5 +- 1e-3
                          noise, one bottom pixel where image == target exactly
  features  32 x 13 x 23  feature channels of magnitude ~3

Usage: python tests/golden/make_golden_loss.py --reference <reference checkout>
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests.golden.make_golden import _load_with_placeholders  # noqa: E402  (_load_module under Open3D's placeholder)

CASES = ("small", "masked", "flat", "features")


def _smooth(gen, ch, h, w, amp=1.0):
    """A low-frequency pattern plus a little noise, in [0, amp] roughly."""
    yy, xx = torch.meshgrid(torch.linspace(0, 1, h), torch.linspace(0, 1, w), indexing="ij")
    f = torch.rand(ch, 4, generator=gen) * 6.0
    base = 0.5 + 0.25 * torch.sin(f[:, 0, None, None] * xx + f[:, 1, None, None]) \
        * torch.cos(f[:, 2, None, None] * yy + f[:, 3, None, None])
    return (amp * (base + 0.05 * torch.randn(ch, h, w, generator=gen))).float()


def case_inputs(name):
    gen = torch.Generator().manual_seed({"small": 11, "masked": 12, "flat": 13, "features": 14}[name])
    if name == "small":
        ch, h, w = 3, 9, 7
        image = _smooth(gen, ch, h, w)
        target = (image + 0.1 * torch.randn(ch, h, w, generator=gen)).float()
    elif name == "masked":
        ch, h, w = 3, 37, 53
        image = _smooth(gen, ch, h, w)
        target = (_smooth(gen, ch, h, w) * 0.5 + image * 0.5).float()
    elif name == "flat":
        ch, h, w = 3, 37, 53
        image = (0.5 + 1e-3 * torch.randn(ch, h, w, generator=gen)).float()
        target = (0.5 + 1e-3 * torch.randn(ch, h, w, generator=gen)).float()
        image[:, : h // 2] = 0.0
        target[:, : h // 2] = 0.0
        target[1, 30, 20] = image[1, 30, 20]  # |x - y| at exactly 0 in the non-zero half
    else:
        ch, h, w = 32, 13, 23
        image = (3.0 * torch.randn(ch, h, w, generator=gen)).float()
        target = (image + 1.5 * torch.randn(ch, h, w, generator=gen)).float()
    mask = torch.ones(h, w, dtype=torch.uint8)
    cam_m, cam_c = torch.zeros(ch), torch.zeros(ch)
    if name == "masked":
        mask = (torch.rand(h, w, generator=gen) < 0.8).to(torch.uint8)
        cam_m = (0.1 * torch.randn(ch, generator=gen)).float()
        cam_c = (0.05 * torch.randn(ch, generator=gen)).float()
    return image, target, mask, cam_m, cam_c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference (helpers.py, external.py)")
    a = ap.parse_args()
    hp = _load_with_placeholders("ref_helpers_loss", os.path.join(a.reference, "helpers.py"))
    ex = _load_with_placeholders("ref_external_loss", os.path.join(a.reference, "external.py"))
    out = {}
    for name in CASES:
        image, target, mask, cam_m, cam_c = case_inputs(name)
        im = image.double().requires_grad_(True)
        m = cam_m.double().requires_grad_(True)
        c = cam_c.double().requires_grad_(True)
        gt = target.double()
        # train.py:161-183, one camera
        cur = torch.exp(m)[:, None, None] * im + c[:, None, None]
        masked_im, masked_gt = cur * mask, gt * mask
        loss = 0.8 * hp.l1_loss_v1(masked_im, masked_gt) + 0.2 * (1.0 - ex.calc_ssim(masked_im, masked_gt))
        g_im, g_m, g_c = torch.autograd.grad(loss, (im, m, c))
        assert loss.dtype == torch.float64 and g_im.dtype == torch.float64
        for k, v in (("image", image), ("target", target), ("mask", mask), ("cam_m", cam_m), ("cam_c", cam_c),
                     ("loss", loss.detach()), ("grad_image", g_im), ("grad_cam_m", g_m), ("grad_cam_c", g_c)):
            out[f"{name}.{k}"] = v.numpy()
        print(f"{name}: loss {loss.item():.12f}")
    path = os.path.join(HERE, "photometric_loss.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
