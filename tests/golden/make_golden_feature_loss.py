#!/usr/bin/env python3
"""Generate tests/golden/feature_loss.npz from the REFERENCE's own statements
(run where the reference checkout exists; the fixture -- data only -- is
committed, the reference never travels).

The reference resamples a render to the size of its prior and takes the loss
there.  The statements are lines inside training loops, not functions, so this
script reads them out of the checkout at run time (after checking that each
one begins and ends where expected) and executes them in a namespace that
supplies what they name.  Nothing of the reference's text is stored here.

  revise_train.py:101, 104    feature_map = F.interpolate(..., align_corners=True);
                              Ll1_feature = l1_loss(feature_map, gt_feature_map)
  sanity_feature.py:442, 487  the same resample; losses['feature'] += 0.8 * l1_loss_v1(...)
                              + 0.2 * (1.0 - calc_ssim(...))
  dyn_double.py:303           depth_pred = F.interpolate(..., size=(288, 512), align_corners=False)

l1_loss comes from the reference's utils/loss_utils.py, l1_loss_v1 from its
helpers.py and calc_ssim from its external.py, loaded as make_golden.py loads
them.  The depth statement names its output size as a literal; the `F` its
namespace gets checks that literal and the mode, and resamples to the case's
small size with the statement's own mode and align_corners (a 288 x 512 map
would not fit a fixture).  The depth case's loss is l1_loss_v1 against a
target, so that a gradient exists.

Everything runs in fp64 on the CPU; the inputs are stored as the fp32 values
they were drawn as.  Recorded per case: feat [B, Ch, H, W], target
[B, Ch, h, w], align_corners, l1_weight, ssim_weight, the resized map
[B, Ch, h, w], the loss (summed over the B cameras, each executed on its own
as the reference does) and its gradient with respect to feat.

Cases (all seeded):
  l1       2 x 4 x 40 x 56 -> 18 x 32   align_corners=True, L1 only
  l1_ssim  2 x 4 x 40 x 56 -> 18 x 32   align_corners=True, 0.8 L1 + 0.2 (1 - SSIM)
  depth    1 x 1 x 37 x 53 -> 12 x 31   align_corners=False

Usage: python tests/golden/make_golden_feature_loss.py --reference <reference checkout>
"""
from __future__ import annotations

import argparse
import os
import sys
import textwrap

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests.golden.make_golden import _load_module, _load_with_placeholders  # noqa: E402

CASES = ("l1", "l1_ssim", "depth")
SHAPES = {"l1": (2, 4, 40, 56, 18, 32), "l1_ssim": (2, 4, 40, 56, 18, 32), "depth": (1, 1, 37, 53, 12, 31)}


def _smooth(gen, ch, h, w):
    """A low-frequency pattern plus a little noise, of magnitude ~1."""
    yy, xx = torch.meshgrid(torch.linspace(0, 1, h), torch.linspace(0, 1, w), indexing="ij")
    f = torch.rand(ch, 4, generator=gen) * 6.0
    base = torch.sin(f[:, 0, None, None] * xx + f[:, 1, None, None]) * torch.cos(f[:, 2, None, None] * yy + f[:, 3, None, None])
    return (base + 0.1 * torch.randn(ch, h, w, generator=gen)).float()


def case_inputs(name):
    gen = torch.Generator().manual_seed({"l1": 41, "l1_ssim": 42, "depth": 43}[name])
    B, Ch, H, W, h, w = SHAPES[name]
    feat = torch.stack([_smooth(gen, Ch, H, W) for _ in range(B)])
    target = torch.stack([_smooth(gen, Ch, h, w) for _ in range(B)])
    if name == "depth":
        feat, target = 1.0 + 4.0 * feat.abs(), 1.0 + 4.0 * target.abs()
    return feat, target


def statements(reference, fname, picks):
    """The 1-based lines `picks` = ((line, begins with, contains), ...) of a reference file as one
    code object."""
    with open(os.path.join(reference, fname)) as fh:
        lines = fh.read().splitlines()
    text = []
    for no, begins, contains in picks:
        line = lines[no - 1].strip()
        assert line.startswith(begins) and contains in line, (fname, no, line)
        text.append(line)
    return compile(textwrap.dedent("\n".join(text)), "%s:%s" % (fname, ",".join(str(p[0]) for p in picks)), "exec")


class _SmallF:
    """torch.nn.functional for dyn_double.py:303: its literal size checked, the case's size used."""

    def __init__(self, size):
        self.size = size

    def interpolate(self, x, size, mode, align_corners):
        assert tuple(size) == (288, 512) and mode == "bilinear", (size, mode)
        return torch.nn.functional.interpolate(x, size=self.size, mode=mode, align_corners=align_corners)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference")
    a = ap.parse_args()
    ref = a.reference
    hp = _load_with_placeholders("ref_helpers_feat", os.path.join(ref, "helpers.py"))
    ex = _load_with_placeholders("ref_external_feat", os.path.join(ref, "external.py"))
    lu = _load_module("ref_loss_utils_feat", os.path.join(ref, "utils", "loss_utils.py"))
    resample = ("feature_map = F.interpolate(feature_map.unsqueeze(0)", "align_corners=True).squeeze(0)")
    code = {
        "l1": statements(ref, "revise_train.py", ((101, *resample), (104, "Ll1_feature = l1_loss(", "gt_feature_map)"))),
        "l1_ssim": statements(ref, "sanity_feature.py", ((442, *resample), (487, "losses['feature'] +=", "calc_ssim("))),
        "depth": statements(ref, "dyn_double.py", ((303, "depth_pred = F.interpolate(depth_pred.unsqueeze(0)",
                                                    "align_corners=False)"),)),
    }
    out = {}
    for name in CASES:
        feat, target = case_inputs(name)
        B, Ch, H, W, h, w = SHAPES[name]
        x = feat.double().requires_grad_(True)
        total, resized = 0.0, []
        for b in range(B):
            if name == "depth":
                ns = {"F": _SmallF((h, w)), "depth_pred": x[b]}
                exec(code[name], ns)
                r = ns["depth_pred"][0]
                loss = hp.l1_loss_v1(r, target[b].double())
            else:
                ns = {"F": torch.nn.functional, "feature_map": x[b], "gt_feature_map": target[b].double(),
                      "l1_loss": lu.l1_loss, "l1_loss_v1": hp.l1_loss_v1, "calc_ssim": ex.calc_ssim,
                      "losses": {"feature": 0.0}}
                exec(code[name], ns)
                r = ns["feature_map"]
                loss = ns["Ll1_feature"] if name == "l1" else ns["losses"]["feature"]
            assert r.shape == (Ch, h, w) and r.dtype == torch.float64 and loss.dtype == torch.float64
            resized.append(r.detach())
            total = total + loss
        (g,) = torch.autograd.grad(total, x)
        l1w, sw = {"l1": (1.0, 0.0), "l1_ssim": (0.8, 0.2), "depth": (1.0, 0.0)}[name]
        for k, v in (("feat", feat), ("target", target), ("align_corners", torch.tensor(name != "depth")),
                     ("l1_weight", torch.tensor(l1w, dtype=torch.float64)),
                     ("ssim_weight", torch.tensor(sw, dtype=torch.float64)), ("resized", torch.stack(resized)),
                     ("loss", total.detach()), ("grad_feat", g)):
            out[f"{name}.{k}"] = v.numpy()
        print(f"{name}: loss {total.item():.12f}  |grad| {g.norm().item():.6e}")
    path = os.path.join(HERE, "feature_loss.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
