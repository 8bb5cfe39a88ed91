#!/usr/bin/env python3
"""Generate tests/golden/feature_decoder.npz from the REFERENCE's own statements (run where the
reference checkout exists; the fixture -- data only -- is committed, the reference never
travels).

The reference's "speedup" route resamples a render to its prior's size, lifts it with a 1x1
decoder and takes the L1 there (revise_train.py:101-104).  Read out of the checkout at run time,
after checking that each slice begins and ends where expected, and executed in a namespace that
supplies what they name; nothing of the reference's text is stored here:

  utils/loss_utils.py:17-18   def l1_loss(network_output, gt): ... .mean()
  revise_train.py:101         feature_map = F.interpolate(..., mode='bilinear', align_corners=True)

The decoder itself (models/networks.py, CNN_decoder) is not part of the reference checkout; it
is taken to be the upstream layer, torch's own nn.Conv2d(in_dim, out_dim, kernel_size=1) with
bias, here in fp64.

Everything runs in fp64 on the CPU.  The inputs are drawn on a grid of 1/16 (feature maps and
priors, stored as float16, which holds them exactly; the fixture stays small) and as fp32 values
(weight, bias).  Recorded per case: feat [F_in, H, W], target [C_out, h, w], weight [C_out, F_in],
bias [C_out], the loss and its gradients with respect to feat, weight and bias.

Cases (seeded):
  32to64   32 x 37 x 53 -> 12 x 31, decoded to 64 channels
  20to48   20 x 12 x 31 -> 37 x 53, decoded to 48 channels

Usage: python tests/golden/make_golden_feature_decoder.py --reference <reference checkout>
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests.golden.make_golden_feature_loss import statements  # noqa: E402

L1_FIRST, L1_LAST = 17, 18  # utils/loss_utils.py, 1-based, inclusive
CASES = {"32to64": (32, 64, 37, 53, 12, 31), "20to48": (20, 48, 12, 31, 37, 53)}


def _grid(gen, *shape):
    """Values on a grid of 1/16 in [-3, 3]: exact in float16."""
    return (torch.randn(*shape, generator=gen).clamp(-3, 3) * 16).round() / 16


def case_inputs(name):
    F_in, C_out, H, W, h, w = CASES[name]
    gen = torch.Generator().manual_seed({"32to64": 51, "20to48": 52}[name])
    feat, target = _grid(gen, F_in, H, W), _grid(gen, C_out, h, w)
    weight = (torch.randn(C_out, F_in, generator=gen) / F_in ** 0.5).float()
    bias = (0.5 * torch.randn(C_out, generator=gen)).float()
    return feat, target, weight, bias


def reference_l1(reference):
    with open(os.path.join(reference, "utils", "loss_utils.py")) as fh:
        lines = fh.read().splitlines()[L1_FIRST - 1:L1_LAST]
    assert lines[0].startswith("def l1_loss(network_output, gt):"), lines[0]
    assert lines[-1].strip().startswith("return torch.abs(") and lines[-1].strip().endswith(".mean()"), lines[-1]
    ns = {"torch": torch}
    exec(compile("\n".join(lines), "utils/loss_utils.py:%d-%d" % (L1_FIRST, L1_LAST), "exec"), ns)
    return ns["l1_loss"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference")
    a = ap.parse_args()
    l1_loss = reference_l1(a.reference)
    resample = statements(a.reference, "revise_train.py",
                          ((101, "feature_map = F.interpolate(feature_map.unsqueeze(0)", "align_corners=True).squeeze(0)"),))
    out = {}
    for name, (F_in, C_out, H, W, h, w) in CASES.items():
        feat, target, weight, bias = case_inputs(name)
        conv = torch.nn.Conv2d(F_in, C_out, kernel_size=1).double()
        with torch.no_grad():
            conv.weight.copy_(weight.double()[:, :, None, None])
            conv.bias.copy_(bias.double())
        x = feat.double().requires_grad_(True)
        ns = {"F": torch.nn.functional, "feature_map": x, "gt_feature_map": target.double()}
        exec(resample, ns)
        assert ns["feature_map"].shape == (F_in, h, w) and ns["feature_map"].dtype == torch.float64
        loss = l1_loss(conv(ns["feature_map"]), target.double())
        g_x, g_w, g_b = torch.autograd.grad(loss, (x, conv.weight, conv.bias))
        assert torch.equal(feat.half().float(), feat) and torch.equal(target.half().float(), target)
        for k, v in (("feat", feat.half()), ("target", target.half()), ("weight", weight), ("bias", bias),
                     ("loss", loss.detach()), ("grad_feat", g_x), ("grad_weight", g_w.reshape(C_out, F_in)),
                     ("grad_bias", g_b)):
            out[f"{name}.{k}"] = v.numpy()
        print(f"{name}: loss {loss.item():.15f}  |d feat| {g_x.norm().item():.6e}  |d W| {g_w.norm().item():.6e}")
    path = os.path.join(HERE, "feature_decoder.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
