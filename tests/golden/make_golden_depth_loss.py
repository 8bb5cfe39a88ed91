#!/usr/bin/env python3
"""Generate tests/golden/depth_loss.npz from the REFERENCE's own statements
(run where the reference checkout exists; the fixture -- data only -- is
committed, the reference never travels).

The reference's depth term is ten lines of get_loss, dyn_train.py:256-265:
boolean indexing of the rendered depth and of the prior by the mask, clamp to
[near, far], reciprocal, standardisation of both sides, 1 - pearson_corrcoef.
They are statements inside a function, not a function, so this script reads
that slice out of the checkout at run time (after checking that it begins and
ends where expected), and executes it in a namespace that supplies what the
statements name: curr_data, im, top_mask, depth_pred, near, far, losses.
Nothing of the reference's text is stored here.

`pearson_corrcoef` comes from the torchmetrics package in the reference; the
namespace supplies the stand-in below instead, so this one step is pinned to
the textbook definition, not to that package.

Everything runs in fp64 on the CPU; the inputs are stored as the fp32 values
they were drawn as.  Recorded per case (one camera each): depth, target, mask
(uint8), near, far, the loss and its autograd gradient with respect to the
depth plane.

Cases (all seeded):
  tiny    3 x 5     no mask
  masked  37 x 53   a random 80 % mask
  gated   37 x 53   10 % of the depths at 80 (beyond far), 2 % at 0 (below
                    near), an 80 % mask

Usage: python tests/golden/make_golden_depth_loss.py --reference <reference checkout>
"""
from __future__ import annotations

import argparse
import os
import textwrap

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ("tiny", "masked", "gated")
FIRST, LAST = 256, 265  # dyn_train.py, 1-based, inclusive
NEAR, FAR = 1e-7, 50.0  # dyn_train.py:20


def pearson_corrcoef(preds, target):
    """Stand-in for torchmetrics.functional.pearson_corrcoef, pinned to the definition of the
    Pearson correlation coefficient (not to the torchmetrics package, which is not needed to
    generate the fixture): covariance over the product of the standard deviations, clamped to
    [-1, 1]."""
    x, y = preds.reshape(-1), target.reshape(-1)
    dx, dy = x - x.mean(), y - y.mean()
    r = (dx * dy).sum() / (torch.sqrt((dx * dx).sum()) * torch.sqrt((dy * dy).sum()))
    return torch.clamp(r, -1.0, 1.0)


def _smooth(gen, h, w):
    """A low-frequency pattern plus a little noise, in [0.2, 0.8] roughly."""
    yy, xx = torch.meshgrid(torch.linspace(0, 1, h), torch.linspace(0, 1, w), indexing="ij")
    f = torch.rand(4, generator=gen) * 6.0
    base = 0.5 + 0.25 * torch.sin(f[0] * xx + f[1]) * torch.cos(f[2] * yy + f[3])
    return (base + 0.05 * torch.randn(h, w, generator=gen)).float()


def case_inputs(name):
    gen = torch.Generator().manual_seed({"tiny": 21, "masked": 22, "gated": 23}[name])
    h, w = (3, 5) if name == "tiny" else (37, 53)
    depth = (1.0 + 9.0 * _smooth(gen, h, w).clamp(0.0, 1.0)).float()  # depths of about 1 to 10
    scale = 1.7  # a monocular prior knows the inverse depth up to scale, plus noise
    target = (1.0 / (scale * depth) + 0.02 * torch.randn(h, w, generator=gen)).float()
    mask = torch.ones(h, w, dtype=torch.uint8)
    if name != "tiny":
        mask = (torch.rand(h, w, generator=gen) < 0.8).to(torch.uint8)
    if name == "gated":
        u = torch.rand(h, w, generator=gen)
        depth[u < 0.10] = 80.0
        depth[u > 0.98] = 0.0
    return depth, target, mask


def reference_statements(reference):
    with open(os.path.join(reference, "dyn_train.py")) as fh:
        lines = fh.read().splitlines()[FIRST - 1:LAST]
    assert lines[0].strip().startswith("ground_truth_depth = curr_data['depth']"), lines[0]
    assert "pearson_corrcoef(" in lines[-1] and lines[-1].strip().startswith("losses['depth']"), lines[-1]
    return compile(textwrap.dedent("\n".join(lines)), "dyn_train.py:%d-%d" % (FIRST, LAST), "exec")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference (dyn_train.py)")
    a = ap.parse_args()
    code = reference_statements(a.reference)
    out = {}
    for name in CASES:
        depth, target, mask = case_inputs(name)
        d = depth.double().requires_grad_(True)
        ns = {"torch": torch, "pearson_corrcoef": pearson_corrcoef, "curr_data": {"depth": target.double()},
              "im": torch.zeros(3, *depth.shape, dtype=torch.float64), "top_mask": mask, "depth_pred": d[None],
              "near": NEAR, "far": FAR, "losses": {"depth": 0}}
        exec(code, ns)
        loss = ns["losses"]["depth"]
        (g,) = torch.autograd.grad(loss, d)
        assert loss.dtype == torch.float64 and g.dtype == torch.float64 and g.shape == depth.shape
        for k, v in (("depth", depth), ("target", target), ("mask", mask), ("near", torch.tensor(NEAR, dtype=torch.float64)),
                     ("far", torch.tensor(FAR, dtype=torch.float64)), ("loss", loss.detach()), ("grad_depth", g)):
            out[f"{name}.{k}"] = v.numpy()
        print(f"{name}: loss {loss.item():.12f}  |grad| {g.norm().item():.6e}  masked {int(mask.sum())}")
    path = os.path.join(HERE, "depth_loss.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
