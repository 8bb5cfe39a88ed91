#!/usr/bin/env python3
"""Generate tests/golden/scene_loss.npz from the REFERENCE's own statements
(run where the reference checkout exists; the fixture -- data only -- is
committed, the reference never travels).

The reference's floor / bg / soft_col_cons terms are eight lines of get_loss,
train.py:275-282: clamp and mean of the foreground heights, boolean indexing of
the means and rotations by ~is_fg, l1_loss_v2 against the background's initial
state, l1_loss_v2 of the colours against the previous timestep's.  They are
statements inside a function, not a function, so this script reads that slice
out of the checkout at run time (after checking that it begins and ends where
expected), and executes it in a namespace that supplies what the statements
name: torch, fg_pts, rendervar, is_fg, variables, params, losses.  l1_loss_v2
is read out of helpers.py:114-115 the same way.  Nothing of the reference's
text is stored here.

Everything runs in fp64 on the CPU; the inputs are stored as the fp32 values
they were drawn as.  Recorded per case: means3D, rotations (unit quaternions),
rgb_colors, is_fg, init_bg_pts, init_bg_rot, prev_col, the three losses, the
upstream weights `up` and the autograd gradients of sum_k up[k] * loss[k] with
respect to the three full tables.

Cases (all seeded):
  tiny    P = 7, 3 fg: one fg row at y exactly 0, one at y < 0, one bg
          coordinate exactly on its anchor, one colour exactly prev_col
  mixed   P = 1000, about 40 % fg
  all_fg  P = 5, no background: the bg loss is the mean of an empty set (NaN);
          the gradients are what autograd gives there

Usage: python tests/golden/make_golden_scene_loss.py --reference <reference checkout>
"""
from __future__ import annotations

import argparse
import os
import textwrap

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ("tiny", "mixed", "all_fg")
FIRST, LAST = 275, 282  # train.py, 1-based, inclusive
L1_FIRST, L1_LAST = 114, 115  # helpers.py
UP = (0.7, -1.3, 2.1)  # distinct, one negative: a swapped or dropped term shows
NAMES = ("floor", "bg", "soft_col_cons")


def case_inputs(name):
    gen = torch.Generator().manual_seed({"tiny": 41, "mixed": 42, "all_fg": 43}[name])
    P = {"tiny": 7, "mixed": 1000, "all_fg": 5}[name]
    if name == "tiny":
        is_fg = torch.tensor([True, False, True, False, False, True, False])
    elif name == "mixed":
        is_fg = torch.rand(P, generator=gen) < 0.4
    else:
        is_fg = torch.ones(P, dtype=torch.bool)
    means = torch.randn(P, 3, generator=gen).float()
    rot = torch.nn.functional.normalize(torch.randn(P, 4, generator=gen).float())
    col = torch.rand(P, 3, generator=gen).float()
    n_bg = int((~is_fg).sum())
    bg_pts = (means[~is_fg] + 0.05 * torch.randn(n_bg, 3, generator=gen)).float()
    bg_rot = torch.nn.functional.normalize(rot[~is_fg] + 0.05 * torch.randn(n_bg, 4, generator=gen)).float()
    prev_col = (col + 0.05 * torch.randn(P, 3, generator=gen)).float()
    if name == "tiny":
        means[0, 1] = 0.0      # fg, y exactly 0: clamp passes the gradient
        means[2, 1] = -0.75    # fg, y < 0: no gradient
        means[5, 1] = 0.5      # fg, y > 0
        bg_pts[1, 2] = means[3, 2]    # bg row 3 (rank 1), z exactly on its anchor: sign 0
        prev_col[4, 0] = col[4, 0]    # a colour exactly on prev_col: sign 0
    return dict(means3D=means, rotations=rot, rgb_colors=col, is_fg=is_fg, init_bg_pts=bg_pts, init_bg_rot=bg_rot,
                prev_col=prev_col)


def _slice(path, first, last):
    with open(path) as fh:
        return fh.read().splitlines()[first - 1:last]


def reference_code(reference):
    lines = _slice(os.path.join(reference, "train.py"), FIRST, LAST)
    assert lines[0].strip().startswith("losses['floor'] = torch.clamp(fg_pts[:, 1], min=0)"), lines[0]
    assert lines[-1].strip().startswith("losses['soft_col_cons'] = l1_loss_v2(params['rgb_colors']"), lines[-1]
    assert any(s.strip().startswith("losses['bg'] = l1_loss_v2(bg_pts") for s in lines), lines
    l1 = _slice(os.path.join(reference, "helpers.py"), L1_FIRST, L1_LAST)
    assert l1[0].startswith("def l1_loss_v2(x, y):") and l1[1].strip().startswith("return"), l1
    return (compile(textwrap.dedent("\n".join(lines)), "train.py:%d-%d" % (FIRST, LAST), "exec"),
            compile("\n".join(l1), "helpers.py:%d-%d" % (L1_FIRST, L1_LAST), "exec"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference (train.py, helpers.py)")
    a = ap.parse_args()
    code, l1_code = reference_code(a.reference)
    helpers = {"torch": torch}
    exec(l1_code, helpers)
    out = {}
    for name in CASES:
        x = case_inputs(name)
        means = x["means3D"].double().requires_grad_(True)
        rot = x["rotations"].double().requires_grad_(True)
        col = x["rgb_colors"].double().requires_grad_(True)
        is_fg = x["is_fg"]
        ns = {"torch": torch, "l1_loss_v2": helpers["l1_loss_v2"], "is_fg": is_fg,
              "rendervar": {"means3D": means, "rotations": rot}, "params": {"rgb_colors": col},
              "variables": {k: x[k].double() for k in ("init_bg_pts", "init_bg_rot", "prev_col")},
              "fg_pts": means[is_fg],  # train.py:256
              "losses": {}}
        exec(code, ns)
        losses = [ns["losses"][k] for k in NAMES]
        total = sum(u * v for u, v in zip(UP, losses))
        grads = torch.autograd.grad(total, (means, rot, col))
        for k, v in x.items():
            out[f"{name}.{k}"] = v.numpy()
        out[f"{name}.losses"] = torch.stack([v.detach() for v in losses]).numpy()
        out[f"{name}.up"] = np.asarray(UP, np.float64)
        for k, g in zip(("grad_means3D", "grad_rotations", "grad_rgb_colors"), grads):
            assert g.dtype == torch.float64
            out[f"{name}.{k}"] = g.numpy()
        print(f"{name}: fg {int(is_fg.sum())}/{len(is_fg)}  losses {[float(v.detach()) for v in losses]}  "
              f"|grads| {[float(g.norm()) for g in grads]}")
    path = os.path.join(HERE, "scene_loss.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
