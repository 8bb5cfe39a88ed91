#!/usr/bin/env python3
"""Generate tests/golden/pose_errors.npz from the REFERENCE's own
compute_pose_errors (metrics.py:46-79), run where the reference checkout
exists; the fixture -- data only -- is committed, the reference never travels.

The reference's metrics.py imports torchmetrics, which is not installed here:
it is imported under the stand-in of make_golden_metrics.py
(load_reference_metrics).  The poses are fp64 camera-to-world matrices; the
reference's own arithmetic (torch for the ATE, numpy for the relative errors)
produces every recorded value.

Cases (seeded):
  perturbed  N = 6 random rigid poses against copies perturbed by a random
             rotation of ~2 degrees and a translation of ~0.02
  identical  preds == targets: all three errors are 0
  pair       N = 2: a single relative pair

Usage: python tests/golden/make_golden_pose_errors.py --reference <reference checkout>
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

CASES = ("perturbed", "identical", "pair")


def _rotation(rng, angle):
    """A rotation by `angle` radians about a random axis (Rodrigues)."""
    k = rng.normal(size=3)
    k /= np.linalg.norm(k)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def _poses(rng, n):
    out = np.tile(np.eye(4), (n, 1, 1))
    for i in range(n):
        out[i, :3, :3] = _rotation(rng, rng.uniform(0.0, np.pi))
        out[i, :3, 3] = rng.normal(size=3) * 2.0
    return out


def _perturb(rng, poses, angle, shift):
    out = poses.copy()
    for i in range(len(poses)):
        out[i, :3, :3] = _rotation(rng, angle * rng.uniform(0.5, 1.5)) @ poses[i, :3, :3]
        out[i, :3, 3] = poses[i, :3, 3] + rng.normal(size=3) * shift
    return out


def case_inputs(name):
    """(preds, targets): [N, 4, 4] fp64 camera-to-world matrices."""
    rng = np.random.default_rng({"perturbed": 41, "identical": 42, "pair": 43}[name])
    n = 2 if name == "pair" else 6
    targets = _poses(rng, n)
    preds = targets.copy() if name == "identical" else _perturb(rng, targets, np.deg2rad(2.0), 0.02)
    return preds, targets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference (metrics.py)")
    a = ap.parse_args()
    from tests.golden.make_golden_metrics import load_reference_metrics
    R = load_reference_metrics(a.reference)
    out = {}
    for name in CASES:
        preds, targets = case_inputs(name)
        errs = R.compute_pose_errors(torch.from_numpy(preds), torch.from_numpy(targets))
        out[f"{name}.preds"], out[f"{name}.targets"] = preds, targets
        out[f"{name}.errors"] = np.array(errs, np.float64)  # ate, rpe_t, rpe_r (degrees)
        print(name, out[f"{name}.errors"])
    path = os.path.join(HERE, "pose_errors.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
