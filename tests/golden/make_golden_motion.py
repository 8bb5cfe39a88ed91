#!/usr/bin/env python3
"""Generate tests/golden/motion_bases.npz from the REFERENCE's own Python code
(run where the reference checkout exists; the fixture -- data only -- is
committed, the reference never travels).

The reference's motion_utils.py is loaded as a module.  Its cont_6d_to_rmat is
used as it is; MotionBases.compute_transforms is called as a plain function on
a stand-in `self` that has a `.params` dict, because the class's __init__
moves its tensors to a GPU.  That method overwrites its `ts` with
list(range(9)) and prints a line: the fixture therefore uses ts = 0..8 on
tables of T >= 9 frames, and stdout is silenced around the call.  The
positions are the einsum of dyn_train.py:427-431 over the transforms with the
means padded by one; the coefficient activation is F.softmax
(dyn_train.py:410).  Everything runs in fp64 on the CPU.

Cases (tests/_motion_cases.py: recipe, seeds and the conditioning margin, which
is asserted here):
  c200  G 200  K 7  T 12
  c64   G 64   K 1  T 9     one basis: softmax of one logit is 1

Recorded per case, fp64: the inputs (means, logits, coefs, rots, transls), ts,
the upstream weights w, and for both coefficient modes ("given": coefs as they
are, "softmax": softmax of logits) the transforms, the positions and the
gradients of sum(w * positions) in means, coefs (or logits), rots and transls.

Usage: python tests/golden/make_golden_motion.py --reference <reference checkout>
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
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import _motion_cases as mc  # noqa: E402
from tests.golden.make_golden import _load_module  # noqa: E402


def reference_outputs(mu, case, softmax, w):
    leaves = {k: case[k].clone().requires_grad_(True) for k in ("means", "rots", "transls")}
    raw = case["logits" if softmax else "coefs"].clone().requires_grad_(True)
    coefs = F.softmax(raw, dim=-1) if softmax else raw
    stand_in = types.SimpleNamespace(params={"rots": leaves["rots"], "transls": leaves["transls"]})
    with contextlib.redirect_stdout(io.StringIO()):
        transfms = mu.MotionBases.compute_transforms(stand_in, list(mc.FIXTURE_TS), coefs)
    positions = torch.einsum("pnij,pj->pni", transfms, F.pad(leaves["means"], (0, 1), value=1.0))
    grads = torch.autograd.grad((w * positions).sum(), (leaves["means"], raw, leaves["rots"], leaves["transls"]))
    return transfms.detach(), positions.detach(), dict(zip(mc.GRADS, grads))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=mc.GOLD)
    args = ap.parse_args()
    mu = _load_module("ref_motion_utils", os.path.join(args.reference, "motion_utils.py"))
    out = {}
    for name, (G, K, T, seed) in mc.FIXTURE_CASES.items():
        case = mc.make_case(G, K, T, seed)
        w = mc.weights(G, len(mc.FIXTURE_TS), seed)
        for k, v in case.items():
            assert v.dtype == torch.float64 and torch.equal(v, v.float().double())
            out[f"{name}.{k}"] = v.numpy()
        out[f"{name}.ts"] = np.asarray(mc.FIXTURE_TS, np.int32)
        out[f"{name}.w"] = w.numpy()
        for mode, softmax in mc.MODES.items():
            m = mc.margins(case, mc.FIXTURE_TS, softmax)
            print(f"{name} {mode}: min |x1| {m[0]:.3f}  min |u| {m[1]:.3f}  min sine {m[2]:.3f}")
            assert mc.margins_ok(case, mc.FIXTURE_TS, softmax), (name, mode, m)
            transfms, positions, grads = reference_outputs(mu, case, softmax, w)
            assert transfms.shape == (G, 9, 3, 4) and positions.shape == (G, 9, 3)
            out[f"{name}.{mode}.transforms"] = transfms.numpy()
            out[f"{name}.{mode}.positions"] = positions.numpy()
            for k, g in grads.items():
                out[f"{name}.{mode}.grad_{k}"] = g.numpy()
    assert all(v.dtype in (np.float64, np.int32) for v in out.values())
    np.savez_compressed(args.out, **out)
    print(f"wrote {args.out}: {os.path.getsize(args.out)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
