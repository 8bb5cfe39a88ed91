#!/usr/bin/env python3
"""Generate tests/golden/depth_geometry.npz from the REFERENCE's own Python code (run where
the reference checkout exists; the fixture -- data only -- is committed, the reference never
travels).

What is recorded, and from where:

  metrics.py   unproject_image (:131-213) on every camera of the z-buffer cases.  It is imported
               under the stand-in torchmetrics of make_golden_metrics.py.  Its save_depth_map is
               replaced by a function that captures the estimated depth map it is handed, and
               its prints are swallowed; the map and the returned score are recorded.  The
               function converts the cloud with .float(), so it runs in fp32 only: its matrices
               are given as fp32 and there is no fp64 record of it.
  ideaII.py    compute_optical_flow (:135-157), warp_flow (:159-198), accumulate_flows
               (:200-206) and resize_optical_flow (:219-257), in fp32 and in fp64 (they follow
               their inputs' dtype; torch.set_default_dtype is set to the run's dtype as well).
  dyn_utils.py depth2point_world (:469-480), in fp32 and fp64.  Its pixel ramp is
               torch.arange(..., dtype=torch.float32) / (W - 1) whatever the default dtype, so
               the fp64 record carries that fp32 round trip of the pixel index.

ideaII.py and dyn_utils.py import modules that are absent here or must not run (Open3D via
helpers, external, the rasterizer package, pytorch3d, torchvision, wandb, cv2, torchmetrics):
each is an inert stand-in in sys.modules while the module loads (_Inert below, a few lines of
our own).  Modules that are installed (PIL, tqdm, matplotlib) are imported as they are.  No
function recorded here touches a stand-in.

Parity unpinned: the 2-D track lifting of dyn_som.py:268-286.  That file is a fragment that
defines neither normalize_coords nor its imports and cannot be imported; nothing of it is
recorded, and depth_geometry.lift_tracks is tested against torch's grid_sample instead.

Inputs (tests/_depth_geometry_cases.py, seeded) are stored as the fp32 values drawn.

Usage: python tests/golden/make_golden_depth_geometry.py --reference <reference checkout>
"""
from __future__ import annotations

import argparse
import contextlib
import importlib.util
import io
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import _depth_geometry_cases as C  # noqa: E402

ALWAYS = ("helpers", "external", "diff_gaussian_rasterization")  # the reference's own neighbours: never run
IF_ABSENT = ("open3d", "pytorch3d", "pytorch3d.transforms", "torchvision", "torchvision.transforms",
             "torchvision.transforms.functional", "torchvision.utils", "wandb", "cv2", "torchmetrics",
             "torchmetrics.functional", "torchmetrics.functional.regression", "matplotlib", "matplotlib.pyplot",
             "PIL", "tqdm")
RESIZE_TO = (21, 40)  # from 37 x 53: neither axis an integer ratio


class _Inert(types.ModuleType):
    """A module whose every attribute is another inert module: `import a.b as c` and
    `from a import x, y` succeed, and nothing behind them can be used by accident."""

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Inert(f"{self.__name__}.{name}")

    def __call__(self, *a, **kw):
        raise RuntimeError(f"{self.__name__} is a stand-in: the reference code under record must not call it")


def _absent(name):
    try:
        return importlib.util.find_spec(name) is None
    except (ImportError, ValueError):
        return True


@contextlib.contextmanager
def stand_ins():
    names = list(ALWAYS) + [n for n in IF_ABSENT if _absent(n.split(".")[0])]
    saved = {n: sys.modules.get(n) for n in names}
    for n in names:
        sys.modules[n] = _Inert(n)
    try:
        yield
    finally:
        for n, m in saved.items():
            if m is None:
                sys.modules.pop(n, None)
            else:
                sys.modules[n] = m


def load_reference(reference):
    from tests.golden.make_golden import _load_module
    from tests.golden.make_golden_metrics import load_reference_metrics
    metrics = load_reference_metrics(reference)
    with stand_ins():
        idea = _load_module("ref_ideaII", os.path.join(reference, "ideaII.py"))
        dyn = _load_module("ref_dyn_utils", os.path.join(reference, "dyn_utils.py"))
    return metrics, idea, dyn


def record_zbuffer(R, out):
    captured = []
    R.save_depth_map = lambda depth_map, filename: captured.append(depth_map.detach().clone())
    R.os = types.SimpleNamespace(makedirs=lambda *a, **kw: None, path=os.path)  # no directory is made
    quiet = io.StringIO()
    for name, (H, W, P, _) in C.ZBUF_CASES.items():
        pts, w2c, K, gt, exclude = C.zbuf_case(name)
        out[f"{name}.points"], out[f"{name}.w2c"], out[f"{name}.K"] = pts.numpy(), w2c.float().numpy(), K.float().numpy()
        out[f"{name}.gt"], out[f"{name}.exclude"] = gt.numpy(), exclude.numpy()
        maps, scores = [], []
        for b in range(2):
            with contextlib.redirect_stdout(quiet):
                s = R.unproject_image(torch.zeros(H, W, 3), w2c[b].float(), K[b].float(), gt[b], exclude[b].float(),
                                      pts[b].numpy(), (W, H))
            maps.append(captured.pop().numpy())
            scores.append(float(s))
        out[f"{name}.est"], out[f"{name}.score"] = np.stack(maps), np.array(scores, np.float64)
        assert out[f"{name}.est"].dtype == np.float32 and out[f"{name}.est"].shape == (2, H, W)
        print(name, "filled", np.isfinite(out[f"{name}.est"]).sum(axis=(1, 2)), "score", scores)


def record_flow(I, D, out):  # noqa: E741
    for name, (H, W, seed) in C.FLOW_CASES.items():
        for away in (False, True):
            depth, K1, c2w1, K2, w2c2 = C.flow_case(name, away)
            key = name + ("_away" if away else "")
            out[f"{key}.depth"] = depth.numpy()
            for n, m in (("K1", K1), ("c2w1", c2w1), ("K2", K2), ("w2c2", w2c2)):
                out[f"{key}.{n}"] = m.float().numpy()
            for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
                torch.set_default_dtype(dt)
                flow = I.compute_optical_flow(depth.to(dt), K1.to(dt), c2w1.to(dt), None, K2.to(dt), w2c2.to(dt))
                assert flow.dtype == dt and flow.shape == (2, H, W)
                out[f"{key}.flow_{tag}"] = flow.numpy()
        depth, K1, c2w1, _, _ = C.flow_case(name)
        w2c1 = C.f32(torch.linalg.inv(c2w1))  # depth2point_world inverts its extrinsic itself
        out[f"{name}.w2c1"] = w2c1.float().numpy()
        for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
            torch.set_default_dtype(dt)
            xyz = D.depth2point_world(depth.to(dt), K1.to(dt), w2c1.to(dt))
            assert xyz.dtype == dt and xyz.shape == (H * W, 3)
            out[f"{name}.world_{tag}"] = xyz.reshape(H, W, 3).numpy()
        fl = C.flows(H, W, 3, seed + 10)
        out[f"{name}.flows"] = fl.numpy()
        for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
            torch.set_default_dtype(dt)
            out[f"{name}.warp_{tag}"] = I.warp_flow(fl[0].to(dt), fl[1].to(dt)).numpy()
            out[f"{name}.accumulate_{tag}"] = I.accumulate_flows([f.to(dt) for f in fl]).numpy()
            assert out[f"{name}.accumulate_{tag}"].dtype == (np.float32 if dt == torch.float32 else np.float64)
    H, W, seed = C.FLOW_CASES["flow_37x53"]
    fl = C.flows(H, W, 1, seed + 20)[0]
    out["resize.flow"] = fl.numpy()
    for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
        torch.set_default_dtype(dt)
        out[f"resize.out_{tag}"] = I.resize_optical_flow(fl.to(dt).clone(), RESIZE_TO).numpy()
    torch.set_default_dtype(torch.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference (metrics.py, ideaII.py, dyn_utils.py)")
    a = ap.parse_args()
    R, I, D = load_reference(a.reference)  # noqa: E741
    out = {}
    record_zbuffer(R, out)
    record_flow(I, D, out)
    path = os.path.join(HERE, "depth_geometry.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
