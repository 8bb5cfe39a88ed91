#!/usr/bin/env python3
"""The reference's `if not is_initial_timestep:` block (train.py:253-282), forward + backward, in
two formulations on the same device, timed as interleaved runs:

  boolean   how a caller must write the block without scene_loss: x[is_fg] / x[~is_fg] boolean
            indexing, neighbor.neighbor_losses on the gathered rows, the floor / bg / colour
            terms in torch (scene_loss.regularizer_losses_torch)
  hip       scene_loss.reference_extra_loss(): the cached split, gather_foreground,
            neighbor_losses, regularizer_losses

Shape: P = 300k rows, 50 % foreground, K = 20 (a synthetic graph of the reference's shape, as
tools/neighbor_bench.py).  Per formulation: wall time (host clock around work that ends in a
device synchronise), device time (HIP events around the same work), both per call as the median
and the range over the rounds, and the number of host-synchronising calls one forward + backward
makes (torch.cuda.set_sync_debug_mode("warn"), counted warnings).  Then the 4-camera step of
timesteps.TimestepDriver (one rank's share of the 27-camera rig over 8 ranks) with each
formulation as its extra_loss, and with none.  Writes profiles/scene_loss/bench.json.

    python tools/scene_loss_bench.py
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
import warnings

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from dynamic3dgaussians_amd import _lib  # noqa: E402
from dynamic3dgaussians_amd.camera import camera_rig  # noqa: E402
from dynamic3dgaussians_amd.neighbor import neighbor_losses  # noqa: E402
from dynamic3dgaussians_amd.optim import FusedAdam  # noqa: E402
from dynamic3dgaussians_amd.rasterizer import GaussianRasterizationSettings  # noqa: E402
from dynamic3dgaussians_amd.scene import make_gaussians  # noqa: E402
from dynamic3dgaussians_amd.scene_loss import WEIGHTS, reference_extra_loss, regularizer_losses_torch  # noqa: E402
from dynamic3dgaussians_amd.timesteps import TimestepDriver, batch_renderer, params2rendervar  # noqa: E402

LRS = {"means3D": 1.6e-4, "rgb_colors": 2.5e-3, "unnorm_rotations": 1e-3, "logit_opacities": 0.05,
       "log_scales": 1e-3}  # train.py:119-135
LEAVES = ("means3D", "unnorm_rotations", "rgb_colors")


def boolean_extra_loss(params, variables, rv, t):
    """The block with boolean indexing: four gathers, each a nonzero the host waits for."""
    if t == 0 or "neighbor_indices" not in variables:
        return None
    w = WEIGHTS
    is_fg = (params["seg_colors"][:, 0] > 0.5).detach()
    rigid, rot, iso = neighbor_losses(rv["means3D"][is_fg], rv["rotations"][is_fg], variables)
    floor, bg, col = regularizer_losses_torch(rv["means3D"], rv["rotations"], params["rgb_colors"], variables, is_fg)
    return (w["rigid"] * rigid + w["rot"] * rot + w["iso"] * iso + w["floor"] * floor + w["bg"] * bg
            + w["soft_col_cons"] * col)


def build(P, K, fg_fraction, seed, dev):
    """The parameters of a synthetic scene with seg colours, and the `variables` the reference holds
    after timestep 0 (graph, previous-timestep state, background anchors), a little off the
    current state."""
    g = make_gaussians(P, seed=seed, device=dev)
    gen = torch.Generator(device=dev).manual_seed(seed + 11)
    seg = torch.zeros(P, 3, device=dev)
    seg[:, 0] = (torch.rand(P, device=dev, generator=gen) < fg_fraction).float()
    base = {"means3D": g["means3D"], "rgb_colors": g["colors"],
            "unnorm_rotations": g["rotations"] * (0.5 + torch.rand(P, 1, device=dev, generator=gen)),
            "logit_opacities": torch.logit(g["opacities"]), "log_scales": torch.log(g["scales"]), "seg_colors": seg}
    is_fg = seg[:, 0] > 0.5
    fg_pts, fg_rot = base["means3D"][is_fg], g["rotations"][is_fg]
    N = fg_pts.shape[0]
    off = torch.randint(1, 64, (N, K), device=dev, generator=gen)
    nbr = (torch.arange(N, device=dev)[:, None] + off) % N
    prev_pts = fg_pts + 0.01 * torch.randn(N, 3, device=dev, generator=gen)
    inv = torch.nn.functional.normalize(fg_rot + 0.05 * torch.randn(N, 4, device=dev, generator=gen))
    inv[:, 1:] = -inv[:, 1:]
    rot = g["rotations"]
    variables = {
        "neighbor_indices": nbr.long().contiguous(),
        "neighbor_weight": torch.rand(N, K, device=dev, generator=gen),
        "neighbor_dist": (fg_pts[nbr] - fg_pts[:, None]).norm(dim=-1).contiguous(),
        "prev_inv_rot_fg": inv.contiguous(),
        "prev_offset": (prev_pts[nbr] - prev_pts[:, None]).contiguous(),
        "init_bg_pts": (base["means3D"][~is_fg] + 0.01 * torch.randn(P - N, 3, device=dev, generator=gen)).contiguous(),
        "init_bg_rot": torch.nn.functional.normalize(
            rot[~is_fg] + 0.05 * torch.randn(P - N, 4, device=dev, generator=gen)).contiguous(),
        "prev_col": (base["rgb_colors"] + 0.05 * torch.randn(P, 3, device=dev, generator=gen)).contiguous()}
    return base, variables, N


def sync_calls(fn) -> int:
    """Host-synchronising calls one fn() makes, as torch's sync debug mode reports them."""
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode(before)
    torch.cuda.synchronize()
    return sum("called a synchronizing" in str(w.message) for w in seen)


def timed(fn, reps):
    """(wall ms, device ms) per call of `reps` back-to-back calls."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps, e0.elapsed_time(e1) / reps


def summary(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def interleaved(fns: dict, reps, rounds):
    """Every formulation warmed up, then `rounds` rounds that time each formulation in turn."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    wall = {k: [] for k in fns}
    device = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            w, d = timed(fn, reps)
            wall[k].append(w)
            device[k].append(d)
    return {k: {"wall_ms": summary(wall[k]), "device_ms": summary(device[k])} for k in fns}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaussians", type=int, default=300_000)
    ap.add_argument("--fg", type=float, default=0.5, help="foreground fraction")
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--reps", type=int, default=50, help="calls per timed window")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--cams", type=int, default=4, help="cameras of the rank step (0: skip it)")
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--steps", type=int, default=20, help="rank steps per timed window")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "scene_loss", "bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("scene_loss_bench needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    _lib.load()
    base, variables, n_fg = build(a.gaussians, a.k, a.fg, a.seed, dev)
    forms = {"boolean": boolean_extra_loss, "hip": reference_extra_loss()}

    # ---- the block alone
    params = {k: v.clone().requires_grad_(k in LEAVES) for k, v in base.items()}
    leaves = [params[k] for k in LEAVES]
    var = {k: dict(variables) for k in forms}  # a cache of its own per formulation

    def block(name):
        def run():
            rv = {"means3D": params["means3D"], "rotations": torch.nn.functional.normalize(params["unnorm_rotations"])}
            torch.autograd.grad(forms[name](params, var[name], rv, 1), leaves)
        return run

    fns = {k: block(k) for k in forms}
    result = {"shape": {"P": a.gaussians, "n_fg": n_fg, "K": a.k}, "reps": a.reps, "rounds": a.rounds,
              "device": torch.cuda.get_device_name(dev), "torch": torch.__version__,
              "block_fwd_bwd": interleaved(fns, a.reps, a.rounds)}
    for k in forms:
        result["block_fwd_bwd"][k]["host_sync_calls"] = sync_calls(fns[k])
    b, h = (result["block_fwd_bwd"][k] for k in ("boolean", "hip"))
    result["block_fwd_bwd"]["boolean_over_hip"] = {
        "wall": round(b["wall_ms"]["median"] / h["wall_ms"]["median"], 3),
        "device": round(b["device_ms"]["median"] / h["device_ms"]["median"], 3)}
    print(json.dumps(result["block_fwd_bwd"]), flush=True)

    # ---- the rank step: `cams` cameras through TimestepDriver, each formulation as its extra_loss
    if a.cams > 0:
        W = H = a.size
        rig = camera_rig(a.cams, W, H, seed=a.seed)
        settings = [GaussianRasterizationSettings(
            image_height=H, image_width=W, tanfovx=c.tanfovx, tanfovy=c.tanfovy, c_x=c.c_x, c_y=c.c_y,
            bg=torch.zeros(3, device=dev), viewmatrix=torch.from_numpy(c.viewmatrix.copy()).to(dev),
            projmatrix=torch.from_numpy(c.projmatrix.copy()).to(dev), sh_degree=0,
            campos=torch.from_numpy(c.campos.copy()).to(dev), compat="reference") for c in rig]
        render = batch_renderer(settings)
        with torch.no_grad():
            tg, _ = render(params2rendervar(base), list(range(a.cams)))
            tg = tg.detach().clone()
        drivers = {}
        for name, extra in (("none", None), *forms.items()):
            p = {k: torch.nn.Parameter(v.clone()) if k in LRS else v.clone() for k, v in base.items()}
            opt = FusedAdam([{"params": [p[k]], "name": k, "lr": lr} for k, lr in LRS.items()], lr=0.0, eps=1e-15)
            drivers[name] = TimestepDriver(p, dict(variables), opt, a.cams, render, extra_loss=extra)
        steps = {k: (lambda d=d: d.step(tg, 1, 0)) for k, d in drivers.items()}
        result["rank_step"] = {"cams": a.cams, "size": [W, H], "steps": a.steps,
                               "note": "TimestepDriver.step reads the loss back once per step in every row",
                               **interleaved(steps, a.steps, a.rounds)}
        r = result["rank_step"]
        r["boolean_over_hip_wall"] = round(r["boolean"]["wall_ms"]["median"] / r["hip"]["wall_ms"]["median"], 3)
        print(json.dumps(result["rank_step"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
