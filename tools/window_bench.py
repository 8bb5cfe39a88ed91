#!/usr/bin/env python3
"""A temporal-window training step's renderer, forward + backward, in its two
formulations on the same device, parameters and upstream gradients:

    (a) MotionBases.compute_means -> ONE windowed camera batch
        (GaussianRasterizerBatch(camera_frames=...), include/gs_window.h)
    (b) MotionBases.compute_means -> one GaussianRasterizerBatch per frame on
        positions[:, b].contiguous(), autograd summing the shared parameters

at a training run's size:

    P = 300 000 Gaussians, F = 32 feature channels, 800 x 800,
    a window of B = 6 frames x 4 cameras (C = 24),
    MotionBases with K = 20 bases of T = 150 frames, coefficients as logits

A step is compute_means, the forward(s) and one backward of sum(upstream x
output) over colour, depth and features down to the leaves (means, logits,
both bases, colours, opacities, scales, rotations, features).  A sample is
`--steps` steps (at least 20) timed with a host clock between two device
synchronisations; every shape is warmed up first (`--warmup` steps of each
formulation); (a) and (b) alternate `--rounds` times in the same process and
every sample is recorded.  Peak memory is the allocator's peak over the live
inputs during one step of each.  The record also holds the largest relative
L2 between (a)'s and (b)'s gradients (reordered camera sums; the blend's
float atomics differ from run to run in the last bits as well).  The
measurement runs in a child process under a time limit.  One JSON record,
written to --out (default profiles/window/bench.json).

    python tools/window_bench.py [--steps 20] [--warmup 3] [--rounds 3]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

T_FRAMES = 150


def inputs(a, dev):
    """The seeded scene: Gaussians in the unit cube under the dome rig, a motion model that moves them by a
    few percent of the scene per frame, upstream gradients per camera."""
    import torch
    from dynamic3dgaussians_amd.camera import camera_rig
    from dynamic3dgaussians_amd.rasterizer import GaussianRasterizationSettings
    from dynamic3dgaussians_amd.scene import make_gaussians
    P, F, K, B, W, H = a.points, a.features, a.bases, a.frames, a.width, a.height
    C = B * a.cams_per_frame
    g = make_gaussians(P, F=F, seed=0, device=dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    rn = lambda *s: torch.randn(*s, device=dev, generator=gen)  # noqa: E731
    ident = torch.tensor([1.0, 0, 0, 0, 1.0, 0], device=dev)
    params = {"means": g["means3D"], "logits": 2.0 * rn(P, K), "rots": ident + 0.02 * rn(K, T_FRAMES, 6),
              "transls": 0.03 * rn(K, T_FRAMES, 3), "colors_precomp": g["colors"], "opacities": g["opacities"],
              "scales": g["scales"], "rotations": g["rotations"], "semantic_feature": g["semantic_feature"]}
    ts = [T_FRAMES - 1 - 7 * b for b in range(B)]
    bg = torch.zeros(3, device=dev)
    sets = [GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=c.tanfovx, tanfovy=c.tanfovy, c_x=c.c_x, c_y=c.c_y, bg=bg,
        viewmatrix=torch.from_numpy(c.viewmatrix.copy()).to(dev),
        projmatrix=torch.from_numpy(c.projmatrix.copy()).to(dev), sh_degree=0,
        campos=torch.from_numpy(c.campos.copy()).to(dev), compat="reference") for c in camera_rig(C, W, H)]
    frames = [c // a.cams_per_frame for c in range(C)]
    ups = {"color": rn(C, 3, H, W), "depth": 0.1 * rn(C, 1, H, W), "feature": rn(C, F, H, W)}
    return params, ts, sets, frames, ups


def run(a):
    import torch
    from dynamic3dgaussians_amd import MotionBases
    from dynamic3dgaussians_amd.rasterizer import GaussianRasterizerBatch
    if not torch.cuda.is_available():
        raise SystemExit("window_bench needs a HIP device: nothing is measured without one")
    dev = torch.device("cuda", 0)
    params, ts, sets, frames, ups = inputs(a, dev)
    P, B, C = a.points, a.frames, len(frames)
    leaves = {k: v.clone().requires_grad_(True) for k, v in params.items() if k not in ("rots", "transls")}
    bases = MotionBases(params["rots"], params["transls"]).to(dev)
    label = torch.ones(P, device=dev)
    m2 = torch.zeros(P, 3, device=dev)
    shared = {k: leaves[k] for k in ("colors_precomp", "opacities", "scales", "rotations", "semantic_feature")}
    ras_window = GaussianRasterizerBatch(sets, camera_frames=frames)
    per_frame = [[c for c, f in enumerate(frames) if f == b] for b in range(B)]
    ras_frames = [GaussianRasterizerBatch([sets[c] for c in idx]) for idx in per_frame]
    ups_frames = [{k: v[idx].contiguous() for k, v in ups.items()} for idx in per_frame]

    def all_leaves():
        return list(leaves.values()) + [bases.params["rots"], bases.params["transls"]]

    def step_window():
        positions = bases.compute_means(ts, leaves["means"], leaves["logits"], softmax=True)
        im, radii, feat, depth, alpha = ras_window(means3D=positions, means2D=m2, label=label, **shared)
        torch.autograd.backward([im, depth, feat], [ups["color"], ups["depth"], ups["feature"]])

    def step_frames():
        positions = bases.compute_means(ts, leaves["means"], leaves["logits"], softmax=True)
        outs, grs = [], []
        for b in range(B):
            im, radii, feat, depth, alpha = ras_frames[b](means3D=positions[:, b].contiguous(), means2D=m2,
                                                         label=label, **shared)
            outs += [im, depth, feat]
            grs += [ups_frames[b]["color"], ups_frames[b]["depth"], ups_frames[b]["feature"]]
        torch.autograd.backward(outs, grs)

    steps = {"a_window": step_window, "b_per_frame": step_frames}

    def clear():
        for t in all_leaves():
            t.grad = None

    def sample(fn):
        clear()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            clear()
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / a.steps

    grads, peak = {}, {}
    for k, fn in steps.items():  # warm-up of every shape, the gradients for the comparison, the peak memory
        for _ in range(a.warmup):
            clear()
            fn()
        clear()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        fn()
        torch.cuda.synchronize()
        peak[k] = torch.cuda.max_memory_allocated(dev) - base
        names = list(leaves) + ["rots", "transls"]
        grads[k] = {n: t.grad.detach().clone() for n, t in zip(names, all_leaves())}
    rel = lambda x, y: float((x.double() - y.double()).norm() / y.double().norm().clamp_min(1e-30))  # noqa: E731
    rels = {n: rel(grads["a_window"][n], grads["b_per_frame"][n]) for n in grads["b_per_frame"]}
    del grads
    ms = {k: [] for k in steps}
    for _ in range(a.rounds):
        for k, fn in steps.items():
            ms[k].append(round(sample(fn), 4))
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = {k: round((max(v) - min(v)) / statistics.median(v), 4) for k, v in ms.items()}
    return {"bench": "window", "P": P, "F": a.features, "width": a.width, "height": a.height, "B": B, "C": C,
            "cams_per_frame": a.cams_per_frame, "K": a.bases, "T": T_FRAMES, "softmax": True,
            "steps_per_sample": a.steps, "warmup_steps": a.warmup, "rounds": a.rounds,
            "timing": "host clock between device synchronisations, ms per step (compute_means + forward + backward)",
            "ms_per_step_runs": ms, "ms_per_step_median": {k: round(v, 4) for k, v in med.items()},
            "spread_max_minus_min_over_median": spread,
            "b_over_a": round(med["b_per_frame"] / med["a_window"], 4),
            "ranges_overlap": not (max(ms["a_window"]) < min(ms["b_per_frame"])
                                   or max(ms["b_per_frame"]) < min(ms["a_window"])),
            "peak_bytes_over_inputs": peak,
            "gradient_rel_l2_a_vs_b": {n: float(f"{v:.3e}") for n, v in rels.items()},
            "gradient_rel_l2_a_vs_b_max": float(f"{max(rels.values()):.3e}")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--points", type=int, default=300_000)
    ap.add_argument("--features", type=int, default=32)
    ap.add_argument("--width", type=int, default=800)
    ap.add_argument("--height", type=int, default=800)
    ap.add_argument("--frames", type=int, default=6)
    ap.add_argument("--cams-per-frame", type=int, default=4)
    ap.add_argument("--bases", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "window", "bench.json"))
    ap.add_argument("--timeout", type=int, default=420)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:  # the measurement, in its own process: print its record
        print("RECORD " + json.dumps(run(a)), flush=True)
        return 0
    if a.steps < 20:
        ap.error("--steps must be at least 20")
    cmd = [sys.executable, os.path.abspath(__file__), "--child"]
    for k in ("steps", "warmup", "rounds", "points", "features", "width", "height", "frames", "cams_per_frame",
              "bases"):
        cmd += ["--" + k.replace("_", "-"), str(getattr(a, k))]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout, cwd=REPO)
    except subprocess.TimeoutExpired:
        print(f"no result within {a.timeout} s", file=sys.stderr)
        return 124
    recs = [ln[7:] for ln in r.stdout.splitlines() if ln.startswith("RECORD ")]
    if r.returncode != 0 or not recs:
        print(f"exit status {r.returncode}\n{r.stderr[-3000:]}", file=sys.stderr)
        return r.returncode or 1
    print(recs[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(recs[-1] + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
