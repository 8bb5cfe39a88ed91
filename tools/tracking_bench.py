#!/usr/bin/env python3
"""What the tracking kernels cost at the headline shape (300 000 Gaussians, 27
cameras of 800 x 800, compat="fixed"; include/gs_track.h):

  * the contributor kernel (gs_contributors_batch) at K = 1 and K = 4, on the
    state of one batch forward: device events around `--reps` calls of the
    binding (its two output allocations and the launch included), ms per call;
  * the forward blend it repeats, render_fwd at F = 0, of the same scene in the
    same process: the library's live stage timing (gs_timing_*: the kernel's own
    start / end timestamps) over `--reps` forwards, ms per launch;
  * three samples of each, alternating (forward, K = 1, K = 4, forward, ...),
    every sample recorded; the ratios of the medians are reported, not
    prescribed;
  * the contributor kernel's bytes under its model -- every 64-B record and 4-B
    list id read once per strip (4 strips per tile) plus 8 K bytes per pixel
    written -- and the rate that makes of the measured time;
  * the projection kernel (gs_track_project) at N = 4096 tracks, T = 150
    timesteps, C = 27 cameras: device events around `--reps` calls.

Every shape is warmed up first.  Needs a HIP device: nothing is measured without
one.  One JSON record, printed and written to --out (default
profiles/tracking/bench.json).

    python tools/tracking_bench.py [--reps 20] [--rounds 3]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

REC_BYTES, ID_BYTES = 64, 4  # a render record and a list id (gs_common.h)


def run(a):
    import torch
    from dynamic3dgaussians_amd import _C, _lib
    from dynamic3dgaussians_amd.camera import camera_rig
    from dynamic3dgaussians_amd.scene import make_gaussians
    if not torch.cuda.is_available():
        raise SystemExit("tracking_bench needs a HIP device: nothing is measured without one")
    dev = torch.device("cuda", 0)
    P, C, W, H = a.points, a.cams, a.width, a.height
    g = make_gaussians(P, seed=0, device=dev)
    cams = camera_rig(C, W, H)
    bg = torch.zeros(3, device=dev)
    none = torch.Tensor([]).to(dev)
    import numpy as np
    v, p, cp = (torch.from_numpy(np.stack([getattr(c, n) for c in cams])).to(dev).reshape(C, -1)
                for n in ("viewmatrix", "projmatrix", "campos"))
    scal = ([c.c_x for c in cams], [c.c_y for c in cams], [c.tanfovx for c in cams], [c.tanfovy for c in cams])

    def forward():
        return _C.rasterize_gaussians_batch(bg, g["means3D"], g["colors"], None, g["opacities"], g["scales"],
                                            g["rotations"], 1.0, none, v, p, *scal, H, W, none, 0, cp, False, False,
                                            compat="fixed")

    NR, color, fmap, depth, alpha, radii, geom, binning, img, NI = forward()

    def contributors(K):
        return _C.rasterize_gaussians_batch_contributors(geom, binning, img, NI, *scal, bg, v, p, cp, H, W, P, K,
                                                         compat="fixed")

    def events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.reps

    def render_fwd_stage():
        torch.cuda.synchronize()
        _lib.timing_enable(True, stages=["render_fwd"])
        for _ in range(a.reps):
            forward()
        torch.cuda.synchronize()
        ms, n = _lib.timing_read()["render_fwd"]
        _lib.timing_enable(False)
        return ms / max(n, 1)

    for _ in range(3):  # every shape warmed up
        forward()
        contributors(1)
        contributors(4)
    torch.cuda.synchronize()
    runs = {"render_fwd_F0": [], "contributors_K1": [], "contributors_K4": []}
    for _ in range(a.rounds):
        runs["render_fwd_F0"].append(round(render_fwd_stage(), 4))
        runs["contributors_K1"].append(round(events(lambda: contributors(1)), 4))
        runs["contributors_K4"].append(round(events(lambda: contributors(4)), 4))
    med = {k: statistics.median(x) for k, x in runs.items()}
    instances = int(sum(NI))
    model = {f"K{K}": 4 * instances * (REC_BYTES + ID_BYTES) + 8 * K * C * H * W for K in (1, 4)}
    top_id, _ = contributors(1)
    rec = {"bench": "tracking", "P": P, "C": C, "width": W, "height": H, "compat": "fixed", "reps_per_sample": a.reps,
           "rounds": a.rounds, "list_instances": instances, "covered_pixel_share": round(float((top_id >= 0).float().mean()), 4),
           "timing": {"contributors": "device events around the binding's calls (allocations and launch included), "
                                      "ms per call",
                      "render_fwd_F0": "gs_timing_* stage time (the kernel's own timestamps), ms per launch"},
           "ms_runs": runs, "ms_median": {k: round(x, 4) for k, x in med.items()},
           "ms_range": {k: [min(x), max(x)] for k, x in runs.items()},
           "ratio_K1_over_render_fwd": round(med["contributors_K1"] / med["render_fwd_F0"], 4),
           "ratio_K4_over_render_fwd": round(med["contributors_K4"] / med["render_fwd_F0"], 4),
           "byte_model": "4 strips x list instances x (64-B record + 4-B id) + 8 K B per pixel",
           "model_bytes": model,
           "model_GBps": {k: round(b / (med["contributors_" + k] * 1e-3) / 1e9, 1) for k, b in model.items()}}
    # the projection kernel
    T, N = a.timesteps, a.tracks
    gen = torch.Generator(device=dev).manual_seed(2)
    means_T = g["means3D"][None] + 0.01 * torch.randn(T, 1, 3, device=dev, generator=gen)
    ids = torch.randint(0, P, (N,), device=dev, generator=gen, dtype=torch.int32)
    project = lambda: _C.track_project(means_T, ids, bg, v, p, *scal, cp, H, W)  # noqa: E731
    for _ in range(3):
        project()
    torch.cuda.synchronize()
    pr = [round(events(project), 4) for _ in range(a.rounds)]
    out_bytes = T * C * N * (8 + 4 + 1)
    rec["track_project"] = {"T": T, "C": C, "N": N, "timing": "device events around the binding's calls, ms per call",
                            "ms_runs": pr, "ms_median": round(statistics.median(pr), 4),
                            "bytes_written": out_bytes, "bytes_gathered": T * C * N * 12}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--points", type=int, default=300_000)
    ap.add_argument("--cams", type=int, default=27)
    ap.add_argument("--width", type=int, default=800)
    ap.add_argument("--height", type=int, default=800)
    ap.add_argument("--timesteps", type=int, default=150)
    ap.add_argument("--tracks", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "tracking", "bench.json"))
    a = ap.parse_args()
    rec = run(a)
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
