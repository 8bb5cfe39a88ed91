#!/usr/bin/env python3
"""What pose gradients cost at the headline shape (300 000 Gaussians, 27
cameras of 800 x 800, F = 32, compat="fixed"): forward + backward of one
camera batch in three configurations, on the same device and inputs:

    (a) without camera tensors (the step as it was);
    (b) with viewmatrices / projmatrices / campos given and all three
        requiring grad (include/gs_camera_grad.h: two more kernels);
    (c) the only way to the same 27 pose gradients without them: one
        batch-of-one call per camera on means and rotations transformed by
        that camera's twist in PyTorch (the world transform w2c^-1 exp(xi) w2c
        of the means, its rotation as a quaternion product on the rotations).

A step is the forward(s) and one backward of sum(upstream x output) over
colour, depth and features down to the Gaussian leaves (and the camera
leaves in (b), the twists in (c)).  A sample is `--steps` steps (at least 20)
timed with a host clock between two device synchronisations; every shape is
warmed up first; the configurations alternate `--rounds` times in the same
process and every sample is recorded, with its spread.  (b) - (a) and
(c) / (b) are reported, not prescribed.

The camera kernels' own time is taken with device events around the binding's
camera call alone, on the scratch one backward left, `--kernel-reps` times,
and set against the byte model of gs_camera_grad.hip: 100 B per (camera,
Gaussian) pair at 8 TB/s.

`--configs a` runs (a) alone and needs nothing of this feature: run from a
checkout of the parent commit in the same session, alternating with this
checkout, it gives the parent's own run-to-run range, which `--parent` and
`--a-alone` (those runs' records, one line per process) and `--headline` /
`--parent-headline` (bench.py result lines of both checkouts, one per run)
merge into the record (`--record`: merge into an earlier run's record).  The
measurement runs in a child process under a time limit.  One JSON record,
written to --out (default profiles/camera_grad/bench.json).

    python tools/camera_grad_bench.py [--steps 20] [--warmup 3] [--rounds 3]
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

BYTES_PER_PAIR = 100  # the 64-B accumulation record, conic, radius, mean and covariance (gs_camera_grad.hip)
PEAK_BYTES_PER_S = 8e12


def quat_mul(a, b):
    import torch
    ar, ax, ay, az = a.unbind(-1)
    br, bx, by, bz = b.unbind(-1)
    return torch.stack([ar * br - ax * bx - ay * by - az * bz, ar * bx + ax * br + ay * bz - az * by,
                        ar * by - ax * bz + ay * br + az * bx, ar * bz + ax * by - ay * bx + az * br], -1)


def run(a):
    import numpy as np
    import torch
    from dynamic3dgaussians_amd import _C
    from dynamic3dgaussians_amd.camera import camera_rig
    from dynamic3dgaussians_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizerBatch
    from dynamic3dgaussians_amd.scene import make_gaussians
    if not torch.cuda.is_available():
        raise SystemExit("camera_grad_bench needs a HIP device: nothing is measured without one")
    dev = torch.device("cuda", 0)
    P, F, C, W, H = a.points, a.features, a.cams, a.width, a.height
    g = make_gaussians(P, F=F, seed=0, device=dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    rn = lambda *s: torch.randn(*s, device=dev, generator=gen)  # noqa: E731
    cams = camera_rig(C, W, H)
    bg = torch.zeros(3, device=dev)
    sets = [GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=c.tanfovx, tanfovy=c.tanfovy, c_x=c.c_x, c_y=c.c_y, bg=bg,
        viewmatrix=torch.from_numpy(c.viewmatrix.copy()).to(dev),
        projmatrix=torch.from_numpy(c.projmatrix.copy()).to(dev), sh_degree=0,
        campos=torch.from_numpy(c.campos.copy()).to(dev), compat="fixed") for c in cams]
    ups = {"color": rn(C, 3, H, W), "depth": 0.1 * rn(C, 1, H, W), "feature": rn(C, F, H, W)}
    names = {"means3D": "means3D", "colors_precomp": "colors", "opacities": "opacities", "scales": "scales",
             "rotations": "rotations", "semantic_feature": "semantic_feature"}
    leaves = {k: g[v].clone().requires_grad_(True) for k, v in names.items()}
    m2 = torch.zeros(P, 3, device=dev)
    label = torch.ones(P, device=dev)
    ras = GaussianRasterizerBatch(sets)
    steps, extra = {}, []

    def step_a():
        im, radii, feat, depth, alpha = ras(means2D=m2, label=label, **leaves)
        torch.autograd.backward([im, depth, feat], [ups["color"], ups["depth"], ups["feature"]])
    steps["a_no_camera_tensors"] = step_a

    if "b" in a.configs:
        camt = [torch.from_numpy(np.stack([getattr(c, n) for c in cams])).to(dev).requires_grad_(True)
                for n in ("viewmatrix", "projmatrix", "campos")]
        extra += camt

        def step_b():
            im, radii, feat, depth, alpha = ras(means2D=m2, label=label, **leaves, viewmatrices=camt[0],
                                                projmatrices=camt[1], campos=camt[2])
            torch.autograd.backward([im, depth, feat], [ups["color"], ups["depth"], ups["feature"]])
        steps["b_camera_gradients"] = step_b

    if "c" in a.configs:
        ones = [GaussianRasterizerBatch([s]) for s in sets]
        w2c = torch.from_numpy(np.stack([c.viewmatrix.T for c in cams])).to(dev)
        c2w = torch.linalg.inv(w2c.double().cpu()).float().to(dev)
        twist = (1e-3 * rn(C, 6)).requires_grad_(True)  # not at zero: theta / theta in the quaternion below
        extra.append(twist)
        rest = {k: v for k, v in leaves.items() if k not in ("means3D", "rotations")}

        def step_c():
            r, t = twist[:, :3], twist[:, 3:]
            xi = twist.new_zeros(C, 4, 4)
            xi[:, 0, 1], xi[:, 0, 2], xi[:, 1, 2] = -r[:, 2], r[:, 1], -r[:, 0]
            xi[:, 1, 0], xi[:, 2, 0], xi[:, 2, 1] = r[:, 2], -r[:, 1], r[:, 0]
            xi[:, :3, 3] = t
            G = c2w @ torch.linalg.matrix_exp(xi) @ w2c  # the scene's world transform per camera
            th = r.norm(dim=1, keepdim=True)
            axis = (w2c[:, :3, :3].transpose(1, 2) @ r[:, :, None]).squeeze(-1)
            qG = torch.cat([torch.cos(th / 2), torch.sin(th / 2) / th * axis], 1)
            outs, grs = [], []
            for c in range(C):
                means = leaves["means3D"] @ G[c, :3, :3].T + G[c, :3, 3]
                rots = quat_mul(qG[c][None], leaves["rotations"])
                im, radii, feat, depth, alpha = ones[c](means3D=means, means2D=m2, label=label, rotations=rots, **rest)
                outs += [im, depth, feat]
                grs += [ups["color"][c:c + 1], ups["depth"][c:c + 1], ups["feature"][c:c + 1]]
            torch.autograd.backward(outs, grs)
        steps["c_per_camera_transformed_scene"] = step_c

    def clear():
        for t in list(leaves.values()) + extra:
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

    for fn in steps.values():  # every shape warmed up
        for _ in range(a.warmup):
            clear()
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in steps}
    for _ in range(a.rounds):
        for k, fn in steps.items():
            ms[k].append(round(sample(fn), 4))
    med = {k: statistics.median(v) for k, v in ms.items()}
    rec = {"bench": "camera_grad", "P": P, "F": F, "C": C, "width": W, "height": H, "compat": "fixed",
           "steps_per_sample": a.steps, "warmup_steps": a.warmup, "rounds": a.rounds,
           "timing": "host clock between device synchronisations, ms per step (forward + backward)",
           "ms_per_step_runs": ms, "ms_per_step_median": {k: round(v, 4) for k, v in med.items()},
           "ms_per_step_range": {k: [min(v), max(v)] for k, v in ms.items()},
           "spread_max_minus_min_over_median": {k: round((max(v) - min(v)) / statistics.median(v), 4)
                                                for k, v in ms.items()}}
    if "b" in a.configs:
        rec["b_minus_a_ms"] = round(med["b_camera_gradients"] - med["a_no_camera_tensors"], 4)
        # the camera kernels alone: device events around the binding's call on one backward's records
        none = torch.Tensor([]).to(dev)
        v, p, cp = (t.detach() for t in camt)
        scal = ([c.c_x for c in cams], [c.c_y for c in cams], [c.tanfovx for c in cams], [c.tanfovy for c in cams])
        d = {k: t.detach() for k, t in leaves.items()}
        NR, color, fmap, depth, alpha, radii, geom, binning, img, NI = _C.rasterize_gaussians_batch(
            bg, d["means3D"], d["colors_precomp"], d["semantic_feature"], d["opacities"], d["scales"], d["rotations"],
            1.0, none, v, p, *scal, H, W, none, 0, cp, False, False, compat="fixed")
        scratch = _C.batch_backward_scratch(d["means3D"], d["semantic_feature"], C)
        _C.rasterize_gaussians_batch_backward(
            bg, d["means3D"], radii, d["colors_precomp"], d["semantic_feature"], d["scales"], d["rotations"], 1.0,
            none, v, p, *scal, ups["color"], ups["feature"], ups["depth"], None, none, 0, cp, geom, NI, binning, img,
            alpha, False, compat="fixed", scratch=scratch)
        call = lambda: _C.rasterize_gaussians_batch_camera_grad(  # noqa: E731
            bg, d["means3D"], radii, none, v, p, *scal, H, W, none, 0, cp, geom, scratch, compat="fixed")
        for _ in range(3):
            call()
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
               for _ in range(a.kernel_reps)]
        for e0, e1 in evs:
            e0.record()
            call()
            e1.record()
        torch.cuda.synchronize()
        kt = sorted(e0.elapsed_time(e1) for e0, e1 in evs)
        pairs = P * C
        visible = int((radii > 0).sum())
        kmed = statistics.median(kt)
        rec["camera_kernels"] = {
            "timing": "device events around the binding's camera call (partial + finishing kernel, its allocations "
                      "and launches), ms",
            "reps": a.kernel_reps, "ms_median": round(kmed, 4), "ms_min": round(kt[0], 4), "ms_max": round(kt[-1], 4),
            "pairs": pairs, "visible_pairs": visible,
            "byte_model": f"{BYTES_PER_PAIR} B per pair", "model_bytes": BYTES_PER_PAIR * pairs,
            "model_floor_ms_at_8TBps": round(BYTES_PER_PAIR * pairs / PEAK_BYTES_PER_S * 1e3, 4),
            "share_of_8TBps": round(BYTES_PER_PAIR * pairs / (kmed * 1e-3) / PEAK_BYTES_PER_S, 4)}
    if "c" in a.configs and "b" in a.configs:
        rec["c_over_b"] = round(med["c_per_camera_transformed_scene"] / med["b_camera_gradients"], 4)
    return rec


def _lines(path):
    """The JSON records of a file of result lines (bench.py prints one per run)."""
    out = []
    with open(path) as f:
        for ln in f:
            ln = ln.strip()
            if ln.startswith("{"):
                out.append(json.loads(ln))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--points", type=int, default=300_000)
    ap.add_argument("--features", type=int, default=32)
    ap.add_argument("--cams", type=int, default=27)
    ap.add_argument("--width", type=int, default=800)
    ap.add_argument("--height", type=int, default=800)
    ap.add_argument("--kernel-reps", type=int, default=50)
    ap.add_argument("--configs", default="abc", help="which of a, b, c to run (a always runs)")
    ap.add_argument("--parent", default="", help="records of `--configs a` runs from a checkout of the parent commit, "
                                                 "one JSON line per process")
    ap.add_argument("--a-alone", default="", help="records of `--configs a` runs of this checkout, one line per process")
    ap.add_argument("--record", default="", help="merge only: the record of an earlier run of this tool")
    ap.add_argument("--headline", default="", help="bench.py result lines of this checkout, one per run")
    ap.add_argument("--parent-headline", default="", help="bench.py result lines of the parent's checkout")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "camera_grad", "bench.json"))
    ap.add_argument("--timeout", type=int, default=540)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:  # the measurement, in its own process: print its record
        print("RECORD " + json.dumps(run(a)), flush=True)
        return 0
    if a.steps < 20:
        ap.error("--steps must be at least 20")
    if a.record:  # merge only: a record measured earlier in the same session
        rec = _lines(a.record)[-1]
    else:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--configs", a.configs]
        for k in ("steps", "warmup", "rounds", "points", "features", "cams", "width", "height", "kernel_reps"):
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
        rec = json.loads(recs[-1])
    k = "a_no_camera_tensors"
    if a.parent:
        # (a) alone, one process per record, the two checkouts alternating: the parent's range over all of its
        # samples is its run-to-run range (a process's three samples agree far better than two processes do)
        theirs = [x["ms_per_step_runs"][k] for x in _lines(a.parent)]
        mine = [x["ms_per_step_runs"][k] for x in _lines(a.a_alone)] if a.a_alone else [rec["ms_per_step_runs"][k]]
        lo, hi = min(min(v) for v in theirs), max(max(v) for v in theirs)
        mlo, mhi = min(min(v) for v in mine), max(max(v) for v in mine)
        med = lambda runs: [round(statistics.median(v), 4) for v in runs]  # noqa: E731
        rec["a_alone_vs_parent_commit"] = {
            "protocol": "--configs a in a process of its own, this checkout and the parent's alternating",
            "runs_per_process": mine, "range": [mlo, mhi], "median_per_process": med(mine),
            "parent_runs_per_process": theirs, "parent_range": [lo, hi], "parent_median_per_process": med(theirs),
            "inside_parent_range": lo <= mlo and mhi <= hi, "ranges_overlap": not (mhi < lo or hi < mlo),
            "median_of_medians_ms": [round(statistics.median(med(mine)), 4), round(statistics.median(med(theirs)), 4)]}
    if a.headline and a.parent_headline:
        mine = [x["ms_per_step"] for x in _lines(a.headline)]
        theirs = [x["ms_per_step"] for x in _lines(a.parent_headline)]
        rec["bench_py_headline"] = {
            "protocol": "bench.py --gpus 1 --steps 20 --warmup 5, the two checkouts alternating, ms per step",
            "runs": mine, "range": [min(mine), max(mine)], "median": round(statistics.median(mine), 4),
            "parent_runs": theirs, "parent_range": [min(theirs), max(theirs)],
            "parent_median": round(statistics.median(theirs), 4),
            "inside_parent_range": min(theirs) <= min(mine) and max(mine) <= max(theirs),
            "ranges_overlap": not (max(mine) < min(theirs) or max(theirs) < min(mine)),
            "Mpix_per_s_runs": [x["value"] for x in _lines(a.headline)],
            "parent_Mpix_per_s_runs": [x["value"] for x in _lines(a.parent_headline)]}
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
