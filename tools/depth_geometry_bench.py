#!/usr/bin/env python3
"""What the depth-map geometry kernels cost at the shapes a user runs
(include/gs_depth_geometry.h, dynamic3dgaussians_amd/depth_geometry.py), each
against its `_torch` twin in fp32 on the same device:

  * mde        point_depth_maps + depth_abs_rel, 300 000 points x 27 cameras of
               800 x 800 (one shared cloud, an exclude mask per image); the twin's
               z-buffer is torch's scatter_reduce(amin), not the reference's loop
  * unproject  unproject_depth at 27 x 800 x 800
  * flow       depth_flow at 27 x 800 x 800 (with the valid map)
  * warp       warp_flow at 27 x 2 x 288 x 512

For each workload three timings, every sample device events around `--reps`
calls after a warm-up of every shape, `--rounds` samples of each taken
alternately (hip, entry, torch, hip, ...), medians and the range reported:

  hip     the Python function (its output allocations, matrix inverses and
          launches included): what a caller pays
  entry   the C entry point alone on preallocated outputs and prepared
          matrices: the kernels' own time, launch overhead included
  torch   the `_torch` twin in fp32

`model_bytes` is the HBM traffic of the byte model in the header, from shapes;
`fill_fraction` is model_bytes / entry time over the measured streaming rate
of the chip (6.29 TB/s, MI355X float4 copy).  For the z-buffer the model
counts one 4-byte atomic per landed point; what bounds that launch (the rate
of integer min atomics) is reported as measured time only.  Peak device
memory above the inputs is recorded for hip and torch.  The per-pixel Python
loop of the reference's manner (argsort, run boundaries, one .item() per
filled pixel) is timed once on the smallest fixture shape (5 x 7, P = 1000).

Needs a HIP device: nothing is measured without one.  One JSON record, printed
and written to --out (default profiles/depth_geometry/bench.json).

    python tools/depth_geometry_bench.py [--reps 20] [--rounds 5]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

STREAM_BPS = 6.29e12  # measured float4 copy rate of the chip


def loop_z_buffer(points, w2c, K, H, W):
    """The z-buffer with a Python loop over the filled pixels and a readback per pixel, as the
    reference fills it (our own restatement; one camera)."""
    import torch
    cam = points @ w2c[:3, :3].T + w2c[:3, 3]
    keep = cam[:, 2] > 0
    cam = cam[keep]
    q = cam @ K.T
    u, v = torch.round(q[:, 0] / q[:, 2]).long(), torch.round(q[:, 1] / q[:, 2]).long()
    inb = (u >= 0) & (u < W) & (v >= 0) & (v < H)
    pix, z = (v * W + u)[inb], cam[inb, 2]
    order = torch.argsort(pix)
    pix, z = pix[order], z[order]
    starts = [0] + ((pix[1:] != pix[:-1]).nonzero()[:, 0] + 1).tolist() + [int(pix.numel())]
    est = torch.full((H * W,), float("inf"), device=points.device)
    for a, b in zip(starts[:-1], starts[1:]):
        est[pix[a].item()] = z[a:b].min()
    return est.reshape(H, W)


def run(a):
    import numpy as np
    import torch
    from dynamic3dgaussians_amd import _lib, depth_geometry as dg
    from dynamic3dgaussians_amd.camera import camera_rig, intrinsics
    from dynamic3dgaussians_amd.scene import make_gaussians
    if not torch.cuda.is_available():
        raise SystemExit("depth_geometry_bench needs a HIP device: nothing is measured without one")
    dev = torch.device("cuda", 0)
    L = _lib.load()
    stream = lambda: _lib.stream(dev)  # noqa: E731
    P, C, W, H = a.points, a.cams, a.width, a.height
    gen = torch.Generator(device=dev).manual_seed(0)

    cams = camera_rig(C, W, H)
    w2c = torch.from_numpy(np.stack([c.viewmatrix.T for c in cams])).float().to(dev).contiguous()
    k = np.asarray(intrinsics(W, H), dtype=np.float32).reshape(3, 3)
    K = torch.from_numpy(k).to(dev)[None].repeat(C, 1, 1).contiguous()
    c2w = torch.linalg.inv(w2c.double()).float().contiguous()
    Kinv = torch.linalg.inv(K.double()).float().contiguous()
    w2c_next = torch.roll(w2c, 1, 0).contiguous()  # camera pairs (c, c + 1) for the flow
    T = (w2c_next.double() @ c2w.double()).float().contiguous()
    pts = make_gaussians(P, seed=0, device=dev)["means3D"].contiguous()
    gt = (1.0 + 3.0 * torch.rand(C, H, W, device=dev, generator=gen)).contiguous()
    exclude = (torch.rand(C, H, W, device=dev, generator=gen) < 0.3).float().contiguous()
    depth = (1.5 + 2.0 * torch.rand(C, H, W, device=dev, generator=gen)).contiguous()
    fh, fw = a.flow_height, a.flow_width
    flow = (3.0 * torch.randn(C, 2, fh, fw, device=dev, generator=gen)).contiguous()
    disp = (3.0 * torch.randn(C, 2, fh, fw, device=dev, generator=gen)).contiguous()

    # preallocated outputs and argument blocks of the bare entry points
    est = torch.empty(C, H, W, device=dev)
    sums = torch.empty(C, 2, dtype=torch.float64, device=dev)
    ws = torch.empty(L.gs_depth_abs_rel_workspace_bytes(C, H, W), dtype=torch.uint8, device=dev)
    xyz = torch.empty(C, H, W, 3, device=dev)
    fl_out = torch.empty(C, 2, H, W, device=dev)
    valid = torch.empty(C, H, W, dtype=torch.uint8, device=dev)
    warped = torch.empty(C, 2, fh * fw, device=dev)
    a_pd = _lib.GsPointDepth(P=P, B=C, H=H, W=W, points=pts.data_ptr(), points_batch_stride=0, w2c=w2c.data_ptr(),
                             K=K.data_ptr(), depth=est.data_ptr())
    a_ar = _lib.GsDepthAbsRel(B=C, H=H, W=W, est=est.data_ptr(), gt=gt.data_ptr(), exclude=exclude.data_ptr(),
                              exclude_batch_stride=H * W, out=sums.data_ptr(), workspace=ws.data_ptr(),
                              workspace_bytes=ws.numel())
    a_un = _lib.GsDepthUnproject(B=C, H=H, W=W, depth=depth.data_ptr(), Kinv=Kinv.data_ptr(), c2w=c2w.data_ptr(),
                                 xyz=xyz.data_ptr())
    a_fl = _lib.GsDepthFlow(B=C, H=H, W=W, depth1=depth.data_ptr(), Kinv1=Kinv.data_ptr(), T=T.data_ptr(),
                            K2=K.data_ptr(), flow=fl_out.data_ptr(), valid=valid.data_ptr())
    a_sa = _lib.GsSampleBilinear(B=C, Ch=2, H=fh, W=fw, mode=_lib.GS_SAMPLE_DISPLACEMENT, N=fh * fw, h=fh, w=fw,
                                 src=flow.data_ptr(), coords=disp.data_ptr(), out=warped.data_ptr())

    def entry_mde():
        _lib.check(L.gs_point_depth(a_pd, stream()), "point depth")
        _lib.check(L.gs_depth_abs_rel(a_ar, stream()), "depth abs-rel")

    def entry_pd():
        _lib.check(L.gs_point_depth(a_pd, stream()), "point depth")

    work = {
        "mde": (lambda: dg.depth_abs_rel(dg.point_depth_maps(pts, w2c, K, (H, W)), gt, exclude), entry_mde,
                lambda: dg.depth_abs_rel_torch(dg.point_depth_maps_torch(pts, w2c, K, (H, W)), gt, exclude)),
        "point_depth": (lambda: dg.point_depth_maps(pts, w2c, K, (H, W)), entry_pd,
                        lambda: dg.point_depth_maps_torch(pts, w2c, K, (H, W))),
        "unproject": (lambda: dg.unproject_depth(depth, K, w2c),
                      lambda: _lib.check(L.gs_depth_unproject(a_un, stream()), "depth unproject"),
                      lambda: dg.unproject_depth_torch(depth, K, w2c)),
        "flow": (lambda: dg.depth_flow(depth, K, c2w, K, w2c_next, return_valid=True),
                 lambda: _lib.check(L.gs_depth_flow(a_fl, stream()), "depth flow"),
                 lambda: dg.depth_flow_torch(depth, K, c2w, K, w2c_next, return_valid=True)),
        "warp": (lambda: dg.warp_flow(flow, disp),
                 lambda: _lib.check(L.gs_sample_bilinear(a_sa, stream()), "sample bilinear"),
                 lambda: dg.warp_flow_torch(flow, disp)),
    }

    def events(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    def peak_above_inputs(fn):
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        out = fn()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated(dev) - base
        del out
        return int(peak)

    entry_mde()
    torch.cuda.synchronize()
    landed = int(torch.isfinite(est).sum())  # filled pixels; every in-image point issues one atomic
    cam = pts @ w2c[:, :3, :3].transpose(1, 2) + w2c[:, None, :3, 3]
    q = cam @ K.transpose(1, 2)
    u, v = torch.round(q[..., 0] / q[..., 2]), torch.round(q[..., 1] / q[..., 2])
    atomics = int(((cam[..., 2] > 0) & (u >= 0) & (u < W) & (v >= 0) & (v < H)).sum())
    del cam, q, u, v
    px, fpx = C * H * W, C * fh * fw
    model = {"point_depth": 4 * px + 12 * C * P + 4 * atomics,
             "mde": 4 * px + 12 * C * P + 4 * atomics + 12 * px,
             "unproject": 16 * px, "flow": 13 * px, "warp": (8 + 8 + 8) * fpx}
    rec = {"bench": "depth_geometry", "P": P, "C": C, "width": W, "height": H, "flow_size": [fh, fw],
           "reps_per_sample": a.reps, "rounds": a.rounds, "stream_rate_Bps": STREAM_BPS,
           "timing": "device events around reps calls, ms per call; samples of hip, entry and torch alternate",
           "z_buffer": {"atomics_issued": atomics, "pixels_filled": landed}, "workloads": {}}
    for name, (hip, entry, twin) in work.items():
        treps = max(2, a.reps // 4) if name in ("mde", "point_depth") else a.reps  # the twins of these are slow
        for fn in (hip, entry, twin):  # every shape warmed up
            fn()
            fn()
        torch.cuda.synchronize()
        runs = {"hip": [], "entry": [], "torch": []}
        for _ in range(a.rounds):
            runs["hip"].append(round(events(hip, a.reps), 4))
            runs["entry"].append(round(events(entry, a.reps), 4))
            runs["torch"].append(round(events(twin, treps), 4))
        med = {k: statistics.median(x) for k, x in runs.items()}
        rec["workloads"][name] = {
            "ms_runs": runs, "ms_median": {k: round(x, 4) for k, x in med.items()},
            "ms_range": {k: [min(x), max(x)] for k, x in runs.items()},
            "torch_over_hip": round(med["torch"] / med["hip"], 2), "torch_over_entry": round(med["torch"] / med["entry"], 2),
            "model_bytes": model[name], "entry_GBps": round(model[name] / (med["entry"] * 1e-3) / 1e9, 1),
            "fill_fraction": round(model[name] / (med["entry"] * 1e-3) / STREAM_BPS, 4),
            "peak_bytes_above_inputs": {"hip": peak_above_inputs(hip), "torch": peak_above_inputs(twin)}}
    # outputs of the timed shapes agree (hip against its twin in fp32, same device)
    e_hip, e_twin = dg.point_depth_maps(pts, w2c, K, (H, W)), dg.point_depth_maps_torch(pts, w2c, K, (H, W))
    e_64 = dg.point_depth_maps_torch(pts.double(), w2c.double(), K.double(), (H, W))

    def differing(x, y, tol=1e-5):
        """Pixels whose winning point differs: filled in one map only, or depths apart by more than rounding."""
        fx, fy = torch.isfinite(x), torch.isfinite(y)
        return int(((fx != fy) | (fx & fy & ((x.double() - y.double()).abs() > tol * y.double().abs()))).sum())

    rec["agreement"] = {
        "note": "the timed cloud is random, not decision-robust: where a projection falls within rounding of a "
                "half-pixel tie, fp32 formulations may pick different pixels (counts are pixels of C*H*W)",
        "z_buffer_pixels_hip_vs_torch_fp32": differing(e_hip, e_twin),
        "z_buffer_pixels_hip_vs_torch_fp64": differing(e_hip, e_64),
        "z_buffer_pixels_torch_fp32_vs_torch_fp64": differing(e_twin, e_64),
        "unproject_max_abs": float((dg.unproject_depth(depth, K, w2c) - dg.unproject_depth_torch(depth, K, w2c)).abs().max()),
        "warp_max_abs": float((dg.warp_flow(flow, disp) - dg.warp_flow_torch(flow, disp)).abs().max())}
    del e_hip, e_twin
    # the per-pixel loop, once, on the smallest fixture shape
    sys.path.insert(0, REPO)
    from tests import _depth_geometry_cases as cases
    lp, lw2c, lK, _, _ = cases.zbuf_case("zbuf_5x7")
    lp, lw2c, lK = lp[0].to(dev), lw2c[0].float().to(dev), lK[0].float().to(dev)
    loop_z_buffer(lp, lw2c, lK, 5, 7)  # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    est_loop = loop_z_buffer(lp, lw2c, lK, 5, 7)
    torch.cuda.synchronize()
    loop_ms = (time.perf_counter() - t0) * 1e3
    small = lambda: dg.point_depth_maps(lp, lw2c, lK, (5, 7))  # noqa: E731
    small()
    rec["python_loop_5x7_P1000"] = {"loop_ms_once": round(loop_ms, 3), "hip_ms": round(events(small, a.reps), 4),
                                    "pixels": int(torch.isfinite(est_loop).sum()),
                                    "same_pixels_as_hip": bool(torch.equal(torch.isfinite(est_loop), torch.isfinite(small())))}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--points", type=int, default=300_000)
    ap.add_argument("--cams", type=int, default=27)
    ap.add_argument("--width", type=int, default=800)
    ap.add_argument("--height", type=int, default=800)
    ap.add_argument("--flow-height", type=int, default=288)
    ap.add_argument("--flow-width", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "depth_geometry", "bench.json"))
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
