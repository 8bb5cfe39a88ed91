#!/usr/bin/env python3
"""Bilinear resample to a prior's size, forward + backward per call: the HIP
kernels (dynamic3dgaussians_amd.bilinear_resize) against torch's F.interpolate
with autograd on the same device, at the rig's two shapes:

    features  27 x 32 x 800 x 800 -> 288 x 512, align_corners=True
    depth     27 x  1 x 800 x 800 -> 288 x 512, align_corners=False

and the end-to-end feature term: feature_distillation_loss (resample + loss at
288 x 512) against the existing same-resolution photometric_loss on the
32 channels at 800 x 800.

Device events around `reps` calls, after a warm-up of all; the variants
alternate inside one process (`rounds` times) and the median round is reported
with every round.  Timings per case:

    hip           the autograd function as a training step calls it
    hip_forward   the forward launch alone through the C ABI on preallocated buffers
    hip_backward  the table launch and the backward launch alone, the same way
    interpolate   F.interpolate forward + autograd backward
    fill          d_x.zero_(): the plain fill of the backward's output, the rate
                  the kernels' byte models are compared with

One child process per case under a time limit.  One JSON line per case,
appended to --out (default profiles/resample/bench.json).  --variant names a
build variant of the library (build.py VARIANT_FLAGS, e.g. rs_pb1) for an
A/B of the same measurement.

    python tools/resample_bench.py [--case features|depth|all] [--reps 10] [--rounds 5]

Bytes, from shapes: the forward reads the input rows some output taps (all
their columns: rows are fetched whole) and writes the output; the backward
reads the upstream gradient and writes every element of d_x.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

FILL_BYTES_PER_S = 8.3e12  # the plain fill
CASES = {"features": (32, True), "depth": (1, False)}


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


def run(a):
    import numpy as np
    import torch
    import torch.nn.functional as F
    from dynamic3dgaussians_amd import _lib, bilinear_resize, feature_distillation_loss, photometric_loss, resample
    dev = torch.device("cuda", 0)
    Ch, align = CASES[a.case]
    B, H, W, h, w = a.cams, a.size, a.size, a.out_h, a.out_w
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(B, Ch, H, W, device=dev, generator=gen).requires_grad_(True)
    g = torch.randn(B, Ch, h, w, device=dev, generator=gen)
    base = torch.cuda.memory_allocated(dev)

    def call(fn):
        x.grad = None
        y = fn(x)
        y.backward(g)
        return y.detach(), x.grad

    L = _lib.load()
    y_buf, d_x = torch.empty(B, Ch, h, w, device=dev), torch.empty(B, Ch, H, W, device=dev)
    ws = torch.empty(L.gs_resample_workspace_bytes(H, W), dtype=torch.uint8, device=dev)
    args = _lib.GsResample(B=B, Ch=Ch, H=H, W=W, h=h, w=w, align_corners=int(align), x=x.data_ptr(),
                           y=y_buf.data_ptr(), workspace=ws.data_ptr(), workspace_bytes=ws.numel())
    stream = _lib.stream(dev)

    def forward_only():
        _lib.check(L.gs_resample_forward(args, stream), "resample forward")

    def backward_only():
        _lib.check(L.gs_resample_backward(args, g.data_ptr(), d_x.data_ptr(), stream), "resample backward")

    impls = {"hip": lambda: call(lambda t: bilinear_resize(t, (h, w), align_corners=align)),
             "interpolate": lambda: call(lambda t: F.interpolate(t, size=(h, w), mode="bilinear", align_corners=align)),
             "hip_forward": forward_only, "hip_backward": backward_only, "fill": lambda: d_x.zero_()}
    peak, out = {}, {}
    for k in ("hip", "interpolate"):  # warm-up, parity and peak memory
        impls[k]()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        res = impls[k]()
        torch.cuda.synchronize()
        peak[k] = torch.cuda.max_memory_allocated(dev) - base
        out[k] = (res[0].clone(), res[1].clone())
    forward_only()
    backward_only()
    torch.cuda.synchronize()
    same_bits = bool(torch.equal(y_buf, out["hip"][0]) and torch.equal(d_x, out["hip"][1]))
    parity = {"y_max_abs": float((out["hip"][0] - out["interpolate"][0]).abs().max()),
              "d_x_rel_l2": _rel(out["hip"][1], out["interpolate"][1])}
    again = impls["interpolate"]()
    torch.cuda.synchronize()
    interp_reproducible = bool(torch.equal(again[1], out["interpolate"][1]))
    del out, again
    x.grad = None

    if a.case == "features":  # the end-to-end feature term
        prior = torch.randn(B, Ch, h, w, device=dev, generator=gen)
        full = torch.randn(B, Ch, H, W, device=dev, generator=gen)

        def term(fn):
            x.grad = None
            loss = fn()
            loss.backward()
            return loss.detach()

        for l1w, sw, tag in ((1.0, 0.0, "l1"), (0.8, 0.2, "l1_ssim")):
            impls[f"term_resized_{tag}"] = lambda l1w=l1w, sw=sw: term(
                lambda: feature_distillation_loss(x, prior, l1_weight=l1w, ssim_weight=sw))
            impls[f"term_same_size_{tag}"] = lambda l1w=l1w, sw=sw: term(
                lambda: photometric_loss(x, full, l1_weight=l1w, ssim_weight=sw))
    for fn in impls.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in impls}
    for _ in range(a.rounds):
        for k, fn in impls.items():
            s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s0.record()
            for _ in range(a.reps):
                fn()
            s1.record()
            torch.cuda.synchronize()
            ms[k].append(s0.elapsed_time(s1) / a.reps)
    med = {k: statistics.median(v) for k, v in ms.items()}
    y0, y1, _, _, _ = resample.axis_tables(H, h, align)
    rows = int(np.union1d(y0, y1).size)
    planes = B * Ch
    fwd_bytes = 4 * planes * (rows * W + h * w)
    bwd_bytes = 4 * planes * (h * w + H * W)
    fill_rate = 4 * planes * H * W / (med["fill"] * 1e-3)
    rate = lambda nbytes, k: nbytes / (med[k] * 1e-3)  # noqa: E731
    rec = {"step": "resample", "case": a.case, "variant": os.environ.get("GSPLAT_VARIANT", ""),
           "shape": [B, Ch, H, W], "size": [h, w], "align_corners": align, "reps": a.reps, "rounds": a.rounds,
           "ms": {k: round(v, 4) for k, v in med.items()},
           "ms_rounds": {k: [round(v, 4) for v in vs] for k, vs in ms.items()},
           "interpolate_over_hip": round(med["interpolate"] / med["hip"], 2),
           "interpolate_over_hip_kernels": round(med["interpolate"] / (med["hip_forward"] + med["hip_backward"]), 2),
           "input_rows_touched": rows,
           "hbm_bytes_model": {"forward": fwd_bytes, "backward": bwd_bytes},
           "hbm_model": "fwd: touched input rows + output; bwd: upstream gradient + all of d_x",
           "TBps": {"forward": round(rate(fwd_bytes, "hip_forward") / 1e12, 3),
                    "backward": round(rate(bwd_bytes, "hip_backward") / 1e12, 3),
                    "fill_this_run": round(fill_rate / 1e12, 3)},
           "share_of_fill_8.3TBps": {"forward": round(rate(fwd_bytes, "hip_forward") / FILL_BYTES_PER_S, 4),
                                     "backward": round(rate(bwd_bytes, "hip_backward") / FILL_BYTES_PER_S, 4)},
           "share_of_fill_this_run": {"forward": round(rate(fwd_bytes, "hip_forward") / fill_rate, 4),
                                      "backward": round(rate(bwd_bytes, "hip_backward") / fill_rate, 4)},
           "peak_bytes_over_inputs": peak, "input_bytes": 4 * planes * (H * W + h * w),
           "workspace_bytes": int(ws.numel()),
           "c_abi_equals_autograd_bits": same_bits, "interpolate_backward_reproducible": interp_reproducible,
           "parity_vs_interpolate_fp32": parity}
    if a.case == "features":
        rec["feature_term_ms"] = {tag: {"resized": round(med[f"term_resized_{tag}"], 4),
                                        "same_size": round(med[f"term_same_size_{tag}"], 4),
                                        "same_size_over_resized": round(med[f"term_same_size_{tag}"]
                                                                        / med[f"term_resized_{tag}"], 2)}
                                  for tag in ("l1", "l1_ssim")}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="all", choices=[*CASES, "all"])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cams", type=int, default=27)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--out-h", type=int, default=288)
    ap.add_argument("--out-w", type=int, default=512)
    ap.add_argument("--variant", default="", help="a build variant of the library (build.py VARIANT_FLAGS)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "resample", "bench.json"))
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:  # the measurement, in its own process: print its record
        print("RECORD " + json.dumps(run(a)), flush=True)
        return 0
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    env = dict(os.environ)
    if a.variant:
        env["GSPLAT_VARIANT"] = a.variant
    for case in (CASES if a.case == "all" else [a.case]):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--case", case, "--reps", str(a.reps),
               "--rounds", str(a.rounds), "--cams", str(a.cams), "--size", str(a.size), "--out-h", str(a.out_h),
               "--out-w", str(a.out_w)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout, cwd=REPO, env=env)
        except subprocess.TimeoutExpired:
            print(f"{case}: no result within {a.step_timeout} s", file=sys.stderr)
            return 124
        recs = [ln[7:] for ln in r.stdout.splitlines() if ln.startswith("RECORD ")]
        if r.returncode != 0 or not recs:  # a fault ends the run: nothing more is started on the device
            print(f"{case}: exit status {r.returncode}\n{r.stderr[-3000:]}", file=sys.stderr)
            return r.returncode or 1
        print(recs[-1], flush=True)
        with open(a.out, "a") as f:
            f.write(recs[-1] + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
