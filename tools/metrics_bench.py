#!/usr/bin/env python3
"""Evaluation metrics (masked PSNR sums + masked SSIM), one call: the HIP
kernel (dynamic3dgaussians_amd.image_metrics) against the PyTorch formulation
of the reference (image_metrics_torch: ten masked depthwise convolutions and
ten mask-count convolutions) on the same device, at the evaluation shapes:

    rig    27 x 3 x 800 x 800   with an 80 % mask per image
    video  27 x 3 x 288 x 512   no mask

Device events around `reps` calls, after a warm-up of both; the two
implementations alternate inside one process (`rounds` times) and the median
round is reported with the spread.  Each shape runs in a child process of its
own under a time limit; a child that fails ends the run.  A last step records
the envelope ratios of tests/test_gpu_metrics.py's cases (the kernel's ssim
error over the fp32 reference formulation's own).  JSON lines, appended to
--out (default profiles/metrics/bench.json).

    python tools/metrics_bench.py [--reps 10] [--rounds 3]

Bytes: the count is the algorithm's HBM traffic from shapes: pred and target
once per pixel-channel and the mask once per pixel, (2 Ch + 1) x 4 B x B H W
(the mask term only with a mask); the writes are 16 B per workgroup.  Halo
re-reads are expected to hit in cache and are not counted.
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

HBM_BYTES_PER_S = 8.0e12
SHAPES = {"rig": (27, 3, 800, 800, True), "video": (27, 3, 288, 512, False)}


def run_shape(name, a):
    import torch
    from dynamic3dgaussians_amd import _lib, image_metrics, image_metrics_torch
    B, ch, H, W, masked = SHAPES[name]
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    pred = torch.rand(B, ch, H, W, device=dev, generator=gen)
    target = (pred + 0.1 * torch.randn(B, ch, H, W, device=dev, generator=gen)).clamp_(0, 1)
    mask = (torch.rand(B, H, W, device=dev, generator=gen) < 0.8).float() if masked else None
    impls = {"hip": lambda: image_metrics(pred, target, mask), "torch": lambda: image_metrics_torch(pred, target, mask)}
    base = torch.cuda.memory_allocated(dev)
    peak, out = {}, {}
    for k, fn in impls.items():  # warm-up, parity and peak memory
        fn()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        out[k] = fn()
        torch.cuda.synchronize()
        peak[k] = torch.cuda.max_memory_allocated(dev) - base
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
    # both fp32 paths against the torch formulation in fp64 on the device, a few images (memory)
    n64 = min(B, 3)
    ref = image_metrics_torch(pred[:n64].double(), target[:n64].double(), None if mask is None else mask[:n64])
    rel = lambda x, y: float(((x[:n64].double() - y).abs() / y.abs()).max())  # noqa: E731
    vs64 = {k: {"ssim_rel_max": rel(out[k].ssim, ref.ssim), "sse_rel_max": rel(out[k].sse, ref.sse),
                "sae_rel_max": rel(out[k].sae, ref.sae)} for k in impls}
    hbm = ((2 * ch + 1) if masked else 2 * ch) * 4 * B * H * W
    med = {k: statistics.median(v) for k, v in ms.items()}
    return {"step": name, "shape": [B, ch, H, W], "mask": masked, "reps": a.reps, "rounds": a.rounds,
            "ms_per_call": {k: round(v, 4) for k, v in med.items()},
            "ms_rounds": {k: [round(x, 4) for x in v] for k, v in ms.items()},
            "torch_over_hip": round(med["torch"] / med["hip"], 3),
            "peak_bytes_over_inputs": peak,
            "workspace_bytes": int(_lib.load().gs_image_metrics_workspace_bytes(B, ch, H, W)),
            "hbm_bytes_model": hbm, "hbm_model": "(2 Ch + 1) floats read per pixel per image; partials written",
            "hbm_share_of_8TBps": round(hbm / (med["hip"] * 1e-3) / HBM_BYTES_PER_S, 4),
            "vs_torch_fp64_on_device_first_images": vs64}


def run_envelope(a):
    """The ssim envelope ratios of the GPU tests' cases."""
    import torch
    from dynamic3dgaussians_amd import image_metrics
    from tests import test_gpu_metrics as T
    ratios = {}
    for name in T.CASES:
        ref, err32 = T._oracle(name)
        got = image_metrics(*T._device(name))
        torch.cuda.synchronize()
        err = T._rel(got.ssim, ref.ssim)
        ratios[name] = {"ssim_rel": err.tolist(), "fp32_reference_rel": err32.tolist(),
                        "ratio": (err / err32.clamp_min(1e-300)).tolist()}
    return {"step": "envelope", "cases": ratios}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "metrics", "bench.json"))
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:  # one step, in its own process: print its record
        rec = run_envelope(a) if a.child == "envelope" else run_shape(a.child, a)
        print("RECORD " + json.dumps(rec), flush=True)
        return 0
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for step in (*SHAPES, "envelope"):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", step, "--reps", str(a.reps), "--rounds",
               str(a.rounds)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout, cwd=REPO)
        except subprocess.TimeoutExpired:
            print(f"{step}: no result within {a.step_timeout} s; stopping", file=sys.stderr)
            return 124
        recs = [ln[7:] for ln in r.stdout.splitlines() if ln.startswith("RECORD ")]
        if r.returncode != 0 or not recs:  # nothing more is started on the device after a failure
            print(f"{step}: exit status {r.returncode}\n{r.stderr[-3000:]}", file=sys.stderr)
            return r.returncode or 1
        print(recs[-1], flush=True)
        with open(a.out, "a") as f:
            f.write(recs[-1] + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
