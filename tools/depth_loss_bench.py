#!/usr/bin/env python3
"""Masked depth-correlation loss, forward + backward per call: the fused HIP
kernels (dynamic3dgaussians_amd.depth_correlation_loss) against the PyTorch
formulation of the reference (depth_correlation_loss_torch: boolean indexing,
standardisation and Pearson camera by camera, autograd) on the same device, at
the rig's shape: 27 x 1 x 800 x 800 with an 80 % mask.

Device events around `reps` calls, after a warm-up of both; the two
implementations alternate inside one process (`rounds` times) and the median
round is reported with the spread.  Three timings of the HIP path:

    hip          the autograd function as a training step calls it (allocations
                 and autograd bookkeeping included)
    hip_kernels  the three launches alone through the C ABI on preallocated
                 buffers (what the byte model is compared with)
    hip_forward  the two forward launches alone, the same way

The run is a child process of its own under a time limit.  One JSON line,
appended to --out (default profiles/depth_loss/bench.json).

    python tools/depth_loss_bench.py [--reps 20] [--rounds 5] [--cams 27] [--size 800]

Bytes: the kernels' HBM traffic from shapes: the forward reads depth (4),
target (4) and the mask byte (1) per pixel, the backward reads the same and
writes the gradient (+4): 9 + 13 = 22 B per pixel.  The per-workgroup records
and the statistics (24 B per 1024 pixels) are not counted.
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
FWD_BYTES, BWD_BYTES = 9, 13  # per pixel


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


def run(a):
    import torch
    from dynamic3dgaussians_amd import _lib, depth_correlation_loss, depth_correlation_loss_torch
    dev = torch.device("cuda", 0)
    B, H, W = a.cams, a.size, a.size
    gen = torch.Generator(device=dev).manual_seed(0)
    depth = (1.0 + 9.0 * torch.rand(B, 1, H, W, device=dev, generator=gen)).requires_grad_(True)
    target = 1.0 / (1.7 * depth.detach()) + 0.05 * torch.randn(B, 1, H, W, device=dev, generator=gen)
    mask = (torch.rand(B, H, W, device=dev, generator=gen) < 0.8).to(torch.uint8)

    def call(fn):
        depth.grad = None
        loss = fn(depth, target, mask=mask) * (0.001 / B)
        loss.backward()
        return loss.detach(), depth.grad

    # the three launches alone, on buffers of their own
    L = _lib.load()
    d3, g3 = depth.detach().reshape(B, H, W), target.reshape(B, H, W)
    losses, stats = torch.empty(B, device=dev), torch.empty(B, 8, device=dev)
    ws = torch.empty(L.gs_depth_loss_workspace_bytes(B, H, W), dtype=torch.uint8, device=dev)
    up, d_depth = torch.full((B,), 0.001 / B, device=dev), torch.empty_like(d3)
    args = _lib.GsDepthLoss(B=B, H=H, W=W, depth=d3.data_ptr(), target=g3.data_ptr(), mask=mask.data_ptr(),
                            mask_batch_stride=H * W, near=1e-7, far=50.0, skip_degenerate=0,
                            losses=losses.data_ptr(), stats=stats.data_ptr(), workspace=ws.data_ptr(),
                            workspace_bytes=ws.numel())
    stream = _lib.stream(dev)

    def forward_only():
        _lib.check(L.gs_depth_loss_forward(args, stream), "depth loss forward")

    def kernels():
        forward_only()
        _lib.check(L.gs_depth_loss_backward(args, up.data_ptr(), d_depth.data_ptr(), stream), "depth loss backward")

    impls = {"hip": lambda: call(depth_correlation_loss), "torch": lambda: call(depth_correlation_loss_torch),
             "hip_kernels": kernels, "hip_forward": forward_only}
    base = torch.cuda.memory_allocated(dev)
    peak, out = {}, {}
    for k in ("hip", "torch"):  # warm-up, parity and peak memory
        impls[k]()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        res = impls[k]()
        torch.cuda.synchronize()
        peak[k] = torch.cuda.max_memory_allocated(dev) - base
        out[k] = (res[0].item(), res[1].clone())
    kernels()
    torch.cuda.synchronize()
    same_bits = bool(torch.equal(d_depth.reshape(depth.shape), out["hip"][1]))
    ms = {k: [] for k in impls}
    for _ in range(a.rounds):
        for k, fn in impls.items():
            reps = max(1, a.reps // 4) if k == "torch" else a.reps
            s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s0.record()
            for _ in range(reps):
                fn()
            s1.record()
            torch.cuda.synchronize()
            ms[k].append(s0.elapsed_time(s1) / reps)
    # both fp32 paths against the torch formulation in fp64 on the device (one call)
    d64 = depth.detach().double().requires_grad_(True)
    loss64 = depth_correlation_loss_torch(d64, target.double(), mask=mask) * (0.001 / B)
    (g64,) = torch.autograd.grad(loss64, d64)
    vs64 = {k: {"loss_rel": abs(out[k][0] - loss64.item()) / abs(loss64.item()), "d_depth_rel_l2": _rel(out[k][1], g64)}
            for k in ("hip", "torch")}
    n = B * H * W
    med = {k: statistics.median(v) for k, v in ms.items()}
    bwd_ms = med["hip_kernels"] - med["hip_forward"]
    return {"step": "depth_loss", "shape": [B, 1, H, W], "mask_fraction": round(float(mask.float().mean()), 4),
            "reps": a.reps, "rounds": a.rounds,
            "ms_fwd_bwd": {k: round(v, 4) for k, v in med.items()},
            "ms_rounds": {k: [round(x, 4) for x in v] for k, v in ms.items()},
            "torch_over_hip": round(med["torch"] / med["hip"], 2),
            "torch_over_hip_kernels": round(med["torch"] / med["hip_kernels"], 2),
            "peak_bytes_over_inputs": peak, "input_bytes": 9 * n,
            "workspace_bytes": int(ws.numel()),
            "hbm_bytes_model": {"forward": FWD_BYTES * n, "backward": BWD_BYTES * n},
            "hbm_model": "fwd 4 + 4 + 1 B read, bwd the same and 4 B written, per pixel",
            "hbm_share_of_8TBps": {
                "forward_and_backward": round((FWD_BYTES + BWD_BYTES) * n / (med["hip_kernels"] * 1e-3) / HBM_BYTES_PER_S, 4),
                "forward": round(FWD_BYTES * n / (med["hip_forward"] * 1e-3) / HBM_BYTES_PER_S, 4),
                "backward_by_difference": round(BWD_BYTES * n / (bwd_ms * 1e-3) / HBM_BYTES_PER_S, 4) if bwd_ms > 0 else None},
            "c_abi_gradient_equals_autograd_bits": same_bits,
            "parity_vs_torch_fp32": {"loss_rel": abs(out["hip"][0] - out["torch"][0]) / max(abs(out["torch"][0]), 1e-30),
                                     "d_depth_rel_l2": _rel(out["hip"][1], out["torch"][1])},
            "vs_torch_fp64_on_device": vs64}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cams", type=int, default=27)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "depth_loss", "bench.json"))
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:  # the measurement, in its own process: print its record
        print("RECORD " + json.dumps(run(a)), flush=True)
        return 0
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--rounds", str(a.rounds),
           "--cams", str(a.cams), "--size", str(a.size)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout, cwd=REPO)
    except subprocess.TimeoutExpired:
        print(f"no result within {a.step_timeout} s", file=sys.stderr)
        return 124
    recs = [ln[7:] for ln in r.stdout.splitlines() if ln.startswith("RECORD ")]
    if r.returncode != 0 or not recs:
        print(f"exit status {r.returncode}\n{r.stderr[-3000:]}", file=sys.stderr)
        return r.returncode or 1
    print(recs[-1], flush=True)
    with open(a.out, "a") as f:
        f.write(recs[-1] + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
