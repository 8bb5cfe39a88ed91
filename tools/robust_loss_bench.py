#!/usr/bin/env python3
"""Quantile-trimmed masked MSE loss, forward + backward per call: the HIP kernels
(dynamic3dgaussians_amd.masked_trimmed_mse_loss) against the reference's formulation on
the same device -- per camera, mse_loss(...).mean(0), torch.quantile, boolean indexing of
(e * mask), mean, autograd; per camera is the only way it runs at this size, torch.quantile
refuses 16 M elements -- at the rig's shapes: 27 x C x 800 x 800 (C = 3 and 32) with an 80 %
mask and q = 0.9.

Device events around `reps` calls, after a warm-up of both; the implementations alternate
inside one process (`rounds` times) and the median round is reported with the rounds.
Timings of the HIP path:

    hip            the autograd function as a training step calls it
    hip_kernels    forward + backward through the C ABI on preallocated buffers
    hip_forward    the forward alone, the same way (a memset and eight launches)
    fill           torch's fill of a buffer of pred's size: the plain streaming rate the byte
                   model is compared with

and of the batched quantile alone (plane_quantile's launches through the C ABI on a
[27, 640000] plane): uniform values against a plane that is 60 % exact zeros, at q = 0.9
(only the first histogram sees the run of ties) and q = 0.5 (the rank lies inside the run:
all three histograms count it).  LDS-atomic contention on one bin is the known hazard there.

Bytes per pixel, from shapes: residual pass 2 C 4 read + 4 written; + 4 for each of the two
further histogram levels; + 5 for the reduce (plane and mask byte); backward 2 C 4 + 1 read
(the residual is recomputed from lines just read) + C 4 written.  Histograms, partial sums
and state are not counted.

The run is a child process of its own under a time limit.  One JSON line per case, appended
to --out (default profiles/robust_loss/bench.json).

    python tools/robust_loss_bench.py [--reps 10] [--rounds 5] [--cams 27] [--size 800] [--channels 3 32]
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

Q = 0.9


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


def reference_formulation(pred, gt, mask, q):
    """helpers.py:16-38 per camera with normalize=False, summed over the cameras."""
    import torch
    import torch.nn.functional as F
    total = 0
    for b in range(pred.shape[0]):
        e = F.mse_loss(pred[b], gt[b], reduction="none").mean(dim=0, keepdim=True)
        keep = e < torch.quantile(e, q)
        total = total + torch.mean((e * mask[b][None])[keep])
    return total


def run(a, C):
    import torch
    from dynamic3dgaussians_amd import _lib, masked_trimmed_mse_loss
    from dynamic3dgaussians_amd.robust_loss import CHANNELS, VALUES
    dev = torch.device("cuda", 0)
    B, H, W = a.cams, a.size, a.size
    N = H * W
    gen = torch.Generator(device=dev).manual_seed(0)
    pred = torch.rand(B, C, H, W, device=dev, generator=gen).requires_grad_(True)
    gt = pred.detach() + 0.02 * torch.exp(1.5 * torch.randn(B, 1, H, W, device=dev, generator=gen)) * \
        torch.randn(B, C, H, W, device=dev, generator=gen)
    mask = (torch.rand(B, H, W, device=dev, generator=gen) < 0.8).to(torch.uint8)
    maskf = mask.float()

    def call(fn, m):
        pred.grad = None
        loss = fn(pred, gt, m) * (1.0 / B)
        loss.backward()
        return loss.detach(), pred.grad

    L = _lib.load()
    stream = _lib.stream(dev)
    losses, stats = torch.empty(B, device=dev), torch.empty(B, 4, dtype=torch.float64, device=dev)
    ws = torch.empty(L.gs_robust_loss_workspace_bytes(B, N, CHANNELS), dtype=torch.uint8, device=dev)
    up, d_pred = torch.full((B,), 1.0 / B, device=dev), torch.empty_like(pred)
    args = _lib.GsRobustLoss(B=B, R=C, N=N, layout=CHANNELS, pred=pred.data_ptr(), gt=gt.data_ptr(),
                             mask=mask.data_ptr(), mask_batch_stride=N, quantile=Q, select=1, losses=losses.data_ptr(),
                             stats=stats.data_ptr(), workspace=ws.data_ptr(), workspace_bytes=ws.numel())

    def forward_only():
        _lib.check(L.gs_robust_loss_forward(args, stream), "robust loss forward")

    def kernels():
        forward_only()
        _lib.check(L.gs_robust_loss_backward(args, up.data_ptr(), d_pred.data_ptr(), stream), "robust loss backward")

    impls = {"hip": lambda: call(lambda p, g, m: masked_trimmed_mse_loss(p, g, mask=m, quantile=Q), mask),
             "torch": lambda: call(lambda p, g, m: reference_formulation(p, g, m, Q), maskf),
             "hip_kernels": kernels, "hip_forward": forward_only, "fill": lambda: d_pred.fill_(1.0)}
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
    same_bits = bool(torch.equal(d_pred, out["hip"][1]))

    # the batched quantile alone: uniform values against 60 % exact zeros
    planes = {"uniform": torch.rand(B, N, device=dev, generator=gen)}
    planes["zeros60"] = planes["uniform"] * (torch.rand(B, N, device=dev, generator=gen) >= 0.6)
    qws = torch.empty(L.gs_robust_loss_workspace_bytes(B, N, VALUES), dtype=torch.uint8, device=dev)

    def quantile_call(x, q):
        qa = _lib.GsRobustLoss(B=B, R=1, N=N, layout=VALUES, pred=x.data_ptr(), quantile=q, select=1,
                               stats=stats.data_ptr(), workspace=qws.data_ptr(), workspace_bytes=qws.numel())
        return lambda: _lib.check(L.gs_robust_loss_forward(qa, stream), "plane quantile")
    for name, x in planes.items():
        for q in (0.9, 0.5):
            impls[f"quantile_{name}_q{q}"] = quantile_call(x, q)

    ms = {k: [] for k in impls}
    for k, fn in impls.items():
        fn()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for k, fn in impls.items():
            reps = max(1, a.reps // 5) if k == "torch" else a.reps
            s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s0.record()
            for _ in range(reps):
                fn()
            s1.record()
            torch.cuda.synchronize()
            ms[k].append(s0.elapsed_time(s1) / reps)
    n = B * N
    med = {k: statistics.median(v) for k, v in ms.items()}
    fill_rate = 4 * C * n / (med["fill"] * 1e-3)
    fwd_bytes, bwd_bytes = (2 * C * 4 + 4) + 4 + 4 + 5, 2 * C * 4 + 1 + C * 4
    bwd_ms = med["hip_kernels"] - med["hip_forward"]
    return {"step": "robust_loss", "shape": [B, C, H, W], "quantile": Q,
            "mask_fraction": round(float(maskf.mean()), 4), "reps": a.reps, "rounds": a.rounds,
            "ms": {k: round(v, 4) for k, v in med.items()},
            "ms_rounds": {k: [round(x, 4) for x in v] for k, v in ms.items()},
            "torch_over_hip": round(med["torch"] / med["hip"], 2),
            "torch_over_hip_kernels": round(med["torch"] / med["hip_kernels"], 2),
            "peak_bytes_over_inputs": peak, "input_bytes": (8 * C + 1) * n, "workspace_bytes": int(ws.numel()),
            "fill_bytes_per_s": round(fill_rate, -9),
            "bytes_per_pixel_model": {"forward": fwd_bytes, "backward": bwd_bytes},
            "share_of_fill_rate": {
                "forward": round(fwd_bytes * n / (med["hip_forward"] * 1e-3) / fill_rate, 4),
                "backward_by_difference": round(bwd_bytes * n / (bwd_ms * 1e-3) / fill_rate, 4) if bwd_ms > 0 else None,
                "quantile_uniform_q0.9": round(12 * n / (med["quantile_uniform_q0.9"] * 1e-3) / fill_rate, 4)},
            "zeros60_over_uniform": {"q0.9": round(med["quantile_zeros60_q0.9"] / med["quantile_uniform_q0.9"], 3),
                                     "q0.5": round(med["quantile_zeros60_q0.5"] / med["quantile_uniform_q0.5"], 3)},
            "c_abi_gradient_equals_autograd_bits": same_bits,
            "parity_vs_torch_fp32": {"loss_rel": abs(out["hip"][0] - out["torch"][0]) / max(abs(out["torch"][0]), 1e-30),
                                     "d_pred_rel_l2": _rel(out["hip"][1], out["torch"][1])}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cams", type=int, default=27)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--channels", type=int, nargs="+", default=[3, 32])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "robust_loss", "bench.json"))
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:  # the measurement of one channel count, in its own process: print its record
        print("RECORD " + json.dumps(run(a, a.child)), flush=True)
        return 0
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for C in a.channels:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(C), "--reps", str(a.reps), "--rounds",
               str(a.rounds), "--cams", str(a.cams), "--size", str(a.size)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout, cwd=REPO)
        except subprocess.TimeoutExpired:
            print(f"C = {C}: no result within {a.step_timeout} s", file=sys.stderr)
            return 124
        recs = [ln[7:] for ln in r.stdout.splitlines() if ln.startswith("RECORD ")]
        if r.returncode != 0 or not recs:
            print(f"C = {C}: exit status {r.returncode}\n{r.stderr[-3000:]}", file=sys.stderr)
            return r.returncode or 1
        print(recs[-1], flush=True)
        with open(a.out, "a") as f:
            f.write(recs[-1] + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
