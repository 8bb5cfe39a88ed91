#!/usr/bin/env python3
"""The motion-basis warp, forward + backward: the HIP path
(dynamic3dgaussians_amd.motion_positions: one launch forward, three backward)
against the PyTorch formulation (motion_positions_torch: softmax, two einsums,
the 6-vector to rotation chain, cat, pad, einsum, and autograd for the
backward) on the same device, at a training run's size:

    G = 300 000 Gaussians, K in {10, 20} bases, B in {6, 9} frames of T = 150,
    coefficients as logits (softmax inside), loss = sum(w * positions)

A sample is `--inner` forward + backward pairs bracketed by device events
(one pair is tens of microseconds of kernels: too short to time alone); the
two implementations alternate, `--runs` samples each after `--warmup` samples
of both; the median per pair is reported with the quartiles.  `ms_forward` is
the forward alone, measured the same way.  Peak memory is the allocator's peak
over the live inputs during one forward + backward.  Each configuration runs
in a child process of its own under a time limit; a child that fails ends the
run.  JSON lines, appended to --out (default profiles/motion/bench.json).

    python tools/motion_bench.py [--runs 20] [--warmup 3] [--inner 50] [--points 300000]

Kernel times come from a run of their own (profiling slows the host):

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/motion_bench.py --trace K B

which only runs the HIP path `--inner` times.  With the trace's average kernel
times (ms), and without a device,

    python tools/motion_bench.py --shares K B --kernel-ms fwd,bwd,sum,scatter

appends each kernel's share of the HBM rate against the byte model below.

Bytes, from shapes (what each kernel must move; the bases are a few KB):
    forward   reads  G (K + 3) 4          writes G B 12
    backward  reads  G (K + 3) 4 + G B 12 writes G K 4 + G 12 + slabs
    slab sum  reads  slabs                 writes B K 36
    scatter                                writes K T 36
    slabs = ceil(G / workgroup) B K 36
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
CONFIGS = [(10, 6), (10, 9), (20, 6), (20, 9)]
T_FRAMES = 150


def inputs(G, K, B, dev):
    """Seeded inputs by the tests' recipe (tests/_motion_cases.py): well-conditioned blends."""
    import torch
    gen = torch.Generator(device=dev).manual_seed(0)
    rn = lambda *s: torch.randn(*s, device=dev, generator=gen)  # noqa: E731
    q, _ = torch.linalg.qr(rn(K, T_FRAMES, 3, 3))
    ident = torch.tensor([1.0, 0, 0, 0, 1.0, 0], device=dev)
    rots = 0.6 * ident + 0.4 * torch.cat([q[..., :, 0], q[..., :, 1]], dim=-1) + 0.05 * rn(K, T_FRAMES, 6)
    t = {"means": rn(G, 3), "logits": 2.0 * rn(G, K), "rots": rots.contiguous(), "transls": 0.5 * rn(K, T_FRAMES, 3)}
    ts = [T_FRAMES - 1 - 7 * b for b in range(B)]
    return t, ts, rn(G, B, 3)


def byte_model(G, K, B, block):
    slabs = -(-G // block) * B * K * 36
    return {"forward": G * (K + 3) * 4 + G * B * 12,
            "backward": G * (K + 3) * 4 + G * B * 12 + G * K * 4 + G * 12 + slabs,
            "slab_sum": slabs + B * K * 36, "scatter": K * T_FRAMES * 36, "slabs": slabs}


def pair(fn, t, ts, w, backward=True):
    leaves = [t[k].requires_grad_(True) for k in ("means", "logits", "rots", "transls")]
    out = fn(*leaves, ts, softmax=True)
    if backward:
        return out, __import__("torch").autograd.grad((w * out).sum(), leaves)
    return out, None


def run_config(K, B, a):
    import torch
    from dynamic3dgaussians_amd import _lib, motion_positions, motion_positions_torch
    dev = torch.device("cuda", 0)
    G = a.points
    t, ts, w = inputs(G, K, B, dev)
    impls = {"hip": motion_positions, "torch": motion_positions_torch}

    def sample(fn, backward=True):
        torch.cuda.synchronize()
        s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s0.record()
        for _ in range(a.inner):
            pair(fn, t, ts, w, backward)
        s1.record()
        torch.cuda.synchronize()
        return s0.elapsed_time(s1) / a.inner

    outs, peak = {}, {}
    for k, fn in impls.items():  # warm-up, the outputs for the parity check, and the peak memory
        for _ in range(a.warmup):
            sample(fn)
            sample(fn, backward=False)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        outs[k] = pair(fn, t, ts, w)
        torch.cuda.synchronize()
        peak[k] = torch.cuda.max_memory_allocated(dev) - base
    rel = lambda x, y: float((x.double() - y.double()).norm() / y.double().norm())  # noqa: E731
    parity = {"positions_max_abs_diff": float((outs["hip"][0] - outs["torch"][0]).abs().max())}
    for n, x, y in zip(("d_means", "d_logits", "d_rots", "d_transls"), outs["hip"][1], outs["torch"][1]):
        parity[n + "_rel_l2"] = rel(x, y)
    again = pair(motion_positions, t, ts, w)
    parity["hip_backward_bit_identical"] = all(torch.equal(x, y) for x, y in zip(outs["hip"][1], again[1]))
    del outs, again
    ms = {k: [] for k in impls}
    ms_fwd = {k: [] for k in impls}
    for _ in range(a.runs):
        for k, fn in impls.items():
            ms[k].append(sample(fn))
            ms_fwd[k].append(sample(fn, backward=False))
    block = _lib.load().gs_motion_backward_block(K, B)
    model = byte_model(G, K, B, block)
    q = lambda v: [round(x, 5) for x in statistics.quantiles(v, n=4)]  # noqa: E731
    med = {k: statistics.median(v) for k, v in ms.items()}
    med_fwd = {k: statistics.median(v) for k, v in ms_fwd.items()}
    rec = {"step": f"K{K}_B{B}", "G": G, "K": K, "B": B, "T": T_FRAMES, "softmax": True, "runs": a.runs,
           "warmup": a.warmup, "pairs_per_sample": a.inner,
           "ms_forward_backward": {k: round(v, 5) for k, v in med.items()},
           "ms_forward_backward_quartiles": {k: q(v) for k, v in ms.items()},
           "ms_forward": {k: round(v, 5) for k, v in med_fwd.items()},
           "torch_over_hip": round(med["torch"] / med["hip"], 2),
           "torch_over_hip_forward": round(med_fwd["torch"] / med_fwd["hip"], 2),
           "peak_bytes_over_inputs": peak, "backward_workgroup": block, "bytes_model": model,
           "hbm_share_of_8TBps_whole_pair_hip": round(
               (model["forward"] + model["backward"] + model["slab_sum"] + model["scatter"])
               / (med["hip"] * 1e-3) / HBM_BYTES_PER_S, 4),
           "parity_hip_vs_torch_on_device": parity}
    return rec


def kernel_shares(K, B, a):
    """Each kernel's bytes over its traced time, as a share of the HBM rate."""
    from dynamic3dgaussians_amd import _lib
    names = ("forward", "backward", "slab_sum", "scatter")
    model = byte_model(a.points, K, B, _lib.load().gs_motion_backward_block(K, B))
    kms = dict(zip(names, (float(x) for x in a.kernel_ms.split(","))))
    return {"step": f"K{K}_B{B}_kernels", "G": a.points, "K": K, "B": B, "T": T_FRAMES,
            "source": "rocprofv3 --kernel-trace --stats, average per launch", "kernel_ms": kms, "bytes_model": model,
            "kernel_hbm_share_of_8TBps": {n: round(model[n] / (kms[n] * 1e-3) / HBM_BYTES_PER_S, 4) for n in names}}


def run_trace(K, B, a):
    """The HIP path alone, for a kernel trace."""
    import torch
    from dynamic3dgaussians_amd import motion_positions
    dev = torch.device("cuda", 0)
    t, ts, w = inputs(a.points, K, B, dev)
    for _ in range(a.inner):
        pair(motion_positions, t, ts, w)
    torch.cuda.synchronize()
    print(f"traced {a.inner} pairs at G {a.points} K {K} B {B}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--points", type=int, default=300_000)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "motion", "bench.json"))
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--trace", nargs=2, type=int, metavar=("K", "B"), default=None)
    ap.add_argument("--shares", nargs=2, type=int, metavar=("K", "B"), default=None)
    ap.add_argument("--kernel-ms", default=None, help="with --shares: fwd,bwd,sum,scatter kernel times in ms")
    ap.add_argument("--child", nargs=2, type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.trace:
        run_trace(a.trace[0], a.trace[1], a)
        return 0
    if a.shares:
        if not a.kernel_ms or len(a.kernel_ms.split(",")) != 4:
            ap.error("--shares needs --kernel-ms fwd,bwd,sum,scatter")
        rec = json.dumps(kernel_shares(a.shares[0], a.shares[1], a))
        print(rec)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(rec + "\n")
        return 0
    if a.child:  # one configuration, in its own process: print its record
        print("RECORD " + json.dumps(run_config(a.child[0], a.child[1], a)), flush=True)
        return 0
    if a.runs < 20:
        ap.error("--runs must be at least 20")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for K, B in CONFIGS:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(K), str(B), "--runs", str(a.runs),
               "--warmup", str(a.warmup), "--inner", str(a.inner), "--points", str(a.points)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout, cwd=REPO)
        except subprocess.TimeoutExpired:
            print(f"K{K}_B{B}: no result within {a.step_timeout} s; stopping", file=sys.stderr)
            return 124
        recs = [ln[7:] for ln in r.stdout.splitlines() if ln.startswith("RECORD ")]
        if r.returncode != 0 or not recs:  # nothing more is started on the device after a failure
            print(f"K{K}_B{B}: exit status {r.returncode}\n{r.stderr[-3000:]}", file=sys.stderr)
            return r.returncode or 1
        print(recs[-1], flush=True)
        with open(a.out, "a") as f:
            f.write(recs[-1] + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
