#!/usr/bin/env python3
"""The fused 1x1 feature decoder + L1 loss, forward + backward per call: the HIP kernels
(dynamic3dgaussians_amd.decoded_l1_loss) against the PyTorch formulation on the same device --
F.conv2d 1x1 -> abs().mean() per camera -> autograd -- at the rig's prior size, 27 x 288 x 512,
for 32 -> 64 channels (the reference's rule on this project's 32 rendered channels) and
64 -> 128, each with no mask and with an 80 % mask.

Device events around `reps` calls, after a warm-up of both; the implementations alternate
inside one process (`rounds` times) and the median round is reported with the rounds.
Timings of the HIP path:

    hip            the autograd function as a training step calls it
    hip_forward    the loss forward through the C ABI on preallocated buffers
    hip_backward   the loss backward, the same way
    fill           torch's fill of a buffer of target's size: the plain streaming rate the byte
                   model is compared with

Models per pixel (include/gs_feature_decoder.h; slabs and partials not counted): forward
4 (F_in + C_out) + 4 bytes and 2 F_in C_out flops, backward 4 (F_in + C_out) + 4 read,
4 F_in written and 6 F_in C_out flops.  The matrix rate the flop model is compared with is the
nominal bf16 rate, 1024 flop per clock and SIMD on 1024 SIMDs at 2.4 GHz; one fp32-equivalent
flop costs six bf16 piece flops (three against the sign tile).

The run is a child process of its own under a time limit.  One JSON line per case, appended
to --out (default profiles/feature_decoder/bench.json).

    python tools/feature_decoder_bench.py [--reps 10] [--rounds 5] [--cams 27] [--size 288 512]
    python tools/feature_decoder_bench.py --parity    # tests/test_gpu_feature_decoder.py's error / bound
                                                      # fractions -> profiles/feature_decoder/parity.json
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

WORKLOADS = ((32, 64), (64, 128))
MATRIX_FLOPS = 1024 * 1024 * 2.4e9


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


def torch_formulation(x, conv_w, bias, target, mask):
    """revise_train.py:102-104 per camera, summed: the decoded map exists, is read back for the
    L1 and kept for autograd."""
    import torch.nn.functional as F
    y = F.conv2d(x, conv_w, bias)
    d = y - target
    if mask is not None:
        d = d * mask[:, None]
    return d.abs().mean(dim=(1, 2, 3)).sum()


def run(a, F_in, C_out, masked):
    import torch
    from dynamic3dgaussians_amd import _lib, decoded_l1_loss
    dev = torch.device("cuda", 0)
    B, (h, w) = a.cams, a.size
    n = B * h * w
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(B, F_in, h, w, device=dev, generator=gen).requires_grad_(True)
    W = (torch.randn(C_out, F_in, device=dev, generator=gen) / F_in ** 0.5).requires_grad_(True)
    b = torch.randn(C_out, device=dev, generator=gen).requires_grad_(True)
    target = torch.randn(B, C_out, h, w, device=dev, generator=gen)
    mask = (torch.rand(B, h, w, device=dev, generator=gen) < 0.8).float() if masked else None
    leaves = (x, W, b)

    def call(fn):
        for t in leaves:
            t.grad = None
        loss = fn() * (1.0 / B)
        loss.backward()
        return loss.detach(), [t.grad for t in leaves]

    L = _lib.load()
    stream = _lib.stream(dev)
    loss = torch.empty(B, device=dev)
    up = torch.full((B,), 1.0 / B, device=dev)
    d_x, d_w, d_b = torch.empty_like(x), torch.empty_like(W), torch.empty_like(b)
    ws_f = torch.empty(L.gs_feature_decoder_workspace_bytes(B, F_in, C_out, h, w, _lib.FD_PASS_LOSS), dtype=torch.uint8,
                       device=dev)
    ws_b = torch.empty(L.gs_feature_decoder_workspace_bytes(B, F_in, C_out, h, w, _lib.FD_PASS_LOSS_BACKWARD),
                       dtype=torch.uint8, device=dev)

    def block(ws):
        return _lib.GsFeatureDecoder(B=B, F_in=F_in, C_out=C_out, h=h, w=w, mask_per_camera=1, x=x.data_ptr(),
                                     weight=W.data_ptr(), bias=b.data_ptr(), target=target.data_ptr(),
                                     mask=mask.data_ptr() if masked else None, up=up.data_ptr(), loss=loss.data_ptr(),
                                     d_x=d_x.data_ptr(), d_weight=d_w.data_ptr(), d_bias=d_b.data_ptr(),
                                     workspace=ws.data_ptr(), workspace_bytes=ws.numel())
    args_f, args_b = block(ws_f), block(ws_b)

    def forward():
        _lib.check(L.gs_feature_decoder_loss_forward(args_f, stream), "feature decoder loss forward")

    def backward():
        _lib.check(L.gs_feature_decoder_loss_backward(args_b, stream), "feature decoder loss backward")

    fill_buf = torch.empty_like(target)
    impls = {"hip": lambda: call(lambda: decoded_l1_loss(x, W, b, target, mask=mask)),
             "torch": lambda: call(lambda: torch_formulation(x, W[:, :, None, None], b, target, mask)),
             "hip_forward": forward, "hip_backward": backward, "fill": lambda: fill_buf.fill_(1.0)}
    base = torch.cuda.memory_allocated(dev)
    peak, out = {}, {}
    for k in ("hip", "torch"):  # warm-up, parity and peak memory
        impls[k]()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        res = impls[k]()
        torch.cuda.synchronize()
        peak[k] = torch.cuda.max_memory_allocated(dev) - base
        out[k] = (res[0].item(), [g.clone() for g in res[1]])
    forward()
    backward()
    torch.cuda.synchronize()
    same_bits = bool(torch.equal(d_x, out["hip"][1][0]) and torch.equal(d_w, out["hip"][1][1]))

    ms = {k: [] for k in impls}
    for fn in impls.values():
        fn()
    torch.cuda.synchronize()
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
    fill_rate = 4 * C_out * n / (med["fill"] * 1e-3)
    fwd_bytes, bwd_bytes = 4 * (F_in + C_out) + 4, 4 * (F_in + C_out) + 4 + 4 * F_in
    fwd_flops, bwd_flops = 2 * F_in * C_out, 6 * F_in * C_out
    return {"step": "feature_decoder", "shape": [B, F_in, C_out, h, w], "masked": bool(masked),
            "reps": a.reps, "rounds": a.rounds,
            "ms": {k: round(v, 4) for k, v in med.items()},
            "ms_rounds": {k: [round(v, 4) for v in vs] for k, vs in ms.items()},
            "torch_over_hip": round(med["torch"] / med["hip"], 2),
            "torch_over_hip_kernels": round(med["torch"] / (med["hip_forward"] + med["hip_backward"]), 2),
            "peak_bytes_over_inputs": peak, "decoded_map_bytes": 4 * C_out * n,
            "workspace_bytes": {"forward": int(ws_f.numel()), "backward": int(ws_b.numel())},
            "fill_bytes_per_s": round(fill_rate, -9),
            "model_per_pixel": {"forward_bytes": fwd_bytes, "backward_bytes": bwd_bytes, "forward_flops": fwd_flops,
                                "backward_flops": bwd_flops},
            "share_of_fill_rate": {"forward": round(fwd_bytes * n / (med["hip_forward"] * 1e-3) / fill_rate, 4),
                                   "backward": round(bwd_bytes * n / (med["hip_backward"] * 1e-3) / fill_rate, 4)},
            "share_of_matrix_rate": {"forward": round(fwd_flops * n / (med["hip_forward"] * 1e-3) / MATRIX_FLOPS, 4),
                                     "backward": round(bwd_flops * n / (med["hip_backward"] * 1e-3) / MATRIX_FLOPS, 4)},
            "c_abi_gradient_equals_autograd_bits": same_bits,
            "parity_vs_torch_fp32": {"loss_rel": abs(out["hip"][0] - out["torch"][0]) / max(abs(out["torch"][0]), 1e-30),
                                     "d_x_rel_l2": _rel(out["hip"][1][0], out["torch"][1][0]),
                                     "d_W_rel_l2": _rel(out["hip"][1][1], out["torch"][1][1]),
                                     "d_b_rel_l2": _rel(out["hip"][1][2], out["torch"][1][2])}}


def parity():
    """Every comparison of tests/test_gpu_feature_decoder.py's fp64 parity test: the largest
    error / bound per quantity over all shapes."""
    from tests import test_gpu_feature_decoder as t
    worst = {}
    for shape in t.SHAPES:
        for with_bias in (True, False):
            t.FRACTIONS.clear()
            t.test_against_the_fp64_twin(shape, with_bias)
            for name, frac in t.FRACTIONS:
                key = name.split("[")[0]
                rec = worst.setdefault(key, {"max_error_over_bound": 0.0, "shape": None})
                if frac >= rec["max_error_over_bound"]:
                    rec.update(max_error_over_bound=round(frac, 4), shape=list(shape))
    return {"step": "feature_decoder_parity", "shapes": [list(s) for s in t.SHAPES], "worst": worst}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cams", type=int, default=27)
    ap.add_argument("--size", type=int, nargs=2, default=[288, 512])
    ap.add_argument("--parity", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:  # one measurement in its own process: print its record
        if a.child == "parity":
            rec = parity()
        else:
            F_in, C_out, masked = (int(v) for v in a.child.split(","))
            rec = run(a, F_in, C_out, masked)
        print("RECORD " + json.dumps(rec), flush=True)
        return 0
    out = a.out or os.path.join(REPO, "profiles", "feature_decoder", "parity.json" if a.parity else "bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    cases = ["parity"] if a.parity else [f"{f},{c},{m}" for f, c in WORKLOADS for m in (0, 1)]
    for case in cases:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", case, "--reps", str(a.reps), "--rounds",
               str(a.rounds), "--cams", str(a.cams), "--size", str(a.size[0]), str(a.size[1])]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout, cwd=REPO)
        except subprocess.TimeoutExpired:
            print(f"{case}: no result within {a.step_timeout} s", file=sys.stderr)
            return 124
        recs = [ln[7:] for ln in r.stdout.splitlines() if ln.startswith("RECORD ")]
        if r.returncode != 0 or not recs:
            print(f"{case}: exit status {r.returncode}\n{r.stderr[-3000:]}", file=sys.stderr)
            return r.returncode or 1
        print(recs[-1], flush=True)
        with open(out, "a") as f:
            f.write(recs[-1] + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
