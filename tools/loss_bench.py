#!/usr/bin/env python3
"""Photometric loss (L1 + SSIM), forward + backward per call: the fused HIP
kernels (dynamic3dgaussians_amd.photometric_image_loss) against the PyTorch
formulation of the reference (photometric_loss_torch: five depthwise
convolutions and autograd) on the same device, at the training step's shapes:

    colour    27 x 3 x 800 x 800   with the per-camera colour correction
    features  27 x 32 x 800 x 800  without

Device events around `reps` calls, after a warm-up of both; the two
implementations alternate inside one process (`rounds` times) and the median
round is reported with the spread.  Each shape runs in a child process of its
own under a time limit; a child that fails ends the run.  A last step records
the envelope ratios of tests/test_gpu_image_loss.py's cases (the kernels'
image-gradient error over the fp32 reference formulation's own).  JSON lines,
appended to --out (default profiles/loss/bench.json).

    python tools/loss_bench.py [--reps 10] [--rounds 3] [--cams 27] [--size 800]

Bytes: the count is the algorithm's HBM traffic of the stored-maps design
 from shapes, in floats per pixel-channel: forward reads
image and target and writes the three derivative maps (5), backward reads the
three maps, image and target and writes the image gradient (6): 11 x 4 B x
B Ch H W.  Halo re-reads are expected to hit in cache and are not counted.
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
SHAPES = {"colour": (3, True), "features": (32, False)}


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


def run_shape(name, a):
    import torch
    from dynamic3dgaussians_amd import _lib, photometric_image_loss, photometric_loss_torch
    ch, corrected = SHAPES[name]
    dev = torch.device("cuda", 0)
    B, H, W = a.cams, a.size, a.size
    gen = torch.Generator(device=dev).manual_seed(0)
    im = torch.rand(B, ch, H, W, device=dev, generator=gen).requires_grad_(True)
    target = (im.detach() + 0.1 * torch.randn(B, ch, H, W, device=dev, generator=gen)).clamp_(0, 1)
    cam_m = cam_c = None
    if corrected:
        cam_m = (0.05 * torch.randn(B, ch, device=dev, generator=gen)).requires_grad_(True)
        cam_c = (0.02 * torch.randn(B, ch, device=dev, generator=gen)).requires_grad_(True)
    leaves = [x for x in (im, cam_m, cam_c) if x is not None]

    def fused():
        return photometric_image_loss(im, target, cam_m=cam_m, cam_c=cam_c)

    def plain():
        if corrected:
            return photometric_loss_torch(im, target, gain=torch.exp(cam_m), offset=cam_c)
        return photometric_loss_torch(im, target)

    def call(fn):
        for x in leaves:
            x.grad = None
        loss = fn() / B
        loss.backward()
        return loss.detach(), [x.grad for x in leaves]

    impls = {"hip": fused, "torch": plain}
    base = torch.cuda.memory_allocated(dev)
    peak, out = {}, {}
    for k, fn in impls.items():  # warm-up, parity and peak memory
        call(fn)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        out[k] = call(fn)
        torch.cuda.synchronize()
        peak[k] = torch.cuda.max_memory_allocated(dev) - base
        out[k] = (out[k][0].item(), [g.clone() for g in out[k][1]])
    ms = {k: [] for k in impls}
    for _ in range(a.rounds):
        for k, fn in impls.items():
            s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s0.record()
            for _ in range(a.reps):
                call(fn)
            s1.record()
            torch.cuda.synchronize()
            ms[k].append(s0.elapsed_time(s1) / a.reps)
    # both fp32 paths against the torch formulation in fp64 on the device (one call): says which
    # of the two is off when they disagree (one pixel of 5e7 on the other side of |x - y|'s kink
    # is a relative L2 of 2 / sqrt(5e7) = 3e-4 in the image gradient)
    im64 = im.detach().double().requires_grad_(True)
    m64 = cam_m.detach().double().requires_grad_(True) if corrected else None
    c64 = cam_c.detach().double().requires_grad_(True) if corrected else None
    kw64 = dict(gain=torch.exp(m64), offset=c64) if corrected else {}
    loss64 = photometric_loss_torch(im64, target.double(), **kw64) / B
    g64 = torch.autograd.grad(loss64, [x for x in (im64, m64, c64) if x is not None])
    def without_largest(x, y, k=16):  # the image gradient's relative L2 with the k worst pixels left out
        d = (x.double() - y).flatten()
        keep = torch.ones_like(d, dtype=torch.bool)
        keep[d.abs().topk(k).indices] = False
        return float(d[keep].norm() / y.norm())

    vs64 = {k: {"loss_rel": abs(out[k][0] - loss64.item()) / abs(loss64.item()),
                "grads_rel_l2": [_rel(x, y) for x, y in zip(out[k][1], g64)],
                "d_image_rel_l2_without_16_largest": without_largest(out[k][1][0], g64[0])} for k in impls}
    del im64, loss64, g64
    n = B * ch * H * W
    hbm = 11 * 4 * n
    med = {k: statistics.median(v) for k, v in ms.items()}
    rec = {"step": name, "shape": [B, ch, H, W], "colour_correction": corrected, "reps": a.reps, "rounds": a.rounds,
           "ms_fwd_bwd": {k: round(v, 4) for k, v in med.items()},
           "ms_rounds": {k: [round(x, 4) for x in v] for k, v in ms.items()},
           "torch_over_hip": round(med["torch"] / med["hip"], 3),
           "peak_bytes_over_inputs": peak,
           "workspace_bytes": int(_lib.load().gs_photo_loss_workspace_bytes(B, ch, H, W)),
           "hbm_bytes_model": hbm, "hbm_model": "stored maps: 11 floats per pixel-channel (fwd 2 r + 3 w, bwd 5 r + 1 w)",
           "hbm_share_of_8TBps": round(hbm / (med["hip"] * 1e-3) / HBM_BYTES_PER_S, 4),
           "parity_vs_torch_fp32": {
               "loss_rel": abs(out["hip"][0] - out["torch"][0]) / max(abs(out["torch"][0]), 1e-30),
               "grads_rel_l2": [_rel(x, y) for x, y in zip(out["hip"][1], out["torch"][1])]},
           "vs_torch_fp64_on_device": vs64}
    return rec


def run_envelope(a):
    """The image-gradient envelope ratios of the GPU tests' cases."""
    import torch
    from dynamic3dgaussians_amd import photometric_loss
    from tests import test_gpu_image_loss as T
    ratios = {}
    for name in ("small", "two_cams", "flat", "tiles", "features"):
        ref, ref32 = T._oracle(name)
        got = T._run(photometric_loss, T._case(name), torch.float32, T.DEV)
        ratios[name] = {"d_image_rel_l2": T._rel(got[1], ref[1]), "fp32_reference_rel_l2": ref32,
                        "ratio": T._rel(got[1], ref[1]) / ref32}
    return {"step": "envelope", "cases": ratios}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cams", type=int, default=27)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "loss", "bench.json"))
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
               str(a.rounds), "--cams", str(a.cams), "--size", str(a.size)]
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
