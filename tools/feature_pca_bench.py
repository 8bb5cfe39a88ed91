#!/usr/bin/env python3
"""The feature-map PCA colouring: the HIP path (dynamic3dgaussians_amd.FeaturePCA) against its
PyTorch twin (FeaturePCATorch: normalize, boolean indexing to [n, C], X^T X in float64,
linalg.eigh, einsum, amin / amax) on the same device, at the rig's sizes 27 x 32 x 800 x 800 and
27 x 64 x 288 x 512 with an 80 % mask.

    fit            FeaturePCA(C).update(x, mask).fit(): the shift pass, the Gram pass, the eigensolve
    colourise      pca.colourise(x, mask): project, min / max range, uint8 colours
    update         one more update on the same object (the shift exists: x is read once)
    project        pca_project with its range reduction
    colour         pca_colour to uint8
    fill           torch's fill of a buffer of x's size: the plain streaming rate the byte models
                   are compared with

Device events around `reps` calls, after a warm-up of both; the implementations alternate inside
one process (`rounds` times) and the median round is reported with the rounds.  Byte models per
pixel (include/gs_feature_pca.h): update 4 C read, project 4 C read + 4 k written, colour 4 k read
+ 3 written (the mask byte not counted).  `eigensolve` is the one-workgroup fit alone at C = 32,
64 and 128.

Every case is a child process of its own under a time limit.  One JSON line per case, appended to
--out (default profiles/feature_pca/bench.json).

    python tools/feature_pca_bench.py [--reps 5] [--rounds 5]
    python tools/feature_pca_bench.py --parity    # tests/test_gpu_feature_pca.py's error / bound
                                                  # fractions -> profiles/feature_pca/parity.json
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

WORKLOADS = ((27, 32, 800, 800), (27, 64, 288, 512))
EIG_ORDERS = (32, 64, 128)


def _timed(impls, reps, rounds):
    import torch
    ms = {k: [] for k in impls}
    for fn in impls.values():
        fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, fn in impls.items():
            s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s0.record()
            for _ in range(reps):
                fn()
            s1.record()
            torch.cuda.synchronize()
            ms[k].append(s0.elapsed_time(s1) / reps)
    return ms


def run(a, B, C, H, W):
    import torch
    from dynamic3dgaussians_amd import FeaturePCA, FeaturePCATorch, pca_colour, pca_project
    dev = torch.device("cuda", 0)
    n = B * H * W
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(B, C, H, W, device=dev, generator=gen)
    x *= torch.linspace(4.0, 0.5, C, device=dev)[None, :, None, None]
    x += 1.0
    mask = (torch.rand(B, H, W, device=dev, generator=gen) < 0.8).to(torch.uint8)

    hip = FeaturePCA(C).update(x, mask).fit()
    twin = FeaturePCATorch(C).update(x, mask).fit()
    t, tmin, tmax = hip.transform(x, mask, return_range=True)
    lo, hi = tmin.amin(1, keepdim=True).double(), tmax.amax(1, keepdim=True).double()
    fill_buf = torch.empty_like(x)
    impls = {"fit": lambda: FeaturePCA(C).update(x, mask).fit(),
             "fit_torch": lambda: FeaturePCATorch(C).update(x, mask).fit(),
             "colourise": lambda: hip.colourise(x, mask),
             "colourise_torch": lambda: twin.colourise(x, mask),
             "update": lambda: hip.update(x, mask),
             "project": lambda: pca_project(x, hip.components_f32_, hip.mean_f32_, mask, return_range=True),
             "colour": lambda: pca_colour(t, lo, hi, mask),
             "fill": lambda: fill_buf.fill_(1.0)}
    base = torch.cuda.memory_allocated(dev)
    peak = {}
    for k in ("fit", "fit_torch", "colourise", "colourise_torch"):  # warm-up and peak memory over the inputs
        impls[k]()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        impls[k]()
        torch.cuda.synchronize()
        peak[k] = torch.cuda.max_memory_allocated(dev) - base
    img, img_t = hip.colourise(x, mask), twin.colourise(x, mask)
    diff = (img.int() - img_t.int()).abs()
    sub = hip.components_.double() @ twin.components_.double().T  # the two top-3 subspaces
    ms = _timed(impls, a.reps, a.rounds)
    med = {k: statistics.median(v) for k, v in ms.items()}
    fill_rate = 4 * C * n / (med["fill"] * 1e-3)
    model = {"update": 4 * C, "project": 4 * C + 4 * 3, "colour": 4 * 3 + 3}
    return {"step": "feature_pca", "shape": [B, C, H, W], "mask_share": 0.8, "reps": a.reps, "rounds": a.rounds,
            "ms": {k: round(v, 4) for k, v in med.items()},
            "ms_rounds": {k: [round(v, 4) for v in vs] for k, vs in ms.items()},
            "torch_over_hip": {"fit": round(med["fit_torch"] / med["fit"], 2),
                               "colourise": round(med["colourise_torch"] / med["colourise"], 2)},
            "peak_bytes_over_inputs": peak, "input_bytes": 4 * C * n,
            "fill_bytes_per_s": round(fill_rate, -9), "model_bytes_per_pixel": model,
            "share_of_fill_rate": {k: round(v * n / (med[k] * 1e-3) / fill_rate, 4) for k, v in model.items()},
            "status": int(hip.status.item()),
            "parity_vs_torch_fp32": {"uint8_differing_share": float((diff > 0).float().mean()),
                                     "uint8_max_difference": int(diff.max()),
                                     "subspace_singular_values_min": float(torch.linalg.svdvals(sub).min())}}


def run_eig(a):
    import torch
    from dynamic3dgaussians_amd import FeaturePCA
    dev = torch.device("cuda", 0)
    out = {}
    for C in EIG_ORDERS:
        gen = torch.Generator(device=dev).manual_seed(C)
        x = torch.randn(1, C, 64, 64, device=dev, generator=gen) * torch.linspace(4.0, 0.5, C, device=dev)[None, :, None, None]
        pca = FeaturePCA(C).update(x).fit()
        ms = _timed({"fit": pca.fit}, a.reps, a.rounds)["fit"]
        out[str(C)] = {"ms": round(statistics.median(ms), 4), "ms_rounds": [round(v, 4) for v in ms],
                       "status": int(pca.status.item())}
    return {"step": "feature_pca_eigensolve", "workgroups": 1, "reps": a.reps, "rounds": a.rounds, "orders": out}


def parity():
    """Every comparison of tests/test_gpu_feature_pca.py's fp64 tests: the largest error / bound per
    quantity over all shapes, masks, normalize and strides."""
    from tests import _feature_pca_cases as K
    from tests import test_gpu_feature_pca as t
    worst = {}
    t.FRACTIONS.clear()
    for shape in K.SHAPES:
        for kind in K.MASKS:
            for normalize in (False, True):
                for stride in (1, 3):
                    t.test_against_fp64(shape, kind, normalize, stride)
    for shape in t.SUBSPACE:
        t.test_top3_subspace_matches_the_fp64_twin(shape)
    for name, frac in t.FRACTIONS:
        case, key = name.split(":")[0] if ":" in name else name.rsplit(" ", 2)[0], name.split(":")[-1].strip()
        if ":" not in name:
            key = "top-3 subspace"
        rec = worst.setdefault(key, {"max_error_over_bound": 0.0, "case": None})
        if frac >= rec["max_error_over_bound"]:
            rec.update(max_error_over_bound=round(frac, 4), case=case)
    return {"step": "feature_pca_parity", "shapes": [list(s) for s in K.SHAPES], "comparisons": len(t.FRACTIONS),
            "worst": worst}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parity", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:  # one measurement in its own process: print its record
        if a.child == "parity":
            rec = parity()
        elif a.child == "eig":
            rec = run_eig(a)
        else:
            rec = run(a, *(int(v) for v in a.child.split(",")))
        print("RECORD " + json.dumps(rec), flush=True)
        return 0
    out = a.out or os.path.join(REPO, "profiles", "feature_pca", "parity.json" if a.parity else "bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    cases = ["parity"] if a.parity else [",".join(map(str, w)) for w in WORKLOADS] + ["eig"]
    for case in cases:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", case, "--reps", str(a.reps), "--rounds", str(a.rounds)]
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
