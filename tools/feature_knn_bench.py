"""Exact cosine top-k in feature space (include/gs_feature_knn.h): time, memory, fallback share.

    python tools/feature_knn_bench.py              # the workloads below -> profiles/feature_knn/bench.json
    python tools/feature_knn_bench.py --parity     # tests/test_gpu_feature_knn.py's measured figures
                                                   # (fallback share per generator, largest |st - s| / B)
                                                   # -> profiles/feature_knn/parity.json
    rocprofv3 --kernel-trace --stats -d <dir> -o fk --output-format csv -- \\
        python tools/feature_knn_bench.py --profile-run self,300000,32,20
    python tools/feature_knn_bench.py --kernel-stats <dir>/.../fk_kernel_stats.csv --case self,300000,32,20
                                                   # per-kernel times and the scan's share of the bf16
                                                   # matrix rate under the 6 * 2 * M * N * E_pad flop model

Workloads: self search at 300k x 32 (k = 20), 100k x 64 (k = 20), 50k x 128 (k = 8); 16 queries of 32
channels against 300k rows; all-equal features at N = 20k, where every row goes to the exhaustive
fp64 search.  Features are clustered (8 centres + 0.15 noise), the realistic case for the
certificate.  The comparison is the reference's formulation where it fits: F.normalize, a chunked
fp32 matmul and topk(k + 1) on the same device (approximate: it orders by fp32 similarities).
Every workload runs in its own process; timings alternate between the two implementations.
"""
from __future__ import annotations

import argparse
import csv
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

WORKLOADS = ("self,300000,32,20", "self,100000,64,20", "self,50000,128,8", "query,300000,32,20,16", "equal,20000,32,20")
BF16_PEAK = 2.5e15  # dense bf16 matrix rate of the MI355X, flop/s


def _features(kind, n, e, dev, seed=0):
    import torch
    gen = torch.Generator(device=dev).manual_seed(seed)
    if kind == "equal":
        return (torch.rand(1, e, device=dev, generator=gen) + 0.05).repeat(n, 1)
    centres = torch.randn(8, e, device=dev, generator=gen)
    pick = torch.randint(0, 8, (n,), device=dev, generator=gen)
    return centres[pick] + 0.15 * torch.randn(n, e, device=dev, generator=gen)


def _matmul_topk(x, k, queries=None, chunk=4096):
    """The reference's search where the matrix is taken in row chunks: fp32, approximate order."""
    import torch
    import torch.nn.functional as F
    d = F.normalize(x, dim=1)
    q = d if queries is None else F.normalize(queries, dim=1)
    kk = min(k + (queries is None), d.shape[0])
    vals, idxs = [], []
    for m0 in range(0, q.shape[0], chunk):
        v, i = torch.topk(q[m0:m0 + chunk] @ d.T, kk, dim=1)
        vals.append(v)
        idxs.append(i)
    v, i = torch.cat(vals), torch.cat(idxs)
    return (v[:, 1:], i[:, 1:]) if queries is None else (v, i)


def _setup(case):
    import torch
    mode, n, e, k, *rest = case.split(",")
    n, e, k = int(n), int(e), int(k)
    dev = torch.device("cuda", 0)
    x = _features("equal" if mode == "equal" else "cluster", n, e, dev)
    q = _features("cluster", n + int(rest[0]), e, dev)[n:] if mode == "query" else None
    return mode, n, e, k, x, q


def run(a, case):
    import torch
    from dynamic3dgaussians_amd import _lib, feature_knn
    mode, n, e, k, x, q = _setup(case)
    dev = x.device
    m = n if q is None else q.shape[0]
    impls = {"hip": lambda: feature_knn(x, k, q), "matmul_topk": lambda: _matmul_topk(x, k, q)}
    base = torch.cuda.memory_allocated(dev)
    peak = {}
    for name, fn in impls.items():  # warm-up and peak memory over the inputs
        fn()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        fn()
        torch.cuda.synchronize()
        peak[name] = torch.cuda.max_memory_allocated(dev) - base
    ms = {name: [] for name in impls}
    for _ in range(a.rounds):
        for name, fn in impls.items():
            s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s0.record()
            for _ in range(a.reps):
                fn()
            s1.record()
            torch.cuda.synchronize()
            ms[name].append(s0.elapsed_time(s1) / a.reps)
    med = {name: statistics.median(v) for name, v in ms.items()}
    sim, index, stats = feature_knn(x, k, q, return_stats=True)
    certified, fallback = (int(v) for v in stats.cpu())
    _, approx = _matmul_topk(x, k, q)
    L = _lib.load()
    e_pad = L.gs_feature_knn_e_pad(e)
    return {"step": "feature_knn", "case": case, "M": m, "N": n, "E": e, "k": k, "reps": a.reps, "rounds": a.rounds,
            "splits": L.gs_feature_knn_splits(m, n, e, k), "ms": {name: round(v, 3) for name, v in med.items()},
            "ms_rounds": {name: [round(v, 3) for v in vs] for name, vs in ms.items()},
            "matmul_topk_over_hip": round(med["matmul_topk"] / med["hip"], 2),
            "peak_bytes_over_inputs": peak, "input_bytes": 4 * e * (n + (0 if q is None else m)),
            "dense_matrix_bytes": 4 * m * n, "certified": certified, "fallback": fallback,
            "fallback_share": round(fallback / m, 6), "scan_flop_model": 12 * m * n * e_pad,
            "whole_call_share_of_bf16_peak": round(12 * m * n * e_pad / (med["hip"] * 1e-3) / BF16_PEAK, 4),
            "rows_where_fp32_matmul_topk_differs": round(float((approx != index).any(dim=1).float().mean()), 4)}


def profile_run(case):
    import torch
    from dynamic3dgaussians_amd import feature_knn
    _, _, _, k, x, q = _setup(case)
    for _ in range(3):
        feature_knn(x, k, q)
    torch.cuda.synchronize()


def kernel_stats(path, case):
    mode, n, e, k, *rest = case.split(",")
    n, e = int(n), int(e)
    m = int(rest[0]) if mode == "query" else n
    e_pad = (e + 15) // 16 * 16
    kernels = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            for short in ("fk_normalize", "fk_pieces", "fk_scan", "fk_rerank", "fk_fallback"):
                if short in row["Name"]:
                    kernels[short] = {"calls": int(row["Calls"]), "average_ms": round(float(row["AverageNs"]) * 1e-6, 4)}
    rec = {"step": "feature_knn_kernels", "case": case, "source": "rocprofv3 --kernel-trace --stats, average per launch",
           "kernels": kernels}
    if "fk_scan" in kernels:
        rate = 12 * m * n * e_pad / (kernels["fk_scan"]["average_ms"] * 1e-3)
        rec["scan_flop_per_s"] = round(rate, -9)
        rec["scan_share_of_bf16_peak"] = round(rate / BF16_PEAK, 4)
    return rec


def parity():
    """The figures tests/test_gpu_feature_knn.py measures while it asserts exactness: the fallback
    share of every case per generator and the largest |st - s| / B over the kept candidates."""
    from tests import _feature_knn_cases as K
    from tests import test_gpu_feature_knn as t
    t.RECORDS.clear()
    for case in K.CASES:
        for kind in K.GENERATORS:
            t.test_self_search_is_exact_on_every_row(*case, kind)
            t.test_certificate_premise_holds_on_every_candidate(*case, kind)
    for which in ("duplicates", "zeros", "equal"):
        t.test_heavy_ties(which)
    share, worst = {}, {}
    for r in t.RECORDS:
        name = "x".join(map(str, r["case"]))
        if r["what"] == "fallback_share":
            share.setdefault(r["kind"], {})[name] = round(r["value"], 4)
        elif r["value"] >= worst.get(r["kind"], {"max_error_over_bound": -1.0})["max_error_over_bound"]:
            worst[r["kind"]] = {"max_error_over_bound": round(r["value"], 5), "case": name}
    return {"step": "feature_knn_parity", "cases": [list(c) for c in K.CASES], "exact_rows": "all, bit for bit",
            "fallback_share": share, "scan_error_over_bound": worst}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parity", action="store_true")
    ap.add_argument("--profile-run", default="")
    ap.add_argument("--kernel-stats", default="")
    ap.add_argument("--case", default=WORKLOADS[0])
    ap.add_argument("--out", default=None)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.profile_run:
        profile_run(a.profile_run)
        return 0
    if a.child:  # one measurement in its own process: print its record
        rec = parity() if a.child == "parity" else run(a, a.child)
        print("RECORD " + json.dumps(rec), flush=True)
        return 0
    out = a.out or os.path.join(REPO, "profiles", "feature_knn", "parity.json" if a.parity else "bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    if a.kernel_stats:
        rec = json.dumps(kernel_stats(a.kernel_stats, a.case))
        print(rec, flush=True)
        with open(out, "a") as f:
            f.write(rec + "\n")
        return 0
    for case in (["parity"] if a.parity else WORKLOADS):
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
