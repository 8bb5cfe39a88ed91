"""Spectral clustering of the feature kNN graph (include/gs_spectral.h): time, memory, iterations.

    python tools/spectral_bench.py              # the workloads below -> profiles/spectral/bench.json
    python tools/spectral_bench.py --parity     # the largest error / bound of every check of
                                                # tests/test_gpu_spectral.py -> profiles/spectral/parity.json
    rocprofv3 --kernel-trace --stats -d <dir> -o sp --output-format csv -- \\
        python tools/spectral_bench.py --profile-run cluster,300000,32,20,49,0.15
    python tools/spectral_bench.py --kernel-stats <dir>/.../sp_kernel_stats.csv --case cluster,300000,32,20,49,0.15
                                                # per-kernel times and the SpMM's share of the plain
                                                # fill's streaming rate under the byte model
                                                # nnz (12 + 8 B) + 3 * 8 n B

Workloads (features: 8 centres + noise, as the feature search's bench): 300k x 32, knn = 20, K = 49
(the reference's hard-coded cluster count) and 100k x 64, knn = 20, K = 10 at noise 0.15, and one
connected, hard case at noise 0.8.  Per workload: the whole spectral_clustering call and its parts
(kNN, graph, embedding, k-means), the outer iterations used, the residual reached, peak memory over
the inputs.  The baseline is spectral_embedding_torch on the same device (torch's sparse CSR fp64
product, torch.linalg.eigh for the small problems); samples alternate in one process; median and
range.  Every workload runs in its own process.
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

WORKLOADS = ("cluster,300000,32,20,49,0.15", "cluster,100000,64,20,10,0.15", "cluster,100000,32,20,10,0.8")
FILL_RATE = 6.9e12  # the plain fill's streaming rate on the MI355X, bytes/s
KERNELS = ("sp_degree", "sp_start", "sp_spmm", "sp_gram_kernel", "sp_gram_reduce", "sp_svqb", "sp_ritz", "sp_rotate",
           "sp_resid", "sp_check", "sp_embed")


def _features(n, e, noise, dev, seed=0):
    import torch
    gen = torch.Generator(device=dev).manual_seed(seed)
    centres = torch.randn(8, e, device=dev, generator=gen)
    pick = torch.randint(0, 8, (n,), device=dev, generator=gen)
    return centres[pick] + noise * torch.randn(n, e, device=dev, generator=gen)


def _setup(case):
    import torch
    _, n, e, knn, K, noise = case.split(",")
    n, e, knn, K, noise = int(n), int(e), int(knn), int(K), float(noise)
    dev = torch.device("cuda", 0)
    return n, e, knn, K, noise, _features(n, e, noise, dev)


def _timed(fn, reps=1):
    import torch
    s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s0.record()
    for _ in range(reps):
        out = fn()
    s1.record()
    torch.cuda.synchronize()
    return s0.elapsed_time(s1) / reps, out


def _summary(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def run(a, case):
    import torch
    from dynamic3dgaussians_amd import (_lib, feature_knn, knn_graph, kmeans, spectral_clustering, spectral_embedding,
                                        spectral_embedding_torch)
    n, e, knn, K, noise, x = _setup(case)
    dev = x.device
    sim, index = feature_knn(x, knn)
    row_ptr, col, val = knn_graph(sim, index, n)
    nnz = col.numel()
    B = _lib.load().gs_spectral_block_width(n, K)
    solver = dict(tol=a.tol, degree=a.degree, max_outer=a.max_outer)
    impls = {"hip": lambda: spectral_embedding(row_ptr, col, val, K, **solver)}
    baseline_error = None
    try:
        spectral_embedding_torch(row_ptr, col, val, K, **solver)
        impls["torch"] = lambda: spectral_embedding_torch(row_ptr, col, val, K, **solver)
    except Exception as ex:  # torch's sparse CSR product may be missing on a build
        baseline_error = f"{type(ex).__name__}: {ex}"[:300]
    base = torch.cuda.memory_allocated(dev)
    peak = {}
    for name, fn in impls.items():
        fn()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        fn()
        torch.cuda.synchronize()
        peak[name] = torch.cuda.max_memory_allocated(dev) - base
    ms = {name: [] for name in impls}
    for _ in range(a.rounds):
        for name, fn in impls.items():
            ms[name].append(_timed(fn, a.reps)[0])
    # the whole call and its parts
    whole, parts = [], {"knn": [], "graph": [], "embedding": [], "kmeans": []}
    for _ in range(a.rounds):
        whole.append(_timed(lambda: spectral_clustering(x, K, knn=knn, **solver))[0])
        t, (s, i) = _timed(lambda: feature_knn(x, knn))
        parts["knn"].append(t)
        t, g = _timed(lambda: knn_graph(s, i, n))
        parts["graph"].append(t)
        t, emb = _timed(lambda: spectral_embedding(*g, K, **solver))
        parts["embedding"].append(t)
        parts["kmeans"].append(_timed(lambda: kmeans(emb.embedding, K, iters=10))[0])
    out = spectral_embedding(row_ptr, col, val, K, **solver)
    status = out.status.tolist()
    rec = {"step": "spectral", "case": case, "n": n, "E": e, "knn": knn, "K": K, "noise": noise, "nnz": nnz, "B": B,
           "solver": solver, "reps": a.reps, "rounds": a.rounds,
           "embedding_ms": {name: _summary(v) for name, v in ms.items()},
           "clustering_ms": _summary(whole), "parts_ms": {k: _summary(v) for k, v in parts.items()},
           "status": status, "outer_iterations": status[1], "largest_residual": float(out.residuals.max()),
           "eigenvalues_first_last": [float(out.eigenvalues[0]), float(out.eigenvalues[-1])],
           "peak_bytes_over_inputs": peak, "input_bytes": 8 * (n + 1) + 12 * nnz,
           "dense_matrix_bytes": 8 * n * n, "spmm_byte_model": nnz * (12 + 8 * B) + 3 * 8 * n * B}
    if "torch" in ms:
        tw = spectral_embedding_torch(row_ptr, col, val, K, **solver)
        rec["torch_status"] = tw.status.tolist()
        rec["torch_over_hip"] = round(statistics.median(ms["torch"]) / statistics.median(ms["hip"]), 2)
    if baseline_error:
        rec["baseline_error"] = baseline_error
    return rec


def profile_run(a, case):
    import torch
    from dynamic3dgaussians_amd import feature_knn, knn_graph, spectral_embedding
    n, e, knn, K, noise, x = _setup(case)
    g = knn_graph(*feature_knn(x, knn), n)
    for _ in range(2):
        spectral_embedding(*g, K, tol=a.tol, degree=a.degree, max_outer=a.max_outer)
    torch.cuda.synchronize()


def kernel_stats(path, case, nnz):
    _, n, e, knn, K, noise = case.split(",")
    n, K = int(n), int(K)
    B = min(n, 8 * ((K + 8 + 7) // 8))
    kernels = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            for short in KERNELS:
                if short in row["Name"]:
                    k = kernels.setdefault(short, {"calls": 0, "total_ms": 0.0})
                    k["calls"] += int(row["Calls"])
                    k["total_ms"] += float(row["TotalDurationNs"]) * 1e-6
    for k in kernels.values():
        k["total_ms"] = round(k["total_ms"], 3)
    rec = {"step": "spectral_kernels", "case": case, "B": B,
           "source": "rocprofv3 --kernel-trace --stats; launches that found the done flag set return at once and "
                     "are counted in calls", "kernels": kernels}
    if nnz:
        rec["nnz"] = nnz
        rec["spmm_byte_model"] = nnz * (12 + 8 * B) + 3 * 8 * n * B
        if "sp_spmm" in kernels:
            avg = kernels["sp_spmm"]["total_ms"] / kernels["sp_spmm"]["calls"]
            rec["spmm_average_ms"] = round(avg, 4)
            rec["spmm_bytes_per_s"] = round(rec["spmm_byte_model"] / (avg * 1e-3), -9)
            rec["spmm_share_of_fill_rate"] = round(rec["spmm_byte_model"] / (avg * 1e-3) / FILL_RATE, 3)
    return rec


def parity():
    """The largest error / bound of every check tests/test_gpu_spectral.py makes while it asserts,
    and, where scikit-learn is importable, the adjusted Rand index of the pipeline's labels against
    its SpectralClustering(affinity='precomputed') on blobs-b and blobs-c."""
    from tests import _spectral_cases as C
    from tests import test_gpu_spectral as t
    t.RECORDS.clear()
    for name, K in C.SMALL:
        t.test_against_the_dense_oracle(name, K)
    t.test_large_sparse_checks_and_labels()
    rec = {"step": "spectral_parity", "cases": [list(c) for c in C.SMALL] + [["large", 12]],
           "largest_error_over_bound": {k: round(v, 6) for k, v in t.RECORDS.items()}}
    try:
        from sklearn.cluster import SpectralClustering
        from sklearn.metrics import adjusted_rand_score
    except ImportError:
        rec["sklearn"] = "not importable here: no adjusted Rand index recorded"
        return rec
    from dynamic3dgaussians_amd import spectral_clustering
    ari = {}
    for name, K in (("blobs-b", 5), ("blobs-c", 8)):
        c = C.small_case(name)
        mine = spectral_clustering(c.feats.to("cuda"), K, knn=c.knn).labels.cpu().numpy()
        A = C.oracle(name).S * 0
        r = C.SP._rows_of(c.row_ptr)
        A[r, c.col.long()] = c.val
        theirs = SpectralClustering(n_clusters=K, affinity="precomputed", random_state=0).fit_predict(A.numpy())
        ari[name] = round(float(adjusted_rand_score(theirs, mine)), 4)
    rec["adjusted_rand_index_vs_sklearn"] = ari
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--degree", type=int, default=8)
    ap.add_argument("--max-outer", type=int, default=30)
    ap.add_argument("--parity", action="store_true")
    ap.add_argument("--profile-run", default="")
    ap.add_argument("--kernel-stats", default="")
    ap.add_argument("--nnz", type=int, default=0, help="with --kernel-stats: the graph's nnz, for the byte model")
    ap.add_argument("--case", default=WORKLOADS[0])
    ap.add_argument("--only", default="", help="run this one workload")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.profile_run:
        profile_run(a, a.profile_run)
        return 0
    if a.child:  # one measurement in its own process: print its record
        rec = parity() if a.child == "parity" else run(a, a.child)
        print("RECORD " + json.dumps(rec), flush=True)
        return 0
    out = a.out or os.path.join(REPO, "profiles", "spectral", "parity.json" if a.parity else "bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    if a.kernel_stats:
        rec = json.dumps(kernel_stats(a.kernel_stats, a.case, a.nnz))
        print(rec, flush=True)
        with open(out, "a") as f:
            f.write(rec + "\n")
        return 0
    for case in (["parity"] if a.parity else ([a.only] if a.only else WORKLOADS)):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", case, "--reps", str(a.reps), "--rounds",
               str(a.rounds), "--tol", str(a.tol), "--degree", str(a.degree), "--max-outer", str(a.max_outer)]
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
