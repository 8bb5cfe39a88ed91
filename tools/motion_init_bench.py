"""Timing of the motion-basis initialisation (dynamic3dgaussians_amd/motion_init.py) against the
PyTorch formulation on the same GPU.  Writes profiles/motion_init/bench.json.

    python tools/motion_init_bench.py                       # wall times, three alternating samples each
    rocprofv3 --kernel-trace --stats -d <dir> -o mi -- python tools/motion_init_bench.py --profile-run
    python tools/motion_init_bench.py --merge-stats <dir>/.../mi_kernel_stats.csv

Workloads: k-means, 10 iterations, at 100k x 447 with K = 20 (velocity directions of 100k tracks x
150 frames) and at 300k x 32 with K = 49 (the dyn_train.py setting); the whole
init_motion_bases_from_tracks at 100k tracks x 150 frames.

Baseline: torch.cdist + argmin + index_add_ for k-means (fp32, on the device); for the Procrustes
part of the whole call a batched torch.linalg.svd Kabsch per frame over zero-padded clusters (on the
device when linalg.svd runs there, else on the host: `svd_device` in the record says which).

--merge-stats adds the kernels' own times (a rocprofv3 run of its own) and each k-means kernel's
share of its larger bound: assign reads 4 N D bytes and does 3 N K D flops, update reads 4 N D + 8 N
bytes and writes and re-reads its partial sums; the bound that takes longer at 6.3 TB/s / 157.3
TFLOP/s is named.  Without a GPU every number is "not measured".
"""
from __future__ import annotations

import argparse
import csv
import json
import os
import re
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from dynamic3dgaussians_amd import motion_init as mi  # noqa: E402

HBM_BPS, FP32_FLOPS = 6.3e12, 157.3e12  # measured streaming rate, vector fp32 peak (MI355X)
KMEANS = {"kmeans_100k_x447_k20": (100_000, 447, 20), "kmeans_300k_x32_k49": (300_000, 32, 49)}
ITERS = 10


def kmeans_baseline(x, init, iters=ITERS):
    """The torch formulation: cdist (the expanded form, a matmul), argmin, index_add_."""
    centers = init.clone()
    K = centers.shape[0]
    for _ in range(iters):
        labels = torch.cdist(x, centers).argmin(dim=1)
        sums = torch.zeros_like(centers).index_add_(0, labels, x)
        counts = torch.zeros(K, dtype=x.dtype, device=x.device).index_add_(0, labels, torch.ones_like(x[:, 0]))
        centers = torch.where(counts[:, None] > 0, sums / counts.clamp(min=1)[:, None], centers)
    return labels, centers


def procrustes_baseline(tracks, labels, K, cano_t, svd_device):
    """A batched SVD Kabsch per frame over zero-padded clusters (weights 1)."""
    N, T = tracks.shape[:2]
    order = torch.sort(torch.where(labels >= 0, labels, torch.full_like(labels, K)), stable=True).indices
    counts = torch.bincount(labels[labels >= 0], minlength=K)
    M = int(counts.max())
    offs = torch.cumsum(counts, 0) - counts
    slot = torch.arange(M, device=tracks.device)[None].expand(K, M)
    live = slot < counts[:, None]
    ids = order[(offs[:, None] + slot).clamp(max=N - 1)]
    w = live.to(tracks.dtype)[..., None]
    src = tracks[ids, cano_t] * w
    cs = src.sum(1) / counts[:, None]
    rots, transls = [], []
    for t in range(T):
        tgt = tracks[ids, t] * w
        cg = tgt.sum(1) / counts[:, None]
        H = ((src - cs[:, None] * w).transpose(1, 2) @ (tgt - cg[:, None] * w)).to(svd_device)
        U, _, Vt = torch.linalg.svd(H)
        d = torch.sign(torch.linalg.det(Vt.transpose(1, 2) @ U.transpose(1, 2)))
        D = torch.diag_embed(torch.stack([torch.ones_like(d), torch.ones_like(d), d], -1))
        R = (Vt.transpose(1, 2) @ D @ U.transpose(1, 2)).to(tracks.device)
        rots.append(R)
        transls.append(cg - (R @ cs[..., None])[..., 0])
    return torch.stack(rots, 1), torch.stack(transls, 1)


def tracks_baseline(tracks, num_bases, cano_t, svd_device):
    means = tracks[:, cano_t]
    dists = (means - means.median(dim=0).values).norm(dim=-1)
    valid = dists < torch.quantile(dists, 0.95)
    x = mi.velocity_directions(tracks)[valid]
    rows = torch.randperm(x.shape[0], generator=torch.Generator().manual_seed(0))[:num_bases].to(x.device)
    labels_v, _ = kmeans_baseline(x, x[rows])
    labels = torch.full((tracks.shape[0],), -1, dtype=torch.int64, device=tracks.device)
    labels[valid] = labels_v
    centers = torch.stack([means[labels == k].median(dim=0).values for k in range(num_bases)])
    coefs = 10 * torch.exp(-torch.cdist(means, centers))
    return coefs, procrustes_baseline(tracks, labels, num_bases, cano_t, svd_device)


def make_tracks(N, T, bodies, dev):
    gen = torch.Generator().manual_seed(0)
    body = torch.randint(0, bodies, (N,), generator=gen)
    base = 4.0 * torch.randn(bodies, 3, generator=gen)[body] + 0.5 * torch.randn(N, 3, generator=gen)
    vel = torch.nn.functional.normalize(torch.randn(bodies, T, 3, generator=gen), dim=-1)[body] * 0.1
    tracks = base[:, None] + torch.cumsum(vel, 1) + 1e-3 * torch.randn(N, T, 3, generator=gen)
    return tracks.to(dev).contiguous()


def sample(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def alternate(hip, base, reps, rounds):
    a, b = [], []
    for _ in range(rounds):
        a.append(sample(hip, reps))
        b.append(sample(base, reps))
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    return {"hip_ms": med(a), "hip_samples_ms": a, "torch_ms": med(b), "torch_samples_ms": b,
            "hip_spread": (max(a) - min(a)) / med(a), "torch_spread": (max(b) - min(b)) / med(b),
            "torch_over_hip": med(b) / med(a)}


def workloads(dev, tracks_n, frames):
    gen = torch.Generator().manual_seed(1)
    out = {}
    for name, (N, D, K) in KMEANS.items():
        blob = 2.0 * torch.randn(K, D, generator=gen)
        x = (blob[torch.randint(0, K, (N,), generator=gen)] + 0.15 * torch.randn(N, D, generator=gen)).to(dev)
        out[name] = (x, x[:K].clone())
    out["tracks"] = make_tracks(tracks_n, frames, 10, dev)
    return out


def merge_stats(path, record):
    rows = {}
    with open(path) as fh:
        for r in csv.DictReader(fh):
            rows[r["Name"]] = r
    kernels = {}
    for name, r in rows.items():
        m = re.search(r"\b((?:km|mi)_\w+(?:<\d+>)?)\(", name)
        if m:
            short = m.group(1)
            kernels[short] = {"calls": int(r["Calls"]), "total_ms": float(r["TotalDurationNs"]) / 1e6,
                              "average_us": float(r["AverageNs"]) / 1e3}
    record["kernels"] = kernels
    record["kernel_note"] = ("one --profile-run: every k-means workload and the whole tracks call once; the "
                             "per-kernel averages mix the workloads, the models below are per workload")
    models = {}
    for name, (N, D, K) in KMEANS.items():
        a_bytes, a_flops = 4 * N * D + 8 * N, 3 * N * K * D
        models[name] = {"assign_bytes_ms": a_bytes / HBM_BPS * 1e3, "assign_flops_ms": a_flops / FP32_FLOPS * 1e3,
                        "assign_bound": "flops" if a_flops / FP32_FLOPS > a_bytes / HBM_BPS else "bytes",
                        "update_bytes_ms": (4 * N * D + 8 * N) / HBM_BPS * 1e3}
    # the assign tiers are unique to a workload in the profile run: K = 20 runs <32>, K = 49 runs <64>
    for name, tier in (("kmeans_100k_x447_k20", "km_assign_kernel<32>"), ("kmeans_300k_x32_k49", "km_assign_kernel<64>")):
        if tier in kernels:
            m = models[name]
            m["assign_us"] = kernels[tier]["average_us"]
            m["assign_share_of_larger_bound"] = max(m["assign_bytes_ms"], m["assign_flops_ms"]) * 1e3 / m["assign_us"]
    record["models"] = models
    return record


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--tracks", type=int, default=100_000)
    ap.add_argument("--frames", type=int, default=150)
    ap.add_argument("--profile-run", action="store_true", help="run every HIP workload once (under rocprofv3)")
    ap.add_argument("--merge-stats", default=None, help="a rocprofv3 kernel_stats.csv to add to the record")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "motion_init", "bench.json"))
    args = ap.parse_args()
    if args.merge_stats:
        with open(args.out) as fh:
            record = json.load(fh)
        with open(args.out, "w") as fh:
            json.dump(merge_stats(args.merge_stats, record), fh, indent=1, sort_keys=True)
        return
    if not torch.cuda.is_available():
        print(json.dumps({"status": "not measured", "reason": "no GPU"}))
        return
    dev = torch.device("cuda", 0)
    w = workloads(dev, args.tracks, args.frames)
    tracks = w.pop("tracks")
    run_tracks = lambda: mi.init_motion_bases_from_tracks(tracks, num_bases=10, cano_t=0)  # noqa: E731
    if args.profile_run:
        for x, init in w.values():
            mi.kmeans(x, init=init, iters=ITERS)
        run_tracks()
        torch.cuda.synchronize()
        return
    try:
        torch.linalg.svd(torch.randn(4, 3, 3, device=dev))
        svd_device = dev
    except RuntimeError:
        svd_device = torch.device("cpu")
    record = {"device": torch.cuda.get_device_name(0), "iters": ITERS, "reps": args.reps, "rounds": args.rounds,
              "svd_device": str(svd_device), "workloads": {}}
    for name, (x, init) in w.items():
        hip = mi.kmeans(x, init=init, iters=ITERS)
        base_labels, _ = kmeans_baseline(x, init)
        r = alternate(lambda: mi.kmeans(x, init=init, iters=ITERS), lambda: kmeans_baseline(x, init), args.reps, args.rounds)
        r["labels_equal_fraction"] = (hip.labels == base_labels).float().mean().item()
        r["shape"] = list(x.shape) + [init.shape[0]]
        record["workloads"][name] = r
        print(name, json.dumps(r), flush=True)
    r = alternate(run_tracks, lambda: tracks_baseline(tracks, 10, 0, svd_device), max(1, args.reps // 3), args.rounds)
    r["shape"] = list(tracks.shape)
    record["workloads"]["init_from_tracks_100k_x150"] = r
    print("init_from_tracks", json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(record, fh, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
