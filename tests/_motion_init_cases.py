"""Decision-robust inputs for the motion-initialisation tests (tests/test_motion_init.py,
tests/test_gpu_motion_init.py).

k-means.  Seeded blobs (blob centres 2 N(0, 1), spread 0.15, fp32), initial centres the first K
rows so that labels really move.  A label is a decision; for the HIP kernels to be held to the
fp64 twin's labels on EVERY point, no point may sit near a tie.  The builder runs the fp64 twin
for ITERS iterations and removes every non-seed point whose margin

    (d2_second - d2_best) / (|x|^2 + max_k |c_k|^2)

is below TAU = 1e-4 in any iteration, and repeats until no such point is left.  TAU exceeds the
worst fp32 error of a distance at D = 447, about D 2^-24 = 2.7e-5 of the same scale, so fp32
arithmetic in any summation order decides as fp64 does.  The builder asserts that it ended with no
point under TAU (the seeds included), that at least 80 % of the points are kept and that labels
moved after the first assignment (moved[1] > 0; moved[0] is N by definition).

Procrustes.  Five clusters of 1, 2, 257, 300 and 300 tracks scattered over N = 1000 ids, the rest
labelled -1; one SE(3) trajectory per cluster plus noise 1e-2, random visibilities and
confidences, and one (basis, frame) forced under the skip threshold by a wide margin.

End to end.  Four rigid bodies of 300 points, at least 3 units apart, on distinct screw motions
over 12 frames, noise-free; every point moves in every frame.
"""
from __future__ import annotations

import functools
import math

import torch
import torch.nn.functional as F

from dynamic3dgaussians_amd import motion_init as mi

TAU = 1e-4
ITERS = 10
KMEANS_CASES = {  # name: (N, D, K, blobs, seed)
    "km_257x3_k5_s0": (257, 3, 5, 5, 0), "km_257x3_k5_s1": (257, 3, 5, 5, 1),
    "km_1000x24_k20_s0": (1000, 24, 20, 20, 0), "km_4097x32_k49_s0": (4097, 32, 49, 36, 0),
    "km_1000x447_k20_s1": (1000, 447, 20, 15, 1),  # the last two end with empty clusters
}


def blobs(N: int, D: int, n_blobs: int, seed: int) -> torch.Tensor:
    gen = torch.Generator().manual_seed(seed)
    centres = 2.0 * torch.randn(n_blobs, D, generator=gen, dtype=torch.float64)
    which = torch.randint(0, n_blobs, (N,), generator=gen)
    return (centres[which] + 0.15 * torch.randn(N, D, generator=gen, dtype=torch.float64)).float()


def margins(x64: torch.Tensor, centers64: torch.Tensor) -> torch.Tensor:
    d2 = ((x64[:, None] - centers64[None]) ** 2).sum(-1)
    if d2.shape[1] < 2:
        return torch.full((x64.shape[0],), float("inf"), dtype=torch.float64)
    two = d2.topk(2, dim=1, largest=False).values
    scale = (x64 ** 2).sum(-1) + (centers64 ** 2).sum(-1).max()
    return (two[:, 1] - two[:, 0]) / scale


def lloyd64(x: torch.Tensor, init: torch.Tensor, iters: int = ITERS):
    """The fp64 twin run step by step: the centres before each assignment, the labels of each
    iteration, the smallest margin seen per point, and the final (centres, counts, moved)."""
    x64, c = x.double(), init.double()
    labels = torch.full((x.shape[0],), -1, dtype=torch.int64)
    worst = torch.full((x.shape[0],), float("inf"), dtype=torch.float64)
    centres, history, moved = [], [], []
    counts = torch.zeros(init.shape[0], dtype=torch.int64)
    for _ in range(iters):
        centres.append(c)
        worst = torch.minimum(worst, margins(x64, c))
        new = mi.kmeans_assign_torch(x64, c)
        moved.append(int((new != labels).sum()))
        labels = new
        history.append(labels)
        c, counts = mi.kmeans_update_torch(x64, labels, c)
    return dict(centres=centres, labels=history, worst=worst, final_centres=c, counts=counts,
                moved=torch.tensor(moved, dtype=torch.int64))


def make_robust(x: torch.Tensor, init_rows, exempt: int):
    """Remove points under TAU until none is left; init_rows(x) -> the rows of the initial centres;
    the first `exempt` rows are never removed."""
    n0 = x.shape[0]
    for _ in range(40):
        run = lloyd64(x, x[init_rows(x)])
        bad = run["worst"] < TAU
        bad[:exempt] = False
        if not bad.any():
            break
        x = x[~bad]
    run = lloyd64(x, x[init_rows(x)])
    assert not (run["worst"] < TAU).any(), "the case did not converge to a decision-robust one"
    assert x.shape[0] >= 0.8 * n0, (x.shape[0], n0)
    assert run["moved"][1] > 0, "labels never moved"
    return x.contiguous(), run


@functools.lru_cache(maxsize=None)
def kmeans_case(name: str):
    """(x fp32 (N', D), init fp32 (K, D), the fp64 run, the fp32 twin's KMeansResult)."""
    N, D, K, n_blobs, seed = KMEANS_CASES[name]
    x, run = make_robust(blobs(N, D, n_blobs, seed), lambda x: torch.arange(K), exempt=K)
    init = x[:K].clone()
    f32 = mi.kmeans_torch(x, init=init, iters=ITERS)
    assert torch.equal(f32.labels, run["labels"][-1]) and torch.equal(f32.moved, run["moved"])
    return x, init, run, f32


@functools.lru_cache(maxsize=None)
def feature_case(N: int = 4097, Fdim: int = 32, K: int = 49, seed: int = 0):
    """(means fp32 (N, 3), feats fp32 (N, F), the fp64 run on the normalised features): robust
    under the initial rows init_motion_coefs_from_features itself draws (seed 0).  Those rows depend
    on N, so a point under TAU is not removed but replaced in its row by a spare one; at most 20 %
    of the rows may be replaced."""
    pool = blobs(2 * N, Fdim, K, seed)
    feats, spare = pool[:N].clone(), N
    rows = mi._init_rows(N, K, 0, None, "cpu")
    for _ in range(40):
        xn = F.normalize(feats, dim=-1)
        run = lloyd64(xn, xn[rows])
        bad = (run["worst"] < TAU).nonzero().flatten()
        if bad.numel() == 0:
            break
        feats[bad] = pool[spare:spare + bad.numel()]
        spare += bad.numel()
    assert bad.numel() == 0 and spare - N <= 0.2 * N and run["moved"][1] > 0
    gen = torch.Generator().manual_seed(seed + 100)
    means = torch.randn(N, 3, generator=gen)
    return means, feats.contiguous(), run


def rotation(axis, angle: float) -> torch.Tensor:
    a = torch.tensor(axis, dtype=torch.float64)
    a = a / a.norm()
    Kx = torch.tensor([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dtype=torch.float64)
    return torch.eye(3, dtype=torch.float64) + math.sin(angle) * Kx + (1 - math.cos(angle)) * (Kx @ Kx)


PROCRUSTES_SIZES = (1, 2, 257, 300, 300)
PROCRUSTES_FULL_RANK = (2, 3, 4)
PROCRUSTES_SKIP = (3, 6)  # the (basis, frame) forced under the threshold
PROCRUSTES_MIN_MEAN_WEIGHT = 0.05  # x T = 9: 0.45, below the smallest weight of a visible pair (0.5)


@functools.lru_cache(maxsize=None)
def procrustes_case():
    """dict(tracks fp64 (1000, 9, 3), labels, visibles, confidences, cano_t, poses): cluster k moves
    by poses[k][t] = (R, t) from its canonical frame, plus noise 1e-2."""
    N, T, cano_t = 1000, 9, 4
    gen = torch.Generator().manual_seed(11)
    ids = torch.randperm(N, generator=gen)
    labels = torch.full((N,), -1, dtype=torch.int64)
    start = 0
    for k, n in enumerate(PROCRUSTES_SIZES):
        labels[ids[start:start + n]] = k
        start += n
    cano = 1.5 * torch.randn(N, 3, generator=gen, dtype=torch.float64) + torch.tensor([2.0, -1.0, 4.0])
    tracks = torch.empty(N, T, 3, dtype=torch.float64)
    poses = {}
    for k in range(-1, len(PROCRUSTES_SIZES)):
        m = labels == k
        axis = (1.0, 0.3 * (k + 2), -0.5 + 0.4 * k)
        for t in range(T):
            R = rotation(axis, 0.2 * (k + 2) * (t - cano_t) / 4)  # at most 1.2 rad from the canonical frame
            tr = torch.tensor([0.3 * (t - cano_t), 0.1 * k * (t - cano_t), 0.05 * (t - cano_t) ** 2], dtype=torch.float64)
            poses[k, t] = (R, tr)
            tracks[m, t] = cano[m] @ R.T + tr
    tracks = tracks + 1e-2 * torch.randn(N, T, 3, generator=gen, dtype=torch.float64)
    visibles = torch.rand(N, T, generator=gen) < 0.8
    confidences = 0.5 + 0.5 * torch.rand(N, T, generator=gen)
    small = (labels == 0) | (labels == 1)
    visibles[small] = True  # a pair weight of the small clusters is in [0.5, 1]: never under 0.45
    k, t = PROCRUSTES_SKIP
    members = (labels == k).nonzero().flatten()
    visibles[members, t] = False
    visibles[members[0], t] = True
    visibles[members[0], cano_t] = True
    confidences[members[0], t] = 0.2
    confidences[members[0], cano_t] = 0.2  # sum w = 0.2 < 0.45
    return dict(tracks=tracks.float().double(), labels=labels, visibles=visibles, confidences=confidences,
                cano_t=cano_t, poses=poses, K=len(PROCRUSTES_SIZES))


@functools.lru_cache(maxsize=None)
def bodies_case():
    """dict(tracks fp64 (1200, 12, 3) exactly representable in fp32, body (1200,), seed): four
    rigid bodies on distinct screw motions.  k-means++ is out of scope and Lloyd's algorithm does
    not leave a start with two centres in one body, so `seed` is the first whose initial rows (of
    the fp64 pipeline) give the bodies back."""
    n, T = 300, 12
    gen = torch.Generator().manual_seed(5)
    offsets = torch.tensor([[0.0, 0, 0], [4.0, 0, 0], [0.0, 4, 0], [0.0, 0, 4]], dtype=torch.float64)
    axes = [(1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (-1.0, -1.0, 0.5)]
    pts, body = [], []
    for b in range(4):
        local = 0.4 * (2 * torch.rand(n, 3, generator=gen, dtype=torch.float64) - 1)  # bodies >= 3.2 apart
        a = torch.tensor(axes[b], dtype=torch.float64)
        a = a / a.norm()
        frames = []
        for t in range(T):
            R = rotation(axes[b], 0.05 * (b + 1) * t)
            frames.append(local @ R.T + offsets[b] + 0.25 * t * a)  # a screw: turn about the axis, slide along it
        pts.append(torch.stack(frames, 1))
        body.append(torch.full((n,), b))
    tracks = torch.cat(pts).float().double()
    body = torch.cat(body)
    perm = torch.randperm(4 * n, generator=gen)
    tracks, body = tracks[perm].contiguous(), body[perm]
    assert (tracks[:, 1:] - tracks[:, :-1]).norm(dim=-1).min() > 0.2  # every point moves in every frame
    cano = tracks[:, 3]
    dists = (cano - cano.median(dim=0).values).norm(dim=-1)
    # the outlier test is a decision too: no distance within fp32 rounding (2^-23 x 8) of the quantile
    assert (dists - torch.quantile(dists, 0.95)).abs().min() > 1e-5
    for seed in range(64):
        out = mi.init_motion_bases_from_tracks(tracks, num_bases=4, cano_t=3, seed=seed)
        if out.centers.shape[0] == 4 and all(
                (out.labels[(body == b) & out.valid_mask] == out.labels[(body == b) & out.valid_mask][0]).all()
                for b in range(4)) and out.labels[out.valid_mask].unique().numel() == 4:
            return dict(tracks=tracks, body=body, seed=seed, cano_t=3, ref=out)
    raise AssertionError("no seed in 0..63 starts Lloyd's algorithm with one centre per body")
