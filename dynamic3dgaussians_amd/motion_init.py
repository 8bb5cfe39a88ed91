"""Initialisation of the motion bases on the HIP kernels of csrc/gs_motion_init.hip (C ABI
include/gs_motion_init.h): Lloyd's k-means, per-cluster medians, the basis coefficients and one
weighted Procrustes solve per (basis, frame).  Forward only: initialisation has no gradients.

What the reference computes on the host, through scikit-learn and Python loops over clusters and
frames, and what replaces it:

    init_motion_params_with_procrustes(tracks_3d, num_bases, cano_t)   dyn_som.py:25-135
        -> init_motion_bases_from_tracks(tracks, visibles, confidences, num_bases=, cano_t=)
    k-means on velocity directions                                     motion_utils.py:219-244
        -> kmeans(velocity_directions(tracks), num_bases)
    feature_bases(...), called at dyn_train.py:392-399                 motion_utils.py:57-162
        -> init_motion_coefs_from_features(means, feats, num_bases, num_frames=)

Parity unpinned.  dyn_som.py is a fragment: solve_procrustes, get_weights_for_procrustes,
TrackObservations and cluster_init_method are defined nowhere in the reference and the file cannot
be imported, so no golden record exists.  The semantics are the ones DESIGN.md 9.16 fixes; the
`_torch` twins below state them in PyTorch operations for any dtype and device.  They are the
fp64 parity oracle, the benchmark's baseline, and the path every call takes when its input is not a
float32 device tensor.

Documented differences.  From scikit-learn: exactly `iters` Lloyd iterations with no convergence
test and no final re-assignment (labels and counts belong to the centres before the last update);
an empty cluster keeps its centre bit for bit and reports count 0 (scikit-learn relocates it); the
initial centres are the rows torch.randperm(N, generator=<CPU generator seeded with seed>)[:K],
not a k-means++ draw.  From the reference: the robust per-cluster weighting
get_weights_for_procrustes does not exist in its tree, a caller passes `weights`;
init_motion_coefs_from_features clusters with k-means, the alternative the reference keeps in
comments, because its spectral clustering builds an N x N affinity; nothing is compacted, a dropped
point keeps its row and gets label -1; a frame whose weights sum to zero is skipped whatever the
threshold.

Nothing is read back except, in init_motion_bases_from_tracks, the K cluster counts that decide
the output's shape.  No floating-point atomic: two calls give the same bits.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch
import torch.nn.functional as F

from . import _lib
from .motion import MotionBases

MAX_CLUSTERS = 64  # include/gs_motion_init.h GS_KMEANS_MAX_K, the warp's GS_MOTION_MAX_K
ROT_DIMS = {"6d": 6, "quat": 4}


class KMeansResult(NamedTuple):
    labels: torch.Tensor   # (N,) int64, -1 for a point masked out
    centers: torch.Tensor  # (K, D)
    counts: torch.Tensor   # (K,) int64
    moved: torch.Tensor    # (iters,) int64: labels changed in each iteration, on x's device


class ProcrustesInit(NamedTuple):
    rots: torch.Tensor        # (K, T, 6) or (K, T, 4)
    transls: torch.Tensor     # (K, T, 3)
    err_after: torch.Tensor   # (K, T), -1 where skipped
    err_before: torch.Tensor  # (K, T), -1 where skipped
    skipped: torch.Tensor     # (K, T) bool


class MotionInit(NamedTuple):
    bases: Optional[MotionBases]  # None for rot_type="quat": MotionBases takes 6-D rotations
    motion_coefs: torch.Tensor    # (N, K)
    means_cano: torch.Tensor      # (N, 3)
    valid_mask: torch.Tensor      # (N,) bool: not an outlier and visible somewhere
    labels: torch.Tensor          # (N,) int64 in [0, K), -1 for a dropped point
    centers: torch.Tensor         # (K, 3)
    procrustes: ProcrustesInit


# ---- argument checks

def _on_hip_path(*tensors) -> bool:
    return all(t.is_cuda and t.dtype == torch.float32 for t in tensors)


def _check_points(x, name: str, last: Optional[int] = None) -> None:
    if not isinstance(x, torch.Tensor) or x.dim() != 2 or not x.is_floating_point():
        raise ValueError(f"{name} must be a floating-point (N, D) tensor")
    if last is not None and x.shape[1] != last:
        raise ValueError(f"{name} must be (N, {last}) (got {tuple(x.shape)})")
    if x.shape[1] < 1:
        raise ValueError(f"{name} needs at least one dimension (got {tuple(x.shape)})")


def _check_centers(x, centers) -> None:
    _check_points(x, "x")
    if not isinstance(centers, torch.Tensor) or centers.dim() != 2 or centers.shape[1] != x.shape[1]:
        raise ValueError(f"centers must be (K, {x.shape[1]})")
    if not 1 <= centers.shape[0] <= MAX_CLUSTERS:
        raise ValueError(f"the number of clusters must be in [1, {MAX_CLUSTERS}] (got {centers.shape[0]})")


def _check_labels(labels, n: int) -> None:
    if not isinstance(labels, torch.Tensor) or labels.dtype != torch.int64 or tuple(labels.shape) != (n,):
        raise ValueError(f"labels must be an int64 ({n},) tensor")


def _check_tracks(tracks) -> None:
    if not isinstance(tracks, torch.Tensor) or tracks.dim() != 3 or tracks.shape[2] != 3 or tracks.shape[1] < 1 \
            or not tracks.is_floating_point():
        raise ValueError("tracks must be a floating-point (N, T, 3) tensor with T >= 1")


def _bucket(labels: torch.Tensor, K: int) -> torch.Tensor:
    """labels with everything outside [0, K) moved to the extra bucket K."""
    return torch.where((labels >= 0) & (labels < K), labels, torch.full_like(labels, K))


def _init_rows(N: int, K: int, seed: int, valid: Optional[torch.Tensor], device) -> torch.Tensor:
    """The rows of the initial centres: torch.randperm(N) of a CPU generator, its first K entries
    (with a mask: its first K valid ones, found without a read-back)."""
    if N < K:
        raise ValueError(f"k-means needs at least as many points as clusters (N = {N}, K = {K})")
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(int(seed))).to(device)
    if valid is None:
        return perm[:K]
    first = torch.sort((~valid[perm]).to(torch.int8), stable=True).indices[:K]
    return perm[first]


# ---- k-means

def kmeans_assign_torch(x: torch.Tensor, centers: torch.Tensor) -> torch.Tensor:
    """labels (N,) int64 = argmin_k sum_d (x - c_k)^2 in x's dtype, the difference form; ties go to
    the lowest k (torch.argmin returns the first minimum).  Any dtype and device."""
    _check_centers(x, centers)
    c = centers.to(x.dtype)
    N, D = x.shape
    rows = max(1, (1 << 24) // (c.shape[0] * D))  # bounds the (rows, K, D) intermediate
    out = [((x[i:i + rows, None] - c[None]) ** 2).sum(-1).argmin(dim=1) for i in range(0, N, rows)]
    return torch.cat(out) if out else torch.empty(0, dtype=torch.int64, device=x.device)


def kmeans_update_torch(x: torch.Tensor, labels: torch.Tensor, centers: torch.Tensor):
    """(centers (K, D) in x's dtype, counts (K,) int64): the mean of each cluster's members, summed
    in fp64 and rounded once; an empty cluster keeps its centre; labels outside [0, K) are ignored."""
    _check_centers(x, centers)
    _check_labels(labels, x.shape[0])
    K, D = centers.shape
    idx = _bucket(labels, K)
    sums = torch.zeros(K + 1, D, dtype=torch.float64, device=x.device).index_add_(0, idx, x.double())[:K]
    counts = torch.zeros(K + 1, dtype=torch.int64, device=x.device).index_add_(0, idx, torch.ones_like(idx))[:K]
    mean = (sums / counts.clamp(min=1)[:, None].double()).to(x.dtype)
    return torch.where(counts[:, None] > 0, mean, centers.to(x.dtype)), counts


def _start(x, num_clusters, init, iters, seed, valid):
    _check_points(x, "x")
    if init is not None:
        _check_centers(x, init)
        if num_clusters is not None and int(num_clusters) != init.shape[0]:
            raise ValueError(f"num_clusters = {num_clusters} but init holds {init.shape[0]} centres")
        K = init.shape[0]
    else:
        if num_clusters is None:
            raise ValueError("kmeans needs num_clusters or init")
        K = int(num_clusters)
        if not 1 <= K <= MAX_CLUSTERS:
            raise ValueError(f"the number of clusters must be in [1, {MAX_CLUSTERS}] (got {K})")
    if int(iters) < 0:
        raise ValueError(f"iters must be >= 0 (got {iters})")
    if valid is not None and (not isinstance(valid, torch.Tensor) or valid.dtype != torch.bool
                              or tuple(valid.shape) != (x.shape[0],)):
        raise ValueError(f"valid must be a bool ({x.shape[0]},) tensor")
    N, D = x.shape
    if N == 0:
        centers = init.to(x.dtype).clone() if init is not None else x.new_zeros(K, D)
    elif init is not None:
        centers = init.to(x.dtype).clone()
    else:
        centers = x[_init_rows(N, K, seed, valid, x.device)].clone()
    return K, centers.contiguous()


def kmeans_torch(x: torch.Tensor, num_clusters: Optional[int] = None, *, init: Optional[torch.Tensor] = None,
                 iters: int = 10, seed: int = 0, valid: Optional[torch.Tensor] = None) -> KMeansResult:
    """kmeans in PyTorch operations, any dtype and device (x's dtype throughout)."""
    K, centers = _start(x, num_clusters, init, iters, seed, valid)
    N = x.shape[0]
    labels = torch.full((N,), -1, dtype=torch.int64, device=x.device)
    counts = torch.zeros(K, dtype=torch.int64, device=x.device)
    moved = torch.zeros(int(iters), dtype=torch.int64, device=x.device)
    if N == 0:
        return KMeansResult(labels, centers, counts, moved)
    for i in range(int(iters)):
        new = kmeans_assign_torch(x, centers)
        if valid is not None:
            new = torch.where(valid, new, torch.full_like(new, -1))
        moved[i] = (new != labels).sum()
        labels = new
        centers, counts = kmeans_update_torch(x, labels, centers)
    return KMeansResult(labels, centers, counts, moved)


def _assign(x, centers, labels, valid=None, prev=None, moved_ptr=None) -> None:
    N, D = x.shape
    L = _lib.load()
    args = _lib.GsKmeansAssign(N=N, D=D, K=centers.shape[0], x=x.data_ptr() if N else None, centers=centers.data_ptr(),
                               valid=valid.data_ptr() if valid is not None and N else None,
                               prev_labels=prev.data_ptr() if prev is not None else None,
                               labels=labels.data_ptr() if N else None, moved=moved_ptr)
    _lib.check(L.gs_kmeans_assign(args, _lib.stream(x.device)), "kmeans assign")


def _update(x, labels, centers, counts, ws) -> None:
    N, D = x.shape
    L = _lib.load()
    args = _lib.GsKmeansUpdate(N=N, D=D, K=centers.shape[0], x=x.data_ptr() if N else None,
                               labels=labels.data_ptr() if N else None, centers=centers.data_ptr(),
                               counts=counts.data_ptr(), workspace=ws.data_ptr(), workspace_bytes=ws.numel())
    _lib.check(L.gs_kmeans_update(args, _lib.stream(x.device)), "kmeans update")


def _workspace(x, K) -> torch.Tensor:
    n = _lib.load().gs_kmeans_workspace_bytes(x.shape[0], K, x.shape[1])
    return torch.empty(n, dtype=torch.uint8, device=x.device)


def kmeans_assign(x: torch.Tensor, centers: torch.Tensor) -> torch.Tensor:
    """labels (N,) int64: the nearest of centers (K, D), K <= 64, for every row of x (N, D) by
    sum_d (x - c)^2 added in index order in fp32; ties go to the lowest k.  float32 device tensors
    run the HIP kernel; anything else takes kmeans_assign_torch."""
    _check_centers(x, centers)
    if not _on_hip_path(x, centers):
        return kmeans_assign_torch(x, centers)
    x, centers = x.detach().contiguous(), centers.detach().contiguous()
    labels = torch.empty(x.shape[0], dtype=torch.int64, device=x.device)
    _assign(x, centers, labels)
    return labels


def kmeans_update(x: torch.Tensor, labels: torch.Tensor, centers: torch.Tensor):
    """(centers (K, D), counts (K,) int64): each cluster's mean, the sum taken in a fixed order in
    fp64 and rounded to fp32 once; an empty cluster keeps its centre bit for bit and counts 0;
    labels outside [0, K) are ignored.  float32 device tensors run the HIP kernels; anything else
    takes kmeans_update_torch."""
    _check_centers(x, centers)
    _check_labels(labels, x.shape[0])
    if not (_on_hip_path(x, centers) and labels.is_cuda):
        return kmeans_update_torch(x, labels, centers)
    x, labels = x.detach().contiguous(), labels.contiguous()
    out = centers.detach().clone().contiguous()
    counts = torch.empty(out.shape[0], dtype=torch.int64, device=x.device)
    _update(x, labels, out, counts, _workspace(x, out.shape[0]))
    return out, counts


def kmeans(x: torch.Tensor, num_clusters: Optional[int] = None, *, init: Optional[torch.Tensor] = None,
           iters: int = 10, seed: int = 0, valid: Optional[torch.Tensor] = None) -> KMeansResult:
    """Lloyd's algorithm on the rows of x (N, D), exactly `iters` iterations of assign and update
    with no convergence read-back; `moved` stays on the device.  The initial centres are `init`
    (K, D) or, with init=None, the rows torch.randperm(N, generator=<CPU generator seeded with
    seed>)[:num_clusters].  K <= 64; N = 0 returns empty results; N < K with init=None raises
    ValueError.  `valid` (N,) bool, optional, keeps the masked-out points out of every cluster
    (label -1) without compacting x.  The labels and counts returned are those of the last
    iteration's assignment.  Inputs must be finite.  float32 device tensors run the HIP kernels;
    anything else takes kmeans_torch."""
    if not isinstance(x, torch.Tensor) or not _on_hip_path(x) or (init is not None and not _on_hip_path(init)):
        return kmeans_torch(x, num_clusters, init=init, iters=iters, seed=seed, valid=valid)
    x = x.detach().contiguous()
    K, centers = _start(x, num_clusters, init.detach() if init is not None else None, iters, seed, valid)
    N, dev = x.shape[0], x.device
    labels = torch.full((N,), -1, dtype=torch.int64, device=dev)
    counts = torch.zeros(K, dtype=torch.int64, device=dev)
    moved = torch.zeros(int(iters), dtype=torch.int64, device=dev)
    if N == 0 or int(iters) == 0:
        return KMeansResult(labels, centers, counts, moved)
    mask = valid.to(device=dev, dtype=torch.uint8).contiguous() if valid is not None else None
    ws = _workspace(x, K)
    prev = labels
    labels = torch.empty_like(prev)
    for i in range(int(iters)):
        _assign(x, centers, labels, mask, prev, moved.data_ptr() + 8 * i)
        _update(x, labels, centers, counts, ws)
        prev, labels = labels, prev
    return KMeansResult(prev, centers, counts, moved)


def velocity_directions(tracks: torch.Tensor) -> torch.Tensor:
    """(N, 3 (T - 1)): the unit steps v / (|v| + 1e-5), v = tracks[:, 1:] - tracks[:, :-1], of tracks
    (N, T, 3), flattened per track (motion_utils.py:219-244's k-means input)."""
    _check_tracks(tracks)
    v = tracks[:, 1:] - tracks[:, :-1]
    v = v / (v.norm(dim=-1, keepdim=True) + 1e-5)
    return v.reshape(tracks.shape[0], -1).contiguous()


# ---- medians and coefficients

def cluster_medians_torch(points: torch.Tensor, labels: torch.Tensor, num_clusters: int) -> torch.Tensor:
    """(K, C): per cluster and coordinate the lower median of points (N, C), what
    points[labels == k].median(dim=0).values returns; a NaN row for an empty cluster.  Two stable
    sorts (by value, then by label) and a gather at offset_k + (count_k - 1) // 2: no loop over the
    clusters and nothing read back, on any device."""
    _check_points(points, "points")
    _check_labels(labels, points.shape[0])
    K = int(num_clusters)
    if K < 1:
        raise ValueError(f"num_clusters must be >= 1 (got {K})")
    N, C = points.shape
    nan = torch.full((K, C), float("nan"), dtype=points.dtype, device=points.device)
    if N == 0:
        return nan
    idx = _bucket(labels, K)
    vals, by_value = points.sort(dim=0, stable=True)
    by_label = idx[by_value].sort(dim=0, stable=True).indices
    vals = vals.gather(0, by_label)  # every column: grouped by label, ascending inside a group
    counts = torch.zeros(K + 1, dtype=torch.int64, device=points.device).index_add_(0, idx, torch.ones_like(idx))[:K]
    offsets = torch.cumsum(counts, 0) - counts
    pos = (offsets + (counts - 1).clamp(min=0) // 2).clamp(max=N - 1)
    return torch.where(counts[:, None] > 0, vals.gather(0, pos[:, None].expand(K, C)), nan)


def cluster_medians(points: torch.Tensor, labels: torch.Tensor, num_clusters: int) -> torch.Tensor:
    """The per-cluster lower medians (K, C) of points (N, C); labels outside [0, K) are ignored and
    an empty cluster gives a NaN row.  On the device this is torch's sort and gather on the points'
    own device (no kernel of this package, no loop over the clusters, no read-back): the same
    statement as cluster_medians_torch."""
    return cluster_medians_torch(points, labels, num_clusters)


def _check_coefs(means, centers) -> None:
    _check_points(means, "means", 3)
    if not isinstance(centers, torch.Tensor) or centers.dim() != 2 or centers.shape[1] != 3 or centers.shape[0] < 1:
        raise ValueError("centers must be (K, 3) with K >= 1")


def coefs_from_centers_torch(means: torch.Tensor, centers: torch.Tensor) -> torch.Tensor:
    """10 exp(-|means[:, None] - centers[None]|), (N, K) (dyn_som.py:64-65); any dtype and device."""
    _check_coefs(means, centers)
    return 10 * torch.exp(-torch.norm(means[:, None] - centers.to(means.dtype)[None], dim=-1))


def coefs_from_centers(means: torch.Tensor, centers: torch.Tensor) -> torch.Tensor:
    """motion_coefs (N, K) = 10 exp(-|mean - centre|) of means (N, 3) and centers (K, 3).  float32
    device tensors run the HIP kernel; anything else takes coefs_from_centers_torch."""
    _check_coefs(means, centers)
    if not _on_hip_path(means, centers):
        return coefs_from_centers_torch(means, centers)
    means, centers = means.detach().contiguous(), centers.detach().contiguous()
    N, K = means.shape[0], centers.shape[0]
    out = torch.empty(N, K, dtype=torch.float32, device=means.device)
    args = _lib.GsCoefsFromCenters(N=N, K=K, means=means.data_ptr() if N else None, centers=centers.data_ptr(),
                                   coefs=out.data_ptr() if N else None)
    _lib.check(_lib.load().gs_coefs_from_centers(args, _lib.stream(means.device)), "coefs from centers")
    return out


# ---- Procrustes

def _check_procrustes(tracks, labels, num_bases, cano_t, visibles, confidences, weights, rot_type):
    _check_tracks(tracks)
    N, T = tracks.shape[:2]
    _check_labels(labels, N)
    K = int(num_bases)
    if not 1 <= K <= MAX_CLUSTERS:
        raise ValueError(f"num_bases must be in [1, {MAX_CLUSTERS}] (got {K})")
    if not 0 <= int(cano_t) < T:
        raise ValueError(f"cano_t = {cano_t} is outside [0, {T})")
    if rot_type not in ROT_DIMS:
        raise ValueError(f"rot_type must be '6d' or 'quat' (got {rot_type!r})")
    for t, name in ((visibles, "visibles"), (confidences, "confidences"), (weights, "weights")):
        if t is not None and (not isinstance(t, torch.Tensor) or tuple(t.shape) != (N, T)):
            raise ValueError(f"{name} must be ({N}, {T})")
    return N, T, K


def _pair_weights(visibles, weights):
    return weights if weights is not None else visibles


def _horn(C: torch.Tensor) -> torch.Tensor:
    """(..., 4, 4): Horn's symmetric matrix of the cross-covariance C[a][b] = sum w s_a g_b, whose
    largest eigenvector is the quaternion (w, x, y, z) of the rotation taking s to g."""
    xx, xy, xz = C[..., 0, 0], C[..., 0, 1], C[..., 0, 2]
    yx, yy, yz = C[..., 1, 0], C[..., 1, 1], C[..., 1, 2]
    zx, zy, zz = C[..., 2, 0], C[..., 2, 1], C[..., 2, 2]
    rows = [torch.stack([xx + yy + zz, yz - zy, zx - xz, xy - yx], -1),
            torch.stack([yz - zy, xx - yy - zz, xy + yx, zx + xz], -1),
            torch.stack([zx - xz, xy + yx, -xx + yy - zz, yz + zy], -1),
            torch.stack([xy - yx, zx + xz, yz + zy, -xx - yy + zz], -1)]
    return torch.stack(rows, -2)


def _quat_to_rmat(q: torch.Tensor) -> torch.Tensor:
    w, x, y, z = q.unbind(-1)
    return torch.stack([
        torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
        torch.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
        torch.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], -2)


def _visiting_order(cano_t: int, T: int):
    return list(range(cano_t - 1, -1, -1)) + list(range(cano_t, T))  # dyn_som.py:76


def solve_procrustes_bases_torch(tracks: torch.Tensor, labels: torch.Tensor, num_bases: int, cano_t: int, *,
                                 visibles: Optional[torch.Tensor] = None,
                                 confidences: Optional[torch.Tensor] = None,
                                 weights: Optional[torch.Tensor] = None, min_mean_weight: float = 0.1,
                                 rot_type: str = "6d") -> ProcrustesInit:
    """solve_procrustes_bases in PyTorch operations, any dtype and device (the tracks' dtype): per
    frame the weighted centroids and the centred cross-covariance of every basis by index_add_,
    Horn's matrix, torch.linalg.eigh, and the walk's copy and sign rules by torch.where.  A loop
    over the frames, none over the bases, nothing read back."""
    N, T, K = _check_procrustes(tracks, labels, num_bases, cano_t, visibles, confidences, weights, rot_type)
    dt, dev = tracks.dtype, tracks.device
    W = _pair_weights(visibles, weights)
    W = W.to(dt) if W is not None else None
    conf = confidences.to(dt) if confidences is not None else None
    idx = _bucket(labels, K)
    thr = float(min_mean_weight) * T

    def seg(v):  # sums per basis, the extra bucket dropped
        return torch.zeros((K + 1,) + tuple(v.shape[1:]), dtype=dt, device=dev).index_add_(0, idx, v)[:K]

    def ext(v, fill):  # one more row for the points of no basis
        return torch.cat([v, fill.to(device=dev, dtype=dt).expand(1, *v.shape[1:])], 0)[idx]

    eye = torch.eye(3, dtype=dt, device=dev)
    q = torch.tensor([1.0, 0.0, 0.0, 0.0], dtype=dt, device=dev).repeat(K, 1)
    R = eye.repeat(K, 1, 1)
    tr = torch.zeros(K, 3, dtype=dt, device=dev)
    rots = torch.empty(K, T, ROT_DIMS[rot_type], dtype=dt, device=dev)
    transls = torch.empty(K, T, 3, dtype=dt, device=dev)
    err_after = torch.empty(K, T, dtype=dt, device=dev)
    err_before = torch.empty(K, T, dtype=dt, device=dev)
    skipped = torch.empty(K, T, dtype=torch.bool, device=dev)
    src = tracks[:, cano_t]
    minus = torch.full((K,), -1.0, dtype=dt, device=dev)
    for t in _visiting_order(int(cano_t), T):
        tgt = tracks[:, t]
        w = torch.ones(N, dtype=dt, device=dev)
        if W is not None:
            w = W[:, cano_t] * W[:, t]
        if conf is not None:
            w = w * (conf[:, cano_t] + conf[:, t]) / 2
        Wk = seg(w)
        skip = (Wk < thr) | ~(Wk > 0)
        safe = torch.where(skip, torch.ones_like(Wk), Wk)
        cs = seg(w[:, None] * src) / safe[:, None]
        cg = seg(w[:, None] * tgt) / safe[:, None]
        sc = src - ext(cs, torch.zeros(1, 3))
        gc = tgt - ext(cg, torch.zeros(1, 3))
        C = seg(w[:, None, None] * sc[:, :, None] * gc[:, None, :]) / safe[:, None, None]
        qn = torch.linalg.eigh(_horn(C)).eigenvectors[..., -1]  # ascending eigenvalues: the largest is last
        Rn = _quat_to_rmat(qn)
        tn = cg - (Rn * cs[:, None, :]).sum(-1)
        pred = (ext(Rn, eye[None]) * src[:, None, :]).sum(-1) + ext(tn, torch.zeros(1, 3))
        ea = torch.sqrt(seg(w * ((pred - tgt) ** 2).sum(-1)) / safe)
        eb = torch.sqrt(seg(w * ((src - tgt) ** 2).sum(-1)) / safe)
        qn = torch.where(((qn * q).sum(-1) < 0)[:, None], -qn, qn)  # the double cover: nearer to the frame before
        q = torch.where(skip[:, None], q, qn)
        R = torch.where(skip[:, None, None], R, Rn)
        tr = torch.where(skip[:, None], tr, tn)
        rots[:, t] = q if rot_type == "quat" else torch.cat([R[:, :, 0], R[:, :, 1]], -1)
        transls[:, t] = tr
        err_after[:, t] = torch.where(skip, minus, ea)
        err_before[:, t] = torch.where(skip, minus, eb)
        skipped[:, t] = skip
    return ProcrustesInit(rots, transls, err_after, err_before, skipped)


def solve_procrustes_bases(tracks: torch.Tensor, labels: torch.Tensor, num_bases: int, cano_t: int, *,
                           visibles: Optional[torch.Tensor] = None, confidences: Optional[torch.Tensor] = None,
                           weights: Optional[torch.Tensor] = None, min_mean_weight: float = 0.1,
                           rot_type: str = "6d") -> ProcrustesInit:
    """One weighted Procrustes solve per (basis, frame) of tracks (N, T, 3) grouped by labels (N,)
    (outside [0, num_bases): ignored), walked outward from the canonical frame (dyn_som.py:76-130).

    For basis n and frame t the pair weights are w_i = W[i, cano_t] W[i, t] (conf[i, cano_t] +
    conf[i, t]) / 2 with W = weights, else visibles as 0 / 1, else 1, and conf = confidences, else
    1.  (R, t) is the proper rigid transform minimising sum w |R src + t - tgt|^2, src the tracks at
    cano_t and tgt at t; det R = +1 always.  err_after = sqrt(sum w |R src + t - tgt|^2 / sum w),
    err_before the same without the transform.  Frames are visited in the order cano_t - 1, ..., 0,
    cano_t, ..., T - 1, starting from the identity; a frame with sum w < min_mean_weight T (or
    sum w = 0) copies the rotation and translation of the frame visited before it, is marked
    skipped and reports -1 for both errors.  rot_type "6d" gives concat(R[:, 0], R[:, 1]), what
    motion.cont_6d_to_rmat inverts; "quat" gives (w, x, y, z) with the sign nearer to the frame
    visited before.  A cluster of fewer than three points, or of collinear ones, has no unique
    answer: the result is some finite proper rotation and t maps the weighted source centroid onto
    the target's.  float32 device tracks run the HIP kernels; anything else takes
    solve_procrustes_bases_torch."""
    N, T, K = _check_procrustes(tracks, labels, num_bases, cano_t, visibles, confidences, weights, rot_type)
    kw = dict(visibles=visibles, confidences=confidences, weights=weights, min_mean_weight=min_mean_weight,
              rot_type=rot_type)
    if not (_on_hip_path(tracks) and labels.is_cuda):
        return solve_procrustes_bases_torch(tracks, labels, num_bases, cano_t, **kw)
    L = _lib.load()
    dev = tracks.device
    tracks = tracks.detach().contiguous()
    W = _pair_weights(visibles, weights)
    W = W.detach().to(device=dev, dtype=torch.float32).contiguous() if W is not None else None
    conf = confidences.detach().to(device=dev, dtype=torch.float32).contiguous() if confidences is not None else None
    idx = _bucket(labels, K)
    order = torch.sort(idx, stable=True).indices.contiguous()  # ids grouped by basis, ascending inside a group
    counts = torch.zeros(K + 1, dtype=torch.int64, device=dev).index_add_(0, idx, torch.ones_like(idx))[:K]
    offsets = torch.cat([counts.new_zeros(1), torch.cumsum(counts, 0)]).contiguous()
    D = ROT_DIMS[rot_type]
    rots = torch.empty(K, T, D, dtype=torch.float32, device=dev)
    transls = torch.empty(K, T, 3, dtype=torch.float32, device=dev)
    err_after = torch.empty(K, T, dtype=torch.float32, device=dev)
    err_before = torch.empty(K, T, dtype=torch.float32, device=dev)
    skipped = torch.empty(K, T, dtype=torch.uint8, device=dev)
    ws = torch.empty(L.gs_procrustes_workspace_bytes(K, T), dtype=torch.uint8, device=dev)
    args = _lib.GsProcrustes(N=N, T=T, K=K, cano_t=int(cano_t), rot_dim=D, min_weight_sum=float(min_mean_weight) * T,
                             tracks=tracks.data_ptr() if N else None, order=order.data_ptr() if N else None,
                             offsets=offsets.data_ptr(), weights=W.data_ptr() if W is not None and N else None,
                             confidences=conf.data_ptr() if conf is not None and N else None, rots=rots.data_ptr(),
                             transls=transls.data_ptr(), err_after=err_after.data_ptr(),
                             err_before=err_before.data_ptr(), skipped=skipped.data_ptr(), workspace=ws.data_ptr(),
                             workspace_bytes=ws.numel())
    _lib.check(L.gs_procrustes(args, _lib.stream(dev)), "procrustes")
    return ProcrustesInit(rots, transls, err_after, err_before, skipped.bool())


# ---- the composed initialisations

def init_motion_bases_from_tracks(tracks: torch.Tensor, visibles: Optional[torch.Tensor] = None,
                                  confidences: Optional[torch.Tensor] = None, *, num_bases: int = 10,
                                  cano_t: int = 0, min_cluster_size: int = 100, outlier_quantile: float = 0.95,
                                  kmeans_iters: int = 10, seed: int = 0, rot_type: str = "6d") -> MotionInit:
    """The motion bases and coefficients of 3-D tracks (N, T, 3), T >= 2, after dyn_som.py:31-135:

    1. means_cano = tracks[:, cano_t];
    2. points whose distance to the coordinate-wise median is not below the `outlier_quantile`
       quantile of the distances are dropped;
    3. so are points visible in no frame (visibles (N, T) bool, optional);
    4. k-means on the velocity directions of the rest, `num_bases` clusters;
    5. per-cluster medians of means_cano;
    6. clusters with counts <= min_cluster_size are dropped (the call's single read-back, of
       num_bases counts: the output's shape depends on it), the surviving ids renumbered;
    7. motion_coefs = 10 exp(-|means_cano - centre|) over the surviving centres;
    8. solve_procrustes_bases over the surviving clusters.

    Nothing is compacted: every output keeps N rows, dropped points have valid_mask False or label
    -1 and take no part in any cluster.  `bases` feeds bases.compute_means(ts, means_cano,
    motion_coefs, softmax=True) unchanged (None for rot_type="quat").  ValueError when no cluster
    survives.  float32 device tracks run the HIP kernels; anything else takes the _torch twins."""
    _check_tracks(tracks)
    N, T = tracks.shape[:2]
    if T < 2:
        raise ValueError("init_motion_bases_from_tracks needs at least two frames")
    if not 0 <= int(cano_t) < T:
        raise ValueError(f"cano_t = {cano_t} is outside [0, {T})")
    if visibles is not None and tuple(visibles.shape) != (N, T):
        raise ValueError(f"visibles must be ({N}, {T})")
    tracks = tracks.detach()
    means_cano = tracks[:, cano_t].contiguous()
    center = means_cano.median(dim=0).values
    dists = torch.norm(means_cano - center, dim=-1)
    valid = dists < torch.quantile(dists, float(outlier_quantile))
    if visibles is not None:
        valid = valid & visibles.to(tracks.device).bool().any(dim=1)
    km = kmeans(velocity_directions(tracks), int(num_bases), iters=kmeans_iters, seed=seed, valid=valid)
    medians = cluster_medians(means_cano, km.labels, int(num_bases))
    keep = (km.counts.cpu() > int(min_cluster_size)).nonzero().flatten()  # the read-back
    if keep.numel() == 0:
        raise ValueError(f"no cluster has more than {min_cluster_size} points")
    remap = torch.full((int(num_bases) + 1,), -1, dtype=torch.int64)
    remap[keep] = torch.arange(keep.numel())
    labels = remap.to(tracks.device)[_bucket(km.labels, int(num_bases))]
    centers = medians[keep.to(tracks.device)].contiguous()
    coefs = coefs_from_centers(means_cano, centers)
    pro = solve_procrustes_bases(tracks, labels, keep.numel(), int(cano_t), visibles=visibles,
                                 confidences=confidences, rot_type=rot_type)
    bases = MotionBases(pro.rots, pro.transls) if rot_type == "6d" else None
    return MotionInit(bases, coefs, means_cano, valid, labels, centers, pro)


def init_motion_coefs_from_features(means: torch.Tensor, feats: torch.Tensor, num_bases: int, *, num_frames: int,
                                    kmeans_iters: int = 10, seed: int = 0, cluster: str = "kmeans", knn: int = 20):
    """(bases, motion_coefs (N, K), labels (N,), centers (K, 3)) from the Gaussians' semantic
    features, after feature_bases (motion_utils.py:122-162): labels from a clustering of feats
    (N, F), per-cluster medians of means (N, 3), motion_coefs = 10 exp(-|mean - centre|) and
    identity 6-D bases of (num_bases, num_frames).  cluster="kmeans" (the default) is k-means on
    the L2-normalised feats; cluster="spectral" is the reference's own similarity_mapping, a
    spectral clustering of the features' cosine affinity, here on the exact `knn`-neighbour graph
    (spectral.spectral_clustering) in place of the dense N x N matrix.  An empty cluster's centre
    is NaN, as its median is.  float32 device tensors run the HIP kernels; anything else takes the
    _torch twins."""
    _check_points(means, "means", 3)
    _check_points(feats, "feats")
    if feats.shape[0] != means.shape[0]:
        raise ValueError(f"feats must have {means.shape[0]} rows (got {feats.shape[0]})")
    if int(num_frames) < 1:
        raise ValueError(f"num_frames must be >= 1 (got {num_frames})")
    if cluster not in ("kmeans", "spectral"):
        raise ValueError(f"cluster must be 'kmeans' or 'spectral' (got {cluster!r})")
    K = int(num_bases)
    if cluster == "spectral":
        from . import spectral  # spectral imports this module
        km = spectral.spectral_clustering(feats.detach().contiguous(), K, knn=int(knn), kmeans_iters=kmeans_iters,
                                          seed=seed)
    else:
        km = kmeans(F.normalize(feats.detach(), dim=-1).contiguous(), K, iters=kmeans_iters, seed=seed)
    centers = cluster_medians(means.detach(), km.labels, K)
    coefs = coefs_from_centers(means.detach().contiguous(), centers.contiguous())
    ident = torch.tensor([1.0, 0.0, 0.0, 0.0, 1.0, 0.0], dtype=torch.float32, device=means.device)
    bases = MotionBases(ident.repeat(K, int(num_frames), 1),
                        torch.zeros(K, int(num_frames), 3, dtype=torch.float32, device=means.device))
    return bases, coefs, km.labels, centers


__all__ = ("KMeansResult", "ProcrustesInit", "MotionInit", "kmeans", "kmeans_torch", "kmeans_assign",
           "kmeans_assign_torch", "kmeans_update", "kmeans_update_torch", "velocity_directions", "cluster_medians",
           "cluster_medians_torch", "coefs_from_centers", "coefs_from_centers_torch", "solve_procrustes_bases",
           "solve_procrustes_bases_torch", "init_motion_bases_from_tracks", "init_motion_coefs_from_features")
