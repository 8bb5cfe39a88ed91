"""Shared builders of the float64 neighbour-loss parity tests
(tests/test_neighbor_float64.py, CPU and device): the (N, K, flags) cases that
reach each dispatch branch of csrc/gs_neighbor.hip, their references
(oracle.neighbor.torch_reference on the CPU in float64 and in fp32, autograd
gradients) computed once per process and shared, and the per-Gaussian metric.

A case is the reference's setup (tests/test_neighbor.py make_state: the k-NN
graph of the initial cloud, weights exp(-2000 d^2), the previous timestep's
state, a small motion) at a constant point density (so the K-th neighbour's
weight does not vanish at any N), with special structures written over
columns of the graph afterwards:

  hub      column 0 of every row := N // 2 (a reverse row of length >= N
           through nb_gather_kernel)
  selfdup  every 7th row names itself in its middle column (zero offset: the
           1e-20 terms carry everything); every 5th row repeats its column 0
           in its last column
  zero_w   every 11th row has its column-1 weight set to 0
  nonunit  fg_rot and prev_inv_rot_fg scaled per row by factors in [0.5, 2]
           (|rel_rot| != 1: the normalisation Jacobian of rotation_bwd)

neighbor_weight / neighbor_dist / prev_offset are recomputed from the final
graph, so they stay consistent with it."""
from __future__ import annotations

import functools
from typing import NamedTuple, Optional

import numpy as np
import torch

from oracle import neighbor as ON

WEIGHTS = (0.4, 0.4, 0.2)  # cvpr_dyn.py:332 loss weights


class Case(NamedTuple):
    N: int
    K: int
    flags: tuple
    reaches: str

    @property
    def id(self):
        return f"N{self.N}-K{self.K}" + "".join("-" + f for f in self.flags)


# Each case is the smallest shape that reaches its branch (G = 64 // K
# Gaussians per wave in the lane-per-pair kernels; 4 waves per block, the
# forward's grid capped at 1024 blocks = 4096 wave groups).  The K > 64
# forward's own grid-stride needs N > 262,144 Gaussians: a float64 autograd
# reference of that size is not a seconds-long test, so it is not covered.
CASES = (
    Case(257, 1, ("nonunit",), "nb_*_lanes_kernel G = 64, partial last wave group (257 = 4 * 64 + 1)"),
    Case(130, 32, ("selfdup",), "nb_*_lanes_kernel G = 2, no idle lanes"),
    Case(130, 33, ("hub", "selfdup"), "nb_*_lanes_kernel G = 1 with 31 idle lanes"),
    Case(4100, 64, ("hub",), "nb_*_lanes_kernel G = 1 full wave; nb_fwd_lanes_kernel grid-stride second trip "
                             "(4100 > 4096 wave groups); nb_gather_kernel reverse row of 4100"),
    Case(13000, 20, ("hub", "nonunit", "zero_w"), "the workload's K; nb_fwd_lanes_kernel grid-stride second trip "
                                                  "(ceil(13000 / 3) = 4334 > 4096 wave groups)"),
    Case(300, 65, ("nonunit", "selfdup"), "K = 65 -> nb_fwd_kernel / nb_bwd_kernel (thread per Gaussian)"),
    Case(1000, 7, ("nonunit",), "nb_*_lanes_kernel G = 9, lane 63 idle"),
    Case(40, 0, (), "K = 0: NaN losses (mean over nothing), nb_bwd_kernel walks nothing"),
)
BY_ID = {c.id: c for c in CASES}
EACH_TERM = ("N130-K33-hub-selfdup", "N300-K65-nonunit-selfdup")  # also run with each loss alone
DETERMINISM = ("N4100-K64-hub", "N300-K65-nonunit-selfdup")


def _k_smallest_with_ties(d2, k):
    """The k smallest of each row of d2 by (value, index): everything below
    the k-th value, and of the entries equal to it the lowest indices."""
    kth = np.partition(d2, k - 1, axis=1)[:, k - 1:k]
    lt, eq = d2 < kth, d2 == kth
    need = k - lt.sum(1, keepdims=True)
    sel = lt | (eq & (np.cumsum(eq, axis=1) <= need))
    cols = np.nonzero(sel)[1].reshape(d2.shape[0], k)  # ascending per row: the stable sort keeps index order
    d = np.take_along_axis(d2, cols, 1)
    o = np.argsort(d, axis=1, kind="stable")
    return np.take_along_axis(d, o, 1), np.take_along_axis(cols, o, 1)


def knn_graph(pts, k, rows=1024):
    """oracle.neighbor.knn (brute force in float64, self excluded, ties to the
    lower index) without its N x N x 3 temporaries and its full sort: row
    blocks, the same three squared differences added in the same order, the
    k + 1 smallest of a row by top-k.  Where the k-th and (k + 1)-th differ the
    set is the oracle's and is ordered by (distance, index); rows tied there go
    through the exact selection above.  Same (sq_dists, indices) bit for bit
    (test_knn_graph_blocks_equal_oracle); small clouds go to the oracle
    itself."""
    p = np.asarray(pts, np.float64)
    N = p.shape[0]
    if N <= 2048 or k < 1 or k >= N - 1:
        return ON.knn(p, k)
    x, y, z = (torch.from_numpy(np.ascontiguousarray(p[:, c])) for c in range(3))
    out_d = np.empty((N, k), np.float64)
    out_i = np.empty((N, k), np.int64)
    for a in range(0, N, rows):
        b = min(a + rows, N)
        d2 = (x[a:b, None] - x[None, :]) ** 2 + (y[a:b, None] - y[None, :]) ** 2 + (z[a:b, None] - z[None, :]) ** 2
        d2[torch.arange(b - a), torch.arange(a, b)] = float("inf")
        vals, idx = (t.numpy() for t in torch.topk(d2, k + 1, dim=1, largest=False))
        o = np.lexsort((idx[:, :k], vals[:, :k]), axis=1)
        out_d[a:b] = np.take_along_axis(vals[:, :k], o, 1)
        out_i[a:b] = np.take_along_axis(idx[:, :k], o, 1)
        tied = np.nonzero(vals[:, k - 1] == vals[:, k])[0]
        if tied.size:
            out_d[a + tied], out_i[a + tied] = _k_smallest_with_ties(d2.numpy()[tied], k)
    return out_d, out_i


@functools.lru_cache(maxsize=None)
def build(case: Case, motion=0.01):
    """(fg_pts [N, 3], fg_rot [N, 4], variables, meta) as fp32 CPU tensors.
    meta: what the recipe wrote into the graph (rows of each structure)."""
    N, K, flags = case.N, case.K, case.flags
    g = torch.Generator().manual_seed(1000 * K + N)
    spread = 0.3 * (N / 2000.0) ** (1.0 / 3.0)  # make_state's density at every N
    init = (torch.rand(N, 3, generator=g) - 0.5) * spread
    _, idx = knn_graph(init.numpy(), K)
    nbr = torch.from_numpy(np.ascontiguousarray(idx)).long().reshape(N, K).clone()
    rows = torch.arange(N)
    meta = {"self_rows": 0, "dup_rows": 0, "zero_w": 0}
    if "hub" in flags:
        nbr[:, 0] = N // 2
    if "selfdup" in flags:
        assert K >= 3  # columns 0, K // 2 and K - 1 are three different columns
        nbr[::7, K // 2] = rows[::7]
        nbr[::5, K - 1] = nbr[::5, 0]
        meta["self_rows"] = len(range(0, N, 7))
        meta["dup_rows"] = len(range(0, N, 5))
    prev_pts = init + motion * torch.randn(N, 3, generator=g)
    prev_rot = torch.nn.functional.normalize(torch.randn(N, 4, generator=g), dim=1)
    prev_inv = prev_rot.clone()
    prev_inv[:, 1:] = -prev_inv[:, 1:]                      # train.py:301-302
    pts = prev_pts + motion * torch.randn(N, 3, generator=g)
    rot = torch.nn.functional.normalize(prev_rot + 0.05 * torch.randn(N, 4, generator=g), dim=1)
    # weight / dist / prev_offset of the final graph (train.py:316-326, 304)
    p64 = init.numpy().astype(np.float64)
    sq = ((p64[nbr.numpy()] - p64[:, None]) ** 2).sum(-1)
    weight = torch.from_numpy(np.exp(-2000 * sq)).float().reshape(N, K)
    dist = torch.from_numpy(np.sqrt(sq)).float().reshape(N, K)
    if "zero_w" in flags:
        assert K >= 2
        weight[::11, 1] = 0.0
        meta["zero_w"] = len(range(0, N, 11))
    if "nonunit" in flags:
        fa = 0.5 * 4.0 ** torch.rand(N, generator=g)
        fb = 0.5 * 4.0 ** torch.rand(N, generator=g)
        fa[0], fb[0] = 0.5, 2.0
        fa[1], fb[1] = 2.0, 0.5
        rot = rot * fa[:, None]
        prev_inv = prev_inv * fb[:, None]
    variables = {
        "neighbor_indices": nbr.contiguous(),
        "neighbor_weight": weight.contiguous(),
        "neighbor_dist": dist.contiguous(),
        "prev_inv_rot_fg": prev_inv.contiguous(),
        "prev_offset": (prev_pts[nbr] - prev_pts[:, None]).reshape(N, K, 3).contiguous(),
    }
    return pts.contiguous(), rot.contiguous(), variables, meta


class Result(NamedTuple):
    losses: np.ndarray            # [3] float64
    d_pts: Optional[np.ndarray]   # [N, 3] float64, None where the term does not reach fg_pts
    d_rot: Optional[np.ndarray]   # [N, 4] float64, None where the term does not reach fg_rot


def _np(t):
    return None if t is None else t.detach().double().cpu().numpy()


def run(fn, pts, rot, variables, term=None) -> Result:
    """Forward + backward of `fn` (neighbor_losses or torch_reference): the
    weighted sum of the three losses, or loss `term` alone."""
    p, r = pts.clone().requires_grad_(True), rot.clone().requires_grad_(True)
    out = fn(p, r, variables)
    (sum(w * l for w, l in zip(WEIGHTS, out)) if term is None else out[term]).backward()
    return Result(np.array([float(o.detach()) for o in out], np.float64), _np(p.grad), _np(r.grad))


@functools.lru_cache(maxsize=None)
def reference(case: Case, dtype, term=None) -> Result:
    """oracle.neighbor.torch_reference on the CPU in `dtype` (torch.float64:
    the reference; torch.float32: the yardstick of fp32 rounding) on the same
    fp32 inputs."""
    pts, rot, v, _ = build(case)
    cast = lambda t: t.to(dtype) if t.is_floating_point() else t  # noqa: E731
    return run(ON.torch_reference, cast(pts), cast(rot), {k: cast(t) for k, t in v.items()}, term)


def row_error(g, h):
    """max_i |g_i - h_i|_inf / max(|h_i|_inf, 1e-3 max_j |h_j|_inf): every row
    counts; the floor only keeps near-cancelled rows from dominating.  Where
    the reference does not reach the input (h is None or all zero) the
    gradient must be exactly zero."""
    if h is None or not np.any(h):
        return 0.0 if (g is None or not np.any(g)) else float("inf")
    g = np.zeros_like(h) if g is None else g
    hr = np.abs(h).max(1)
    return float((np.abs(g - h).max(1) / np.maximum(hr, 1e-3 * hr.max())).max())


def rel_error(a, b):
    return float(abs(a - b) / abs(b))
