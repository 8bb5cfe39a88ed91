"""Seeded graphs for the spectral embedding's tests (tests/test_spectral.py on the CPU,
tests/test_gpu_spectral.py on the device), the checks both share, and an fp64 k-means with the
decision margins the label comparison needs.  Every builder returns a Case on the CPU; what the
case promises (components, gaps) is asserted here, so that no check can be skipped silently."""
from __future__ import annotations

import functools
import math
from typing import NamedTuple, Optional

import numpy as np
import torch

from dynamic3dgaussians_amd import spectral as SP
from dynamic3dgaussians_amd.feature_knn import feature_knn_torch

EPS = 2.0 ** -53
ORTHO_BOUND = 2.0 ** -40
TOL = 1e-10


class Case(NamedTuple):
    name: str
    n: int
    row_ptr: torch.Tensor  # int64 [n + 1]
    col: torch.Tensor      # int32 [nnz]
    val: torch.Tensor      # float64 [nnz]
    feats: Optional[torch.Tensor] = None    # float32 [n, E] for the blob cases
    planted: Optional[torch.Tensor] = None  # int64 [n]
    knn: int = 0


def csr_from_edges(n, rows, cols, vals) -> tuple:
    """CSR of the given entries (each stored as given: pass both directions), sorted by (row, column)."""
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    vals = np.asarray(vals, np.float64)
    order = np.lexsort((cols, rows))
    rows, cols, vals = rows[order], cols[order], vals[order]
    row_ptr = np.zeros(n + 1, np.int64)
    np.add.at(row_ptr, rows + 1, 1)
    return (torch.from_numpy(np.cumsum(row_ptr)), torch.from_numpy(cols.astype(np.int32)), torch.from_numpy(vals))


def cycle(n=64) -> Case:
    i = np.arange(n)
    return Case("cycle", n, *csr_from_edges(n, np.r_[i, i], np.r_[(i + 1) % n, (i - 1) % n], np.ones(2 * n)))


def cycle_theta(n, K):
    """The K largest eigenvalues of the cycle's S = A / 2: cos(2 pi k / n), k = 0, 1, 1, 2, 2, ..."""
    return [math.cos(2 * math.pi * ((j + 1) // 2) / n) for j in range(K)]


def path(n=10) -> Case:
    i = np.arange(n - 1)
    return Case("tiny", n, *csr_from_edges(n, np.r_[i, i + 1], np.r_[i + 1, i], np.ones(2 * (n - 1))))


def star(leaves=299, isolated=20) -> Case:
    n = 1 + leaves + isolated
    l = 1 + np.arange(leaves)
    z = np.zeros(leaves, np.int64)
    return Case("star", n, *csr_from_edges(n, np.r_[z, l], np.r_[l, z], np.ones(2 * leaves)))


def single(loop: bool) -> Case:
    if loop:
        return Case("single-loop", 1, *csr_from_edges(1, [0], [0], [2.5]))
    return Case("single", 1, *csr_from_edges(1, [], [], []))


def empty(n=50) -> Case:
    return Case("empty", n, *csr_from_edges(n, [], [], []))


def blob_features(blobs, noise, n, E, seed):
    """`blobs` unit centres, each point its centre plus noise * N(0, I / E); blob b owns a
    contiguous run of rows.  (feats float32 [n, E], planted int64 [n])."""
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((blobs, E))
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    lab = (np.arange(n) * blobs) // n
    x = c[lab] + noise * rng.standard_normal((n, E)) / math.sqrt(E)
    return torch.from_numpy(x.astype(np.float32)), torch.from_numpy(lab.astype(np.int64))


def blobs(name, nb, noise, n, E, knn, seed, knn_fn=feature_knn_torch) -> Case:
    """The clamp-weighted symmetric kNN graph of blob features.  knn_fn: the exact search to use
    (the twin here; the device test passes feature_knn for the large case, which returns the same
    lists)."""
    feats, lab = blob_features(nb, noise, n, E, seed)
    dev = "cpu" if knn_fn is feature_knn_torch else "cuda"
    sim, index = knn_fn(feats.to(dev), knn)
    rp, c, v = SP.knn_graph(sim.cpu(), index.cpu(), n)
    return Case(name, n, rp, c, v, feats, lab, knn)


@functools.lru_cache(maxsize=None)
def small_case(name: str) -> Case:
    if name == "cycle":
        return cycle()
    if name == "blobs-a":
        c = blobs(name, 3, 0.15, 257, 8, 8, 11)
        assert components(c)[0] == 3, "blobs-a must fall into its three blobs"
        return c
    if name == "blobs-b":
        c = blobs(name, 5, 0.8, 1000, 16, 10, 12)
        assert components(c)[0] == 1, "blobs-b must be connected"
        return c
    if name == "blobs-c":
        return blobs(name, 8, 0.5, 1500, 32, 12, 13)
    if name == "star":
        return star()
    if name == "tiny":
        return path()
    if name == "single":
        return single(False)
    if name == "single-loop":
        return single(True)
    if name == "empty":
        return empty()
    raise KeyError(name)


# (case, K): every case with n <= 1500
SMALL = [("cycle", 5), ("blobs-a", 3), ("blobs-b", 5), ("blobs-c", 8), ("blobs-c", 9), ("blobs-c", 56),
         ("blobs-c", 64), ("star", 2), ("tiny", 3), ("tiny", 10), ("single", 1), ("single-loop", 1), ("empty", 2)]
# the pairs whose gap lambda_K - lambda_{K+1} must be >= 1e-3 (asserted in oracle()): the projector bound applies
GAPPED = {("cycle", 5), ("blobs-a", 3), ("blobs-b", 5), ("blobs-c", 8), ("blobs-c", 9)}
# The interior of blobs-c's spectrum is dense (lambda_64 = 0.4339, lambda_73 close under it), so the
# 8 guard columns buy little there: the two wide cases run the filter at degree 16 (at degree 8 the
# twin needs 33 outer iterations for K = 64, over the default cap of 30).
SOLVER = {("blobs-c", 56): dict(degree=16), ("blobs-c", 64): dict(degree=16)}
BLOCK_WIDTH = {("blobs-c", 8): 16, ("blobs-c", 9): 24, ("blobs-c", 56): 64, ("blobs-c", 64): 72, ("tiny", 3): 10,
               ("tiny", 10): 10, ("single", 1): 1, ("cycle", 5): 16}


def large_case(knn_fn=feature_knn_torch) -> Case:
    return blobs("large", 12, 0.9, 20000, 32, 16, 14, knn_fn)


def components(case: Case):
    """(count, label int64 [n]) of the graph's connected components over entries with val > 0;
    an isolated node is its own component.  Min-label propagation with pointer jumping, numpy."""
    n = case.n
    rp = case.row_ptr.numpy()
    r = np.repeat(np.arange(n), np.diff(rp))
    c = case.col.numpy().astype(np.int64)
    keep = case.val.numpy() > 0
    r, c = r[keep], c[keep]
    lab = np.arange(n)
    while True:
        new = lab.copy()
        np.minimum.at(new, r, lab[c])
        new = new[new]
        if np.array_equal(new, lab):
            break
        lab = new
    return len(np.unique(lab)), torch.from_numpy(lab)


class Oracle(NamedTuple):
    S: torch.Tensor       # dense [n, n]
    g: torch.Tensor       # [n]
    lam: torch.Tensor     # all n eigenvalues, descending
    Q: torch.Tensor       # their eigenvectors in columns


@functools.lru_cache(maxsize=None)
def oracle(name: str) -> Oracle:
    c = small_case(name)
    S, g = SP._dense_s(c.row_ptr, c.col, c.val, c.n)
    assert SP.graph_check(c.row_ptr, c.col, c.val) is None, "the case builders make valid symmetric graphs"
    S = (S + S.T) / 2  # (g_i a) g_j and (g_j a) g_i round apart
    lam, Q = torch.linalg.eigh(S)
    lam, Q = lam.flip(0).contiguous(), Q.flip(1).contiguous()
    for nm, K in GAPPED:
        if nm == name:
            assert float(lam[K - 1] - lam[K]) >= 1e-3, (name, K, float(lam[K - 1] - lam[K]))
    return Oracle(S, g, lam, Q)


def eigh_term(n):
    """What torch.linalg.eigh's own error adds to a bound on |theta - lambda|: 64 n 2^-53."""
    return 64 * n * EPS


def check_against_oracle(name, K, out, tol=TOL, report=None):
    """Every check of a solver's result `out` (tensors on the CPU) against the dense oracle; the
    bounds are derived, not tuned.  report: a dict that collects the largest error / bound."""
    c, o = small_case(name), oracle(name)
    n, extra = c.n, eigh_term(c.n)
    note = (lambda k, e, b: report.__setitem__(k, max(report.get(k, 0.0), e / b))) if report is not None else \
        (lambda k, e, b: None)
    st = out.status.tolist()
    assert st[0] == 0, st
    assert st[2] == K and st[3] == SP.block_width(n, K)
    if (name, K) in BLOCK_WIDTH:
        assert st[3] == BLOCK_WIDTH[(name, K)]
    theta, V, res = out.eigenvalues, out.vectors, out.residuals
    assert theta.dtype == V.dtype == res.dtype == torch.float64 and out.embedding.dtype == torch.float32
    assert tuple(V.shape) == (n, K) and tuple(out.embedding.shape) == (n, K)
    for t in (theta, V, res, out.embedding):
        assert bool(torch.isfinite(t).all())
    assert bool((theta[:-1] >= theta[1:]).all())
    assert bool((res <= tol).all()), res.max()
    # a Ritz value of a symmetric matrix lies within its residual of an eigenvalue
    err = (theta - o.lam[:K]).abs()
    assert bool((err <= res + extra).all()), (err - res).max()
    note("ritz_value", float((err / (res + extra)).max()), 1.0)
    ortho = float((V.T @ V - torch.eye(K, dtype=torch.float64)).abs().max())
    assert ortho <= ORTHO_BOUND, ortho
    note("orthonormality", ortho, ORTHO_BOUND)
    # residuals recomputed from the returned vectors and the dense S
    R = o.S @ V - V * theta
    mine = torch.linalg.norm(R, dim=0)
    assert bool((mine <= tol + extra).all()), mine.max()
    assert bool(((mine - res).abs() <= extra).all()), (mine - res).abs().max()
    note("residual", float(mine.max()), tol + extra)
    note("residual_agreement", float((mine - res).abs().max()), extra)
    if (name, K) in GAPPED:  # Davis-Kahan
        gap = float(o.lam[K - 1] - o.lam[K])
        Qk = o.Q[:, :K]
        dist = float(torch.linalg.matrix_norm(V @ V.T - Qk @ Qk.T, ord=2))
        bound = 2 * float(torch.linalg.norm(R)) / (gap - tol)
        assert dist <= bound, (dist, bound)
        note("projector", dist, bound)
    # the embedding convention, bit for bit
    want = (o.g[:, None] * V).to(torch.float32)
    want[o.g == 0] = 0.0
    assert out.embedding.numpy().tobytes() == want.numpy().tobytes()


def check_known_answers(name, K, out):
    c = small_case(name)
    theta = out.eigenvalues
    if name == "cycle":
        assert float((theta - torch.tensor(cycle_theta(c.n, K), dtype=torch.float64)).abs().max()) <= 1e-12
    if name == "blobs-a":
        assert float((theta - 1.0).abs().max()) <= 1e-12
    if name == "star":
        assert abs(float(theta[0]) - 1.0) <= 1e-12
        iso = oracle(name).g == 0
        assert int(iso.sum()) == 20
        assert out.embedding[iso].numpy().tobytes() == bytes(4 * K * 20)  # +0, bit for bit
    if name == "empty":
        assert not theta.any() and not out.embedding.any() and not out.residuals.any()
    if name == "single":
        assert float(theta[0]) == 0.0 and abs(abs(float(out.vectors[0, 0])) - 1.0) <= 2 * EPS
    if name == "single-loop":
        assert abs(float(theta[0]) - 1.0) <= 4 * EPS


# ---- fp64 k-means with decision margins (the label comparison)

def kmeans_f64(u: torch.Tensor, init_rows, iters=10, margin=1e-4):
    """Lloyd's algorithm in float64 on the rows of u from the centres u[init_rows]: `iters`
    iterations of assign (argmin of the squared distance, ties to the lower index) and update (an
    empty cluster keeps its centre).  Returns (labels of the last assignment, robust bool [n]): a
    point is decision-robust when (d2_second - d2_best) / (|u|^2 + max |c|^2) >= margin in every
    iteration."""
    u = u.to(torch.float64)
    c = u[torch.as_tensor(init_rows)].clone()
    K = c.shape[0]
    robust = torch.ones(u.shape[0], dtype=torch.bool)
    labels = None
    for _ in range(iters):
        d2 = ((u[:, None, :] - c[None, :, :]) ** 2).sum(-1)
        best = d2.topk(min(2, K), dim=1, largest=False).values
        labels = d2.argmin(dim=1)
        if K > 1:
            rel = (best[:, 1] - best[:, 0]) / ((u * u).sum(1) + (c * c).sum(1).max())
            robust &= rel >= margin
        for k in range(K):
            m = labels == k
            if bool(m.any()):
                c[k] = u[m].mean(0)
    return labels, robust


def first_rows(planted: torch.Tensor, K: int):
    return [int((planted == b).nonzero()[0]) for b in range(K)]
