"""Spectral embedding and clustering of a sparse symmetric graph on the kernels of
csrc/gs_spectral.hip (C ABI, definition and method: include/gs_spectral.h).

The reference clusters the Gaussians' semantic features spectrally through a dense matrix:

    cos_sim_matrix = feats @ feats.T                                       # motion_utils.py:57-116 similarity_mapping
    SpectralClustering(n_clusters=49, affinity='precomputed').fit_predict(cos_sim_matrix)

which at 300k Gaussians is 360 GB.  Here the affinity is the exact cosine kNN graph of
feature_knn and the embedding comes from a block eigensolver on the device:

    sim, index = feature_knn(feats, 20)
    row_ptr, col, val = knn_graph(sim, index, n)                           # CSR of max(A, A^T), weights max(s, 0)
    emb = spectral_embedding(row_ptr, col, val, 49)                        # eigenvalues, embedding, vectors, residuals, status
    out = spectral_clustering(feats, 49)                                   # the chain, then k-means on the embedding

With d_i = sum_j val_ij (fp64, CSR order), g_i = 1 / sqrt(d_i) (0 where d_i = 0) and
S = diag(g) A diag(g): `eigenvalues` [K] are the K largest Ritz values of S, descending (the
normalised Laplacian's are 1 - theta), `vectors` [n, K] float64 has orthonormal columns,
`embedding` [n, K] float32 is fl32(g_i V[i, j]) -- sklearn's spectral_embedding(norm_laplacian=True,
drop_first=False), what its SpectralClustering hands to k-means -- `residuals` [K] are
|S v - theta v|, `status` int32 [4] on the device is (code, outer iterations, converged columns,
block width) with code 0 converged, 1 iteration cap, 2 bad input (all outputs zero).  Eigenvectors
are unique only up to sign and to rotation inside a degenerate eigenvalue: the guarantees are on
residuals, orthonormality and bit-identical reruns.

`spectral_embedding_torch` is the same algorithm in fp64 torch operations on any device (the CPU
path and the timing baseline); `spectral_embedding_dense` takes torch.linalg.eigh of the dense S
(the test oracle, n <= 8192).
"""
from __future__ import annotations

import warnings
from typing import NamedTuple, Optional

import torch

from . import _args, _lib, motion_init
from ._lib import GsplatError
from .feature_knn import feature_knn, feature_knn_torch, knn_affinity

MAX_K, MAX_N, MAX_DEGREE, MAX_OUTER = (_lib.SPECTRAL_MAX_K, _lib.SPECTRAL_MAX_N, _lib.SPECTRAL_MAX_DEGREE,
                                       _lib.SPECTRAL_MAX_OUTER)
GUARD = _lib.SPECTRAL_GUARD
DENSE_MAX_N = 8192
RANK_TOL = 2.0 ** -40
_TWIN = "spectral_embedding_torch runs"
_M64 = (1 << 64) - 1


class SpectralEmbedding(NamedTuple):
    eigenvalues: torch.Tensor  # (K,) float64, descending
    embedding: torch.Tensor    # (n, K) float32
    vectors: torch.Tensor      # (n, K) float64, orthonormal columns
    residuals: torch.Tensor    # (K,) float64
    status: torch.Tensor       # (4,) int32: code, outer iterations, converged columns, block width


class SpectralClustering(NamedTuple):
    labels: torch.Tensor       # (n,) int64
    centers: torch.Tensor      # (K, K) centres in the embedding
    counts: torch.Tensor       # (K,) int64
    embedding: torch.Tensor    # (n, K) float32
    eigenvalues: torch.Tensor  # (K,) float64
    residuals: torch.Tensor    # (K,) float64
    status: torch.Tensor       # (4,) int32


# ---- graphs

def knn_graph(sim: torch.Tensor, index: torch.Tensor, n: int, *, transform: str = "clamp"):
    """(row_ptr int64 [n + 1], col int32 [nnz], val float64 [nnz]): the CSR form of
    knn_affinity(w, index, n, symmetric=True) with the weights w = max(sim, 0) ("clamp") or
    (1 + sim) / 2 ("shift").  Always symmetric, columns ascending and unique within a row.  Plain
    torch, any device."""
    if transform not in ("clamp", "shift"):
        raise ValueError(f"transform must be 'clamp' or 'shift' (got {transform!r})")
    if not isinstance(sim, torch.Tensor) or not isinstance(index, torch.Tensor):
        raise GsplatError("sim and index must be tensors")
    s = sim.to(torch.float64)
    w = s.clamp_min(0.0) if transform == "clamp" else (1.0 + s) / 2.0
    A = knn_affinity(w, index, int(n))
    rc = A.indices()  # coalesced: sorted by (row, column)
    counts = torch.bincount(rc[0], minlength=int(n))
    row_ptr = torch.zeros(int(n) + 1, dtype=torch.int64, device=rc.device)
    row_ptr[1:] = torch.cumsum(counts, 0)
    return row_ptr, rc[1].to(torch.int32).contiguous(), A.values().to(torch.float64).contiguous()


def _check_csr(row_ptr, col, val) -> int:
    for t, name in ((row_ptr, "row_ptr"), (col, "col"), (val, "val")):
        if not isinstance(t, torch.Tensor) or t.dim() != 1:
            raise GsplatError(f"{name} must be a one-dimensional tensor")
    if row_ptr.dtype != torch.int64 or row_ptr.numel() < 1:
        raise GsplatError(f"row_ptr must be int64 [n + 1] (got {row_ptr.dtype}, {tuple(row_ptr.shape)})")
    if col.dtype != torch.int32:
        raise GsplatError(f"col must be int32 (got {col.dtype})")
    if not val.is_floating_point() or val.shape != col.shape:
        raise GsplatError(f"val must be a floating-point tensor of col's shape (got {val.dtype}, {tuple(val.shape)})")
    if not (row_ptr.device == col.device == val.device):
        raise GsplatError("row_ptr, col and val must be on one device")
    return row_ptr.numel() - 1


def graph_check(row_ptr: torch.Tensor, col: torch.Tensor, val: torch.Tensor) -> Optional[str]:
    """None for a valid graph, otherwise a sentence naming the first violation found: the walk of
    row_ptr, the range of col, its order within a row, the sign of val, symmetry.  A debug helper
    in torch (it reads back); the HIP entry itself does not verify symmetry."""
    n = _check_csr(row_ptr, col, val)
    nnz = col.numel()
    rp = row_ptr.cpu()
    if int(rp[0]) != 0 or int(rp[-1]) != nnz or bool((rp[1:] < rp[:-1]).any()):
        return f"row_ptr must rise from 0 to nnz = {nnz}"
    c, v = col.cpu().to(torch.int64), val.cpu().to(torch.float64)
    if nnz == 0:
        return None
    bad = ((c < 0) | (c >= n)).nonzero()
    if bad.numel():
        return f"col[{int(bad[0])}] = {int(c[bad[0]])} is out of range [0, {n})"
    bad = (~(v >= 0) | ~torch.isfinite(v)).nonzero()
    if bad.numel():
        return f"val[{int(bad[0])}] = {float(v[bad[0]])} is negative or not finite"
    r = torch.repeat_interleave(torch.arange(n), rp[1:] - rp[:-1])
    bad = ((r[1:] == r[:-1]) & (c[1:] <= c[:-1])).nonzero()
    if bad.numel():
        return f"the columns of row {int(r[bad[0] + 1])} are not ascending and unique (entry {int(bad[0]) + 1})"
    flat, flat_t = r * n + c, c * n + r
    order = torch.argsort(flat_t)
    if not torch.equal(flat, flat_t[order]) or not torch.equal(v, v[order]):
        diff = (flat != flat_t[order]) | (v != v[order])
        p = int(diff.nonzero()[0])
        return f"the graph is not symmetric (entry {p}: row {int(r[p])}, column {int(c[p])})"
    return None


def csr_degrees(row_ptr: torch.Tensor, val: torch.Tensor) -> torch.Tensor:
    """d_i = sum_j val_ij in float64, added in CSR order (the definition's order; it reads the
    longest row's length back)."""
    n = row_ptr.numel() - 1
    lo, ln = row_ptr[:-1], row_ptr[1:] - row_ptr[:-1]
    d = torch.zeros(n, dtype=torch.float64, device=val.device)
    if val.numel() == 0 or n == 0:
        return d
    v = val.to(torch.float64)
    for p in range(int(ln.max())):
        live = ln > p
        d = d + torch.where(live, v[(lo + p).clamp_max(v.numel() - 1)], torch.zeros_like(d))
    return d


def _inv_sqrt(d: torch.Tensor) -> torch.Tensor:
    return torch.where(d > 0, 1.0 / d.sqrt(), torch.zeros_like(d))


def _rows_of(row_ptr: torch.Tensor) -> torch.Tensor:
    n = row_ptr.numel() - 1
    return torch.repeat_interleave(torch.arange(n, device=row_ptr.device), row_ptr[1:] - row_ptr[:-1])


def _bad_graph(row_ptr, col, val, n) -> bool:
    nnz = col.numel()
    rp = row_ptr
    if int(rp[0]) != 0 or int(rp[-1]) != nnz or bool((rp[1:] < rp[:-1]).any()):
        return True
    if nnz == 0:
        return False
    v = val.to(torch.float64)
    return bool(((col < 0) | (col >= n)).any() or (~(v >= 0)).any() or (~torch.isfinite(v)).any()
                or (~torch.isfinite(csr_degrees(row_ptr, v))).any())


def _embed(g: torch.Tensor, V: torch.Tensor, row_normalize: bool) -> torch.Tensor:
    u = g[:, None] * V
    if row_normalize:
        ss = torch.zeros_like(g)
        for k in range(V.shape[1]):
            ss = ss + u[:, k] * u[:, k]
        nrm = ss.sqrt()
        u = torch.where((nrm > 0)[:, None], u / nrm.clamp_min(torch.finfo(torch.float64).tiny)[:, None], u)
    e = u.to(torch.float32)
    e[g == 0] = 0.0
    return e


def _zero_result(n, K, B, code, dev) -> SpectralEmbedding:
    return SpectralEmbedding(torch.zeros(K, dtype=torch.float64, device=dev),
                             torch.zeros(n, K, dtype=torch.float32, device=dev),
                             torch.zeros(n, K, dtype=torch.float64, device=dev),
                             torch.zeros(K, dtype=torch.float64, device=dev),
                             torch.tensor([code, 0, 0, B], dtype=torch.int32, device=dev))


def _check_solver(n, K, tol, degree, max_outer, seed, limit_k=True) -> None:
    for v, name in ((K, "num_vectors"), (degree, "degree"), (max_outer, "max_outer"), (seed, "seed")):
        if isinstance(v, bool) or not isinstance(v, int):
            raise GsplatError(f"{name} must be an integer (got {v!r})")
    if K < 1 or (limit_k and K > MAX_K):
        raise GsplatError(f"num_vectors must be in [1, {MAX_K}] (got {K}); spectral_embedding_torch takes any size")
    if n < K:
        raise GsplatError(f"the graph needs at least num_vectors = {K} nodes (got n = {n})")
    if not 1 <= degree <= MAX_DEGREE:
        raise GsplatError(f"degree must be in [1, {MAX_DEGREE}] (got {degree})")
    if not 1 <= max_outer <= MAX_OUTER:
        raise GsplatError(f"max_outer must be in [1, {MAX_OUTER}] (got {max_outer})")
    if not (isinstance(tol, (int, float)) and tol > 0 and tol < float("inf")):
        raise GsplatError(f"tol must be positive and finite (got {tol!r})")
    if seed < 0 or seed > _M64:
        raise GsplatError(f"seed must be in [0, 2^64) (got {seed})")


def block_width(n: int, num_vectors: int) -> int:
    """min(n, 8 ceil((K + 8) / 8)): the K wanted columns and at least 8 guard columns."""
    return min(int(n), 8 * ((int(num_vectors) + GUARD + 7) // 8))


# ---- the dense oracle and the torch twin

def _dense_s(row_ptr, col, val, n):
    v = val.to(torch.float64)
    g = _inv_sqrt(csr_degrees(row_ptr, v))
    r, c = _rows_of(row_ptr), col.to(torch.int64)
    S = torch.zeros(n, n, dtype=torch.float64, device=val.device)
    S[r, c] = g[r] * v * g[c]
    return S, g


def spectral_embedding_dense(row_ptr: torch.Tensor, col: torch.Tensor, val: torch.Tensor, num_vectors: int, *,
                             row_normalize: bool = False) -> SpectralEmbedding:
    """The definition through torch.linalg.eigh of the dense S (symmetrised as (S + S^T) / 2): the
    test oracle for small graphs, n <= 8192.  Residuals are those of the returned vectors."""
    n = _check_csr(row_ptr, col, val)
    K = int(num_vectors)
    if n > DENSE_MAX_N:
        raise GsplatError(f"spectral_embedding_dense takes n <= {DENSE_MAX_N} (got {n}): it builds the n x n matrix")
    if not 1 <= K <= n:
        raise GsplatError(f"num_vectors must be in [1, n = {n}] (got {K})")
    if _bad_graph(row_ptr, col, val, n):
        return _zero_result(n, K, n, 2, val.device)
    S, g = _dense_s(row_ptr, col, val, n)
    S = (S + S.T) / 2
    lam, Q = torch.linalg.eigh(S)
    theta, V = lam.flip(0)[:K].contiguous(), Q.flip(1)[:, :K].contiguous()
    res = torch.linalg.norm(S @ V - V * theta, dim=0)
    return SpectralEmbedding(theta, _embed(g, V, row_normalize), V, res,
                             torch.tensor([0, 0, K, n], dtype=torch.int32, device=val.device))


def _mix_py(z: int) -> int:
    z &= _M64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & _M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & _M64
    z ^= z >> 31
    return z


def _signed(z: int) -> int:
    return z - (1 << 64) if z >= (1 << 63) else z


def _lsr(z: torch.Tensor, s: int) -> torch.Tensor:
    return (z >> s) & ((1 << (64 - s)) - 1)


def start_block(seed: int, epoch: int, n: int, cols, device="cpu") -> torch.Tensor:
    """x(seed, epoch, i, j) of include/gs_spectral.h for i < n and the columns `cols`: float64
    [n, len(cols)] in (-1, 1).  64-bit wrapping integer arithmetic, restated on int64."""
    base = _mix_py(int(seed) + (int(epoch) + 1) * 0x9E3779B97F4A7C15)
    j = torch.as_tensor(list(cols), dtype=torch.int64, device=device)
    z = (torch.arange(n, dtype=torch.int64, device=device)[:, None] * 128 + j[None, :]) ^ _signed(base)
    z = z ^ _lsr(z, 30)
    z = z * _signed(0xBF58476D1CE4E5B9)
    z = z ^ _lsr(z, 27)
    z = z * _signed(0x94D049BB133111EB)
    z = z ^ _lsr(z, 31)
    return (_lsr(z, 12).to(torch.float64) + 0.5) * 2.0 ** -51 - 1.0


def cheb_step(theta_1: float, theta_b: float, s: int):
    """(alpha, beta, gamma) of step s of the scaled Chebyshev filter that damps [-1, theta_B] and
    is scaled at theta_1: csrc/gs_spectral_small.h sp_cheb_step."""
    a = -1.0
    b = min(max(theta_b, a + 2.0 ** -10), 1.0)
    a0 = min(max(theta_1, b), 1.0)
    e, c = (b - a) / 2.0, (b + a) / 2.0
    sigma = e / (a0 - c)
    tau = 2.0 / sigma
    alpha, gamma = sigma / e, 0.0
    for _ in range(2, s + 1):
        sn = 1.0 / (tau - sigma)
        alpha, gamma = 2.0 * sn / e, -sigma * sn
        sigma = sn
    return alpha, -c * alpha, gamma


def _svqb(X, seed, epoch):
    G = X.T @ X
    d = torch.diagonal(G)
    s = torch.where((d > 0) & torch.isfinite(d), 1.0 / d.sqrt(), torch.zeros_like(d))
    A = s[:, None] * G * s[None, :]
    A = (A + A.T) / 2
    A.diagonal().copy_((s > 0).to(A.dtype))
    lam, Q = torch.linalg.eigh(A)
    ok = (lam > RANK_TOL * lam.max()) & (lam.max() > 0)
    T = s[:, None] * Q / lam.clamp_min(torch.finfo(torch.float64).tiny).sqrt()[None, :]
    X = X @ torch.where(ok[None, :], T, torch.zeros_like(T))
    gone = (~ok).nonzero().flatten().tolist()
    if gone:
        X[:, gone] = start_block(seed, epoch, X.shape[0], gone, X.device)
    return X


def spectral_embedding_torch(row_ptr: torch.Tensor, col: torch.Tensor, val: torch.Tensor, num_vectors: int, *,
                             tol: float = 1e-8, degree: int = 8, max_outer: int = 30, seed: int = 0,
                             row_normalize: bool = False) -> SpectralEmbedding:
    """spectral_embedding in fp64 torch operations on any device: the same Chebyshev-filtered
    subspace iteration with a sparse CSR product and torch.linalg.eigh for the small problems.  It
    reads the convergence test back every outer iteration.  Any num_vectors <= n."""
    n = _check_csr(row_ptr, col, val)
    K = num_vectors
    _check_solver(n, K, tol, degree, max_outer, seed, limit_k=False)
    dev = val.device
    B = block_width(n, K)
    if _bad_graph(row_ptr, col, val, n):
        return _zero_result(n, K, B, 2, dev)
    v = val.to(torch.float64)
    g = _inv_sqrt(csr_degrees(row_ptr, v))
    r, c = _rows_of(row_ptr), col.to(torch.int64)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)  # "Sparse CSR tensor support is in beta state"
        S = torch.sparse_csr_tensor(row_ptr, c, g[r] * v * g[c], size=(n, n), dtype=torch.float64, device=dev)
    X = start_block(seed, 0, n, range(B), dev)
    for t in range(max_outer):
        for p in range(2):
            X = _svqb(X, seed, 1 + 2 * t + p)
        W = S @ X
        H = X.T @ W
        H = torch.triu(H) + torch.triu(H, 1).T
        lam, Q = torch.linalg.eigh(H)
        order = torch.sort(lam, descending=True, stable=True).indices
        theta, Q = lam[order], Q[:, order]
        X, W = X @ Q, W @ Q
        res = torch.linalg.norm(W - X * theta, dim=0)
        conv = int((res[:K] <= tol).sum())
        if conv == K or t + 1 == max_outer:
            V = X[:, :K].contiguous()
            return SpectralEmbedding(theta[:K].contiguous(), _embed(g, V, row_normalize), V, res[:K].contiguous(),
                                     torch.tensor([0 if conv == K else 1, t + 1, conv, B], dtype=torch.int32,
                                                  device=dev))
        th1, thb = float(theta[0]), float(theta[-1])
        Y, Z = X, None
        for s in range(1, degree + 1):
            al, be, ga = cheb_step(th1, thb, s)
            Yn = al * (S @ Y) + be * Y
            if Z is not None:
                Yn = Yn + ga * Z
            Y, Z = Yn, Y
        X = Y
    raise AssertionError("unreachable")


# ---- the HIP path

def spectral_embedding(row_ptr: torch.Tensor, col: torch.Tensor, val: torch.Tensor, num_vectors: int, *,
                       tol: float = 1e-8, degree: int = 8, max_outer: int = 30, seed: int = 0,
                       row_normalize: bool = False) -> SpectralEmbedding:
    """The K = num_vectors leading eigenpairs of the normalised affinity of the symmetric CSR graph
    (row_ptr int64 [n + 1], col int32 [nnz], val [nnz] finite and >= 0, columns ascending and
    unique within a row; symmetry is the caller's promise, graph_check verifies it).  1 <= K <= 64,
    K <= n.  float64 device values run the HIP kernels: everything is enqueued at once, nothing is
    read back, reruns are bit-identical; anything else takes spectral_embedding_torch."""
    n = _check_csr(row_ptr, col, val)
    if not (val.is_cuda and val.dtype == torch.float64):
        return spectral_embedding_torch(row_ptr, col, val, num_vectors, tol=tol, degree=degree, max_outer=max_outer,
                                        seed=seed, row_normalize=row_normalize)
    K = num_vectors
    _check_solver(n, K, tol, degree, max_outer, seed)
    if n > MAX_N:
        raise GsplatError(f"the HIP spectral embedding takes n <= {MAX_N} (got {n}); {_TWIN} anywhere")
    need = dict(op="spectral embedding needs", twin=_TWIN)
    rp = _args.need(row_ptr.detach().contiguous(), "row_ptr", dtype=torch.int64, **need)
    cc = _args.need(col.detach().contiguous(), "col", dtype=torch.int32, **need)
    vv = _args.need(val.detach().contiguous(), "val", dtype=torch.float64, **need)
    dev, nnz = val.device, col.numel()
    L = _lib.load()
    nbytes = L.gs_spectral_workspace_bytes(n, nnz, K)
    if nbytes == 0:
        raise GsplatError(f"the HIP spectral embedding takes nnz < 2^31 (got {nnz})")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out = SpectralEmbedding(torch.empty(K, dtype=torch.float64, device=dev),
                            torch.empty(n, K, dtype=torch.float32, device=dev),
                            torch.empty(n, K, dtype=torch.float64, device=dev),
                            torch.empty(K, dtype=torch.float64, device=dev),
                            torch.empty(4, dtype=torch.int32, device=dev))
    a = _lib.GsSpectral(n=n, num_vectors=K, nnz=nnz, degree=degree, max_outer=max_outer,
                        row_normalize=int(bool(row_normalize)), seed=seed, tol=float(tol), row_ptr=rp.data_ptr(),
                        col=_args.ptr(cc, True), val=_args.ptr(vv, True), eigenvalues=out.eigenvalues.data_ptr(),
                        vectors=out.vectors.data_ptr(), embedding=out.embedding.data_ptr(),
                        residuals=out.residuals.data_ptr(), status=out.status.data_ptr(), workspace=ws.data_ptr(),
                        workspace_bytes=nbytes)
    _lib.check(L.gs_spectral_embedding(a, _lib.stream(dev)), "spectral embedding")
    return out


# ---- clustering

def spectral_clustering_graph(row_ptr: torch.Tensor, col: torch.Tensor, val: torch.Tensor, num_clusters: int, *,
                              kmeans_iters: int = 10, init_rows: Optional[torch.Tensor] = None, seed: int = 0,
                              **solver) -> SpectralClustering:
    """spectral_embedding(K = num_clusters) of the graph, then motion_init.kmeans (exactly
    kmeans_iters iterations) on the float32 embedding.  The initial centres are
    embedding[init_rows] (num_clusters row indices) or, with init_rows=None, k-means' own seeded
    rows.  **solver goes to spectral_embedding (tol, degree, max_outer, row_normalize)."""
    emb = spectral_embedding(row_ptr, col, val, num_clusters, seed=seed, **solver)
    init = None
    if init_rows is not None:
        rows = torch.as_tensor(init_rows, dtype=torch.int64, device=emb.embedding.device)
        if rows.dim() != 1 or rows.numel() != num_clusters:
            raise ValueError(f"init_rows must hold num_clusters = {num_clusters} row indices (got {tuple(rows.shape)})")
        init = emb.embedding[rows].contiguous()
    km = motion_init.kmeans(emb.embedding, num_clusters, init=init, iters=kmeans_iters, seed=seed)
    return SpectralClustering(km.labels, km.centers, km.counts, emb.embedding, emb.eigenvalues, emb.residuals,
                              emb.status)


def spectral_clustering(feats: torch.Tensor, num_clusters: int, *, knn: int = 20, transform: str = "clamp",
                        kmeans_iters: int = 10, init_rows: Optional[torch.Tensor] = None, seed: int = 0,
                        **solver) -> SpectralClustering:
    """The reference's similarity_mapping without the N x N matrix: feature_knn(feats, knn) ->
    knn_graph -> spectral_embedding(K = num_clusters) -> k-means on the embedding.  float32 device
    features run the HIP kernels end to end; host features take the torch twins."""
    if not isinstance(feats, torch.Tensor) or feats.dim() != 2:
        raise GsplatError(f"feats must be a [N, E] tensor (got {tuple(getattr(feats, 'shape', ()))})")
    x = feats.detach()
    sim, index = (feature_knn if x.is_cuda else feature_knn_torch)(x, int(knn))
    row_ptr, col, val = knn_graph(sim, index, x.shape[0], transform=transform)
    return spectral_clustering_graph(row_ptr, col, val, num_clusters, kmeans_iters=kmeans_iters, init_rows=init_rows,
                                     seed=seed, **solver)


__all__ = ("SpectralEmbedding", "SpectralClustering", "knn_graph", "graph_check", "csr_degrees", "block_width",
           "start_block", "cheb_step", "spectral_embedding", "spectral_embedding_torch", "spectral_embedding_dense",
           "spectral_clustering", "spectral_clustering_graph")
