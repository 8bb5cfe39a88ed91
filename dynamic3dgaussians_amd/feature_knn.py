"""Exact cosine top-k neighbours in feature space on the matrix-core kernels of
csrc/gs_feature_knn.hip (C ABI, definition and certificate: include/gs_feature_knn.h).

The reference searches its 32-128-channel semantic features through a dense N x N
cosine matrix, twice:

    tensor = F.normalize(tensor, dim=1); sim = tensor @ tensor.T       # feature_rendering/feature_utils.py:7-16
    values, indices = torch.topk(sim, k + 1); indices[:, 1:]
    cos_sim_matrix = feats @ feats.T -> SpectralClustering(precomputed)  # motion_utils.py:57-116 similarity_mapping

which at 300k Gaussians is 360 GB.  Here the matrix is never formed:

    values, indices = cosine_topk(feats, k)                # the feature_utils.py drop-in
    sim, index = feature_knn(feats, k)                     # float64 similarities, int64 indices
    sim, index = feature_knn(feats, k, queries=text_emb)   # open-vocabulary queries against the table
    A = knn_affinity(sim, index, n)                        # sparse max(A, A^T) for similarity_mapping's clustering

The answer is exact and unique: similarities are fp64 sums over the fp32-rounded unit
rows in channel order, neighbours ordered by (similarity descending, index ascending),
a row never its own neighbour in the self search, (-inf, -1) where fewer than k rows
exist.  The matrix cores only propose candidates; an fp64 rerank with a proven bound
certifies them, and the rows it cannot certify (ties, duplicated or all-zero features)
are searched exhaustively in fp64 on the device.  Reruns are bit-identical.

`feature_knn_torch` states the definition in PyTorch operations for any device: the
parity oracle and the CPU path.  The HIP path has no CPU fallback: host tensors raise.
Features must be finite.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _args, _lib
from ._lib import GsplatError

MAX_E, MAX_K, MAX_SPLITS, SLACK = _lib.FKNN_MAX_E, _lib.FKNN_MAX_K, _lib.FKNN_MAX_SPLITS, _lib.FKNN_SLACK
_TWIN = "feature_knn_torch runs"


def _shapes(feats, k, queries):
    """(N, M, E) after the checks the device entry and the twin share."""
    if not isinstance(feats, torch.Tensor) or feats.dim() != 2:
        raise GsplatError(f"feats must be a [N, E] tensor (got {tuple(getattr(feats, 'shape', ()))})")
    if isinstance(k, bool) or not isinstance(k, int) or k < 1:
        raise GsplatError(f"k must be an integer >= 1 (got {k!r})")
    N, E = feats.shape
    if E < 1:
        raise GsplatError("feats must have at least one channel")
    M = N
    if queries is not None:
        if not isinstance(queries, torch.Tensor) or queries.dim() != 2 or queries.shape[1] != E:
            raise GsplatError(f"queries must be [M, E] with feats' E = {E} channels "
                              f"(got {tuple(getattr(queries, 'shape', ()))})")
        if queries.dtype != feats.dtype or queries.device != feats.device:
            raise GsplatError("queries must have feats' dtype and device")
        M = queries.shape[0]
    return N, M, E


def _limits(E, k):
    if E > MAX_E:
        raise GsplatError(f"the HIP feature search takes E <= {MAX_E} channels (got {E}); feature_knn_torch takes any size")
    if k > MAX_K:
        raise GsplatError(f"the HIP feature search takes k <= {MAX_K} (got {k}); feature_knn_torch takes any size")


def _unit_rows(x: torch.Tensor) -> torch.Tensor:
    """fl32(x / max(|x|, 1e-12)): the squares added in channel order in float64."""
    xd = x.to(torch.float64)
    ss = torch.zeros(x.shape[0], dtype=torch.float64, device=x.device)
    for c in range(x.shape[1]):
        ss = ss + xd[:, c] * xd[:, c]
    return (xd / ss.sqrt().clamp_min(1e-12)[:, None]).to(torch.float32)


def feature_knn_torch(feats: torch.Tensor, k: int, queries: Optional[torch.Tensor] = None, *,
                      chunk_bytes: int = 256 << 20):
    """feature_knn in PyTorch operations on any device: the definition, channel loop included.
    Queries are taken in chunks so that no intermediate exceeds chunk_bytes."""
    N, M, E = _shapes(feats, k, queries)
    if feats.dtype != torch.float32:
        raise GsplatError(f"feats must be float32 (got {feats.dtype})")
    dev = feats.device
    xd = _unit_rows(feats.detach()).to(torch.float64)
    xq = xd if queries is None else _unit_rows(queries.detach()).to(torch.float64)
    sim = torch.full((M, k), float("-inf"), dtype=torch.float64, device=dev)
    index = torch.full((M, k), -1, dtype=torch.int64, device=dev)
    rows = max(1, int(chunk_bytes // (24 * max(N, 1))))  # s, its sorted copy and the int64 order
    kk = min(k, N)
    for m0 in range(0, M, rows):
        m1 = min(M, m0 + rows)
        s = torch.zeros(m1 - m0, N, dtype=torch.float64, device=dev)
        for c in range(E):
            s = s + xq[m0:m1, c, None] * xd[None, :, c]
        if queries is None:
            r = torch.arange(m0, m1, device=dev)
            s[r - m0, r] = float("-inf")
        # stable: equal similarities keep ascending index order
        v, i = torch.sort(s, dim=1, descending=True, stable=True)
        v, i = v[:, :kk], i[:, :kk]
        sim[m0:m1, :kk] = v
        index[m0:m1, :kk] = torch.where(v == float("-inf"), torch.full_like(i, -1), i)
    return sim, index


def _call(feats, k, queries, splits, debug):
    N, M, E = _shapes(feats, k, queries)
    need = dict(op="feature search needs", twin=_TWIN)
    _limits(E, k)
    if splits is not None and (isinstance(splits, bool) or not isinstance(splits, int)
                               or not 1 <= splits <= MAX_SPLITS):
        raise GsplatError(f"splits must be an integer in [1, {MAX_SPLITS}] or None (got {splits!r})")
    if feats.dtype != torch.float32:
        raise GsplatError(f"feats must be float32 (got {feats.dtype})")
    _args.need(feats.detach().contiguous(), "feats", **need)  # a host tensor is refused before anything is allocated
    dev = feats.device
    sim = torch.empty(M, k, dtype=torch.float64, device=dev)
    index = torch.empty(M, k, dtype=torch.int64, device=dev)
    stats = torch.zeros(2, dtype=torch.int64, device=dev)
    if N == 0 or M == 0:
        return sim.fill_(float("-inf")), index.fill_(-1), stats, None
    x = _args.need(feats.detach().contiguous(), "feats", **need)
    q = None if queries is None else _args.need(queries.detach().contiguous(), "queries", **need)
    L = _lib.load()
    S = int(splits or 0)
    nbytes = L.gs_feature_knn_workspace_bytes(M, N, E, k, S, int(q is None))
    if nbytes == 0:
        raise GsplatError(f"the HIP feature search takes at most {_lib.FKNN_MAX_ROWS} rows (got N = {N}, M = {M})")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    a = _lib.GsFeatureKnn(N=N, M=M, E=E, k=k, splits=S, feats=x.data_ptr(), queries=_args.ptr(q), sim=sim.data_ptr(),
                          index=index.data_ptr(), stats=stats.data_ptr(), workspace=ws.data_ptr(),
                          workspace_bytes=nbytes)
    cand = None
    if debug:
        S_used = S or L.gs_feature_knn_splits(M, N, E, k)
        kp = k + SLACK
        cand = (torch.empty(M, S_used, kp, dtype=torch.float32, device=dev),
                torch.empty(M, S_used, kp, dtype=torch.int32, device=dev),
                torch.empty(M, S_used, dtype=torch.int32, device=dev),
                torch.empty(M, S_used, dtype=torch.float32, device=dev))
        a.cand_sim, a.cand_index, a.cand_count, a.cand_theta = (t.data_ptr() for t in cand)
    _lib.check(L.gs_feature_knn(a, _lib.stream(dev)), "feature knn")
    return sim, index, stats, cand


def feature_knn(feats: torch.Tensor, k: int, queries: Optional[torch.Tensor] = None, *, splits: Optional[int] = None,
                return_stats: bool = False):
    """The k rows of feats [N, E] most cosine-similar to every query: (sim [M, k] float64, index
    [M, k] int64), ordered by (sim descending, index ascending), (-inf, -1) past the rows that
    exist.  queries [M, E] or None: the rows of feats themselves, none its own neighbour.  float32
    device tensors, E <= 128, k <= 32; exact and bit-identical from run to run.  splits forces the
    number of database chunks of the scan (None: chosen from the sizes; the answer does not depend
    on it).  return_stats adds an int64 [2] device tensor: the queries the scan's candidates were
    certified for, and those searched exhaustively."""
    sim, index, stats, _ = _call(feats, k, queries, splits, False)
    return (sim, index, stats) if return_stats else (sim, index)


def feature_knn_candidates(feats: torch.Tensor, k: int, queries: Optional[torch.Tensor] = None, *,
                           splits: Optional[int] = None):
    """Debug: what the matrix-core scan kept before the exact rerank, per (query, chunk):
    (st float32 [M, S, k + 16], index int32 [M, S, k + 16], count int32 [M, S], theta float32
    [M, S]); entries past count are (-inf, -1), theta is -inf where the chunk dropped nothing.
    Every database row of the chunk that is not listed has st <= theta."""
    return _call(feats, k, queries, splits, True)[3]


def certificate_bound(E: int) -> float:
    """The bound on |st - s| the certificate uses for E channels."""
    return float(_lib.load().gs_feature_knn_bound(int(E)))


def cosine_topk(feats: torch.Tensor, k: int):
    """feature_utils.py's search: (values float32 [N, k], indices int64 [N, k]) of the k most
    similar other rows.  The values are feature_knn's, rounded to float32."""
    sim, index = feature_knn(feats, k)
    return sim.to(torch.float32), index


def knn_affinity(sim: torch.Tensor, index: torch.Tensor, n: int, symmetric: bool = True) -> torch.Tensor:
    """The sparse [n, n] COO affinity of a neighbour list: A[i, index[i, j]] = sim[i, j] (entries
    with index -1 skipped), and max(A, A^T) over the stored entries with symmetric=True -- the
    kNN-sparsified stand-in for similarity_mapping's dense cos_sim_matrix.  Plain torch, any
    device."""
    if sim.shape != index.shape or sim.dim() != 2:
        raise GsplatError(f"sim and index must be [M, k] alike (got {tuple(sim.shape)}, {tuple(index.shape)})")
    if symmetric and sim.shape[0] != n:
        raise GsplatError(f"a symmetric affinity needs one row of neighbours per node (got {sim.shape[0]} for n = {n})")
    rows = torch.arange(sim.shape[0], device=index.device)[:, None].expand_as(index)
    keep = index >= 0
    r, c, v = rows[keep], index[keep], sim[keep]
    if symmetric:
        r, c, v = torch.cat([r, c]), torch.cat([c, r]), torch.cat([v, v])
        # one entry per (row, column): the largest value.  Sort by value, then stably by position,
        # and keep the last of every run.
        order = torch.argsort(v, stable=True)
        r, c, v = r[order], c[order], v[order]
        order = torch.argsort(r * n + c, stable=True)
        r, c, v = r[order], c[order], v[order]
        flat = r * n + c
        last = torch.ones_like(flat, dtype=torch.bool)
        last[:-1] = flat[1:] != flat[:-1]
        r, c, v = r[last], c[last], v[last]
    return torch.sparse_coo_tensor(torch.stack([r, c]), v, (sim.shape[0] if not symmetric else n, n)).coalesce()
