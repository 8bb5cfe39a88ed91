"""The cosine top-k search's definition (include/gs_feature_knn.h) stated in numpy, the cases and
the feature generators of tests/test_feature_knn.py and tests/test_gpu_feature_knn.py.  Every sum
is a loop over channels in float64, as the definition is; nothing here calls the package.

    norm_i = sqrt(sum_c x_ic^2)                    float64, c ascending
    xh_ic  = float32(x_ic / max(norm_i, 1e-12))
    s_ij   = sum_c xh_ic xh_jc                     float64, c ascending

Products of float32 values are exact in float64, so only the order of the additions matters.
"""
from __future__ import annotations

import functools

import numpy as np

# (N, E, k): tile edges on both axes (32-row tiles, 128-row query blocks), channel padding (E = 35
# pads to 48, 3 to 16), k > N - 1, every k-step count of the matrix instruction between them
CASES = ((1, 8, 1), (2, 3, 5), (33, 1, 4), (130, 16, 32), (1000, 3, 5), (2049, 32, 20), (2049, 35, 8),
         (1537, 64, 32), (1025, 128, 20))
GENERATORS = ("gauss", "cluster", "positive")
QUERY_DB = (2049, 32, 20)  # the database of the query-mode tests
QUERY_M = (1, 7, 300)
SPLITS = (1, 3, 8)


def features(kind: str, n: int, e: int, seed: int = 0) -> np.ndarray:
    rng = np.random.default_rng([seed, n, e, GENERATORS.index(kind)])
    if kind == "gauss":
        x = rng.standard_normal((n, e))
    elif kind == "cluster":  # 8 centres + 0.15 noise
        centres = rng.standard_normal((8, e))
        x = centres[rng.integers(0, 8, n)] + 0.15 * rng.standard_normal((n, e))
    else:  # every similarity near 1
        x = rng.random((n, e)) + 0.05
    return np.ascontiguousarray(x, dtype=np.float32)


def unit_rows(x: np.ndarray) -> np.ndarray:
    xd = x.astype(np.float64)
    ss = np.zeros(x.shape[0], np.float64)
    for c in range(x.shape[1]):
        ss += xd[:, c] * xd[:, c]
    return (xd / np.maximum(np.sqrt(ss), 1e-12)[:, None]).astype(np.float32)


def similarities(xq: np.ndarray, xd: np.ndarray) -> np.ndarray:
    """s [M, N] of unit rows, float64, channel by channel."""
    q, d = xq.astype(np.float64), xd.astype(np.float64)
    s = np.zeros((q.shape[0], d.shape[0]), np.float64)
    for c in range(q.shape[1]):
        s += q[:, c, None] * d[None, :, c]
    return s


def topk(feats: np.ndarray, k: int, queries: np.ndarray | None = None):
    """(sim float64 [M, k], index int64 [M, k]): by (s descending, index ascending), self excluded
    by index without queries, (-inf, -1) past the rows that exist."""
    xd = unit_rows(feats)
    xq = xd if queries is None else unit_rows(queries)
    s = similarities(xq, xd)
    m, n = s.shape
    sim = np.full((m, k), -np.inf)
    index = np.full((m, k), -1, np.int64)
    for i in range(m):
        cols = np.arange(n) if queries is not None else np.delete(np.arange(n), i)
        order = cols[np.argsort(-s[i, cols], kind="stable")][:k]  # stable: ties keep ascending index
        sim[i, :len(order)] = s[i, order]
        index[i, :len(order)] = order
    return sim, index


@functools.lru_cache(maxsize=None)
def case(kind: str, n: int, e: int, k: int):
    """(feats, sim, index) of a self-search case, computed once and shared (read-only)."""
    x = features(kind, n, e)
    sim, index = topk(x, k)
    for a in (x, sim, index):
        a.setflags(write=False)
    return x, sim, index


@functools.lru_cache(maxsize=None)
def query_case(kind: str, m: int):
    """(feats, queries, sim, index) of a query-mode case against QUERY_DB."""
    n, e, k = QUERY_DB
    both = features(kind, n + m, e, seed=1)  # one draw, so the queries share the database's clusters
    x, q = np.ascontiguousarray(both[:n]), np.ascontiguousarray(both[n:])
    sim, index = topk(x, k, q)
    for a in (x, q, sim, index):
        a.setflags(write=False)
    return x, q, sim, index


def tie_features(which: str) -> tuple[np.ndarray, int]:
    """Heavy-tie inputs and their k: 40 exact duplicates of one row inside N = 1000, 100 all-zero
    rows inside N = 1000, all rows equal at N = 300."""
    if which == "duplicates":
        x = features("gauss", 1000, 16, seed=2).copy()
        x[np.random.default_rng(5).choice(1000, 40, replace=False)] = x[17]
        return x, 20
    if which == "zeros":
        x = features("cluster", 1000, 32, seed=3).copy()
        x[np.random.default_rng(6).choice(1000, 100, replace=False)] = 0.0
        return x, 8
    return np.tile(features("positive", 1, 24, seed=4), (300, 1)), 20
