"""The cosine top-k search (include/gs_feature_knn.h) without a GPU: the torch twin against the
numpy statement of the definition (tests/_feature_knn_cases.py), the argument checks, the sparse
affinity, the host validator under the sanitizers and the workspace layout."""
from __future__ import annotations

import ctypes
import os

import numpy as np
import pytest
import torch

from dynamic3dgaussians_amd import (_lib, build, cosine_topk, feature_knn, feature_knn_candidates, feature_knn_torch,
                                    knn_affinity)
from dynamic3dgaussians_amd._lib import GsplatError
from tests import _feature_knn_cases as K
from tests._harness import run_host_sanitizer

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("kind", K.GENERATORS)
@pytest.mark.parametrize("n,e,k", K.CASES)
def test_twin_is_the_numpy_statement_bit_for_bit(n, e, k, kind):
    x, sim, index = K.case(kind, n, e, k)
    s, i = feature_knn_torch(torch.from_numpy(x.copy()), k)
    assert s.dtype == torch.float64 and i.dtype == torch.int64
    assert _same_bits(i.numpy(), index)
    assert _same_bits(s.numpy(), sim)


@pytest.mark.parametrize("m", K.QUERY_M)
def test_twin_query_mode_and_query_chunks(m):
    x, q, sim, index = K.query_case("cluster", m)
    n, _, k = K.QUERY_DB
    for chunk_bytes in (256 << 20, 24 * n * 5):  # one chunk of queries, and chunks of five
        s, i = feature_knn_torch(torch.from_numpy(x.copy()), k, torch.from_numpy(q.copy()), chunk_bytes=chunk_bytes)
        assert _same_bits(i.numpy(), index) and _same_bits(s.numpy(), sim)


@pytest.mark.parametrize("which", ("duplicates", "zeros", "equal"))
def test_twin_ties_go_to_the_lower_index(which):
    x, k = K.tie_features(which)
    sim, index = K.topk(x, k)
    s, i = feature_knn_torch(torch.from_numpy(x), k)
    assert _same_bits(i.numpy(), index) and _same_bits(s.numpy(), sim)
    if which == "equal":  # every row's neighbours are the k lowest other indices
        assert index[0].tolist() == list(range(1, k + 1)) and index[5].tolist() == [0, 1, 2, 3, 4] + list(range(6, k + 1))
    if which == "zeros":  # a zero row has similarity 0 to everything
        zero = np.flatnonzero(~x.any(axis=1))
        assert (sim[zero] == 0).all() and index[zero[0]].tolist() == [j for j in range(k + 1) if j != zero[0]][:k]


def test_argument_refusals():
    x = torch.zeros(10, 8)
    for fn in (feature_knn, feature_knn_candidates):
        with pytest.raises(GsplatError, match="E <= 128"):
            fn(torch.zeros(4, 129), 2)
        with pytest.raises(GsplatError, match="k <= 32"):
            fn(x, 33)
        with pytest.raises(GsplatError, match="k must be an integer >= 1"):
            fn(x, 0)
        with pytest.raises(GsplatError, match="must be float32"):
            fn(x.double(), 2)
        with pytest.raises(GsplatError, match="queries must be \\[M, E\\]"):
            fn(x, 2, torch.zeros(3, 7))
        with pytest.raises(GsplatError, match="dtype and device"):
            fn(x, 2, torch.zeros(3, 8, dtype=torch.float64))
        with pytest.raises(GsplatError, match="feats must be a \\[N, E\\]"):
            fn(torch.zeros(10), 2)
        with pytest.raises(GsplatError, match="splits must be"):
            fn(x, 2, splits=33)
        with pytest.raises(GsplatError, match="on the CPU.*feature_knn_torch"):  # no quiet CPU path
            fn(x, 2)
    with pytest.raises(GsplatError, match="on the CPU"):
        cosine_topk(x, 2)
    with pytest.raises(GsplatError, match="k must be an integer"):
        feature_knn_torch(x, -1)
    with pytest.raises(GsplatError, match="must be float32"):
        feature_knn_torch(x.double(), 1)
    # the twin takes what the kernels refuse
    s, i = feature_knn_torch(torch.randn(40, 130), 35)
    assert s.shape == (40, 35) and i.shape == (40, 35) and bool((i >= 0).all())


def test_knn_affinity_against_a_dense_construction():
    n, k = 50, 6
    x, sim, index = K.features("cluster", n, 12), None, None
    sim, index = K.topk(x, k)
    A = knn_affinity(torch.from_numpy(sim), torch.from_numpy(index), n)
    assert A.is_sparse and tuple(A.shape) == (n, n) and A.dtype == torch.float64
    dense = np.zeros((n, n))
    for i in range(n):
        dense[i, index[i]] = sim[i]
    want = np.maximum(dense, dense.T)
    got = A.to_dense().numpy()
    assert _same_bits(got, want)
    assert _same_bits(got, got.T)
    assert A._nnz() == int((want != 0).sum())
    # one-sided, with missing neighbours skipped
    sim2, index2 = K.topk(x[:4], k)  # only three other rows: the tail is (-inf, -1)
    B = knn_affinity(torch.from_numpy(sim2), torch.from_numpy(index2), 4, symmetric=False).to_dense().numpy()
    assert np.isfinite(B).all() and (B != 0).sum() == 12
    with pytest.raises(GsplatError, match="alike"):
        knn_affinity(torch.zeros(3, 2), torch.zeros(3, 3, dtype=torch.int64), 3)
    with pytest.raises(GsplatError, match="one row of neighbours per node"):
        knn_affinity(torch.zeros(3, 2), torch.zeros(3, 2, dtype=torch.int64), 5)


def test_build_lists_the_new_sources_and_the_mirror_matches():
    assert build.SOURCES["gs_feature_knn.hip"] == ["-ffp-contract=off"]
    assert "gs_feature_knn_host.cpp" in build.SOURCES
    for f in ("gs_feature_knn.hip", "gs_feature_knn_host.cpp", "gs_feature_knn_layout.h"):
        assert os.path.exists(os.path.join(build.CSRC, f))
    L = _lib.load()
    assert ctypes.sizeof(_lib.GsFeatureKnn) == L.gs_feature_knn_struct_bytes()
    with open(os.path.join(REPO, "include", "gs_feature_knn.h")) as fh:
        header = fh.read()
    for name, value in (("GS_FKNN_MAX_E", _lib.FKNN_MAX_E), ("GS_FKNN_MAX_ROWS", "(1 << 26)"),
                        ("GS_FKNN_MAX_SPLITS", _lib.FKNN_MAX_SPLITS), ("GS_FKNN_SLACK", _lib.FKNN_SLACK),
                        ("GS_FKNN_ROW_BLOCK", _lib.FKNN_ROW_BLOCK), ("GS_FKNN_TILE", _lib.FKNN_TILE)):
        assert f"#define {name} {value}\n" in header or f"#define {name} {value} " in header, name
    assert _lib.FKNN_MAX_ROWS == 1 << 26 and _lib.FKNN_MAX_K == 32
    for E in (1, 16, 17, 35, 128):
        assert L.gs_feature_knn_e_pad(E) == -(-E // 16) * 16
    # the bound as DESIGN.md derives it: 1.01 (2 * 6 E_pad * 2^-23 + 2^-25)
    for E in (1, 32, 35, 128):
        assert L.gs_feature_knn_bound(E) == 1.01 * (2.0 * 6 * L.gs_feature_knn_e_pad(E) * 2.0 ** -23 + 2.0 ** -25)
    assert L.gs_feature_knn_bound(0) == 0.0 and L.gs_feature_knn_bound(129) == 0.0


def test_splits_rule_is_a_pure_function_of_the_sizes():
    L = _lib.load()
    assert L.gs_feature_knn_splits(300_000, 300_000, 32, 20) == 1  # the query blocks fill the chip
    assert L.gs_feature_knn_splits(16, 300_000, 32, 20) == _lib.FKNN_MAX_SPLITS
    assert L.gs_feature_knn_splits(1, 100, 32, 20) == 1  # four tiles: not worth a split
    assert L.gs_feature_knn_splits(300, 2049, 32, 20) == 16  # 65 tiles, at least four per chunk
    for bad in ((0, 5, 8, 1), (5, 0, 8, 1), (5, 5, 129, 1), (5, 5, 8, 33), (5, 5, 8, 0), ((1 << 26) + 1, 5, 8, 1)):
        assert L.gs_feature_knn_splits(*bad) == 0


def test_workspace_is_monotone_and_covers_the_layout():
    L = _lib.load()
    ws = L.gs_feature_knn_workspace_bytes

    def model(M, N, E, k, S, self_):
        pad = lambda v: -(-v // 256) * 256  # noqa: E731
        e_pad, kp = -(-E // 16) * 16, k + _lib.FKNN_SLACK
        rows = lambda r: -(-r // 32) * 32  # noqa: E731
        side = lambda r: pad(rows(r) * e_pad * 4) + pad(rows(r) * e_pad * 6)  # noqa: E731
        total = side(N) + (0 if self_ else side(M))
        total += 2 * pad(M * S * kp * 4) + 2 * pad(M * S * 4) + pad(M * 4) + 256
        return total

    for M, N, E, k, S, self_ in ((1, 1, 1, 1, 1, 1), (2049, 2049, 35, 8, 3, 1), (7, 2049, 32, 20, 8, 0),
                                 (300, 1025, 128, 32, 1, 0), (300_000, 300_000, 32, 20, 1, 1)):
        assert ws(M, N, E, k, S, self_) == model(M, N, E, k, S, self_), (M, N, E, k, S, self_)
    assert ws(16, 300_000, 32, 20, 0, 0) == model(16, 300_000, 32, 20, L.gs_feature_knn_splits(16, 300_000, 32, 20), 0)
    base = ws(1000, 1000, 32, 8, 2, 1)
    assert ws(1001, 1001, 32, 8, 2, 1) >= base and ws(1000, 1000, 33, 8, 2, 1) > base
    assert ws(1000, 1000, 32, 9, 2, 1) > base and ws(1000, 1000, 32, 8, 3, 1) > base
    assert ws(1000, 1000, 32, 8, 2, 0) > base  # separate queries bring their own rows
    for bad in ((0, 5, 8, 1, 1, 0), (5, 5, 129, 1, 1, 1), (5, 5, 8, 33, 1, 1), (5, 5, 8, 1, 33, 1), (5, 5, 8, 1, -1, 1),
                (4, 5, 8, 1, 1, 1)):  # the last: a self search has M = N
        assert ws(*bad) == 0


def _block(**kw):
    buf = ctypes.create_string_buffer(4096)
    base = ctypes.addressof(buf) // 16 * 16 + 16
    a = _lib.GsFeatureKnn(N=100, M=7, E=32, k=5, splits=0, feats=base, queries=base, sim=base, index=base, stats=base,
                          workspace=base, workspace_bytes=1 << 30)
    for name, v in kw.items():
        setattr(a, name, v)
    a._keep = buf
    return a


@pytest.mark.parametrize("field,value,message", [
    ("E", 0, "E must be in"), ("E", 129, "feature_knn_torch"), ("k", 0, "k must be in"), ("k", 33, "feature_knn_torch"),
    ("N", 0, "N must be in"), ("M", 0, "M must be in"), ("N", (1 << 26) + 1, "N must be in"),
    ("queries", None, "M must equal N"), ("splits", 33, "splits must be in"), ("splits", -1, "splits must be in"),
    ("feats", None, "feats is required"), ("sim", None, "sim and index are required"),
    ("index", None, "sim and index are required"), ("cand_sim", 4096, "go together"),
    ("workspace", None, "workspace is required"), ("workspace_bytes", 64, "needed"),
])
def test_validator_refuses_with_a_message(field, value, message):
    L = _lib.load()
    assert L.gs_feature_knn_validate(ctypes.byref(_block())) == 0
    assert L.gs_feature_knn_validate(ctypes.byref(_block(stats=None))) == 0
    assert L.gs_feature_knn_validate(ctypes.byref(_block(**{field: value}))) != 0
    assert message in L.gs_last_error().decode()
    assert L.gs_feature_knn_validate(None) != 0 and "null argument block" in L.gs_last_error().decode()


def test_validator_is_sanitizer_clean(tmp_path):
    """gs_feature_knn_host.cpp (with gs_host.cpp's error state) under ASan + UBSan in a plain CPU
    executable with its own main: nothing preloaded, nothing loaded into Python."""
    run_host_sanitizer(tmp_path, "feature_knn_host_sanitize.c", ["gs_feature_knn_host.cpp", "gs_host.cpp"],
                       "feature knn host sanitize ok")
