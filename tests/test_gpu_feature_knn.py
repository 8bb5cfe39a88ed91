"""The cosine top-k search (include/gs_feature_knn.h) on the GPU against the numpy statement of its
definition (tests/_feature_knn_cases.py), never against the code under test.

Exactness is bit for bit on every row, none excluded: similarities float64, indices int64, ties to
the lower index.  The certificate's premise |st - s| <= B (B = gs_feature_knn_bound(E), derived in
DESIGN.md 9.20 from the number formats, not measured) is checked on every candidate the scan kept;
the largest |st - s| / B and the fallback share of each generator are printed and collected in
RECORDS (tools/feature_knn_bench.py --parity -> profiles/feature_knn/parity.json).

Measured on an MI355X over all cases (profiles/feature_knn/parity.json): largest |st - s| / B 0.0058 (2049 x 32
cluster); fallback share 0 on every case and generator but 33 x 1 "positive" (one channel: every similarity is
exactly 1), where it is 1; the all-equal tie case sends all 300 rows to the fallback.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

from dynamic3dgaussians_amd import (_lib, cosine_topk, feature_knn, feature_knn_candidates, feature_knn_torch)
from dynamic3dgaussians_amd.feature_knn import certificate_bound
from tests import _feature_knn_cases as K

pytestmark = pytest.mark.gpu
DEV = "cuda"

RECORDS = []  # {"what", "case", "kind", ...}: what tools/feature_knn_bench.py --parity writes down


def _dev(x):
    return torch.from_numpy(np.array(x)).to(DEV)


def _same_bits(t, ref):
    a = np.ascontiguousarray(t.cpu().numpy())
    ref = np.ascontiguousarray(ref)
    return a.shape == ref.shape and a.dtype == ref.dtype and a.tobytes() == ref.tobytes()


def _check(out, sim, index, what):
    s, i = out[0], out[1]
    assert s.dtype == torch.float64 and i.dtype == torch.int64
    wrong = np.flatnonzero((i.cpu().numpy() != index).any(axis=1))
    assert wrong.size == 0, f"{what}: {wrong.size} rows differ in index, first {wrong[:5]}"
    assert _same_bits(s, sim), f"{what}: similarities differ in bits"


@pytest.mark.parametrize("kind", K.GENERATORS)
@pytest.mark.parametrize("n,e,k", K.CASES)
def test_self_search_is_exact_on_every_row(n, e, k, kind):
    x, sim, index = K.case(kind, n, e, k)
    s, i, stats = feature_knn(_dev(x), k, return_stats=True)
    _check((s, i), sim, index, f"{n}x{e} k={k} {kind}")
    certified, fallback = (int(v) for v in stats.cpu())
    assert certified + fallback == n
    if kind == "gauss" and n > k + _lib.FKNN_SLACK + 1:
        assert certified >= 1  # the scan's path is what was tested
    print(f"{n}x{e} k={k} {kind}: fallback share {fallback / n:.4f}")
    RECORDS.append({"what": "fallback_share", "case": [n, e, k], "kind": kind, "value": fallback / n})


@pytest.mark.parametrize("splits", K.SPLITS)
@pytest.mark.parametrize("n,e,k", [c for c in K.CASES if c[0] >= 1000])
def test_self_search_with_forced_splits(n, e, k, splits):
    # chunk boundaries ceil(N / splits): 683 and 1366 at N = 2049, 257 ... at splits = 8 -- no multiple of 32
    x, sim, index = K.case("cluster", n, e, k)
    assert -(-n // 3) % 32 != 0
    s, i, stats = feature_knn(_dev(x), k, splits=splits, return_stats=True)
    _check((s, i), sim, index, f"{n}x{e} k={k} splits={splits}")
    assert int(stats.sum()) == n


@pytest.mark.parametrize("kind", K.GENERATORS)
@pytest.mark.parametrize("splits", (None,) + K.SPLITS)
@pytest.mark.parametrize("m", K.QUERY_M)
def test_query_search_is_exact(m, splits, kind):
    x, q, sim, index = K.query_case(kind, m)
    k = K.QUERY_DB[2]
    s, i, stats = feature_knn(_dev(x), k, _dev(q), splits=splits, return_stats=True)
    _check((s, i), sim, index, f"M={m} splits={splits} {kind}")
    assert int(stats.sum()) == m


def test_query_may_be_a_database_row():
    """Only the self search excludes by index: a query equal to a database row finds it first."""
    x, _, _ = K.case("gauss", 130, 16, 32)
    s, i = feature_knn(_dev(x), 3, _dev(x[40:45]))
    assert i[:, 0].tolist() == [40, 41, 42, 43, 44]
    sim, index = K.topk(x, 3, x[40:45])
    _check((s, i), sim, index, "rows as queries")


@pytest.mark.parametrize("which", ("duplicates", "zeros", "equal"))
def test_heavy_ties(which):
    x, k = K.tie_features(which)
    sim, index = K.topk(x, k)
    s, i, stats = feature_knn(_dev(x), k, return_stats=True)
    _check((s, i), sim, index, which)
    certified, fallback = (int(v) for v in stats.cpu())
    assert certified + fallback == x.shape[0]
    if which == "equal":
        assert fallback == x.shape[0] and certified == 0  # nothing separates the k-th from the rest
    if which == "zeros":
        assert fallback >= 100  # a zero row ties with everything
    if which == "duplicates":
        assert fallback < x.shape[0]


@pytest.mark.parametrize("kind", K.GENERATORS)
@pytest.mark.parametrize("n,e,k", K.CASES)
def test_certificate_premise_holds_on_every_candidate(n, e, k, kind):
    x, _, _ = K.case(kind, n, e, k)
    for splits in (None, 3):
        st, idx, count, theta = (t.cpu().numpy() for t in feature_knn_candidates(_dev(x), k, splits=splits))
        S, kp = st.shape[1], k + _lib.FKNN_SLACK
        assert st.shape == (n, S, kp) and idx.shape == st.shape and count.shape == (n, S) and theta.shape == (n, S)
        xh = K.unit_rows(x)
        s = K.similarities(xh, xh)
        B = certificate_bound(e)
        assert 0 < B < 2e-4
        slot = np.arange(kp)[None, None, :]
        kept = slot < count[:, :, None]
        assert (idx[~kept] == -1).all() and np.isneginf(st[~kept]).all()
        assert (count <= kp).all() and (idx[kept] >= 0).all() and (idx[kept] < n).all()
        rows = np.broadcast_to(np.arange(n)[:, None, None], idx.shape)
        assert (idx[kept] != rows[kept]).all()  # a row is never its own candidate
        err = np.abs(st[kept].astype(np.float64) - s[rows[kept], idx[kept]])
        frac = float(err.max() / B) if err.size else 0.0
        print(f"{n}x{e} k={k} {kind} splits={S}: max |st - s| / B = {frac:.4g}")
        RECORDS.append({"what": "error_over_bound", "case": [n, e, k], "kind": kind, "value": frac})
        assert frac <= 1.0
        # the invariant: every row of a chunk that was not kept has st <= theta, so s <= theta + B
        L = -(-n // S)
        for c in range(S):
            lo, hi = c * L, min(n, (c + 1) * L)
            if lo >= hi:
                assert (count[:, c] == 0).all() and np.isneginf(theta[:, c]).all()
                continue
            inside = s[:, lo:hi].copy()
            inside[np.arange(n)[(np.arange(n) >= lo) & (np.arange(n) < hi)], np.arange(lo, hi) - lo] = -np.inf
            for r in range(0, n, max(1, n // 64)):  # a sample of rows
                keep = idx[r, c, :count[r, c]]
                left = np.delete(inside[r], keep - lo)
                left = left[np.isfinite(left)]
                if left.size:
                    assert np.isfinite(theta[r, c]) and left.max() <= float(theta[r, c]) + B
                else:
                    assert np.isneginf(theta[r, c])


def test_reruns_are_bit_identical():
    x, _, _ = K.case("cluster", 2049, 32, 20)
    xd = _dev(x)
    first = feature_knn(xd, 20)
    for _ in range(2):
        again = feature_knn(xd, 20)
        assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    q = _dev(K.query_case("positive", 7)[1])
    a, b, c = (feature_knn(xd, 20, q) for _ in range(3))
    assert torch.equal(a[0], b[0]) and torch.equal(a[0], c[0]) and torch.equal(a[1], b[1]) and torch.equal(a[1], c[1])


def test_foreign_stream_and_slices():
    x, sim, index = K.case("gauss", 2049, 35, 8)
    xd = _dev(x)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        s, i = feature_knn(xd, 8)
    stream.synchronize()
    _check((s, i), sim, index, "foreign stream")
    wide = torch.zeros(2049, 70, device=DEV)
    wide[:, ::2] = xd
    assert not wide[:, ::2].is_contiguous()
    _check(feature_knn(wide[:, ::2], 8), sim, index, "strided columns")
    tall = torch.zeros(4098, 35, device=DEV)
    tall[1::2] = xd
    _check(feature_knn(tall[1::2], 8), sim, index, "strided rows")


def test_cosine_topk_is_feature_knn_rounded():
    x, sim, index = K.case("cluster", 1537, 64, 32)
    values, indices = cosine_topk(_dev(x), 32)
    assert values.dtype == torch.float32 and indices.dtype == torch.int64
    assert _same_bits(indices, index) and _same_bits(values, sim.astype(np.float32))


def test_twin_on_the_device_agrees():
    x, sim, index = K.case("positive", 1000, 3, 5)
    _check(feature_knn_torch(_dev(x), 5), sim, index, "twin on the device")
