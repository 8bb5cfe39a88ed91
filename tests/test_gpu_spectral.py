"""The spectral embedding (include/gs_spectral.h) on the GPU against torch.linalg.eigh of the dense
normalised affinity (tests/_spectral_cases.py), never against the code under test.

Eigenvectors are unique only up to sign and to rotation inside a degenerate eigenvalue, so every
check is on an invariant with a derived bound: a Ritz value lies within its residual of an
eigenvalue (+ 64 n 2^-53 for eigh's own error), |V^T V - I|_max <= 2^-40, the residuals recomputed
from the returned vectors are <= tol + 64 n 2^-53 and agree with the reported ones to 64 n 2^-53,
the projector onto the K leading vectors is within Davis-Kahan's 2 |R|_F / (gap - tol) of the
oracle's wherever the gap is >= 1e-3, the embedding is fl32(g V) bit for bit.  The largest
error / bound of each check is collected in RECORDS (tools/spectral_bench.py --parity ->
profiles/spectral/parity.json).  Labels are compared with an fp64 k-means on the oracle's embedding
on every decision-robust point, with no permutation.
"""
from __future__ import annotations

import functools

import pytest
import torch

from dynamic3dgaussians_amd import (SpectralEmbedding, cluster_medians, coefs_from_centers, feature_knn,
                                    init_motion_coefs_from_features, spectral_clustering, spectral_embedding,
                                    spectral_embedding_torch)
from tests import _spectral_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda"

RECORDS = {}  # check -> largest error / bound over the cases run


def _graph(c):
    return c.row_ptr.to(DEV), c.col.to(DEV), c.val.to(DEV)


def _hip(c, K, **kw):
    kw = {"tol": C.TOL, **C.SOLVER.get((c.name, K), {}), **kw}
    out = spectral_embedding(*_graph(c), K, **kw)
    assert all(t.is_cuda for t in out)
    return SpectralEmbedding(*(t.cpu() for t in out))


@functools.lru_cache(maxsize=None)
def _large():
    c = C.large_case(feature_knn)
    return c, C.components(c)


@pytest.mark.parametrize("name,K", C.SMALL)
def test_against_the_dense_oracle(name, K):
    out = _hip(C.small_case(name), K)
    print(name, K, "status", out.status.tolist(), "largest residual", float(out.residuals.max()))
    C.check_against_oracle(name, K, out, report=RECORDS)
    C.check_known_answers(name, K, out)


@pytest.mark.parametrize("name,K", [("star", 2), ("blobs-b", 5), ("blobs-c", 9)])
def test_row_normalize_gives_unit_rows(name, K):
    c, g = C.small_case(name), C.oracle(name).g
    out = _hip(c, K, row_normalize=True)
    assert out.status.tolist()[0] == 0
    norms = out.embedding.double().norm(dim=1)
    err = float((norms[g > 0] - 1).abs().max())
    print(name, K, "largest |row norm - 1|", err)
    assert err <= 2.0 ** -23
    assert out.embedding[g == 0].numpy().tobytes() == bytes(4 * K * int((g == 0).sum()))
    # the rows are the plain embedding's, scaled
    plain = _hip(c, K)
    u = C.oracle(name).g[:, None] * plain.vectors
    want = (u / u.norm(dim=1, keepdim=True).clamp_min(1e-300)).float()
    assert float((out.embedding[g > 0] - want[g > 0]).abs().max()) <= 2.0 ** -22


def _compare_labels(c, K, labels, oracle_embedding):
    want, robust = C.kmeans_f64(oracle_embedding, C.first_rows(c.planted, K))
    excluded = 1.0 - float(robust.double().mean())
    agree_planted = float((want == c.planted).double().mean())
    print(c.name, K, "excluded share", excluded, "oracle labels equal the planted ones on", agree_planted)
    assert excluded <= 0.05
    wrong = (labels.cpu() != want) & robust
    assert int(wrong.sum()) == 0, f"{int(wrong.sum())} decision-robust points differ, first {wrong.nonzero()[:5].flatten()}"


@pytest.mark.parametrize("name,K", [("blobs-b", 5), ("blobs-c", 8)])
def test_labels_equal_kmeans_on_the_oracle_embedding(name, K):
    c = C.small_case(name)
    out = spectral_clustering(c.feats.to(DEV), K, knn=c.knn, init_rows=C.first_rows(c.planted, K), tol=C.TOL)
    assert out.status.tolist()[0] == 0 and out.labels.dtype == torch.int64 and tuple(out.centers.shape) == (K, K)
    o = C.oracle(name)
    _compare_labels(c, K, out.labels, o.g[:, None] * o.Q[:, :K])


def test_labels_on_blobs_a_are_the_three_components():
    c = C.small_case("blobs-a")
    out = spectral_clustering(c.feats.to(DEV), 3, knn=c.knn, init_rows=C.first_rows(c.planted, 3), tol=C.TOL)
    ncomp, comp = C.components(c)
    labels = out.labels.cpu()
    assert ncomp == 3 and out.status.tolist()[0] == 0
    assert sorted(torch.unique(labels).tolist()) == [0, 1, 2]
    for k in torch.unique(comp):
        assert len(torch.unique(labels[comp == k])) == 1
    assert torch.equal(labels, c.planted)  # centre b starts in blob b


def test_large_sparse_checks_and_labels():
    c, (ncomp, _) = _large()
    K, n, extra = 12, c.n, C.eigh_term(c.n)
    assert C.SP.graph_check(c.row_ptr, c.col, c.val) is None
    out = _hip(c, K)
    theta, V, res = out.eigenvalues, out.vectors, out.residuals
    print("large: components", ncomp, "status", out.status.tolist(), "theta", theta.tolist(), "residuals", res.tolist())
    assert out.status.tolist() == [0, out.status.tolist()[1], K, 24]
    at_one = (theta - 1).abs() <= res + extra
    assert int(at_one.sum()) == min(ncomp, K) and bool(at_one[:min(ncomp, K)].all())
    ortho = float((V.T @ V - torch.eye(K, dtype=torch.float64)).abs().max())
    assert ortho <= C.ORTHO_BOUND
    # residuals from a torch sparse fp64 product
    g = C.SP._inv_sqrt(C.SP.csr_degrees(c.row_ptr, c.val))
    r, cc = C.SP._rows_of(c.row_ptr), c.col.long()
    S = torch.sparse_coo_tensor(torch.stack([r, cc]), g[r] * c.val * g[cc], (n, n)).coalesce()
    mine = torch.linalg.norm(torch.sparse.mm(S, V) - V * theta, dim=0)
    print("large: largest recomputed residual", float(mine.max()), "orthonormality", ortho)
    assert bool((mine <= C.TOL + extra).all()) and bool(((mine - res).abs() <= extra).all())
    want = (g[:, None] * V).float()
    want[g == 0] = 0.0
    assert out.embedding.numpy().tobytes() == want.numpy().tobytes()
    RECORDS["large_residual"] = float(mine.max()) / (C.TOL + extra)
    # labels: the HIP pipeline from the features against fp64 k-means on the twin's embedding
    twin = spectral_embedding_torch(c.row_ptr, c.col, c.val, K, tol=1e-12)
    assert twin.status.tolist()[0] == 0
    pipe = spectral_clustering(c.feats.to(DEV), K, knn=c.knn, init_rows=C.first_rows(c.planted, K), tol=C.TOL)
    assert pipe.status.tolist()[0] == 0
    _compare_labels(c, K, pipe.labels, g[:, None] * twin.vectors)


def test_reruns_are_bit_identical_also_beside_another_stream():
    c = C.small_case("blobs-c")
    graph = _graph(c)
    kw = dict(tol=C.TOL, **C.SOLVER[("blobs-c", 56)])
    first = spectral_embedding(*graph, 56, **kw)
    second = spectral_embedding(*graph, 56, **kw)
    side = torch.cuda.Stream()
    a = torch.randn(1024, 1024, device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(20):
            a = torch.tanh(a @ a * 1e-3)
    third = spectral_embedding(*graph, 56, **kw)
    torch.cuda.synchronize()
    assert int(first.status[0]) == 0
    for x, y, z in zip(first, second, third):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() == z.cpu().numpy().tobytes()
    other = spectral_embedding(*graph, 56, seed=1, **kw)
    assert not torch.equal(other.vectors, first.vectors)  # the seed reaches the start block


def test_iteration_cap_returns_the_best_pairs():
    c, o = C.small_case("cycle"), C.oracle("cycle")
    out = _hip(c, 5, max_outer=1)
    assert out.status.tolist()[0] == 1 and out.status.tolist()[1] == 1 and out.status.tolist()[3] == 16
    for t in out:
        assert bool(torch.isfinite(t.double()).all())
    mine = torch.linalg.norm(o.S @ out.vectors - out.vectors * out.eigenvalues, dim=0)
    assert bool(((mine - out.residuals).abs() <= C.eigh_term(c.n)).all())
    assert int(out.status[2]) == int((out.residuals <= C.TOL).sum())
    assert float((out.vectors.T @ out.vectors - torch.eye(5, dtype=torch.float64)).abs().max()) <= C.ORTHO_BOUND


@pytest.mark.parametrize("which", ("negative", "nan", "col"))
def test_bad_input_is_code_2_and_zero_outputs(which):
    c = C.small_case("blobs-a")
    rp, col, val = c.row_ptr.clone(), c.col.clone(), c.val.clone()
    if which == "negative":
        val[100] = -1e-3
    elif which == "nan":
        val[2000] = float("nan")
    else:
        col[int(rp[200]) - 1] = c.n  # the last entry of a row: still ascending
    out = spectral_embedding(rp.to(DEV), col.to(DEV), val.to(DEV), 3)
    assert int(out.status[0].cpu()) == 2 and out.status.tolist()[1:3] == [0, 0]
    for t in (out.eigenvalues, out.embedding, out.vectors, out.residuals):
        assert not bool(t.cpu().any())
    good = spectral_embedding(*_graph(c), 3)  # the next call is not affected
    assert int(good.status[0].cpu()) == 0


def test_feature_bases_wiring():
    c = C.small_case("blobs-b")
    feats = c.feats.to(DEV)
    means = torch.randn(c.n, 3, generator=torch.Generator().manual_seed(0)).to(DEV)
    K = 5
    bases, coefs, labels, centers = init_motion_coefs_from_features(means, feats, K, num_frames=3, cluster="spectral",
                                                                    knn=c.knn)
    sc = spectral_clustering(feats, K, knn=c.knn)
    assert int(sc.status[0].cpu()) == 0
    assert torch.equal(labels, sc.labels)
    med = cluster_medians(means, sc.labels, K)
    assert centers.cpu().numpy().tobytes() == med.cpu().numpy().tobytes()
    want = coefs_from_centers(means.contiguous(), med.contiguous())
    assert coefs.cpu().numpy().tobytes() == want.cpu().numpy().tobytes()
    assert bases.num_frames == 3
    a = init_motion_coefs_from_features(means, feats, K, num_frames=3)
    b = init_motion_coefs_from_features(means, feats, K, num_frames=3, cluster="kmeans")
    for x, y in zip(a[1:], b[1:]):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
