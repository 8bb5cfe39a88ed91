"""The spectral embedding (include/gs_spectral.h) without a GPU: the torch twin against the dense
oracle on every small case (tests/_spectral_cases.py) with the device tests' bounds, the graph
helpers, the argument checks, the host validator and the host build of the small problems under
the sanitizers."""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from dynamic3dgaussians_amd import (_lib, build, feature_knn_torch, graph_check, init_motion_coefs_from_features,
                                    knn_affinity, knn_graph, spectral, spectral_clustering, spectral_clustering_graph,
                                    spectral_embedding, spectral_embedding_dense, spectral_embedding_torch)
from dynamic3dgaussians_amd._lib import GsplatError
from tests import _spectral_cases as C
from tests._harness import run_host_sanitizer

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _twin(name, K, **kw):
    c = C.small_case(name)
    kw = {**C.SOLVER.get((name, K), {}), **kw}
    return spectral_embedding_torch(c.row_ptr, c.col, c.val, K, tol=C.TOL, **kw)


@pytest.mark.parametrize("name,K", C.SMALL)
def test_twin_against_the_dense_oracle(name, K):
    out = _twin(name, K)
    C.check_against_oracle(name, K, out)
    C.check_known_answers(name, K, out)


def test_cases_are_what_the_table_says():
    assert C.small_case("cycle").n == 64 and C.small_case("blobs-a").n == 257 and C.small_case("blobs-b").n == 1000
    assert C.small_case("blobs-c").n == 1500 and C.small_case("star").n == 320 and C.small_case("tiny").n == 10
    hub = C.small_case("star").row_ptr
    assert int(hub[1] - hub[0]) == 299 and int((hub[1:] == hub[:-1]).sum()) == 20
    for name, _ in C.SMALL:
        c = C.small_case(name)
        assert graph_check(c.row_ptr, c.col, c.val) is None, name
    for name, K in C.GAPPED:  # asserted in the builder, so a projector check is never skipped silently
        o = C.oracle(name)
        assert float(o.lam[K - 1] - o.lam[K]) >= 1e-3


def test_dense_oracle_is_the_definition_and_refuses_large_graphs():
    c = C.small_case("tiny")
    out = spectral_embedding_dense(c.row_ptr, c.col, c.val, 3)
    # the path's normalised affinity by hand
    A = np.zeros((10, 10))
    for i in range(9):
        A[i, i + 1] = A[i + 1, i] = 1.0
    g = 1 / np.sqrt(A.sum(1))
    lam = np.linalg.eigvalsh(g[:, None] * A * g[None, :])[::-1]
    assert np.abs(out.eigenvalues.numpy() - lam[:3]).max() <= 64 * 10 * C.EPS
    assert float(out.residuals.max()) <= 64 * 10 * C.EPS and out.status.tolist() == [0, 0, 3, 10]
    n = spectral.DENSE_MAX_N + 1
    with pytest.raises(GsplatError, match="n <= 8192"):
        spectral_embedding_dense(torch.zeros(n + 1, dtype=torch.int64), torch.zeros(0, dtype=torch.int32),
                                 torch.zeros(0, dtype=torch.float64), 2)


def test_row_normalize_and_the_iteration_cap_in_the_twin():
    c = C.small_case("star")
    out = spectral_embedding_torch(c.row_ptr, c.col, c.val, 2, tol=C.TOL, row_normalize=True)
    g = C.oracle("star").g
    norms = out.embedding.double().norm(dim=1)
    assert bool(((norms[g > 0] - 1).abs() <= 2.0 ** -23).all()) and not out.embedding[g == 0].any()
    c = C.small_case("cycle")
    out = spectral_embedding_torch(c.row_ptr, c.col, c.val, 5, tol=C.TOL, max_outer=1)
    assert out.status.tolist()[:2] == [1, 1] and out.status.tolist()[3] == 16
    R = C.oracle("cycle").S @ out.vectors - out.vectors * out.eigenvalues
    assert float((torch.linalg.norm(R, dim=0) - out.residuals).abs().max()) <= C.eigh_term(64)
    assert float((out.vectors.T @ out.vectors - torch.eye(5, dtype=torch.float64)).abs().max()) <= C.ORTHO_BOUND


@pytest.mark.parametrize("which", ("negative", "nan", "col", "row_ptr"))
def test_twin_bad_input_is_code_2_and_zeros(which):
    c = C.small_case("cycle")
    rp, col, val = c.row_ptr.clone(), c.col.clone(), c.val.clone()
    if which == "negative":
        val[7] = -1.0
    elif which == "nan":
        val[9] = float("nan")
    elif which == "col":
        col[11] = c.n
    else:
        rp[5] = rp[6] + 1
    for out in (spectral_embedding_torch(rp, col, val, 5), spectral_embedding_dense(rp, col, val, 5)):
        assert int(out.status[0]) == 2
        assert not out.eigenvalues.any() and not out.vectors.any() and not out.embedding.any() and not out.residuals.any()
    assert graph_check(rp, col, val) is not None


def test_start_block_is_the_stated_counter_function():
    def mix(z):
        z &= (1 << 64) - 1
        z ^= z >> 30
        z = z * 0xBF58476D1CE4E5B9 & ((1 << 64) - 1)
        z ^= z >> 27
        z = z * 0x94D049BB133111EB & ((1 << 64) - 1)
        return z ^ (z >> 31)

    for seed, epoch in ((0, 0), (12345, 3), ((1 << 64) - 1, 7)):
        x = spectral.start_block(seed, epoch, 40, range(16))
        for i, j in ((0, 0), (39, 15), (17, 4)):
            h = mix(mix(seed + (epoch + 1) * 0x9E3779B97F4A7C15) ^ (i * 128 + j))
            assert float(x[i, j]) == ((h >> 12) + 0.5) * 2.0 ** -51 - 1.0
        assert bool(((x > -1) & (x < 1) & (x != 0)).all()) and abs(float(x.mean())) < 0.2
    assert not torch.equal(spectral.start_block(0, 0, 8, range(4)), spectral.start_block(0, 1, 8, range(4)))
    assert torch.equal(spectral.start_block(5, 2, 8, [3]), spectral.start_block(5, 2, 8, range(4))[:, 3:])


def test_cheb_step_is_the_scaled_three_term_recurrence():
    # p_m(x) = T_m((x - c) / e) / T_m((a0 - c) / e): 1 at theta_1, at most 1 / T_m(..) on [-1, theta_B]
    th1, thb, m = 0.99, 0.6, 8
    x = torch.linspace(-1, 1, 401, dtype=torch.float64)
    y, z = x.clone().fill_(1.0), None
    for s in range(1, m + 1):
        al, be, ga = spectral.cheb_step(th1, thb, s)
        yn = al * x * y + be * y + (ga * z if z is not None else 0)
        y, z = yn, y
    e, c = (thb + 1) / 2, (thb - 1) / 2
    T = lambda u: np.cosh(m * np.arccosh(u)) if u >= 1 else np.cos(m * np.arccos(u))  # noqa: E731
    want = torch.tensor([T((float(v) - c) / e) / T((th1 - c) / e) for v in x], dtype=torch.float64)
    assert float((y - want).abs().max()) <= 1e-12
    assert float(y[x <= thb].abs().max()) <= 1 / T((th1 - c) / e) + 1e-12
    # a degenerate interval stays finite
    for s in range(1, 9):
        assert all(np.isfinite(v) for v in spectral.cheb_step(-1.0, -1.0, s))
        assert all(np.isfinite(v) for v in spectral.cheb_step(1.0, 1.0, s))


def test_knn_graph_against_the_dense_affinity():
    x, _ = C.blob_features(4, 0.6, 60, 8, 3)
    sim, index = feature_knn_torch(x, 5)
    for transform, w in (("clamp", sim.clamp_min(0)), ("shift", (1 + sim) / 2)):
        rp, col, val = knn_graph(sim, index, 60, transform=transform)
        assert rp.dtype == torch.int64 and col.dtype == torch.int32 and val.dtype == torch.float64
        dense = torch.zeros(60, 60, dtype=torch.float64)
        r = torch.repeat_interleave(torch.arange(60), rp[1:] - rp[:-1])
        dense[r, col.long()] = val
        want = knn_affinity(w, index, 60).to_dense()
        assert torch.equal(dense, want) and torch.equal(dense, dense.T)
        assert graph_check(rp, col, val) is None
        assert int(rp[-1]) == col.numel() == knn_affinity(w, index, 60)._nnz()
    with pytest.raises(ValueError, match="transform"):
        knn_graph(sim, index, 60, transform="exp")


def test_graph_check_names_each_violation():
    c = C.small_case("cycle")
    assert graph_check(c.row_ptr, c.col, c.val) is None
    rp, col, val = c.row_ptr.clone(), c.col.clone(), c.val.clone()
    col[0], col[1] = c.col[1], c.col[0]
    assert "not ascending" in graph_check(rp, col, val)
    col = c.col.clone()
    col[3] = 64
    assert "out of range" in graph_check(rp, col, val)
    val[5] = -0.5
    assert "negative or not finite" in graph_check(rp, c.col, val)
    val = c.val.clone()
    val[2] = 2.0
    assert "not symmetric" in graph_check(rp, c.col, val)
    rp[10] = rp[11] + 1
    assert "row_ptr must rise" in graph_check(rp, c.col, c.val)
    one_way = C.csr_from_edges(3, [0], [1], [1.0])
    assert "not symmetric" in graph_check(*one_way)
    with pytest.raises(GsplatError, match="col must be int32"):
        graph_check(c.row_ptr, c.col.long(), c.val)


def test_argument_refusals():
    c = C.small_case("cycle")
    g = (c.row_ptr, c.col, c.val)
    t = C.small_case("tiny")
    for fn in (spectral_embedding, spectral_embedding_torch):
        with pytest.raises(GsplatError, match="num_vectors must be in"):
            fn(*g, 0)
        with pytest.raises(GsplatError, match="at least num_vectors"):
            fn(t.row_ptr, t.col, t.val, 11)
        with pytest.raises(GsplatError, match="degree must be in"):
            fn(*g, 2, degree=0)
        with pytest.raises(GsplatError, match="degree must be in"):
            fn(*g, 2, degree=65)
        with pytest.raises(GsplatError, match="max_outer must be in"):
            fn(*g, 2, max_outer=1001)
        with pytest.raises(GsplatError, match="tol must be positive"):
            fn(*g, 2, tol=0.0)
        with pytest.raises(GsplatError, match="seed must be in"):
            fn(*g, 2, seed=-1)
        with pytest.raises(GsplatError, match="row_ptr must be int64"):
            fn(c.row_ptr.int(), c.col, c.val, 2)
        with pytest.raises(GsplatError, match="col must be int32"):
            fn(c.row_ptr, c.col.long(), c.val, 2)
        with pytest.raises(GsplatError, match="val must be a floating-point tensor of col's shape"):
            fn(c.row_ptr, c.col, c.val[:-1], 2)
    # host tensors take the twin: the same result as calling it
    a, b = spectral_embedding(*g, 5, tol=C.TOL), spectral_embedding_torch(*g, 5, tol=C.TOL)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    # the twin takes a K the kernels refuse
    big = C.small_case("blobs-b")
    out = spectral_embedding_torch(big.row_ptr, big.col, big.val, 65, max_outer=1)
    assert tuple(out.vectors.shape) == (1000, 65) and int(out.status[3]) == 80
    with pytest.raises(ValueError, match="init_rows must hold"):
        spectral_clustering_graph(*g, 3, init_rows=[0, 1])
    with pytest.raises(ValueError, match="cluster must be"):
        init_motion_coefs_from_features(torch.zeros(4, 3), torch.zeros(4, 8), 2, num_frames=1, cluster="dbscan")


def test_clustering_on_the_cpu_path_recovers_the_components_and_the_blobs():
    c = C.small_case("blobs-a")
    out = spectral_clustering(c.feats, 3, knn=c.knn, init_rows=C.first_rows(c.planted, 3), tol=C.TOL)
    assert out.status.tolist()[0] == 0 and out.labels.dtype == torch.int64
    assert torch.equal(out.labels, c.planted)  # the three components are the three blobs, in order
    ncomp, comp = C.components(c)
    assert ncomp == 3 and all(len(torch.unique(out.labels[comp == k])) == 1 for k in torch.unique(comp))
    # cluster="spectral" is the same labels, and the default is untouched by the new arguments
    means = torch.from_numpy(np.random.default_rng(0).standard_normal((c.n, 3)).astype(np.float32))
    _, coefs, labels, centers = init_motion_coefs_from_features(means, c.feats, 3, num_frames=2, cluster="spectral",
                                                                knn=c.knn)
    assert torch.equal(labels, spectral_clustering(c.feats, 3, knn=c.knn).labels)
    a = init_motion_coefs_from_features(means, c.feats, 3, num_frames=2)
    b = init_motion_coefs_from_features(means, c.feats, 3, num_frames=2, cluster="kmeans")
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])


def test_build_lists_the_new_sources_and_the_mirror_matches():
    assert build.SOURCES["gs_spectral.hip"] == ["-ffp-contract=off"]
    assert "gs_spectral_host.cpp" in build.SOURCES
    for f in ("gs_spectral.hip", "gs_spectral_host.cpp", "gs_spectral_layout.h", "gs_spectral_small.h"):
        assert os.path.exists(os.path.join(build.CSRC, f))
    L = _lib.load()
    assert ctypes.sizeof(_lib.GsSpectral) == L.gs_spectral_struct_bytes()
    assert L.gs_version() == 13
    with open(os.path.join(REPO, "include", "gsplat_hip.h")) as fh:
        assert "#define GS_ABI_VERSION 13\n" in fh.read()
    with open(os.path.join(REPO, "include", "gs_spectral.h")) as fh:
        header = fh.read()
    for name, value in (("GS_SPECTRAL_MAX_K", _lib.SPECTRAL_MAX_K), ("GS_SPECTRAL_MAX_N", "(1 << 26)"),
                        ("GS_SPECTRAL_MAX_DEGREE", _lib.SPECTRAL_MAX_DEGREE),
                        ("GS_SPECTRAL_MAX_OUTER", _lib.SPECTRAL_MAX_OUTER), ("GS_SPECTRAL_GUARD", _lib.SPECTRAL_GUARD),
                        ("GS_SPECTRAL_MAX_B", _lib.SPECTRAL_MAX_B)):
        assert f"#define {name} {value}\n" in header or f"#define {name} {value} " in header, name
    assert _lib.SPECTRAL_MAX_N == 1 << 26


def test_block_width_tiers():
    L = _lib.load()
    assert [L.gs_spectral_block_width(1500, K) for K in (1, 8, 9, 56, 64)] == [16, 16, 24, 64, 72]
    assert [spectral.block_width(1500, K) for K in (1, 8, 9, 56, 64)] == [16, 16, 24, 64, 72]
    assert L.gs_spectral_block_width(10, 3) == 10 and L.gs_spectral_block_width(1, 1) == 1
    assert L.gs_spectral_block_width(12, 12) == 12 and L.gs_spectral_block_width(20, 9) == 20
    for bad in ((5, 0), (5, 65), (3, 4), ((1 << 26) + 1, 2)):
        assert L.gs_spectral_block_width(*bad) == 0
    ws = L.gs_spectral_workspace_bytes
    assert ws(1500, 27000, 9) >= 4 * 1500 * 24 * 8 and ws(1500, 27000, 64) > ws(1500, 27000, 56) > ws(1500, 27000, 9)
    assert ws(300_000, 9_000_000, 49) < 1 << 30  # 300k Gaussians, K = 49: under a gigabyte
    assert ws(1500, 1 << 31, 9) == 0 and ws(1500, -1, 9) == 0 and ws(8, 10, 9) == 0 and ws(1500, 10, 65) == 0


def _block(**kw):
    buf = ctypes.create_string_buffer(4096)
    base = ctypes.addressof(buf) // 16 * 16 + 16
    a = _lib.GsSpectral(n=1500, num_vectors=9, nnz=27000, degree=8, max_outer=30, row_normalize=0, seed=0, tol=1e-8,
                        row_ptr=base, col=base, val=base, eigenvalues=base, vectors=base, embedding=base,
                        residuals=base, status=base, workspace=base, workspace_bytes=1 << 40)
    for name, v in kw.items():
        setattr(a, name, v)
    a._keep = buf
    return a


@pytest.mark.parametrize("field,value,message", [
    ("num_vectors", 0, "num_vectors must be in [1, 64]"), ("num_vectors", 65, "spectral_embedding_torch"),
    ("n", 8, "n must be in [num_vectors, 67108864]"), ("n", (1 << 26) + 1, "n must be in"),
    ("nnz", -1, "nnz must be in [0, 2^31)"), ("nnz", 1 << 31, "nnz must be in [0, 2^31)"),
    ("degree", 0, "degree must be in [1, 64]"), ("degree", 65, "degree must be in [1, 64]"),
    ("max_outer", 0, "max_outer must be in [1, 1000]"), ("max_outer", 1001, "max_outer must be in [1, 1000]"),
    ("tol", 0.0, "tol must be positive"), ("tol", float("nan"), "tol must be positive"),
    ("row_normalize", 2, "row_normalize must be 0 or 1"), ("row_ptr", None, "row_ptr is required"),
    ("col", None, "col and val are required"), ("vectors", None, "are required"),
    ("workspace", None, "workspace is required"), ("workspace_bytes", 64, "needed"),
])
def test_validator_refuses_with_a_message_that_names_the_limit(field, value, message):
    L = _lib.load()
    assert L.gs_spectral_validate(ctypes.byref(_block())) == 0
    assert L.gs_spectral_validate(ctypes.byref(_block(nnz=0, col=None, val=None))) == 0
    assert L.gs_spectral_validate(ctypes.byref(_block(**{field: value}))) != 0
    assert message in L.gs_last_error().decode()
    assert L.gs_spectral_validate(None) != 0 and "null argument block" in L.gs_last_error().decode()


def test_header_parses_as_c(tmp_path):
    src = tmp_path / "h.c"
    src.write_text('#include "gs_spectral.h"\nint main(void) { return (int)sizeof(gs_spectral_args) == 0; }\n')
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", "-I",
                    os.path.join(REPO, "include"), str(src)], check=True, capture_output=True, timeout=120)


def test_small_problems_on_the_host_match_eigh():
    """gs_spectral_small.h through the library's host entries, against torch.linalg.eigh."""
    L = _lib.load()
    rng = np.random.default_rng(5)
    for B in (1, 2, 7, 24, 72):
        X = rng.standard_normal((B + 30, B))
        X[:, B // 2] *= 1e-4
        G = np.ascontiguousarray(X.T @ X)
        T, rep = np.zeros((B, B)), np.zeros(B, np.int32)
        assert L.gs_spectral_svqb_host(B, G.ctypes.data, T.ctypes.data, rep.ctypes.data) == 0
        Y = X @ T
        assert not rep.any() and np.abs(Y.T @ Y - np.eye(B)).max() <= 1e-10
        H = rng.standard_normal((B, B))
        H = np.ascontiguousarray(np.triu(H) + np.triu(H, 1).T)
        theta, Q = np.zeros(B), np.zeros((B, B))
        assert L.gs_spectral_ritz_host(B, H.ctypes.data, theta.ctypes.data, Q.ctypes.data) == 0
        lam = np.linalg.eigvalsh(H)[::-1]
        scale = max(1.0, np.abs(lam).max())
        assert np.abs(theta - lam).max() <= 64 * B * C.EPS * scale
        assert np.abs(H @ Q - Q * theta).max() <= 64 * B * C.EPS * scale and np.abs(Q.T @ Q - np.eye(B)).max() <= 64 * B * C.EPS


def test_host_code_is_sanitizer_clean(tmp_path):
    """gs_spectral_host.cpp (the validator, the size functions and the host build of the small
    problems on a 24 x 24 case; with gs_host.cpp's error state) under ASan + UBSan in a plain CPU
    executable with its own main: nothing preloaded, nothing loaded into Python."""
    run_host_sanitizer(tmp_path, "spectral_host_sanitize.c", ["gs_spectral_host.cpp", "gs_host.cpp"],
                       "spectral host sanitize ok")
