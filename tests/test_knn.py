"""Exact k-NN against a brute-force float64 oracle
(oracle/neighbor.py knn: the reference's o3d_knn contract -- k nearest other
points, squared distances in double, here ties to the lower index) and the
params.npz format of helpers.py:149-167."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from oracle import neighbor as ON


def _cloud(N, kind, seed=0):
    g = np.random.default_rng(seed)
    if kind == "uniform":
        p = g.random((N, 3))
    elif kind == "clusters":  # dense blobs + sparse outliers, like a capture
        c = g.random((8, 3)) * 4
        p = c[g.integers(0, 8, N)] + g.normal(0, 0.02, (N, 3))
        p[: N // 50] = g.random((N // 50, 3)) * 10 - 3
    elif kind == "plane":  # flat (one extent ~0) and grid-aligned: many ties
        p = np.stack([g.integers(0, 40, N) * 0.05, g.integers(0, 40, N) * 0.05, np.zeros(N)], 1)
    else:
        raise ValueError(kind)
    return p.astype(np.float32)


# ------------------------------------------------------------------- CPU

def test_params_npz_roundtrip(tmp_path):
    from dynamic3dgaussians_amd.params_io import load_params, params2cpu, save_params
    t0 = {k: torch.randn(5, c) for k, c in (("means3D", 3), ("rgb_colors", 3), ("unnorm_rotations", 4),
                                             ("log_scales", 3), ("seg_colors", 3))}
    t1 = {k: v + 1 for k, v in t0.items()}
    outs = [params2cpu(t0, True), params2cpu(t1, False)]
    assert set(outs[1]) == {"means3D", "rgb_colors", "unnorm_rotations"}
    path = save_params(outs, "seq", "exp", root=str(tmp_path))
    z = load_params(path)
    assert z["means3D"].shape == (2, 5, 3) and z["log_scales"].shape == (5, 3)
    np.testing.assert_array_equal(z["means3D"][1], t1["means3D"].numpy())
    np.testing.assert_array_equal(z["seg_colors"], t0["seg_colors"].numpy())


# ------------------------------------------------------------------- GPU

@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["uniform", "clusters", "plane"])
@pytest.mark.parametrize("k", [1, 3, 20, 32])
def test_knn_matches_bruteforce(kind, k):
    from dynamic3dgaussians_amd.knn import knn
    p = _cloud(3000, kind, seed=k)
    d, i = knn(torch.from_numpy(p).cuda(), k)
    od, oi = ON.knn(p, k)
    np.testing.assert_array_equal(d.cpu().numpy(), od)  # same double arithmetic, bit-exact
    if kind == "plane":
        # grid ties: the oracle's stable argsort also breaks ties by index
        np.testing.assert_array_equal(i.cpu().numpy(), oi)
    else:
        np.testing.assert_array_equal(i.cpu().numpy(), oi)


@pytest.mark.gpu
def test_knn_large_cloud_sampled_rows():
    """300k points (the bench scale): 256 sampled rows checked against a
    brute-force scan of the whole cloud."""
    from dynamic3dgaussians_amd.knn import knn
    N, k = 300000, 20
    p = _cloud(N, "clusters", seed=7)
    d, i = knn(torch.from_numpy(p).cuda(), k)
    d, i = d.cpu().numpy(), i.cpu().numpy()
    rows = np.random.default_rng(1).choice(N, 256, replace=False)
    P = p.astype(np.float64)
    for r in rows:
        dd = ((P - P[r]) ** 2).sum(-1)
        dd[r] = np.inf
        o = np.argsort(dd, kind="stable")[:k]
        np.testing.assert_array_equal(i[r], o)
        np.testing.assert_array_equal(d[r], dd[o])


@pytest.mark.gpu
def test_knn_edge_cases_and_dropins():
    from dynamic3dgaussians_amd import _lib
    from dynamic3dgaussians_amd.knn import distCUDA2, knn, o3d_knn
    # fewer points than k: tail is (+inf, -1)
    d, i = knn(torch.tensor([[0, 0, 0], [1, 0, 0], [3, 0, 0]], dtype=torch.float32, device="cuda"), 4)
    assert i.cpu().tolist()[0] == [1, 2, -1, -1] and np.isinf(d.cpu().numpy()[0, 2:]).all()
    # duplicates: the point itself is excluded by index, its twin kept at 0
    d, i = knn(torch.tensor([[1, 1, 1], [1, 1, 1], [2, 1, 1]], dtype=torch.float32, device="cuda"), 1)
    assert i.cpu().tolist() == [[1], [0], [0]] and d.cpu().tolist()[0] == [0.0]
    with pytest.raises(_lib.GsplatError):
        knn(torch.zeros(10, 3, device="cuda"), 33)
    # the reference's call shapes
    p = _cloud(2000, "uniform", seed=3)
    sq, idx = o3d_knn(p.astype(np.float64), 3)       # train.py:95
    od, oi = ON.knn(p, 3)
    assert sq.dtype == np.float64 and idx.dtype == np.int64
    np.testing.assert_array_equal(sq, od)
    means, nn = distCUDA2(torch.from_numpy(p).cuda())  # scene/gaussian_model.py:162
    assert means.dtype == torch.float32 and nn.dtype == torch.int32 and nn.shape == (2000, 3)
    np.testing.assert_allclose(means.cpu().numpy(), od.mean(1), rtol=1e-6)
    np.testing.assert_array_equal(nn.cpu().numpy(), oi)


# ---- template boundaries (knn_query_kernel<4 | 8 | 16 | 20 | 32>), the
# 256-point box boundary, N <= K and clouds whose Morton code degenerates

DEV = "cuda"


def _assert_knn_exact(p, k):
    """Bit-exact against the oracle; rows with fewer than k other points end
    in (+inf, -1) after the exact valid prefix."""
    from dynamic3dgaussians_amd.knn import knn
    N = p.shape[0]
    d, i = knn(torch.from_numpy(p).to(DEV), k)
    d, i = d.cpu().numpy(), i.cpu().numpy()
    assert d.shape == (N, k) and i.shape == (N, k) and d.dtype == np.float64 and i.dtype == np.int64
    m = min(k, N - 1)
    od, oi = ON.knn(p, m)
    np.testing.assert_array_equal(d[:, :m], od)
    np.testing.assert_array_equal(i[:, :m], oi)
    assert np.isposinf(d[:, m:]).all() and (i[:, m:] == -1).all()


@pytest.mark.gpu
# N: one box less a point | one full box | two boxes, one point in the second | three boxes
# k: both sides of every template (4|5, 8|9, 16|17, 20|21) and the widest
@pytest.mark.parametrize("N", [255, 256, 257, 513])
@pytest.mark.parametrize("k", [4, 5, 8, 9, 16, 17, 20, 21, 32])
def test_knn_template_and_box_boundaries(N, k):
    _assert_knn_exact(_cloud(N, "clusters", seed=N + k), k)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 2, 9, 20])
@pytest.mark.parametrize("k", [8, 20, 32])  # knn_query_kernel<8 | 20 | 32>: slots >= N - 1 stay (+inf, -1)
def test_knn_fewer_points_than_k(N, k):
    _assert_knn_exact(_cloud(N, "uniform", seed=N + k), k)


def _degenerate(kind, N=600):
    g = np.random.default_rng(11)
    if kind == "identical":  # extent 0 on every axis: every Morton code 0, ties by index across 3 boxes
        p = np.tile(np.array([[0.25, -1.5, 3.0]]), (N, 1))
    elif kind == "half_identical":  # 300 copies of one point + 300 uniform points
        p = g.random((N, 3))
        p[::2] = p[0]
    elif kind == "collinear":  # two zero extents, 40 grid positions: ~15 exact copies of each
        p = np.stack([g.integers(0, 40, N) * 0.05, np.zeros(N), np.zeros(N)], 1)
    elif kind == "offset":  # fp32 spacing at 1e4 is 2^-10: coordinates collapse to 1024 values per axis
        p = g.random((N, 3)) + np.array([1e4, -1e4, 1e4])
    else:
        raise ValueError(kind)
    return p.astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["identical", "half_identical", "collinear", "offset"])
@pytest.mark.parametrize("k", [3, 20])
def test_knn_degenerate_clouds(kind, k):
    _assert_knn_exact(_degenerate(kind), k)


@pytest.mark.gpu
def test_distcuda2_identical_points():
    from dynamic3dgaussians_amd.knn import distCUDA2
    p = _degenerate("identical")
    means, nn = distCUDA2(torch.from_numpy(p).to(DEV))
    assert torch.equal(means, torch.zeros(600, device=DEV))  # mean 0, not NaN
    np.testing.assert_array_equal(nn.cpu().numpy(), ON.knn(p, 3)[1])
