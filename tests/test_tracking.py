"""Point tracking (include/gs_track.h, dynamic3dgaussians_amd/tracking.py), the parts that need
no GPU: the reference replay of the blend chain against the CPU oracle, the host validators
(through ctypes and in a stand-alone sanitizer program), metrics.PCK on hand-computed cases and
the torch fallbacks of select_gaussians, project_tracks and the visibility gather."""
from __future__ import annotations

import ctypes
import os
import re
import shutil

import numpy as np
import pytest
import torch

import dynamic3dgaussians_amd as D
from dynamic3dgaussians_amd import _lib, tracking
from dynamic3dgaussians_amd.camera import camera_rig
from dynamic3dgaussians_amd.rasterizer import GaussianRasterizationSettings
from dynamic3dgaussians_amd.scene import camera_tensors
from tests import _track_ref as R
from tests._harness import run_host_sanitizer

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference replay

@pytest.mark.parametrize("name,cam", [("p2000", 0), ("p2000", 1), ("edges", 0), ("long", 0)])
def test_replay_weights_sum_to_the_oracles_alpha(name, cam):
    """The fp64 replay's weights of a pixel sum to the C oracle's fixed-mode alpha (fp32 chain):
    measured 1.7e-7 .. 4.3e-7 max abs on these scenes; the bound is the issue's 1e-6."""
    top_id, top_w, alpha, count = R.reference(name, cam)
    o = R.oracle(name, cam)
    err = np.abs(alpha - o[4][0].astype(np.float64)).max()
    print(f"{name} cam {cam}: max |sum w - alpha| = {err:.3e}")
    assert err <= 1e-6
    # the replay's own invariants: ranks ordered, ids distinct, -1 exactly where the weight is 0
    assert (np.diff(top_w, axis=0) <= 0).all()
    assert ((top_id == -1) == (top_w[:-1] == 0.0)).all()
    K = top_id.shape[0]
    for a in range(K):
        for b in range(a + 1, K):
            assert not ((top_id[a] == top_id[b]) & (top_id[a] >= 0)).any()
    assert ((count == 0) == (top_id[0] == -1)).all()


def test_near_tie_share_is_under_the_cap():
    """The pixels a rank's comparison excludes for a near tie (1e-3 relative): under 1 % per
    scene, camera and rank (measured 0.09-0.27 %), the condition of the GPU comparison."""
    for name in R.SCENES:
        for cam in range(3):
            top_w = R.reference(name, cam)[1]
            for k in range(4):
                share = 1.0 - R.robust(top_w, k).mean()
                assert share <= 0.01, (name, cam, k, share)


# ---- the C ABI

def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "gs_track.h")).read(), flags=re.S)


def test_library_exports_every_function_of_gs_track_h():
    L = _lib.load()
    names = set(re.findall(r"\b(gs_[a-z_0-9]+)\s*\(", _header()))
    assert names == {"gs_check_contributors", "gs_contributors_batch", "gs_check_track_project", "gs_track_project"}
    for n in names:
        assert hasattr(L, n) and n in _lib.PROTOTYPES, n
    assert re.search(r"#define GS_TRACK_MAX_K 4\b", _header()) and _lib.GS_TRACK_MAX_K == 4
    assert _lib.load().gs_version() == _lib.ABI_VERSION == 13  # a new header, no existing struct changed


def _buf(n):
    return (ctypes.c_float * max(n, 1))()


@pytest.mark.parametrize("args,msg", [
    ((2000, 1, 128, 96, 0), b"K = 0 outside 1..4"),
    ((2000, 1, 128, 96, 5), b"K = 5 outside 1..4"),
    ((2000, 0, 128, 96, 1), b"camera batch size 0 outside 1..64"),
    ((2000, 65, 128, 96, 1), b"camera batch size 65 outside 1..64"),
    ((-1, 1, 128, 96, 1), b"P must be in [0, 2^31)"),
    ((1 << 31, 1, 128, 96, 1), b"P must be in [0, 2^31)"),
    ((2000, 1, -1, 96, 1), b"image size must not be negative"),
    ((2000, 1, 128, -96, 1), b"image size must not be negative"),
    ((2000, 64, 2 ** 31 - 1, 2 ** 31 - 1, 4), b"exceed 2^62"),
])
def test_check_contributors_refuses(args, msg):
    L = _lib.load()
    ids, w = _buf(16), _buf(16)
    assert L.gs_check_contributors(*args, ids, w) != 0
    assert msg in L.gs_last_error(), L.gs_last_error()


def test_check_contributors_outputs():
    L = _lib.load()
    ids, w = _buf(16), _buf(16)
    assert L.gs_check_contributors(10, 1, 2, 2, 4, ids, w) == 0
    assert L.gs_check_contributors(0, 3, 2, 2, 1, ids, w) == 0                 # P = 0 is a valid call
    assert L.gs_check_contributors(10, 1, 0, 2, 4, None, None) == 0            # nothing to write
    assert L.gs_check_contributors(10, 1, 2, 2, 4, None, w) != 0 and b"are required" in L.gs_last_error()
    assert L.gs_check_contributors(10, 1, 2, 2, 4, ids, None) != 0 and b"are required" in L.gs_last_error()
    odd = ctypes.c_void_p(ctypes.addressof(w) + 2)
    assert L.gs_check_contributors(10, 1, 2, 2, 4, ids, odd) != 0 and b"4-byte aligned" in L.gs_last_error()


@pytest.mark.parametrize("args,msg", [
    ((2000, -1, 3, 17), b"T must not be negative"),
    ((2000, 3, 3, -1), b"N must not be negative"),
    ((2000, 3, 0, 17), b"camera batch size 0 outside 1..64"),
    ((2000, 3, 65, 17), b"camera batch size 65 outside 1..64"),
    ((-1, 3, 3, 17), b"P must be in [0, 2^31)"),
    ((2000, 2 ** 31 - 1, 64, 1 << 40), b"exceed 2^62"),
])
def test_check_track_project_refuses(args, msg):
    L = _lib.load()
    ids, uv, d, ins = _buf(64), _buf(128), _buf(64), _buf(64)
    assert L.gs_check_track_project(*args, ids, uv, d, ins) != 0
    assert msg in L.gs_last_error(), L.gs_last_error()


def test_check_track_project_outputs():
    L = _lib.load()
    ids, uv, d, ins = _buf(4), _buf(10), _buf(4), _buf(4)
    assert L.gs_check_track_project(10, 1, 1, 4, ids, uv, d, ins) == 0
    assert L.gs_check_track_project(10, 0, 1, 4, None, None, None, None) == 0  # nothing to write
    for bad, msg in (((None, uv, d, ins), b"ids are required"), ((ids, None, d, ins), b"are required"),
                     ((ids, uv, None, ins), b"are required"), ((ids, uv, d, None), b"are required")):
        assert L.gs_check_track_project(10, 1, 1, 4, *bad) != 0 and msg in L.gs_last_error()
    a = ctypes.addressof(uv)
    odd8 = ctypes.c_void_p(a + 4 if a % 8 == 0 else a)
    assert L.gs_check_track_project(10, 1, 1, 4, ids, odd8, d, ins) != 0 and b"8-byte aligned" in L.gs_last_error()


def test_entry_points_run_the_validators_first():
    """A bad K / camera count is refused by the entry points with the validator's message before
    any buffer or the device is looked at."""
    L = _lib.load()
    cams = (_lib.GsCamera * 1)()
    cams[0].image_width, cams[0].image_height = 128, 96
    assert L.gs_contributors_batch(cams, 1, 2000, 1, None, None, None, None, 7, None, None, None) != 0
    assert b"K = 7 outside 1..4" in L.gs_last_error()
    assert L.gs_contributors_batch(cams, 1, 2000, 5, None, None, None, None, 1, None, None, None) != 0
    assert b"unknown compat 5" in L.gs_last_error()
    assert L.gs_track_project(cams, 99, 2000, 1, None, None, 3, None, None, None, None) != 0
    assert b"camera batch size 99 outside 1..64" in L.gs_last_error()


@pytest.mark.skipif(shutil.which("gcc") is None or shutil.which("g++") is None, reason="gcc / g++ not available")
def test_validators_are_sanitizer_clean(tmp_path):
    """gs_track_host.cpp (with gs_host.cpp's error state) under ASan + UBSan in a plain CPU
    executable with its own main: nothing preloaded, nothing loaded into Python."""
    run_host_sanitizer(tmp_path, "track_host_sanitize.c", ["gs_track_host.cpp", "gs_host.cpp"],
                       "track host sanitize ok")


# ---- PCK

def test_pck_hand_computed():
    pck = D.PCK()
    targets = torch.tensor([[0.0, 0.0], [10.0, 10.0], [5.0, 5.0], [1.0, 1.0]])
    preds = torch.tensor([[0.3, 0.4],     # distance 0.5: exactly at the threshold, not counted (strict <)
                          [10.0, 10.25],  # 0.25
                          [8.0, 9.0],     # 5
                          [1.0, 1.0]])    # 0
    pck.update(preds, targets, 0.5)
    assert len(pck) == 1 and pck.compute() == pytest.approx(2 / 4, abs=0)
    pck.update(preds, targets, 0.5000001)  # just over: the first point counts
    assert pck.compute() == pytest.approx((2 / 4 + 3 / 4) / 2, abs=1e-15)
    pck.update(preds, targets, 6.0)  # the mean of per-update ratios (the reference's final line)
    assert pck.compute() == pytest.approx((0.5 + 0.75 + 1.0) / 3, abs=1e-15)


def test_pck_empty_update_and_visible_mask():
    pck = D.PCK()
    with pytest.raises(D.metrics.GsplatError):
        pck.compute()
    pck.update(torch.zeros(0, 2), torch.zeros(0, 2), 1.0)  # 0 / max(0, 1e-8) = 0, as the reference
    assert pck.compute() == 0.0
    targets = torch.tensor([[0.0, 0.0], [10.0, 10.0], [5.0, 5.0]])
    preds = torch.tensor([[0.1, 0.0], [20.0, 10.0], [5.0, 5.2]])
    vis = torch.tensor([True, True, False])
    p2 = D.PCK()
    p2.update(preds, targets, 0.5, visible=vis)  # the visible targets: one of two correct
    assert p2.compute() == 0.5
    p3 = D.PCK()
    p3.update(preds[vis], targets[vis], 0.5)  # what the reference's callers do
    assert p3.compute() == p2.compute()
    p2.update(preds, targets, 0.5, visible=torch.zeros(3, dtype=torch.bool))  # nothing visible: 0
    assert p2.compute() == 0.25
    with pytest.raises(D.metrics.GsplatError):
        p2.update(preds, targets[:2], 0.5)
    with pytest.raises(D.metrics.GsplatError):
        p2.update(preds, targets, 0.5, visible=vis[:2])


# ---- the torch fallbacks

def _settings(cams, device="cpu"):
    return [GaussianRasterizationSettings(**camera_tensors(c, device), compat="fixed") for c in cams]


def test_select_gaussians_cpu():
    rng = np.random.default_rng(0)
    C, K, H_, W = 2, 3, 7, 9
    top = rng.integers(-1, 50, size=(C, K, H_, W)).astype(np.int32)
    xy = np.array([[0.0, 0.0], [8.49, 6.49], [8.5, 3.0], [-0.5, 2.0], [-0.51, 2.0], [3.4, 6.5], [4.5, 2.5],
                   [2.2, -3.0]], np.float32)
    cam = np.array([0, 1, 1, 0, 0, 1, 0, 1])
    for rank in range(K):
        got = D.select_gaussians(torch.from_numpy(top), torch.from_numpy(xy), torch.from_numpy(cam), rank).numpy()
        px, py = np.floor(xy[:, 0] + 0.5).astype(int), np.floor(xy[:, 1] + 0.5).astype(int)
        want = np.array([top[c, rank, y, x] if 0 <= x < W and 0 <= y < H_ else -1 for c, x, y in zip(cam, px, py)])
        np.testing.assert_array_equal(got, want)
    assert px[2] == W and px[3] == 0 and px[4] == -1  # x = 8.5 rounds out, x = -0.5 rounds in, -0.51 out
    one =D.select_gaussians(torch.from_numpy(top), torch.from_numpy(xy), 1)
    np.testing.assert_array_equal(one.numpy(), [top[1, 0, y, x] if 0 <= x < W and 0 <= y < H_ else -1
                                                for x, y in zip(px, py)])
    with pytest.raises(ValueError):
        D.select_gaussians(torch.from_numpy(top), torch.from_numpy(xy), 2)
    with pytest.raises(ValueError):
        D.select_gaussians(torch.from_numpy(top), torch.from_numpy(xy), 0, rank=3)


def test_project_tracks_cpu_matches_the_oracle():
    """The torch statement of the projection kernel gives the oracle's means2D / depths for every
    Gaussian the oracle projects (radii > 0): the same fp32 operations in the same order, so
    bit for bit."""
    name = "p2000"
    kw = R.SCENES[name]
    cams = camera_rig(27, kw["W"], kw["H"])[:3]
    means = R.scene(name)["means3D"]
    ids = torch.arange(means.shape[0])
    uv, depth, inside = D.project_tracks(means[None], ids, _settings(cams))
    assert uv.shape == (1, 3, means.shape[0], 2) and depth.shape == inside.shape == (1, 3, means.shape[0])
    for c in range(3):
        o = R.oracle(name, c)
        st, vis = o[6], o[5] > 0
        assert vis.sum() > 1000
        np.testing.assert_array_equal(uv[0, c].numpy()[vis], st.means2D[vis])
        np.testing.assert_array_equal(depth[0, c].numpy()[vis], st.depths[vis])
        # inside, against a direct evaluation
        u, v = uv[0, c].numpy().astype(np.float64).T
        z = depth[0, c].numpy()
        want = (z > 0) & (np.floor(u + 0.5) >= 0) & (np.floor(u + 0.5) < kw["W"]) & (np.floor(v + 0.5) >= 0) & \
            (np.floor(v + 0.5) < kw["H"])
        np.testing.assert_array_equal(inside[0, c].numpy(), want)


def test_project_tracks_cpu_ids_and_timesteps():
    kw = R.SCENES["p2000"]
    cams = camera_rig(27, kw["W"], kw["H"])[:2]
    means = R.scene("p2000")["means3D"][:50]
    seq = torch.stack([means, means + torch.tensor([0.05, 0.0, 0.0]), means * 8.0])  # the last: some behind the rig
    ids = torch.tensor([3, -1, 49, 0])
    uv, depth, inside = D.project_tracks(seq, ids, _settings(cams))
    assert uv.shape == (3, 2, 4, 2)
    assert (uv[:, :, 1] == 0).all() and (depth[:, :, 1] == 0).all() and not inside[:, :, 1].any()
    full = D.project_tracks(seq, torch.arange(50), _settings(cams))
    for n, i in enumerate(ids.tolist()):
        if i >= 0:
            assert torch.equal(uv[:, :, n], full[0][:, :, i]) and torch.equal(depth[:, :, n], full[1][:, :, i])
            assert torch.equal(inside[:, :, n], full[2][:, :, i])
    # a point behind a camera is never inside
    behind = full[1] <= 0
    assert behind.any() and not full[2][behind].any()
    with pytest.raises(ValueError):
        D.project_tracks(seq, torch.tensor([50]), _settings(cams))
    with pytest.raises(ValueError):
        D.project_tracks(seq[0], ids, _settings(cams))


def test_visibility_gather_cpu():
    rng = np.random.default_rng(1)
    C, K, H_, W, N = 2, 2, 6, 8, 40
    top = rng.integers(-1, 6, size=(C, K, H_, W)).astype(np.int32)
    ids = rng.integers(-1, 6, size=N)
    uv = rng.uniform(-1.0, 9.0, size=(C, N, 2)).astype(np.float32)
    px, py = np.floor(uv[..., 0] + 0.5).astype(int), np.floor(uv[..., 1] + 0.5).astype(int)
    inside = (px >= 0) & (px < W) & (py >= 0) & (py < H_)
    got = tracking.visible_in_maps(torch.from_numpy(top), torch.from_numpy(ids), torch.from_numpy(uv),
                                   torch.from_numpy(inside)).numpy()
    want = np.zeros((C, N), bool)
    for c in range(C):
        for n in range(N):
            want[c, n] = inside[c, n] and ids[n] >= 0 and ids[n] in top[c, :, py[c, n], px[c, n]]
    np.testing.assert_array_equal(got, want)
    assert want.any() and not want.all()


def test_track_points_reads_the_three_forms_of_a_sequence(tmp_path):
    """A list of per-timestep params, the dict params_io reads back and a callable give the same
    rendervars per timestep."""
    from dynamic3dgaussians_amd import params_io
    from dynamic3dgaussians_amd.timesteps import params2rendervar
    g = torch.Generator().manual_seed(0)
    T, P = 3, 5
    first = dict(means3D=torch.randn(P, 3, generator=g), rgb_colors=torch.rand(P, 3, generator=g),
                 unnorm_rotations=torch.randn(P, 4, generator=g), logit_opacities=torch.randn(P, 1, generator=g),
                 log_scales=torch.randn(P, 3, generator=g))
    seq = [dict(first, means3D=first["means3D"] + 0.1 * t, unnorm_rotations=first["unnorm_rotations"] * (1 + t))
           for t in range(T)]
    path = params_io.save_params([params_io.params2cpu(p, t == 0) for t, p in enumerate(seq)], "seq", "exp",
                                 root=str(tmp_path))
    forms = [tracking._rendervars(seq, None, "cpu"), tracking._rendervars(params_io.load_params(path), None, "cpu"),
             tracking._rendervars(lambda t: params2rendervar(seq[t]), T, "cpu")]
    assert [f[1] for f in forms] == [T, T, T]
    for t in range(T):
        rvs = [f[0](t) for f in forms]
        for k in ("means3D", "colors_precomp", "rotations", "opacities", "scales"):
            assert rvs[0][k].shape[0] == P
            assert torch.equal(rvs[0][k], rvs[1][k]) and torch.equal(rvs[0][k], rvs[2][k]), (t, k)
    with pytest.raises(ValueError):
        tracking._rendervars(lambda t: seq[t], None, "cpu")  # a callable needs num_timesteps


def test_public_names():
    for name in ("contributor_maps", "select_gaussians", "project_tracks", "track_points", "PCK", "Tracks"):
        assert hasattr(D, name), name
    from dynamic3dgaussians_amd import _C
    assert callable(_C.rasterize_gaussians_batch_contributors) and callable(_C.track_project)
    from dynamic3dgaussians_amd import build
    assert "gs_track.hip" in build.SOURCES and "gs_track_host.cpp" in build.SOURCES
    with pytest.raises(D.metrics.GsplatError):  # no CPU rasterizer: contributor_maps needs the device
        D.contributor_maps(_settings(camera_rig(1, 32, 32)), {"means3D": torch.zeros(1, 3)})
    with pytest.raises(ValueError):
        D.contributor_maps(_settings(camera_rig(1, 32, 32)), {"means3D": torch.zeros(1, 3)}, K=5)
