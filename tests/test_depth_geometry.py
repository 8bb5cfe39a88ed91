"""CPU tests of the depth-map geometry (no GPU needed):
  * the _torch twins in fp64 reproduce what the reference's own code recorded in
    tests/golden/depth_geometry.npz (tests/golden/make_golden_depth_geometry.py):
    unproject_image's estimated depth maps and scores, compute_optical_flow, warp_flow,
    accumulate_flows, resize_optical_flow and depth2point_world;
  * the library exports every symbol include/gs_depth_geometry.h declares, each with a ctypes
    prototype, the ctypes mirrors have the library's sizes and the header's fields, and the ABI
    is still 13;
  * every host validator refuses each kind of bad argument with a message;
  * the wrappers refuse what the kernels cannot take (no CPU fallback);
  * the validators run clean under AddressSanitizer + UndefinedBehaviorSanitizer in a
    stand-alone program (tools/depth_geometry_host_sanitize.c).

Bounds against the fixture.  Where the reference ran in fp64 (ideaII's four functions) both
sides are fp64 torch on the CPU doing the same arithmetic in a slightly different order
(K^-1 against a division by fx): 1e-12 of max(|value|, 1).  unproject_image runs in fp32 only
(it converts the cloud with .float()): the same pixels must be filled, and a depth is one
four-term fp32 dot product, <= 4 roundings of 2^-24 on terms that cancel at most ~10-fold
here: 4e-6 relative.  Its score is an fp32 mean of O(1) terms: 1e-5 relative.
depth2point_world builds its pixel ramp in fp32 whatever the dtype (i / (W - 1) * (W - 1)
moves index i by <= 2^-23 i): 1e-5 of max(|value|, 1) covers W = 53 at depth 3.

Parity unpinned: lift_tracks (dyn_som.py is a fragment that cannot be imported); its twin is
checked against torch's grid_sample here.
"""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dynamic3dgaussians_amd as pkg
from dynamic3dgaussians_amd import _lib, depth_geometry as dg, metrics
from tests._harness import run_host_sanitizer

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden", "depth_geometry.npz")
ZBUF = {"zbuf_5x7": (5, 7, 1000), "zbuf_37x53": (37, 53, 4097)}
FLOW = {"flow_5x7": (5, 7), "flow_37x53": (37, 53)}
TOL64, TOL_Z, TOL_SCORE, TOL_RAMP = 1e-12, 4e-6, 1e-5, 1e-5
MIRRORS = {"gs_point_depth": _lib.GsPointDepth, "gs_depth_abs_rel": _lib.GsDepthAbsRel,
           "gs_depth_unproject": _lib.GsDepthUnproject, "gs_depth_flow": _lib.GsDepthFlow,
           "gs_sample_bilinear": _lib.GsSampleBilinear}


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def _t(gold, key, dtype=torch.float64):
    return torch.from_numpy(gold[key]).to(dtype)


def _close(got, want, tol):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    err = np.abs(got - want) / np.maximum(np.abs(want), 1.0)
    assert np.all(err <= tol), float(err.max())


def test_fixture_is_small_and_complete(gold):
    assert os.path.getsize(GOLD) < 768 * 1024
    for name, (H, W, P) in ZBUF.items():
        assert gold[f"{name}.points"].shape == (2, P, 3) and gold[f"{name}.points"].dtype == np.float32
        assert gold[f"{name}.est"].shape == (2, H, W) and gold[f"{name}.est"].dtype == np.float32
        assert gold[f"{name}.score"].shape == (2,) and np.all(np.isfinite(gold[f"{name}.score"]))
        assert gold[f"{name}.exclude"].dtype == np.uint8 and 0.15 < gold[f"{name}.exclude"].mean() < 0.45
        assert (gold[f"{name}.gt"] == 0).any()
    assert np.isfinite(gold["zbuf_5x7.est"]).all()  # all 35 pixels of both cameras are filled
    filled = np.isfinite(gold["zbuf_37x53.est"]).mean()
    assert 0.5 < filled < 0.95  # and the larger map has holes
    for name, (H, W) in FLOW.items():
        for key in (name, name + "_away"):
            assert gold[f"{key}.flow_f64"].shape == (2, H, W) and gold[f"{key}.flow_f64"].dtype == np.float64
            assert gold[f"{key}.flow_f32"].dtype == np.float32
            assert (gold[f"{key}.depth"] == 0).sum() == 2
        assert gold[f"{name}.world_f64"].shape == (H, W, 3)
        assert gold[f"{name}.flows"].shape == (3, 2, H, W)
        assert np.abs(gold[f"{name}.flows"]).max() > 2.0  # samples past the border exist
    assert gold["resize.out_f64"].shape == (2, 21, 40)


@pytest.mark.parametrize("name", tuple(ZBUF))
def test_z_buffer_and_score_match_the_reference(gold, name):
    pts, w2c, K = _t(gold, f"{name}.points"), _t(gold, f"{name}.w2c"), _t(gold, f"{name}.K")
    gt, exclude = _t(gold, f"{name}.gt"), torch.from_numpy(gold[f"{name}.exclude"])
    want = gold[f"{name}.est"]
    for dt in (torch.float64, torch.float32):
        est = dg.point_depth_maps_torch(pts.to(dt), w2c, K, want.shape[1:])
        assert est.dtype == dt and est.shape == want.shape
        assert np.array_equal(np.isfinite(est.numpy()), np.isfinite(want))  # the same pixels, none excluded
        fin = np.isfinite(want)
        assert np.all(np.abs(est.numpy()[fin] - want[fin].astype(np.float64)) <= TOL_Z * want[fin])
        score = dg.depth_abs_rel_torch(est, gt.to(dt), exclude)
        _close(score, gold[f"{name}.score"], TOL_SCORE)
    # one camera, a shared cloud, an [H, W] exclude: the unbatched forms
    one = dg.point_depth_maps_torch(pts[1], w2c[1], K[1], want.shape[1:])
    assert one.shape == want.shape[1:] and torch.equal(one, dg.point_depth_maps_torch(pts, w2c, K, want.shape[1:])[1])
    s1 = dg.depth_abs_rel_torch(one, gt[1], exclude[1])
    assert s1.dim() == 0
    _close(s1, gold[f"{name}.score"][1], TOL_SCORE)
    acc = metrics.MeanDepthError(dg.point_depth_maps_torch, dg.depth_abs_rel_torch)
    acc.update(pts, w2c, K, gt, exclude)
    assert len(acc) == 1
    _close(acc.compute(), gold[f"{name}.score"].mean(), TOL_SCORE)


def test_z_buffer_twin_rejects_what_the_kernel_rejects():
    eye4, eye3 = torch.eye(4, dtype=torch.float64), torch.eye(3, dtype=torch.float64)
    H, W = 3, 4
    # u = 0.5, 1.5, 2.5 at z = 2 land on columns 0, 2, 2 (half to even), row 1
    pts = torch.tensor([[1.0, 2, 2], [3.0, 2, 2], [5.0, 2, 2]], dtype=torch.float64)
    d = dg.point_depth_maps_torch(pts, eye4, eye3, (H, W))
    assert torch.isfinite(d).nonzero().tolist() == [[1, 0], [1, 2]] and d[1, 2] == 2.0
    nan, inf = float("nan"), float("inf")
    bad = torch.tensor([[1.0, 1, 0], [1.0, 1, -2], [(W - 0.5 + 1) * 2, 2, 2], [nan, 1, 1], [1.0, nan, 1],
                        [1.0, 1, nan], [inf, 1, 1], [1.0, -inf, 1], [1e30, 1, 1e-8], [-1e30, 1, 1e-8]],
                       dtype=torch.float64)
    for dt in (torch.float64, torch.float32):
        assert torch.isinf(dg.point_depth_maps_torch(bad.to(dt), eye4, eye3, (H, W))).all()
    assert torch.isinf(dg.point_depth_maps_torch(torch.zeros(0, 3), eye4, eye3, (H, W))).all()


def test_abs_rel_of_an_image_without_a_valid_pixel_is_nan():
    est = torch.full((2, 3, 4), float("inf"), dtype=torch.float64)
    est[1] = 2.0
    gt = torch.ones(2, 3, 4, dtype=torch.float64)
    r = dg.depth_abs_rel_torch(est, gt)
    assert torch.isnan(r[0]) and r[1] == 1.0
    assert torch.isnan(dg.depth_abs_rel_torch(est[1], gt[1], torch.ones(3, 4)))  # everything excluded
    assert dg.depth_abs_rel_torch(est[1], gt[1], torch.full((3, 4), 0.5)) == 1.0  # only exclude == 1 excludes


@pytest.mark.parametrize("name", tuple(FLOW))
def test_flow_and_unprojection_match_the_reference_in_fp64(gold, name):
    for key in (name, name + "_away"):
        depth = _t(gold, f"{key}.depth")
        K1, c2w1, K2, w2c2 = (_t(gold, f"{key}.{n}") for n in ("K1", "c2w1", "K2", "w2c2"))
        flow, valid = dg.depth_flow_torch(depth, K1, c2w1, K2, w2c2, return_valid=True)
        assert flow.dtype == torch.float64 and valid.dtype == torch.uint8
        _close(flow, gold[f"{key}.flow_f64"], TOL64)
        if key.endswith("_away"):
            assert not valid.any()  # every point is behind camera 2: all clamped
        else:
            assert valid.sum() == depth.numel() - 2 and valid[1, 2] == 0  # all but the two zero depths
        batched = dg.depth_flow_torch(depth[None], K1[None], c2w1[None], K2[None], w2c2[None])
        assert torch.equal(batched[0], flow)
    depth, K1, w2c1 = _t(gold, f"{name}.depth"), _t(gold, f"{name}.K1"), _t(gold, f"{name}.w2c1")
    _close(dg.unproject_depth_torch(depth, K1, w2c1), gold[f"{name}.world_f64"], TOL_RAMP)
    # ideaII's pair (pixel_to_camera_coordinates, camera_to_world_coordinates) is the flow's first half:
    # reprojecting the unprojected points into camera 2 gives pixel + flow
    K2, w2c2 = _t(gold, f"{name}.K2"), _t(gold, f"{name}.w2c2")
    xyz = dg.unproject_depth_torch(depth, K1, w2c1)
    cam2 = xyz @ w2c2[:3, :3].T + w2c2[:3, 3]
    q = cam2 @ K2.T
    ok = depth > 0
    x, y = dg._pixel_grid(*depth.shape, depth)
    uv = q[..., :2] / q[..., 2:]
    # w2c1 is the fp32-rounded inverse of c2w1, so the two routes differ by that rounding
    assert torch.all((uv[..., 0] - x - _t(gold, f"{name}.flow_f64")[0]).abs()[ok] < 1e-4)
    assert torch.all((uv[..., 1] - y - _t(gold, f"{name}.flow_f64")[1]).abs()[ok] < 1e-4)


@pytest.mark.parametrize("name", tuple(FLOW))
def test_warp_and_accumulate_match_the_reference_in_fp64(gold, name):
    fl = _t(gold, f"{name}.flows")
    _close(dg.warp_flow_torch(fl[0], fl[1]), gold[f"{name}.warp_f64"], TOL64)
    _close(dg.accumulate_flows_torch(list(fl)), gold[f"{name}.accumulate_f64"], TOL64)
    batched = dg.accumulate_flows_torch([torch.stack([f, f]) for f in fl])
    assert torch.equal(batched[0], batched[1])
    _close(batched[0], gold[f"{name}.accumulate_f64"], TOL64)


def test_resize_flow_matches_the_reference_in_fp64(gold):
    _close(dg.resize_flow_torch(_t(gold, "resize.flow"), (21, 40)), gold["resize.out_f64"], TOL64)


def test_sampler_twin_is_grid_sample_in_fp64():
    gen = torch.Generator().manual_seed(7)
    for B, Ch, H, W in ((2, 3, 5, 7), (1, 2, 1, 6), (1, 2, 4, 1), (1, 1, 1, 1)):
        src = torch.randn(B, Ch, H, W, generator=gen, dtype=torch.float64)
        xy = torch.rand(B, 257, 2, generator=gen, dtype=torch.float64) * torch.tensor([W + 3.0, H + 3.0]) - 2.0
        xy[:, 0] = torch.tensor([0.0, 0.0])
        xy[:, 1] = torch.tensor([W - 1.0, H - 1.0])
        xy[:, 2] = torch.tensor([min(2.0, W - 1.0), min(3.0, H - 1.0)])
        xy[:, 3] = torch.tensor([1e9, -1e9])
        got = dg.sample_bilinear_torch(src, xy)
        if H > 1 and W > 1:  # grid_sample's normalised coordinates divide by W - 1 and H - 1
            grid = torch.stack([2 * xy[..., 0] / (W - 1) - 1, 2 * xy[..., 1] / (H - 1) - 1], dim=-1)[:, None]
            want = F.grid_sample(src, grid, mode="bilinear", padding_mode="border", align_corners=True)[:, :, 0]
            assert (got - want).abs().max() < 1e-12
        else:  # one row or column: linear interpolation along the other axis, clamped
            line = src.reshape(B, Ch, -1)
            t = (xy[..., 0] if W > 1 else xy[..., 1]).clamp(0, line.shape[-1] - 1)
            i0 = t.floor().clamp(max=max(line.shape[-1] - 2, 0)).long()
            i1 = (i0 + 1).clamp(max=line.shape[-1] - 1)
            f = (t - i0)[:, None]
            want = torch.gather(line, 2, i0[:, None].expand(B, Ch, -1)) * (1 - f) + \
                torch.gather(line, 2, i1[:, None].expand(B, Ch, -1)) * f
            assert (got - want).abs().max() < 1e-12
        assert torch.equal(got[:, :, 0], src[:, :, 0, 0]) and torch.equal(got[:, :, 1], src[:, :, H - 1, W - 1])
    xy = torch.tensor([[float("nan"), 1.0], [1.0, float("nan")], [1.0, 1.0]], dtype=torch.float64)
    out = dg.sample_bilinear_torch(torch.ones(2, 4, 5, dtype=torch.float64), xy)
    assert torch.isnan(out[:, :2]).all() and torch.all(out[:, 2] == 1.0)  # a NaN coordinate gives NaN


def test_lift_tracks_twin_against_grid_sample():
    """Parity unpinned (module docstring): the oracle is torch's grid_sample and the
    unprojection formula written out."""
    gen = torch.Generator().manual_seed(9)
    T, N, H, W = 3, 65, 9, 12
    depths = 1.0 + torch.rand(T, H, W, generator=gen, dtype=torch.float64)
    xy = torch.rand(T, N, 2, generator=gen, dtype=torch.float64) * torch.tensor([W + 1.0, H + 1.0]) - 1.0
    from tests import _depth_geometry_cases as C
    K = torch.stack([C.pinhole(H, W, k) for k in range(T)])
    w2c = torch.stack([C.rigid(C.rotation(0.1 * k, -0.05, 0.02 * k), (0.1, 0.2 * k, 0.3)) for k in range(T)])
    got = dg.lift_tracks_torch(xy, depths, K, w2c)
    assert got.shape == (N, T, 3)
    grid = torch.stack([2 * xy[..., 0] / (W - 1) - 1, 2 * xy[..., 1] / (H - 1) - 1], dim=-1)[:, None]
    d = F.grid_sample(depths[:, None], grid, align_corners=True, padding_mode="border")[:, 0, 0]
    cam = torch.einsum("nij,npj->npi", torch.linalg.inv(K), F.pad(xy, (0, 1), value=1.0)) * d[..., None]
    want = torch.einsum("nij,npj->npi", torch.linalg.inv(w2c), F.pad(cam, (0, 1), value=1.0))[..., :3]
    assert (got - want.transpose(0, 1)).abs().max() < 1e-12


def test_package_exports():
    for n in ("point_depth_maps", "depth_abs_rel", "unproject_depth", "depth_flow", "sample_bilinear", "warp_flow",
              "accumulate_flows", "resize_flow", "lift_tracks"):
        assert getattr(pkg, n) is getattr(dg, n), n
        assert getattr(pkg, n + "_torch") is getattr(dg, n + "_torch"), n
    assert pkg.MeanDepthError is metrics.MeanDepthError
    assert "mMDE" in metrics.__doc__ and "Open3D" not in metrics.__doc__


def _header():
    txt = open(os.path.join(REPO, "include", "gs_depth_geometry.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_library_exports_every_symbol_of_the_header_and_the_abi_is_13():
    L = _lib.load()
    names = sorted(set(re.findall(r"\b(gs_[a-z_0-9]+)\s*\(", _header())))
    want = {s + suffix for s in MIRRORS for suffix in ("", "_validate", "_struct_bytes")}
    assert set(names) == want | {"gs_depth_abs_rel_workspace_bytes"}
    for n in names:
        assert hasattr(L, n), n
        assert n in _lib.PROTOTYPES, f"{n} has no ctypes prototype"
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.lib_path()], capture_output=True, text=True).stdout
    assert set(names) <= set(re.findall(r" T (gs_[a-z_0-9]+)", out))
    assert L.gs_version() == _lib.ABI_VERSION == 13  # a new header, no existing struct changed
    base = open(os.path.join(REPO, "include", "gsplat_hip.h")).read()
    assert re.search(r"#define\s+GS_ABI_VERSION\s+13\b", base)


@pytest.mark.parametrize("struct", tuple(MIRRORS))
def test_ctypes_mirrors_have_the_library_sizes_and_the_header_fields(struct):
    L = _lib.load()
    mirror = MIRRORS[struct]
    assert ctypes.sizeof(mirror) == getattr(L, struct + "_struct_bytes")()
    body = re.search(r"struct %s \{(.*?)\};" % struct, _header(), flags=re.S).group(1)
    names = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        names += [re.findall(r"[A-Za-z_]\w*", part)[-1] for part in decl.split(",")]
    assert [f for f, _ in mirror._fields_] == names


def test_workspace_bytes():
    L = _lib.load()
    ws = L.gs_depth_abs_rel_workspace_bytes(2, 45, 77)
    assert 2 * 16 <= ws <= 2 * 16 + 256  # one {sum, count} pair per 4096-pixel chunk
    assert L.gs_depth_abs_rel_workspace_bytes(27, 800, 800) >= 27 * 157 * 16
    for bad in [(0, 16, 16), (1, 0, 16), (1, 16, -2)]:
        assert L.gs_depth_abs_rel_workspace_bytes(*bad) == 0


def _blocks(keep):
    """A valid argument block per entry over host arrays (the validators dereference nothing)."""
    L = _lib.load()
    B, Ch, H, W, P, N = 2, 3, 13, 29, 100, 50
    ws_bytes = L.gs_depth_abs_rel_workspace_bytes(B, H, W)
    bufs = {"f": np.zeros(B * max(Ch * H * W, P * 3, Ch * N), np.float32), "g": np.zeros(B * Ch * H * W, np.float32),
            "m4": np.zeros(B * 16, np.float32), "m3": np.zeros(B * 9, np.float32), "d": np.zeros(B * 2, np.float64),
            "u8": np.zeros(B * H * W, np.uint8), "ws": np.zeros(ws_bytes // 4 + 64, np.float32)}
    keep.append(bufs)
    p = {k: v.ctypes.data for k, v in bufs.items()}
    p["ws"] = (p["ws"] + 255) // 256 * 256
    return p, {
        "gs_point_depth": _lib.GsPointDepth(P=P, B=B, H=H, W=W, points=p["f"], w2c=p["m4"], K=p["m3"], depth=p["g"]),
        "gs_depth_abs_rel": _lib.GsDepthAbsRel(B=B, H=H, W=W, est=p["f"], gt=p["g"], out=p["d"], workspace=p["ws"],
                                               workspace_bytes=ws_bytes),
        "gs_depth_unproject": _lib.GsDepthUnproject(B=B, H=H, W=W, depth=p["g"], Kinv=p["m3"], c2w=p["m4"], xyz=p["f"]),
        "gs_depth_flow": _lib.GsDepthFlow(B=B, H=H, W=W, depth1=p["g"], Kinv1=p["m3"], T=p["m4"], K2=p["m3"],
                                          flow=p["f"]),
        "gs_sample_bilinear": _lib.GsSampleBilinear(B=B, Ch=Ch, H=H, W=W, mode=_lib.GS_SAMPLE_POINTS, N=N, src=p["g"],
                                                    coords=p["m4"], out=p["f"]),
    }


BAD = {
    "gs_point_depth": [("B", 0, b"must be > 0"), ("H", -1, b"must be > 0"), ("W", 0, b"must be > 0"),
                       ("W", 1 << 20, b"too large"), ("P", -1, b"P must be"), ("points", None, b"points are required"),
                       ("w2c", None, b"required"), ("K", None, b"required"), ("depth", None, b"depth is required"),
                       ("points_batch_stride", 7, b"points_batch_stride"),
                       ("points_batch_stride", 100, b"points_batch_stride")],
    "gs_depth_abs_rel": [("B", 0, b"must be > 0"), ("H", 0, b"must be > 0"), ("W", -5, b"must be > 0"),
                         ("est", None, b"required"), ("gt", None, b"required"), ("out", None, b"out is required"),
                         ("workspace", None, b"workspace is required"), ("workspace_bytes", 8, b"needed")],
    "gs_depth_unproject": [("B", -1, b"must be > 0"), ("H", 0, b"must be > 0"), ("W", 0, b"must be > 0"),
                           ("depth", None, b"depth is required"), ("Kinv", None, b"required"),
                           ("c2w", None, b"required"), ("xyz", None, b"xyz is required")],
    "gs_depth_flow": [("B", 0, b"must be > 0"), ("H", 0, b"must be > 0"), ("W", 0, b"must be > 0"),
                      ("H", 1 << 16, b"too large"), ("depth1", None, b"depth1 is required"),
                      ("Kinv1", None, b"required"), ("T", None, b"required"), ("K2", None, b"required"),
                      ("flow", None, b"flow is required")],
    "gs_sample_bilinear": [("B", 0, b"must be > 0"), ("Ch", 0, b"Ch must be > 0"), ("H", 0, b"must be > 0"),
                           ("W", -2, b"must be > 0"), ("mode", 2, b"mode must be"), ("N", 0, b"N must be"),
                           ("src", None, b"src is required"), ("coords", None, b"coords are required"),
                           ("out", None, b"out is required"), ("add_displacement", 1, b"add_displacement")],
}


@pytest.mark.parametrize("entry", tuple(BAD))
def test_validators_reject_bad_arguments_without_gpu(entry):
    L = _lib.load()
    keep = []
    validate, call = getattr(L, entry + "_validate"), getattr(L, entry)
    p, good = _blocks(keep)
    assert validate(ctypes.byref(good[entry])) == 0, L.gs_last_error()
    assert validate(None) < 0 and b"null argument" in L.gs_last_error()
    for field, value, msg in BAD[entry]:
        bad = _blocks(keep)[1][entry]
        setattr(bad, field, value)
        assert validate(ctypes.byref(bad)) < 0, (field, value)
        assert msg in L.gs_last_error(), (field, L.gs_last_error())
        # the entry point runs the validator before anything touches a device
        assert call(ctypes.byref(bad), None) < 0 and msg in L.gs_last_error(), field
    for field in [f for f, t in MIRRORS[entry]._fields_ if t is ctypes.c_void_p and f != "workspace"]:
        bad = _blocks(keep)[1][entry]
        if getattr(bad, field):
            setattr(bad, field, getattr(bad, field) + 2)
            assert validate(ctypes.byref(bad)) < 0 and b"aligned" in L.gs_last_error(), field


def test_validators_accept_the_optional_forms():
    L = _lib.load()
    keep = []
    p, good = _blocks(keep)
    a = good["gs_point_depth"]
    a.points_batch_stride = 300
    assert L.gs_point_depth_validate(ctypes.byref(a)) == 0
    a.P, a.points, a.points_batch_stride = 0, None, 0
    assert L.gs_point_depth_validate(ctypes.byref(a)) == 0  # an empty cloud needs no pointer
    a = good["gs_depth_abs_rel"]
    a.exclude, a.exclude_batch_stride = p["g"], 13 * 29
    assert L.gs_depth_abs_rel_validate(ctypes.byref(a)) == 0
    a.exclude_batch_stride = 0
    assert L.gs_depth_abs_rel_validate(ctypes.byref(a)) == 0
    a.exclude_batch_stride = 7
    assert L.gs_depth_abs_rel_validate(ctypes.byref(a)) < 0 and b"exclude_batch_stride" in L.gs_last_error()
    a = good["gs_depth_unproject"]
    a.xy = p["f"]
    assert L.gs_depth_unproject_validate(ctypes.byref(a)) == 0
    a = good["gs_depth_flow"]
    a.valid = p["u8"]
    assert L.gs_depth_flow_validate(ctypes.byref(a)) == 0
    a = good["gs_sample_bilinear"]
    a.Ch, a.mode, a.h, a.w, a.N, a.add_displacement = 2, _lib.GS_SAMPLE_DISPLACEMENT, 5, 10, 50, 1
    assert L.gs_sample_bilinear_validate(ctypes.byref(a)) == 0
    a.N = 49
    assert L.gs_sample_bilinear_validate(ctypes.byref(a)) < 0 and b"h*w" in L.gs_last_error()
    a.N, a.h = 50, 0
    assert L.gs_sample_bilinear_validate(ctypes.byref(a)) < 0 and b"h, w must be" in L.gs_last_error()
    a.h, a.Ch = 5, 3
    assert L.gs_sample_bilinear_validate(ctypes.byref(a)) < 0 and b"add_displacement" in L.gs_last_error()


class _DeviceClaim(torch.Tensor):
    """A host tensor that reports is_cuda, so the wrappers' dtype / layout / shape rules (all
    checked before any device work) can be exercised where there is no GPU."""

    @staticmethod
    def __new__(cls, t):
        return torch.Tensor._make_subclass(cls, t, t.requires_grad)

    @property
    def is_cuda(self):
        return True


def test_wrappers_reject_what_the_kernels_cannot_take():
    D, E = _DeviceClaim, _lib.GsplatError
    pts, w2c, K = torch.rand(10, 3), torch.eye(4)[None], torch.eye(3)[None]
    depth, flow = torch.rand(1, 5, 7), torch.rand(2, 5, 7)
    for call in (lambda: dg.point_depth_maps(pts, w2c, K, (5, 7)), lambda: dg.depth_abs_rel(depth, depth),
                 lambda: dg.unproject_depth(depth, K, w2c), lambda: dg.depth_flow(depth, K, w2c, K, w2c),
                 lambda: dg.sample_bilinear(flow, torch.rand(4, 2)), lambda: dg.warp_flow(flow, flow),
                 lambda: dg.accumulate_flows([flow, flow]), lambda: dg.lift_tracks(torch.rand(1, 4, 2), depth, K, w2c),
                 lambda: metrics.MeanDepthError().update(pts, w2c, K, depth)):
        with pytest.raises(E, match="device tensors"):
            call()
    with pytest.raises(E, match="device tensors"):
        dg.resize_flow(flow, (3, 4))
    with pytest.raises(E, match="float32"):
        dg.point_depth_maps(D(pts.double()), D(w2c), D(K), (5, 7))
    with pytest.raises(E, match="float32"):
        dg.depth_abs_rel(D(depth.half()), D(depth.half()))
    with pytest.raises(E, match="contiguous"):
        dg.unproject_depth(D(torch.rand(1, 7, 5).transpose(1, 2)), D(K), D(w2c))
    with pytest.raises(E, match="contiguous"):
        dg.sample_bilinear(D(torch.rand(2, 7, 5).transpose(1, 2)), D(torch.rand(4, 2)))
    with pytest.raises(E, match="shape"):
        dg.depth_abs_rel(D(depth), D(torch.rand(1, 5, 6)))
    with pytest.raises(E, match="exclude must have shape"):
        dg.depth_abs_rel(D(depth), D(depth), D(torch.ones(2, 5, 7)))
    with pytest.raises(E, match="exclude must be a device tensor"):
        dg.depth_abs_rel(D(depth), D(depth), torch.ones(5, 7))
    with pytest.raises(E, match=r"\[P, 3\]"):
        dg.point_depth_maps(D(torch.rand(10, 2)), D(w2c), D(K), (5, 7))
    with pytest.raises(E, match="one cloud per camera"):
        dg.point_depth_maps(D(torch.rand(3, 10, 3)), D(w2c), D(K), (5, 7))
    with pytest.raises(E, match="K must have 1 matrices"):
        dg.point_depth_maps(D(pts), D(w2c), D(torch.eye(3).repeat(2, 1, 1)), (5, 7))
    with pytest.raises(E, match="hw must be"):
        dg.point_depth_maps(D(pts), D(w2c), D(K), (0, 7))
    with pytest.raises(E, match=r"w2c must be a \[B, 4, 4\]"):
        dg.unproject_depth(D(depth), D(K), D(torch.eye(3)[None]))
    with pytest.raises(E, match=r"xy must be"):
        dg.sample_bilinear(D(flow), D(torch.rand(4, 3)))
    with pytest.raises(E, match="displacement must be"):
        dg.warp_flow(D(flow), D(torch.rand(3, 5, 7)))
    with pytest.raises(E, match="first flow's shape"):
        dg.accumulate_flows([D(flow), D(torch.rand(2, 5, 8))])
    with pytest.raises(E, match="no flow"):
        dg.accumulate_flows([])
    with pytest.raises(E, match=r"tracks_xy must be \[T, N, 2\]"):
        dg.lift_tracks(D(torch.rand(2, 4, 2)), D(depth), D(K), D(w2c))
    with pytest.raises(E, match="empty"):
        dg.depth_abs_rel(D(torch.rand(0, 5, 7)), D(torch.rand(0, 5, 7)))
    with pytest.raises(E, match="before any update"):
        metrics.MeanDepthError().compute()


@pytest.mark.skipif(shutil.which("gcc") is None or shutil.which("g++") is None, reason="gcc / g++ not available")
def test_validators_are_sanitizer_clean(tmp_path):
    """gs_depth_geometry_host.cpp (with gs_host.cpp's error state) under ASan + UBSan in a plain
    CPU executable with its own main: nothing preloaded, nothing loaded into Python."""
    run_host_sanitizer(tmp_path, "depth_geometry_host_sanitize.c", ["gs_depth_geometry_host.cpp", "gs_host.cpp"],
                       "depth geometry host sanitize ok")
