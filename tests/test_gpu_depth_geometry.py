"""The depth-map geometry kernels (csrc/gs_depth_geometry.hip) on the GPU against the fp64
_torch twins of depth_geometry.py on the CPU (never the HIP code's own output), and against
the reference's fp64 records in tests/golden/depth_geometry.npz where they exist.

Bounds.  For each case the bound is 4 x the deviation of the reference formulation itself run
in fp32 (the _torch twin in fp32 on the CPU) from the fp64 twin on the same inputs, computed
here: the kernel may order its three-term dot products differently from torch, and each result
is a handful of fp32 roundings, so a small multiple of the formulation's own rounding is the
honest envelope.  Where that deviation is 0 the floor is one fp32 ulp of the value.  Decisions
(which pixels the z-buffer fills, the flow's valid map) must be exact: the clouds are built
backwards from the pixels so that none hangs on rounding (tests/_depth_geometry_cases.py), and
no pixel is excluded.

Shapes are the smallest at which the kernels can go wrong: 5 x 7 (one workgroup, ragged) and
37 x 53 (1961 pixels: eight workgroups of 256, the last ragged), P = 1000 and 4097 (neither a
multiple of 256), N = 257 sample positions, 2 x 45 x 77 for the score, 1 x W and H x 1
sources for the sampler's degenerate axes.

With GS_PARITY_JSON set to a path, the measured deviations and their bounds are written there
at the end of the module (profiles/depth_geometry/parity.json is such a record).

Parity unpinned: lift_tracks is checked against its torch twin only (dyn_som.py cannot be
imported; the twin is checked against torch's grid_sample in tests/test_depth_geometry.py).
"""
from __future__ import annotations

import functools
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dynamic3dgaussians_amd import depth_geometry as dg
from dynamic3dgaussians_amd import metrics as M
from dynamic3dgaussians_amd.camera import camera_rig
from dynamic3dgaussians_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizerBatch
from dynamic3dgaussians_amd.scene import make_gaussians
from tests import _depth_geometry_cases as C

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "depth_geometry.npz")
ENVELOPE = 4.0
ZBUF, FLOW = tuple(C.ZBUF_CASES), tuple(C.FLOW_CASES)
RECORD = {}


@pytest.fixture(scope="module", autouse=True)
def _write_parity_record():
    yield
    path = os.environ.get("GS_PARITY_JSON")
    if path and RECORD:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            json.dump({"envelope": ENVELOPE, "cases": RECORD}, fh, indent=1, sort_keys=True)


@functools.lru_cache(maxsize=None)
def _gold():
    g = np.load(GOLD)
    return {k: torch.from_numpy(g[k]) for k in g.files}


def _ulp32(v: torch.Tensor) -> torch.Tensor:
    return torch.from_numpy(np.spacing(v.abs().float().numpy())).double()


def _check(name, got, ref64, twin32, scale=None):
    """got (device, fp32) within ENVELOPE x max|twin32 - ref64| of ref64, per element at least one
    fp32 ulp of the value; with `scale` both deviations are divided by it first (relative forms)."""
    got, ref64, twin32 = got.detach().cpu().double(), ref64.double(), twin32.double()
    assert got.shape == ref64.shape, (got.shape, ref64.shape)
    s = torch.ones_like(ref64) if scale is None else scale.double()
    own = ((twin32 - ref64).abs() / s).max().item()
    err = (got - ref64).abs() / s
    bound = torch.maximum(torch.full_like(err, ENVELOPE * own), _ulp32(ref64) / s)
    RECORD[name] = {"hip_deviation": err.max().item(), "fp32_formulation_deviation": own,
                    "bound": max(ENVELOPE * own, (_ulp32(ref64) / s).max().item())}
    print(f"{name}: hip {err.max().item():.3e} fp32 formulation {own:.3e} bound {RECORD[name]['bound']:.3e}")
    assert torch.all(err <= bound), RECORD[name]


def _dev(*ts):
    return tuple(None if t is None else t.to(DEV).contiguous() for t in ts)


# ---- the z-buffer

@functools.lru_cache(maxsize=None)
def _zbuf(name):
    pts, w2c, K, gt, exclude = C.zbuf_case(name)
    H, W = C.ZBUF_CASES[name][:2]
    ref = dg.point_depth_maps_torch(pts.double(), w2c, K, (H, W))
    f32 = dg.point_depth_maps_torch(pts, w2c.float(), K.float(), (H, W))
    assert torch.equal(torch.isfinite(ref), torch.isfinite(f32))  # the cloud is decision-robust
    return pts, w2c, K, gt, exclude, ref, f32


def _check_zbuf(name, got, ref, f32):
    got = got.cpu()
    assert torch.equal(torch.isfinite(got), torch.isfinite(ref)), "another set of filled pixels (cap 0)"
    assert torch.all(got[~torch.isfinite(ref)] == float("inf"))
    fin = torch.isfinite(ref)
    _check(name, got[fin], ref[fin], f32[fin], scale=ref[fin])


@pytest.mark.parametrize("name", ZBUF)
def test_z_buffer_parity_on_decision_robust_clouds(name):
    pts, w2c, K, _, _, ref, f32 = _zbuf(name)
    H, W = C.ZBUF_CASES[name][:2]
    if name == "zbuf_5x7":
        assert torch.isfinite(ref).all()  # all 35 pixels of both cameras are filled
    d_pts, d_w2c, d_K = _dev(pts, w2c.float(), K.float())
    got = dg.point_depth_maps(d_pts, d_w2c, d_K, (H, W))  # a cloud per camera, B = 2 in one call
    torch.cuda.synchronize()
    assert got.shape == (2, H, W) and got.dtype == torch.float32
    _check_zbuf(name, got, ref, f32)
    again = dg.point_depth_maps(d_pts, d_w2c, d_K, (H, W))
    assert torch.equal(got, again)  # integer min: no dependence on the order of arrival
    # the per-camera stride gives the maps of B separate calls (each a shared cloud, B = 1)
    for b in range(2):
        one = dg.point_depth_maps(d_pts[b].contiguous(), d_w2c[b:b + 1], d_K[b:b + 1], (H, W))
        assert torch.equal(one[0], got[b])
        assert torch.equal(dg.point_depth_maps(d_pts[b].contiguous(), d_w2c[b], d_K[b], (H, W)), got[b])
    # one cloud seen by both cameras: against the fp64 twin's set of pixels wherever the fp32 twin agrees with it
    shared_ref = dg.point_depth_maps_torch(pts[0].double(), w2c, K, (H, W))
    shared = dg.point_depth_maps(d_pts[0].contiguous(), d_w2c, d_K, (H, W)).cpu()
    assert torch.equal(shared[0], got[0].cpu())
    assert torch.equal(torch.isfinite(shared[0]), torch.isfinite(shared_ref[0]))


def test_z_buffer_known_answers():
    H, W = 3, 4
    eye4, eye3 = torch.eye(4, device=DEV)[None], torch.eye(3, device=DEV)[None]
    # u = 0.5, 1.5, 2.5 at v = 1: columns 0, 2, 2 (round half to even)
    pts = torch.tensor([[1.0, 2, 2], [3.75, 2.5, 2.5], [5.0, 2, 2]], device=DEV)
    d = dg.point_depth_maps(pts, eye4, eye3, (H, W))[0].cpu()
    assert torch.isfinite(d).nonzero().tolist() == [[1, 0], [1, 2]]  # columns 1 and 3 stay empty
    assert d[1, 0] == 2.0 and d[1, 2] == 2.0  # the nearer of column 2's two points (z = 2.5 at u = 1.5, z = 2 at u = 2.5)
    nan, inf = float("nan"), float("inf")
    # rejected by the kernel's own bounds test, in float, before any index exists
    bad = torch.tensor([[1.0, 1, 0],                  # z = 0
                        [1.0, 1, -2],                 # z < 0
                        [(W - 0.5 + 1) * 2, 2, 2],    # u = W - 0.5 + 1: past the last column
                        [-1.2, 2, 2],                 # u = -0.6: rounds to -1
                        [2.0, (H - 0.5 + 0.1) * 2, 2],  # v = H - 0.4: rounds to H
                        [nan, 1, 1], [1.0, nan, 1], [1.0, 1, nan],
                        [inf, 1, 1], [1.0, -inf, 1], [1.0, 1, inf],
                        [1e30, 1, 1e-8], [-1e30, 1, 1e-8],  # |u| = 1e38: far beyond the int32 range
                        [3e38, 3e38, 1e-30]], device=DEV)   # u overflows to inf
    out = dg.point_depth_maps(bad, eye4, eye3, (H, W))
    torch.cuda.synchronize()
    assert torch.all(out == inf)
    assert torch.equal(out.cpu(), dg.point_depth_maps_torch(bad.cpu(), eye4.cpu(), eye3.cpu(), (H, W)))
    empty = dg.point_depth_maps(torch.zeros(0, 3, device=DEV), eye4, eye3, (H, W))
    assert empty.shape == (1, H, W) and torch.all(empty == inf)
    # in range up to the last pixel: u = W - 1 + 0.4, v = H - 1 + 0.4
    edge = torch.tensor([[(W - 0.6) * 2, (H - 0.6) * 2, 2.0]], device=DEV)
    d = dg.point_depth_maps(edge, eye4, eye3, (H, W))[0].cpu()
    assert torch.isfinite(d).nonzero().tolist() == [[H - 1, W - 1]]


# ---- the abs-rel score

def _abs_rel_case(name):
    if name == "ragged":
        gen = torch.Generator().manual_seed(61)
        gt = 0.5 + 3.0 * torch.rand(2, 45, 77, generator=gen, dtype=torch.float32)
        est = gt * (1.0 + 0.2 * torch.randn(2, 45, 77, generator=gen, dtype=torch.float32))
        gt[torch.rand(2, 45, 77, generator=gen, dtype=torch.float32) < 0.1] = 0.0
        gt[0, 3, 5] = -1.0
        est[torch.rand(2, 45, 77, generator=gen, dtype=torch.float32) < 0.2] = float("inf")
        exclude = (torch.rand(2, 45, 77, generator=gen, dtype=torch.float32) < 0.8).float()
        return est, gt, exclude
    g = _gold()
    return g[f"{name}.est"], g[f"{name}.gt"], g[f"{name}.exclude"].float()


@pytest.mark.parametrize("name", ZBUF + ("ragged",))
def test_abs_rel_against_the_fp64_twin(name):
    est, gt, exclude = _abs_rel_case(name)
    ref = dg.depth_abs_rel_torch(est.double(), gt.double(), exclude)
    f32 = dg.depth_abs_rel_torch(est, gt, exclude)
    d_est, d_gt, d_ex = _dev(est, gt, exclude)
    got = dg.depth_abs_rel(d_est, d_gt, d_ex)
    assert got.dtype == torch.float64 and got.shape == (2,) and got.is_cuda
    _check(f"abs_rel.{name}", got, ref, f32, scale=ref)
    sums = dg.depth_abs_rel_sums(d_est, d_gt, d_ex).cpu()
    ok = torch.isfinite(est) & (gt > 0) & (exclude != 1)
    assert sums[:, 1].tolist() == ok.sum(dim=(1, 2)).double().tolist()  # the counts are exact
    assert torch.equal(dg.depth_abs_rel(d_est, d_gt, d_ex), got)  # fixed-order sums: the same bits
    if name in ZBUF:  # the reference's own fp32 score, within the fp32 mean's rounding
        want = _gold()[f"{name}.score"]
        assert torch.all((got.cpu() - want).abs() <= 1e-5 * want)
    # a shared [H, W] mask, no mask, one [H, W] pair, a uint8 mask
    shared = dg.depth_abs_rel(d_est, d_gt, d_ex[1].contiguous())
    _check(f"abs_rel.{name}.shared", shared, dg.depth_abs_rel_torch(est.double(), gt.double(), exclude[1]),
           dg.depth_abs_rel_torch(est, gt, exclude[1]), scale=ref)
    plain = dg.depth_abs_rel(d_est, d_gt)
    _check(f"abs_rel.{name}.plain", plain, dg.depth_abs_rel_torch(est.double(), gt.double()),
           dg.depth_abs_rel_torch(est, gt), scale=ref)
    one = dg.depth_abs_rel(d_est[0].contiguous(), d_gt[0].contiguous(), d_ex[0].to(torch.uint8).contiguous())
    assert one.dim() == 0 and one == got[0]


def test_abs_rel_without_a_valid_pixel_is_nan():
    est = torch.full((2, 5, 7), float("inf"), device=DEV)
    est[1] = 2.0
    gt = torch.ones(2, 5, 7, device=DEV)
    r = dg.depth_abs_rel(est, gt).cpu()
    assert torch.isnan(r[0]) and r[1] == 1.0
    assert torch.isnan(dg.depth_abs_rel(est[1].contiguous(), gt[1].contiguous(), torch.ones(5, 7, device=DEV)).cpu())
    est[1, 0, 0] = float("nan")  # neither finite nor counted
    assert dg.depth_abs_rel_sums(est, gt).cpu()[1].tolist() == [34.0, 34.0]


def test_mean_depth_error_is_the_mean_of_the_per_image_scores():
    acc = M.MeanDepthError()
    scores, scores32 = [], []
    for name in ZBUF:
        pts, w2c, K, gt, exclude, ref, f32 = _zbuf(name)
        d = _dev(pts, w2c.float(), K.float(), gt, exclude.float())
        acc.update(*d)
        scores.append(dg.depth_abs_rel_torch(ref, gt.double(), exclude))
        scores32.append(dg.depth_abs_rel_torch(f32, gt, exclude))
    assert len(acc) == 2
    entries = torch.cat(acc._entries)
    want = torch.cat(scores)
    _check("mean_depth_error.entries", entries, want, torch.cat(scores32), scale=want)
    assert acc.compute() == entries.mean().item()


# ---- evaluate_cameras

def _settings(n, W, H):
    return [GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=c.tanfovx, tanfovy=c.tanfovy, c_x=c.c_x, c_y=c.c_y,
        bg=torch.zeros(3, device=DEV), viewmatrix=torch.from_numpy(c.viewmatrix.copy()).to(DEV),
        projmatrix=torch.from_numpy(c.projmatrix.copy()).to(DEV), sh_degree=0,
        campos=torch.from_numpy(c.campos.copy()).to(DEV), compat="reference") for c in camera_rig(27, W, H)[:n]]


@functools.lru_cache(maxsize=None)
def _scene(P=600, W=48, H=40, seed=3):
    g = make_gaussians(P, seed=seed, scale_mult=6.0, device=DEV)
    rv = {"means3D": g["means3D"], "colors_precomp": g["colors"], "rotations": g["rotations"],
          "opacities": g["opacities"], "scales": g["scales"], "means2D": torch.zeros_like(g["means3D"])}
    gen = torch.Generator().manual_seed(seed)
    targets = torch.rand(2, 3, H, W, generator=gen).to(DEV)
    depth_gt = 1.0 + 3.0 * torch.rand(2, H, W, generator=gen)
    depth_gt[torch.rand(2, H, W, generator=gen) < 0.1] = 0.0
    exclude = (torch.rand(2, H, W, generator=gen) < 0.3).float()
    return rv, _settings(2, W, H), targets, depth_gt.to(DEV), exclude.to(DEV)


def test_evaluate_cameras_reports_the_mde_of_the_separate_calls():
    rv, sets, targets, depth_gt, exclude = _scene()
    base = M.evaluate_cameras(rv, sets, targets)
    out = M.evaluate_cameras(rv, sets, targets, depth_gt=depth_gt, depth_exclude=exclude)
    assert set(out) == set(base) | {"mde"} and "mde" not in base  # the default returns exactly today's dict
    assert set(base) == {"image", "metrics", "sse", "sae", "mask_sum", "ssim", "l1", "psnr"}
    for k in ("image", "sse", "sae", "mask_sum", "ssim", "l1", "psnr"):
        assert torch.equal(out[k], base[k]), k
    w2c, K, hw = dg.cameras_of_settings(sets)
    assert hw == (40, 48)
    rig = camera_rig(27, 48, 40)[:2]
    assert torch.equal(w2c.cpu(), torch.stack([torch.from_numpy(c.viewmatrix.copy()).t() for c in rig]))
    est = dg.point_depth_maps(rv["means3D"], w2c, K, hw)
    assert torch.isfinite(est).sum() > 100  # the cloud is in view
    want = dg.depth_abs_rel(est, depth_gt, exclude)
    assert out["mde"].shape == (2,) and out["mde"].dtype == torch.float64 and torch.equal(out["mde"], want)
    acc = M.MeanDepthError()
    acc.update(rv["means3D"], w2c, K, depth_gt, exclude)
    assert acc.compute() == want.mean().item()
    # and against the fp64 twin wherever the fp32 twin makes the same decisions as it
    ref_map = dg.point_depth_maps_torch(rv["means3D"].cpu().double(), w2c.cpu().double(), K.cpu().double(), hw)
    if torch.equal(torch.isfinite(ref_map), torch.isfinite(est.cpu())):
        ref = dg.depth_abs_rel_torch(ref_map, depth_gt.cpu().double(), exclude.cpu())
        map32 = dg.point_depth_maps_torch(rv["means3D"].cpu(), w2c.cpu(), K.cpu(), hw)
        _check("evaluate_cameras.mde", out["mde"], ref, dg.depth_abs_rel_torch(map32, depth_gt.cpu(), exclude.cpu()),
               scale=ref)
    with pytest.raises(M.GsplatError, match="comes with depth_gt"):
        M.evaluate_cameras(rv, sets, targets, depth_exclude=exclude)


def test_mde_updates_and_evaluate_cameras_make_no_host_sync():
    """torch.cuda.set_sync_debug_mode("error") raises at every torch call that makes the host wait
    for the device.  Armed on an .item() first, which must raise.  compute() runs outside."""
    rv, sets, targets, depth_gt, exclude = _scene()
    ras = GaussianRasterizerBatch(sets)
    w2c, K, _ = dg.cameras_of_settings(sets)
    pts = rv["means3D"]
    # warm-ups outside the mode: the library is loaded, the rasterizer's plan is sized
    M.evaluate_cameras(rv, ras, targets, depth_gt=depth_gt, depth_exclude=exclude)
    acc = M.MeanDepthError()
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode("error")
        try:
            pts.sum().item()
            armed = False
        except RuntimeError as e:
            armed = "synchroniz" in str(e)
        if armed:
            for _ in range(3):
                acc.update(pts, w2c, K, depth_gt, exclude)
            out = M.evaluate_cameras(rv, ras, targets, depth_gt=depth_gt, depth_exclude=exclude)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert armed, "torch's sync debug mode did not raise at .item(): the guard checked nothing"
    want = out["mde"].mean().item()
    assert len(acc) == 3 and abs(acc.compute() - want) <= 1e-14 * abs(want)


# ---- unprojection and flow

@pytest.mark.parametrize("name", FLOW)
def test_unprojection_against_the_fp64_twin(name):
    depth, K1, c2w1, _, _ = C.flow_case(name)
    w2c1 = C.f32(torch.linalg.inv(c2w1))
    assert (depth == 0).sum() == 2
    ref = dg.unproject_depth_torch(depth.double(), K1, w2c1)
    f32 = dg.unproject_depth_torch(depth, K1.float(), w2c1.float())
    d_depth, d_K, d_w2c = _dev(depth, K1.float(), w2c1.float())
    got = dg.unproject_depth(d_depth, d_K, d_w2c)
    assert got.shape == (*depth.shape, 3)
    _check(f"unproject.{name}", got, ref, f32)
    two = dg.unproject_depth(torch.stack([d_depth, d_depth * 2]), torch.stack([d_K, d_K]), torch.stack([d_w2c, d_w2c]))
    assert torch.equal(two[0], got)
    _check(f"unproject.{name}.batched", two[1], dg.unproject_depth_torch(depth.double() * 2, K1, w2c1),
           dg.unproject_depth_torch(depth * 2, K1.float(), w2c1.float()))
    # the reference's own fp64 record (dyn_utils.depth2point_world; its pixel ramp is fp32: 1e-5)
    want = _gold()[f"{name}.world_f64"]
    assert torch.all((got.cpu().double() - want).abs() <= 1e-5 * want.abs().clamp(min=1.0))


@pytest.mark.parametrize("name", FLOW)
@pytest.mark.parametrize("away", (False, True))
def test_flow_against_the_fp64_twin(name, away):
    depth, K1, c2w1, K2, w2c2 = C.flow_case(name, away)
    ref, ref_valid = dg.depth_flow_torch(depth.double(), K1, c2w1, K2, w2c2, return_valid=True)
    f32 = dg.depth_flow_torch(depth, K1.float(), c2w1.float(), K2.float(), w2c2.float())
    # q.z of every pixel, in fp64: far from the clamp on either side, so `valid` is robust
    xyz = dg._unproject_torch(depth.double()[None], *(g[None] for g in dg._pixel_grid(*depth.shape, depth.double())),
                              K1[None], torch.linalg.inv(c2w1)[None])[0]
    qz = (xyz @ w2c2[:3, :3].T + w2c2[:3, 3])[..., 2]
    seen = depth > 0  # the two zero-depth pixels sit at camera 1's centre: q.z = -0.6 in both cases, clamped
    assert qz[~seen].max() < -0.5
    if away:
        assert qz.max() < -0.5 and qz[seen].max() < -1.0 and not ref_valid.any()  # every pixel is clamped
    else:
        assert qz[seen].min() > 0.5 and ref_valid.sum() == depth.numel() - 2  # none near the clamp
    d = _dev(depth, K1.float(), c2w1.float(), K2.float(), w2c2.float())
    got, valid = dg.depth_flow(*d, return_valid=True)
    assert got.shape == (2, *depth.shape) and valid.dtype == torch.uint8
    assert torch.equal(valid.cpu(), ref_valid)  # exact
    key = f"flow.{name}" + (".away" if away else "")
    want = _gold()[f"{name}{'_away' if away else ''}.flow_f64"]  # ideaII.compute_optical_flow's own fp64 record
    g = got.cpu()
    for tag, oracle in (("", ref), (".reference", want)):
        if away:  # every pixel is clamped (|flow| ~ 1e7): relative to max(|value|, 1)
            _check(key + tag, g, oracle, f32, scale=oracle.abs().clamp(min=1.0))
        else:  # in pixels where the depth is seen; the two clamped pixels relative, as the away case
            _check(key + tag, g[:, seen], oracle[:, seen], f32[:, seen])
            _check(key + tag + ".clamped", g[:, ~seen], oracle[:, ~seen], f32[:, ~seen],
                   scale=oracle[:, ~seen].abs().clamp(min=1.0))
    assert torch.equal(dg.depth_flow(*d), got)
    b = [torch.stack([t, t]) for t in d]
    two, v2 = dg.depth_flow(*b, return_valid=True)
    assert torch.equal(two[1], got) and torch.equal(v2[0], valid)


# ---- the sampler

def _grid_sample64(src, xy):
    H, W = src.shape[-2:]
    xy = xy.double()  # the normalisation itself in fp64
    grid = torch.stack([2 * xy[..., 0] / (W - 1) - 1, 2 * xy[..., 1] / (H - 1) - 1], dim=-1)[:, None]
    return F.grid_sample(src.double(), grid, mode="bilinear", padding_mode="border", align_corners=True)[:, :, 0]


def test_sampler_against_fp64_grid_sample():
    gen = torch.Generator().manual_seed(71)
    B, Ch, H, W, N = 2, 3, 5, 7, 257
    src = torch.randn(B, Ch, H, W, generator=gen, dtype=torch.float32)
    xy = torch.rand(B, N, 2, generator=gen, dtype=torch.float32) * torch.tensor([W + 3.0, H + 3.0]) - 2.0
    xy[:, 0] = torch.tensor([0.0, 0.0])
    xy[:, 1] = torch.tensor([W - 1.0, H - 1.0])
    xy[:, 2] = torch.tensor([2.0, 3.0])  # an exact integer position
    xy[:, 3] = torch.tensor([1e9, -1e9])  # far outside: the border
    ref = _grid_sample64(src, xy)
    assert (dg.sample_bilinear_torch(src.double(), xy.double()) - ref).abs().max() < 1e-12
    f32 = dg.sample_bilinear_torch(src, xy)
    d_src, d_xy = _dev(src, xy)
    got = dg.sample_bilinear(d_src, d_xy)
    assert got.shape == (B, Ch, N)
    _check("sample.5x7", got, ref, f32)
    g = got.cpu()
    assert torch.equal(g[:, :, 0], src[:, :, 0, 0]) and torch.equal(g[:, :, 1], src[:, :, H - 1, W - 1])
    assert torch.equal(g[:, :, 2], src[:, :, 3, 2]) and torch.equal(g[:, :, 3], src[:, :, 0, W - 1])
    assert torch.equal(dg.sample_bilinear(d_src[0].contiguous(), d_xy[0].contiguous()), got[0])
    # H = 1 and W = 1 sources: grid_sample's normalisation divides by zero there, so the fp64 twin is the oracle
    for h, w in ((1, 6), (4, 1), (1, 1)):
        s = torch.randn(1, 2, h, w, generator=gen, dtype=torch.float32)
        p = torch.rand(1, N, 2, generator=gen, dtype=torch.float32) * torch.tensor([w + 3.0, h + 3.0]) - 2.0
        got = dg.sample_bilinear(*_dev(s, p))
        _check(f"sample.{h}x{w}", got, dg.sample_bilinear_torch(s.double(), p.double()), dg.sample_bilinear_torch(s, p))
    # a NaN coordinate gives a NaN output and touches nothing else
    p = torch.tensor([[[float("nan"), 1.0], [1.0, float("nan")], [1.5, 2.5]]])
    got = dg.sample_bilinear(*_dev(src[:1], p)).cpu()
    assert torch.isnan(got[:, :, :2]).all() and torch.isfinite(got[:, :, 2]).all()


@pytest.mark.parametrize("name", FLOW)
def test_warp_and_accumulate_against_the_reference_record(name):
    g = _gold()
    fl = g[f"{name}.flows"]
    d = _dev(*fl)
    got = dg.warp_flow(d[0], d[1])
    assert got.shape == fl[0].shape
    _check(f"warp.{name}", got, g[f"{name}.warp_f64"], dg.warp_flow_torch(fl[0], fl[1]))
    acc = dg.accumulate_flows(list(d))
    _check(f"accumulate.{name}", acc, g[f"{name}.accumulate_f64"], dg.accumulate_flows_torch(list(fl)))
    # the fused step is the sum it replaces, bit for bit
    step = d[0] + dg.warp_flow(d[1], d[0])
    assert torch.equal(dg.accumulate_flows([d[0], d[1]]), step)
    assert torch.equal(dg.accumulate_flows([d[0]]), d[0])
    batched = dg.accumulate_flows([torch.stack([f, f]) for f in d])
    assert torch.equal(batched[0], acc) and torch.equal(batched[1], acc)
    # a displacement grid of another size than the source
    small = dg.warp_flow(d[0], d[1][:, :3, :4].contiguous())
    _check(f"warp.{name}.crop", small, dg.warp_flow_torch(fl[0].double(), fl[1][:, :3, :4].double()),
           dg.warp_flow_torch(fl[0], fl[1][:, :3, :4]))


def test_resize_flow_against_the_reference_record():
    g = _gold()
    fl = g["resize.flow"]
    got = dg.resize_flow(fl.to(DEV), (21, 40))
    assert got.shape == (2, 21, 40)
    _check("resize_flow", got, g["resize.out_f64"], dg.resize_flow_torch(fl, (21, 40)))
    assert torch.equal(dg.resize_flow(torch.stack([fl, fl]).to(DEV), (21, 40))[1], got)


def test_lift_tracks_against_the_torch_twin():
    gen = torch.Generator().manual_seed(81)
    T, N, H, W = 3, 65, 9, 12
    depths = 1.0 + torch.rand(T, H, W, generator=gen, dtype=torch.float32)
    xy = torch.rand(T, N, 2, generator=gen, dtype=torch.float32) * torch.tensor([W + 1.0, H + 1.0]) - 1.0
    K = torch.stack([C.pinhole(H, W, k) for k in range(T)])
    w2c = C.f32(torch.stack([C.rigid(C.rotation(0.1 * k, -0.05, 0.02 * k), (0.1, 0.2 * k, 0.3)) for k in range(T)]))
    ref = dg.lift_tracks_torch(xy.double(), depths.double(), K, w2c)
    f32 = dg.lift_tracks_torch(xy, depths, K.float(), w2c.float())
    got = dg.lift_tracks(*_dev(xy, depths, K.float(), w2c.float()))
    assert got.shape == (N, T, 3) and got.is_contiguous()
    _check("lift_tracks", got, ref, f32)
