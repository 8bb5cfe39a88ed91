"""Point tracking on the GPU (include/gs_track.h, csrc/gs_track.hip,
dynamic3dgaussians_amd/tracking.py): the top-K contributor maps against the fp64
replay of the blend chain over the CPU oracle's records (tests/_track_ref.py),
their invariants on every pixel, their agreement with the forward they repeat
(batch / single camera, sync-free / two-phase, tile windows, untouched images),
the track projection against the forward's own means2D / depths, and
track_points + PCK end to end on a scene with known motion.

Scenes (tests/_track_ref.SCENES, tests._harness.scene): P = 2000 at 128 x 96
(tile lists up to 236 entries: several 64-entry chunks and a chunk tail),
P = 2000 seed 3 at 100 x 70 (partial tiles on both edges), P = 800 at
scale_mult 6 (long overlapping lists)."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import dynamic3dgaussians_amd as D
from dynamic3dgaussians_amd import _C
from dynamic3dgaussians_amd.camera import camera_rig, intrinsics, look_at_w2c, setup_camera
from dynamic3dgaussians_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizerBatch
from dynamic3dgaussians_amd.scene import camera_tensors
from tests import _harness as H
from tests import _track_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL_W = 1e-5   # the project's per-pixel image tolerance: w is a term of alpha
CAP = 0.01     # share of a scene's pixels a rank's comparison may exclude (a condition, not a tolerance)


def _rendervar(inp, means=None):
    m = inp["means3D"] if means is None else means
    return dict(means3D=m.to(DEV), colors_precomp=inp["colors"].to(DEV), opacities=inp["opacity"].to(DEV),
                scales=inp["scales"].to(DEV), rotations=inp["rotations"].to(DEV))


def _settings(name, cams, compat="fixed", windows=None):
    kw = R.SCENES[name]
    rig = camera_rig(27, kw["W"], kw["H"])  # tests._harness.scene's cameras
    return [GaussianRasterizationSettings(**camera_tensors(rig[c], DEV), compat=compat,
                                          tile_window=None if windows is None else windows[i])
            for i, c in enumerate(cams)]


@functools.lru_cache(maxsize=None)
def _gpu_state(name, cam):
    """The single-camera HIP forward (fixed mode) of a scene and its exported state."""
    inp = R.scene(name, cam)
    kw = R.SCENES[name]
    fwd = H.gpu_forward(inp, compat="fixed")
    return fwd, H.export_state(kw["P"], kw["W"], kw["H"], fwd)


@functools.lru_cache(maxsize=None)
def _flipped(name, cam):
    """Pixels where the HIP forward's walk ended at another entry than the oracle's (H x W bool)."""
    kw = R.SCENES[name]
    px = H.flipped_pixels(_gpu_state(name, cam)[1], R.oracle(name, cam)[6], kw["W"], kw["H"])
    out = np.zeros(kw["W"] * kw["H"], bool)
    out[px] = True
    return out.reshape(kw["H"], kw["W"])


# ---- 1. ids and weights against the replay

@pytest.mark.parametrize("cams", [(0,), (0, 1, 2)], ids=["single", "batch3"])
@pytest.mark.parametrize("name", list(R.SCENES))
def test_ids_and_weights_match_the_replay(name, cams):
    rv = _rendervar(R.scene(name))
    for compat in ("reference", "fixed"):
        for K in (1, 4):
            top_id, top_w = (t.cpu().numpy() for t in D.contributor_maps(_settings(name, cams, compat), rv, K)[:2])
            assert top_id.shape == top_w.shape == (len(cams), K, R.SCENES[name]["H"], R.SCENES[name]["W"])
            assert top_id.dtype == np.int32 and top_w.dtype == np.float32
            for i, c in enumerate(cams):
                ref_id, ref_w, _, _ = R.reference(name, c)
                same_walk = ~_flipped(name, c)
                for k in range(K):
                    m = R.robust(ref_w, k) & same_walk
                    excluded = 1.0 - m.mean()
                    werr = np.abs(top_w[i, k].astype(np.float64) - ref_w[k])[m].max()
                    print(f"{name} cam {c} {compat} K={K} rank {k}: excluded {100 * excluded:.3f} %, "
                          f"max |w - replay| {werr:.2e}, id mismatches {(top_id[i, k] != ref_id[k])[m].sum()}")
                    assert excluded <= CAP
                    np.testing.assert_array_equal(top_id[i, k][m], ref_id[k][m])
                    assert werr <= TOL_W


# ---- 2. invariants on every pixel

@pytest.mark.parametrize("name", list(R.SCENES))
def test_invariants_on_every_pixel(name):
    """On the single-camera forward's own state (the C = 1 case of the ABI), K = 4, fixed mode."""
    kw = R.SCENES[name]
    inp = R.scene(name)
    fwd, st = _gpu_state(name, 0)
    _, _, _, _, alpha, radii, geom, binning, img = fwd
    d = lambda k: inp[k].to(DEV)  # noqa: E731
    maps = {}
    for K in (1, 2, 3, 4):
        top_id, top_w = _C.rasterize_gaussians_batch_contributors(
            geom, binning, img, [st["num_instances"]], [inp["c_x"]], [inp["c_y"]], [inp["tan_fovx"]],
            [inp["tan_fovy"]], d("bg"), d("viewmatrix"), d("projmatrix"), d("campos"), kw["H"], kw["W"], kw["P"], K,
            compat="fixed")
        assert top_id.shape == top_w.shape == (1, K, kw["H"], kw["W"])
        maps[K] = (top_id[0].cpu().numpy(), top_w[0].cpu().numpy())
    id4, w4 = maps[4]
    for K in (1, 2, 3):  # K = 3 stores the K = 4 kernel's first three ranks, K = 1 / 2 their own kernels': the same ranks
        np.testing.assert_array_equal(maps[K][0], id4[:K])
        np.testing.assert_array_equal(maps[K][1], w4[:K])
    assert (np.diff(w4, axis=0) <= 0).all()                      # non-increasing in k
    assert ((id4 == -1) == (w4 == 0)).all()                      # id -1 <=> w 0
    assert ((id4 >= -1) & (id4 < kw["P"])).all()
    for a in range(4):
        for b in range(a + 1, 4):
            assert not ((id4[a] == id4[b]) & (id4[a] >= 0)).any()  # distinct ids
    n_contrib = st["n_contrib"].reshape(kw["H"], kw["W"])
    assert ((id4[0] == -1) == (n_contrib == 0)).all()
    assert (n_contrib > 0).mean() > 0.3
    r = radii.cpu().numpy()
    assert (r[id4[id4 >= 0]] > 0).all()
    a = alpha[0].cpu().numpy().astype(np.float64)
    assert (w4.astype(np.float64).sum(axis=0) <= a + 1e-5).all()  # fixed mode: alpha is the sum of ALL weights


# ---- 3. one opaque Gaussian alone in view

def test_single_opaque_gaussian():
    """Fixed mode.  With one Gaussian the forward's alpha image is 1 - T = 1 - (1 - w) in fp32,
    which is w itself wherever 1 - w is exact (w >= 0.5, Sterbenz) and w rounded to the spacing of
    1 - w (2^-24) below: top_w[0] must reproduce the alpha image through that very expression,
    bit for bit, on every pixel, and equal it bit for bit where w >= 0.5."""
    W, H_ = 64, 48
    cam = camera_rig(27, W, H_)[0]
    s = [GaussianRasterizationSettings(**camera_tensors(cam, DEV), compat="fixed")]
    rv = dict(means3D=torch.zeros(1, 3, device=DEV), colors_precomp=torch.full((1, 3), 0.5, device=DEV),
              opacities=torch.full((1, 1), 0.99, device=DEV), scales=torch.full((1, 3), 0.25, device=DEV),
              rotations=torch.tensor([[1.0, 0.0, 0.0, 0.0]], device=DEV))
    top_id, top_w, _, _, alpha = D.contributor_maps(s, rv, K=2)
    top_id, top_w, alpha = top_id[0].cpu().numpy(), top_w[0].cpu().numpy(), alpha[0, 0].cpu().numpy()
    hit = alpha > 0
    assert 0.2 < hit.mean() < 1.0 and (top_w[0] >= 0.5).sum() > 50 and ((top_w[0] > 0) & (top_w[0] < 0.5)).sum() > 50
    np.testing.assert_array_equal(top_id[0], np.where(hit, 0, -1))
    assert (top_id[1] == -1).all() and (top_w[1] == 0).all()
    one = np.float32(1.0)
    np.testing.assert_array_equal((one - (one - top_w[0])).view(np.uint32), alpha.view(np.uint32))
    big = top_w[0] >= 0.5
    np.testing.assert_array_equal(top_w[0][big].view(np.uint32), alpha[big].view(np.uint32))
    assert np.abs(top_w[0].astype(np.float64) - alpha).max() <= 2.0 ** -25


# ---- 4. batch against single camera, reruns

def test_batch_equals_single_camera_and_reruns_are_identical():
    name, cams = "edges", (0, 1, 2)
    rv = _rendervar(R.scene(name))
    batch = D.contributor_maps(_settings(name, cams), rv, 4)
    again = D.contributor_maps(_settings(name, cams), rv, 4)
    for a, b in zip(batch, again):
        assert torch.equal(a, b)
    for i, c in enumerate(cams):
        single = D.contributor_maps(_settings(name, (c,)), rv, 4)
        for a, b in zip(batch, single):
            assert torch.equal(a[i], b[0])


# ---- 5. sync-free forward

def test_sync_free_forward_gives_the_same_maps():
    name, cams = "long", (0, 1, 2)
    rv = _rendervar(R.scene(name))
    s = _settings(name, cams)
    two_phase = D.contributor_maps(s, rv, 4)
    plan = _C.BinningPlan()
    first = D.contributor_maps(s, rv, 4, plan_state=plan)    # no capacity yet: the retry with the exact lengths
    second = D.contributor_maps(s, rv, 4, plan_state=plan)   # the sized buffer: one sync-free pass
    assert plan.calls == 2
    for a, b, c in zip(two_phase, first, second):
        assert torch.equal(a, b) and torch.equal(a, c)


# ---- 6. tile windows

def test_tile_windows():
    name, cams = "p2000", (0, 1, 2)
    kw = R.SCENES[name]
    rv = _rendervar(R.scene(name))
    windows = [(1, 1, 5, 4), (0, 0, 3, 6), None]  # tiles [x0, x1) x [y0, y1) of the 8 x 6 grid
    full = D.contributor_maps(_settings(name, cams), rv, 4)
    part = D.contributor_maps(_settings(name, cams, windows=windows), rv, 4)
    for i, w in enumerate(windows):
        inside = torch.zeros(kw["H"], kw["W"], dtype=torch.bool, device=DEV)
        if w is None:
            inside[:] = True
        else:
            inside[16 * w[1]:16 * w[3], 16 * w[0]:16 * w[2]] = True
        assert inside.any() and (w is None or not inside.all())
        assert (part[0][i][:, ~inside] == -1).all() and (part[1][i][:, ~inside] == 0).all()
        assert torch.equal(part[0][i][:, inside], full[0][i][:, inside])
        assert torch.equal(part[1][i][:, inside], full[1][i][:, inside])


# ---- 7. the forward's images are undisturbed

@pytest.mark.parametrize("compat", ["reference", "fixed"])
def test_images_equal_the_batch_rasterizers(compat):
    name, cams = "p2000", (0, 1, 2)
    rv = _rendervar(R.scene(name))
    s = _settings(name, cams, compat)
    _, _, color, depth, alpha = D.contributor_maps(s, rv, 2)
    with torch.no_grad():
        c2, _, d2, a2 = GaussianRasterizerBatch(s)(**rv, means2D=torch.zeros_like(rv["means3D"]), label=None)
    assert torch.equal(color, c2) and torch.equal(depth, d2) and torch.equal(alpha, a2)


# ---- 8. project_tracks

def test_project_tracks_equals_the_forwards_means2d_and_depths():
    name, cams = "p2000", (0, 1, 2)
    kw = R.SCENES[name]
    P = kw["P"]
    base = R.scene(name)["means3D"]
    rig = camera_rig(27, kw["W"], kw["H"])
    ang = np.radians(10.0)
    rot = torch.tensor([[np.cos(ang), 0.0, np.sin(ang)], [0.0, 1.0, 0.0], [-np.sin(ang), 0.0, np.cos(ang)]],
                       dtype=torch.float32)
    # a rigid motion per step, rendered below; a fourth set, projected only, carries the scene onto
    # camera 0: half of it behind that camera
    seq = torch.stack([base, base @ rot.T + torch.tensor([0.05, -0.02, 0.03]),
                       base @ rot.T @ rot.T + torch.tensor([0.1, -0.04, 0.06]),
                       base + torch.from_numpy(rig[0].campos.copy())]).contiguous()
    ids = torch.cat([torch.arange(P), torch.tensor([-1, -7, P + 5])]).int()  # every Gaussian, none, none, past the end
    uv, depth, inside = (t.cpu().numpy() for t in D.project_tracks(seq.to(DEV), ids.to(DEV), _settings(name, cams)))
    assert uv.shape == (4, 3, P + 3, 2) and depth.shape == inside.shape == (4, 3, P + 3)
    seen = 0
    for t in range(3):
        for i, c in enumerate(cams):
            inp = dict(R.scene(name, c), means3D=seq[t])
            fwd = H.gpu_forward(inp, compat="fixed")
            st = H.export_state(P, kw["W"], kw["H"], fwd)
            vis = fwd[5].cpu().numpy() > 0
            seen += int(vis.sum())
            np.testing.assert_array_equal(uv[t, i, :P][vis].view(np.uint32), st["means2D"][vis].view(np.uint32))
            np.testing.assert_array_equal(depth[t, i, :P][vis].view(np.uint32), st["depths"][vis].view(np.uint32))
            assert inside[t, i, :P][vis & _in_image(st["means2D"], kw)].all()
    assert seen > 9 * 500
    behind = depth[..., :P] <= 0
    assert behind[3, 0].sum() > 200 and not inside[..., :P][behind].any()
    assert not inside[..., P:].any()
    assert (uv[..., P:P + 2, :] == 0).all() and (depth[..., P:P + 2] == 0).all()
    # an id past the end reads the last Gaussian and is flagged outside
    np.testing.assert_array_equal(uv[..., P + 2, :], uv[..., P - 1, :])
    ru, rv_ = np.floor(uv[..., 0] + 0.5), np.floor(uv[..., 1] + 0.5)
    want = (depth > 0) & (ru >= 0) & (ru < kw["W"]) & (rv_ >= 0) & (rv_ < kw["H"])
    np.testing.assert_array_equal(inside[..., :P], want[..., :P])


def _in_image(m2, kw):
    ru, rv = np.floor(m2[:, 0] + 0.5), np.floor(m2[:, 1] + 0.5)
    return (ru >= 0) & (ru < kw["W"]) & (rv >= 0) & (rv < kw["H"])


# ---- 9. end to end

def _project64(cam, p, W, H_):
    ph = np.concatenate([p, np.ones((len(p), 1))], 1) @ cam.projmatrix.astype(np.float64)
    ndc = ph[:, :2] / (ph[:, 3:4] + 1e-7)
    z = (np.concatenate([p, np.ones((len(p), 1))], 1) @ cam.viewmatrix.astype(np.float64))[:, 2]
    return np.stack([((ndc[:, 0] + 1) * W - 1) * 0.5, ((ndc[:, 1] + 1) * H_ - 1) * 0.5], 1), z


def test_track_points_end_to_end():
    """300 Gaussians: 280 small ones in a ball at the origin and 20 large opaque ones on the plane
    z = 1 between them and three cameras near (0, -0.5, 2.5); the front ones move by a known
    translation per frame over T = 4.  No front Gaussian reaches another's centre (22 px apart,
    radius 7 px) and nothing is nearer to any camera, so each is the largest contributor at its
    own centre in every camera and frame."""
    W, H_, T = 128, 96, 4
    cams = [setup_camera(W, H_, intrinsics(W, H_, 60.0), look_at_w2c(np.array([0.3 * c - 0.3, -0.5, 2.5])))
            for c in range(3)]
    settings = [GaussianRasterizationSettings(**camera_tensors(c, DEV), compat="fixed") for c in cams]
    g = torch.Generator().manual_seed(11)
    n_bg, n_fr = 280, 20
    gx, gy = torch.meshgrid(torch.arange(5) - 2.0, torch.arange(4) - 1.5, indexing="ij")
    front = torch.stack([0.3 * gx.reshape(-1), 0.3 * gy.reshape(-1), torch.ones(n_fr)], 1)
    means0 = torch.cat([(torch.rand(n_bg, 3, generator=g) * 2 - 1) * 0.4, front])
    scales = torch.cat([torch.full((n_bg, 3), 0.015), torch.full((n_fr, 3), 0.03)])
    opac = torch.cat([torch.rand(n_bg, 1, generator=g) * 0.5 + 0.2, torch.full((n_fr, 1), 0.99)])
    rots = torch.tensor([[1.0, 0.0, 0.0, 0.0]]).repeat(n_bg + n_fr, 1)
    cols = torch.rand(n_bg + n_fr, 3, generator=g)
    step = torch.tensor([0.05, -0.02, 0.0])  # right and down the image: 3.7 and 1.5 px per frame
    seq = []
    for t in range(T):
        m = means0.clone()
        m[n_bg:] += t * step
        seq.append(dict(means3D=m.to(DEV), colors_precomp=cols.to(DEV), opacities=opac.to(DEV),
                        scales=scales.to(DEV), rotations=rots.to(DEV)))
    q, _ = _project64(cams[0], front.double().numpy(), W, H_)
    queries = np.concatenate([q, [[2.0, 2.0]]]).astype(np.float32)  # the last: empty background, a corner
    tr = D.track_points(seq, settings, torch.from_numpy(queries), 0, query_t=0, K=1)
    ids = tr.ids.cpu().numpy()
    np.testing.assert_array_equal(ids[:n_fr], n_bg + np.arange(n_fr))
    assert ids[n_fr] == -1 and not tr.visible[:, :, n_fr].any() and not tr.inside[:, :, n_fr].any()
    assert tr.uv.shape == (T, 3, n_fr + 1, 2) and tr.visible.dtype == torch.bool
    pck = D.PCK()
    for t in range(T):
        for c in range(3):
            want, z = _project64(cams[c], (front + t * step).double().numpy(), W, H_)
            got = tr.uv[t, c, :n_fr].cpu().numpy().astype(np.float64)
            assert np.abs(got - want).max() <= 1e-3
            np.testing.assert_allclose(tr.depth[t, c, :n_fr].cpu().numpy(), z, rtol=1e-5)
            in_front = (z > 0) & (np.floor(want[:, 0] + 0.5) >= 0) & (np.floor(want[:, 0] + 0.5) < W) & \
                (np.floor(want[:, 1] + 0.5) >= 0) & (np.floor(want[:, 1] + 0.5) < H_)
            assert in_front.all()  # the scene keeps every front Gaussian in view and in front
            np.testing.assert_array_equal(tr.visible[t, c, :n_fr].cpu().numpy(), in_front)
            pck.update(tr.uv[t, c, :n_fr], torch.from_numpy(want).float().to(DEV), 0.5, visible=tr.visible[t, c, :n_fr])
    assert len(pck) == 3 * T and pck.compute() == 1.0
    # the same sequence as a callable, and K = 2: the same tracks
    tr2 = D.track_points(lambda t: seq[t], settings, torch.from_numpy(queries), 0, K=2, num_timesteps=T)
    assert torch.equal(tr2.ids, tr.ids) and torch.equal(tr2.uv, tr.uv) and torch.equal(tr2.visible, tr.visible)
