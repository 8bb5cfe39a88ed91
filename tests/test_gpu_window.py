"""Temporal-window camera batches (include/gs_window.h,
GaussianRasterizerBatch(camera_frames=...)): the cameras of B frames of a
motion model in ONE batch call over means3D (P, B, 3), against the reference
formulation -- for each distinct frame b in order one GaussianRasterizerBatch
over that frame's cameras on positions[:, b].contiguous(), autograd summing
the shared parameters.

Forward: every camera's outputs are bit-identical (the per-camera arithmetic
is the same, only the address of the mean differs).  Backward: every gradient
within 1e-5 relative L2 (tests/test_gpu_batch.py's bound for the same kind of
reordered camera sum); positions.grad[:, b] of a frame no camera uses and the
rows with label == 0 are exactly zero."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from dynamic3dgaussians_amd import MotionBases
from dynamic3dgaussians_amd.camera import camera_rig
from dynamic3dgaussians_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizerBatch
from dynamic3dgaussians_amd.scene import make_gaussians

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
TOL = 1e-5
OUT_NAMES = ("color", "radii", "features", "depth", "alpha")


def _settings(cams, W, H, compat, sh_degree=0):
    bg = torch.tensor([0.1, 0.2, 0.3], device=DEV)
    return [GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=c.tanfovx, tanfovy=c.tanfovy, c_x=c.c_x, c_y=c.c_y, bg=bg,
        viewmatrix=torch.from_numpy(c.viewmatrix.copy()).to(DEV),
        projmatrix=torch.from_numpy(c.projmatrix.copy()).to(DEV), sh_degree=sh_degree,
        campos=torch.from_numpy(c.campos.copy()).to(DEV), compat=compat) for c in cams]


def _scene(P, F, use_sh, B, seed=0, raw=False):
    """The shared parameters and the (P, B, 3) means: frame b = the base means
    moved by its own small random offsets."""
    g = make_gaussians(P, F=F, seed=seed, device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(seed + 11)
    src = dict(opacities=g["opacities"], scales=g["scales"], rotations=g["rotations"])
    if raw:  # logit_opacities, log_scales, unnorm_rotations (helpers.py:98-107)
        src = dict(opacities=torch.logit(g["opacities"]), scales=g["scales"].log(), rotations=g["rotations"] * 1.7)
    if F:
        src["semantic_feature"] = g["semantic_feature"]
    if use_sh:
        src["shs"] = torch.randn(P, 16, 3, device=DEV, generator=gen) * 0.2
    else:
        src["colors_precomp"] = g["colors"]
    positions = (g["means3D"][:, None, :] + 0.04 * torch.randn(P, B, 3, device=DEV, generator=gen)).contiguous()
    return src, positions


def _ups(C, F, W, H, seed=3):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    ups = dict(color=torch.randn(C, 3, H, W, device=DEV, generator=gen),
               depth=torch.randn(C, 1, H, W, device=DEV, generator=gen),
               alpha=torch.randn(C, 1, H, W, device=DEV, generator=gen))
    if F:
        ups["features"] = torch.randn(C, F, H, W, device=DEV, generator=gen)
    return ups


def _rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _call(ras, positions, leaves, label, m2, has_feat, **kw):
    out = ras(means3D=positions, means2D=m2, label=label, **leaves, **kw)
    if has_feat:
        im, radii, feat, depth, alpha = out
    else:
        im, radii, depth, alpha = out
        feat = None
    return dict(color=im, radii=radii, features=feat, depth=depth, alpha=alpha)


def _backward(out, ups, idx=None):
    names = [k for k in ("color", "depth", "alpha", "features") if k in ups and out[k] is not None]
    torch.autograd.backward([out[k] for k in names], [ups[k] if idx is None else ups[k][idx] for k in names])


def _detach(out):
    return {k: (None if v is None else v.detach().clone()) for k, v in out.items()}


def _grads(leaves, positions, m2):
    g = {k: v.grad.detach().clone() for k, v in leaves.items()}
    g["means3D"] = positions.grad.detach().clone()
    g["means2D"] = m2.grad.detach().clone()
    return g


def run_reference(src, positions, sets, frames, ups, label, **ras_kw):
    """The reference formulation: one batch per distinct frame, in order, on
    positions[:, b].contiguous(); autograd sums.  Returns the outputs in
    camera order, the gradients (means3D: (P, B, 3)) and the rasterizers."""
    P = positions.shape[0]
    leaves = {k: v.clone().requires_grad_(True) for k, v in src.items()}
    pos = positions.clone().requires_grad_(True)
    m2 = torch.zeros(P, 3, device=DEV, requires_grad=True)
    outs, rasters = {}, []
    for b in sorted(set(frames)):
        idx = [c for c, f in enumerate(frames) if f == b]
        ras = GaussianRasterizerBatch([sets[c] for c in idx], **ras_kw)
        out = _call(ras, pos[:, b].contiguous(), leaves, label, m2, "semantic_feature" in src)
        _backward(out, ups, idx)
        rasters.append(ras)
        for j, c in enumerate(idx):
            outs[c] = {k: (None if v is None else v[j].detach().clone()) for k, v in out.items()}
    return [outs[c] for c in range(len(frames))], _grads(leaves, pos, m2), rasters


def run_window(src, positions, sets, frames, ups, label, ras=None, call_kw=None, **ras_kw):
    P = positions.shape[0]
    leaves = {k: v.clone().requires_grad_(True) for k, v in src.items()}
    pos = positions.clone().requires_grad_(True)
    m2 = torch.zeros(P, 3, device=DEV, requires_grad=True)
    ras = GaussianRasterizerBatch(sets, camera_frames=frames, **ras_kw) if ras is None else ras
    out = _call(ras, pos, leaves, label, m2, "semantic_feature" in src, **(call_kw or {}))
    _backward(out, ups)
    if call_kw and "means3D" in call_kw.get("grad_into", {}):
        assert pos.grad is None  # written into the caller's destination: autograd got None
        pos.grad = torch.zeros_like(pos)
    return _detach(out), _grads(leaves, pos, m2), ras


def check_forward(out, ref_outs):
    for c, ref in enumerate(ref_outs):
        for k in OUT_NAMES:
            if ref[k] is not None:
                assert torch.equal(out[k][c], ref[k]), (c, k)


def check_grads(grads, ref_grads, frames, B, label=None, tol=TOL):
    rels = {k: _rel(grads[k], ref_grads[k]) for k in ref_grads}
    print("relative L2 of the gradients:", {k: f"{v:.2e}" for k, v in rels.items()})
    assert grads["means3D"].shape == ref_grads["means3D"].shape and grads["means3D"].shape[1] == B
    for k, r in rels.items():
        assert r <= tol, (k, r)
    for b in range(B):
        r = _rel(grads["means3D"][:, b], ref_grads["means3D"][:, b])
        if b in frames:
            assert r <= tol, (b, r)
        else:  # a frame no camera uses
            assert torch.all(grads["means3D"][:, b] == 0), b
    if label is not None:
        off = label == 0
        for k in grads:
            if k not in ("means2D", "semantic_feature"):  # Q12: those two are not masked
                assert torch.all(grads[k][off] == 0), k


def _label(P, seed=5):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.rand(P, device=DEV, generator=gen) > 0.25).float()


# ---- cases 1 and 2: an unused frame, an odd C (the last PB_GROUP is short), a group of two cameras that
# straddles the frame change (cameras 2 | 3), P no multiple of the 256-thread workgroup

CASE1 = dict(P=3001, B=3, frames=[0, 0, 0, 2, 2], W=128, H=96)


@functools.lru_cache(maxsize=None)
def _case(W, H, F, frames):
    """Case 1's scene at an image size, feature width and frame tuple (B = 3): the inputs and the
    reference formulation, computed once and shared (read-only)."""
    P, B = CASE1["P"], CASE1["B"]
    src, positions = _scene(P, F, False, B, seed=1)
    sets = _settings(camera_rig(len(frames), W, H), W, H, "reference")
    ups, label = _ups(len(frames), F, W, H), _label(P)
    ref_outs, ref_grads, _ = run_reference(src, positions, sets, frames, ups, label)
    return src, positions, sets, frames, ups, label, ref_outs, ref_grads


def _case1():
    return _case(CASE1["W"], CASE1["H"], 32, tuple(CASE1["frames"]))


def test_window_matches_per_frame_batches_precomputed_colours():
    src, positions, sets, frames, ups, label, ref_outs, ref_grads = _case1()
    out, grads, _ = run_window(src, positions, sets, frames, ups, label)
    assert out["color"].shape == (5, 3, CASE1["H"], CASE1["W"]) and out["radii"].shape == (5, CASE1["P"])
    check_forward(out, ref_outs)
    check_grads(grads, ref_grads, frames, CASE1["B"], label)


def test_window_matches_per_frame_batches_sh_fixed():
    """SH degree 3, F = 8, compat "fixed": the shared dsh / sh_written run across the frame boundary."""
    P, B, frames, W, H = 3001, 3, [0, 0, 0, 2, 2], 128, 96
    src, positions = _scene(P, 8, True, B, seed=2)
    sets = _settings(camera_rig(len(frames), W, H), W, H, "fixed", sh_degree=3)
    ups, label = _ups(len(frames), 8, W, H), _label(P)
    ref_outs, ref_grads, _ = run_reference(src, positions, sets, frames, ups, label)
    out, grads, _ = run_window(src, positions, sets, frames, ups, label)
    check_forward(out, ref_outs)
    check_grads(grads, ref_grads, frames, B, label)


def test_visibility_differs_per_frame():
    """Frame 1 has half of the Gaussians behind every camera (pv.z <= 0), frame 0 a disjoint quarter: a row
    unseen in one frame has a zero mean gradient there and a non-zero one in the other; the scale and
    rotation gradients (summed over both frames) match the reference formulation."""
    P, B, frames, W, H = 4000, 2, [0, 0, 1, 1], 128, 96
    src, positions = _scene(P, 0, False, B, seed=3)
    rig = camera_rig(len(frames), W, H)
    sets = _settings(rig, W, H, "reference")
    behind = torch.tensor([0.0, -40.0, 0.0], device=DEV)  # under the dome: behind every camera looking at the origin
    half, quarter = slice(0, P // 2), slice(P // 2, P // 2 + P // 4)
    positions = positions.clone()
    positions[half, 1] = behind + positions[half, 1] * 0.01
    positions[quarter, 0] = behind + positions[quarter, 0] * 0.01
    ups = _ups(len(frames), 0, W, H)
    ref_outs, ref_grads, _ = run_reference(src, positions, sets, frames, ups, None)
    out, grads, _ = run_window(src, positions, sets, frames, ups, None)
    assert torch.all(out["radii"][2:, half] == 0) and torch.all(out["radii"][:2, quarter] == 0)
    check_forward(out, ref_outs)
    check_grads(grads, ref_grads, frames, B)
    gm = grads["means3D"]
    assert torch.all(gm[half, 1] == 0) and torch.all(gm[quarter, 0] == 0)
    seen0 = (out["radii"][:2, half] > 0).any(0)   # rows of `half` that frame 0's cameras see
    seen1 = (out["radii"][2:, quarter] > 0).any(0)
    assert seen0.sum() > 100 and seen1.sum() > 100
    assert (gm[half, 0][seen0].abs().sum(1) > 0).float().mean() > 0.9
    assert (gm[quarter, 1][seen1].abs().sum(1) > 0).float().mean() > 0.9
    for k in ("scales", "rotations"):
        assert _rel(grads[k], ref_grads[k]) <= TOL, k


def test_window_of_two_blend_camera_groups():
    """C = 11 over four frames: the blend launches' two camera groups (8 + 3), frames of 3, 4, 1 and 3 cameras."""
    P, B, frames, W, H = 9000, 4, [0, 0, 0, 1, 1, 1, 1, 2, 3, 3, 3], 112, 96
    src, positions = _scene(P, 32, False, B, seed=4)
    sets = _settings(camera_rig(len(frames), W, H), W, H, "reference")
    ups, label = _ups(len(frames), 32, W, H), _label(P)
    ref_outs, ref_grads, _ = run_reference(src, positions, sets, frames, ups, label)
    out, grads, _ = run_window(src, positions, sets, frames, ups, label)
    check_forward(out, ref_outs)
    check_grads(grads, ref_grads, frames, B, label)


def test_raw_params_and_densify_statistics():
    """raw_params=True and track_densify=True: the gradients of the raw parameters match the reference
    formulation, and the statistics are the sum over all cameras of all frames -- the per-frame batches'
    statistics added (denom, exactly), maximised (max_2D_radius, exactly) and added (the gradient norms,
    1e-5)."""
    P, B, frames, W, H = 3001, 3, [0, 0, 0, 2, 2], 128, 96
    src, positions = _scene(P, 8, False, B, seed=7, raw=True)
    sets = _settings(camera_rig(len(frames), W, H), W, H, "reference")
    ups, label = _ups(len(frames), 8, W, H), _label(P)
    kw = dict(raw_params=True, track_densify=True)
    ref_outs, ref_grads, rasters = run_reference(src, positions, sets, frames, ups, label, **kw)
    out, grads, ras = run_window(src, positions, sets, frames, ups, label, **kw)
    check_forward(out, ref_outs)
    check_grads(grads, ref_grads, frames, B, label)
    st = ras.densify_stats
    den = sum(r.densify_stats["denom"] for r in rasters)
    acc = sum(r.densify_stats["means2D_gradient_accum"] for r in rasters)
    rad = functools.reduce(torch.maximum, [r.densify_stats["max_2D_radius"] for r in rasters])
    assert den.max() >= 4  # some Gaussian is seen from both frames
    assert torch.equal(st["denom"], den) and torch.equal(st["max_2D_radius"], rad)
    assert _rel(st["means2D_gradient_accum"], acc) <= TOL


# ---- cases 5 and 7: pairs of runs that must give the same bits
#
# Every gradient starts in the backward blend, where each wave that blends a Gaussian in its 8 x 8 pixel
# strip adds its sums to the Gaussian's record of that camera (and its feature gradient to the one row
# all cameras share) with float atomics, in whatever order the waves get there; preprocess_bwd, the only
# backward code a window changes, then reads the records and is deterministic.  Float addition is
# commutative but not associative: with three or more addends the order shows in the last bits.  At
# 128 x 96 two runs of the SAME call therefore differ (measured on an MI355X, P = 3001, 5 cameras, F = 32:
# 99-742 of the 3001-27009 elements of each gradient, 34k-37k of the 96032 feature gradients, relative L2
# below 4e-7; bench.py dump_outputs says the same of its gradients), with a window or without, so no
# comparison of gradient bits can hold there.  The gradients' bits are compared where the blend's sums
# have at most two addends and so one possible value: an 8 x 8 image is a single strip, so a record gets
# one wave's sum per camera (the tile's three strips outside the image add zeros), and a feature row gets
# one per camera -- F = 0 with the five cameras of case 1, F = 32 with two cameras, one per used frame.
# preprocess_bwd works per Gaussian whatever the image size: the same 3001 Gaussians in 12 workgroups,
# the same frame changes.  The forward outputs are compared at 128 x 96.

RENDER = (CASE1["W"], CASE1["H"], 32, tuple(CASE1["frames"]))
SINGLE_STRIP = [(8, 8, 0, tuple(CASE1["frames"])), (8, 8, 32, (0, 2))]


def _pair_one_frame(W, H, F, frames):
    """B = 1, camera_frames = [0] * C on means3D.unsqueeze(1) against camera_frames=None on means3D."""
    P, C = CASE1["P"], len(frames)
    src, positions = _scene(P, F, False, 1, seed=6)
    sets = _settings(camera_rig(C, W, H), W, H, "reference")
    ups, label = _ups(C, F, W, H), _label(P)
    out, grads, _ = run_window(src, positions, sets, [0] * C, ups, label, sync_free=False)
    leaves = {k: v.clone().requires_grad_(True) for k, v in src.items()}
    means = positions[:, 0].clone().requires_grad_(True)
    m2 = torch.zeros(P, 3, device=DEV, requires_grad=True)
    plain = _call(GaussianRasterizerBatch(sets, sync_free=False), means, leaves, label, m2, F > 0)
    _backward(plain, ups)
    assert grads["means3D"].shape == (P, 1, 3)
    plain_grads = _grads(leaves, means, m2)
    plain_grads["means3D"] = plain_grads["means3D"].unsqueeze(1)
    return (out, grads), (_detach(plain), plain_grads)


def _pair_sync_free(*size):
    src, positions, sets, frames, ups, label, ref_outs, _ = _case(*size)
    a = run_window(src, positions, sets, frames, ups, label, sync_free=True)
    b = run_window(src, positions, sets, frames, ups, label, sync_free=False)
    assert a[2].plan is not None and b[2].plan is None
    check_forward(a[0], ref_outs)
    return a[:2], b[:2]


def _pair_spatial_order(*size):
    src, positions, sets, frames, ups, label, ref_outs, _ = _case(*size)
    a = run_window(src, positions, sets, frames, ups, label, spatial_order=True)
    b = run_window(src, positions, sets, frames, ups, label, spatial_order=False)
    assert a[2]._walk is not None and a[2]._walk.shape == (CASE1["P"],) and b[2]._walk is None
    check_forward(a[0], ref_outs)
    return a[:2], b[:2]


def _pair_hinted(*size):
    """A second sync-free call on the same rasterizer against the first: the first has no capacity and
    retries with the exact lengths; the second is sized and hinted from it and must have fitted
    (tests/test_gpu_sync_free.py reads the same counters)."""
    src, positions, sets, frames, ups, label, ref_outs, _ = _case(*size)
    first_out, first_grads, ras = run_window(src, positions, sets, frames, ups, label, sync_free=True)
    assert ras.plan.calls == 1 and ras.plan.hint[0] == 1
    second = run_window(src, positions, sets, frames, ups, label, ras=ras)[:2]
    assert ras.plan.calls == 2 and ras.plan.retries == 0, (ras.plan.calls, ras.plan.retries)
    assert all(c >= n for c, n in zip(ras.plan.capacity, ras.plan.num_instances))
    check_forward(second[0], ref_outs)
    return second, (first_out, first_grads)


PAIRS = dict(one_frame=_pair_one_frame, sync_free=_pair_sync_free, spatial_order=_pair_spatial_order,
             hinted=_pair_hinted)


@functools.lru_cache(maxsize=None)
def _pair(kind, size):
    return PAIRS[kind](*size)


@pytest.mark.parametrize("kind", list(PAIRS))
def test_outputs_are_bit_identical(kind):
    """Colour, features, depth, alpha and radii of both runs of the pair are the same bits, the pair's path
    indicators hold (two-phase / sync-free plan, Morton walk, the hinted call fitted) and the gradients
    agree within the reordered-sum bound."""
    (out_a, grads_a), (out_b, grads_b) = _pair(kind, RENDER)
    for k in OUT_NAMES:
        assert torch.equal(out_a[k], out_b[k]), k
    for k in grads_b:
        assert _rel(grads_a[k], grads_b[k]) <= TOL, (k, _rel(grads_a[k], grads_b[k]))


@pytest.mark.parametrize("kind", list(PAIRS))
def test_gradients_are_bit_identical(kind):
    """Every output and every gradient of both runs of the pair is the same bits, at the sizes where the
    blend's atomic sums have one possible value (the note above); most Gaussians get a gradient there."""
    for size in SINGLE_STRIP:
        (out_a, grads_a), (out_b, grads_b) = _pair(kind, size)
        for k in OUT_NAMES:
            if out_b[k] is not None:
                assert torch.equal(out_a[k], out_b[k]), (size, k)
        diff = {k: int((grads_a[k] != grads_b[k]).sum()) for k in grads_b}
        rows = {k: int((grads_b[k].reshape(grads_b[k].shape[0], -1) != 0).any(1).sum()) for k in grads_b}
        print(f"{kind} {size}: gradient elements that differ:", diff, "rows with a gradient:", rows)
        assert set(grads_b) >= {"means3D", "means2D", "opacities", "scales", "rotations", "colors_precomp"}
        for k, n in diff.items():
            assert rows[k] >= 100, (size, k, rows[k])
            assert n == 0, (kind, size, k, n)


def test_grad_into_takes_the_window_shaped_mean_gradient():
    """grad_into={"means3D": buf} with a (P, B, 3) destination holds the gradient the call otherwise returns:
    against the returned gradient of a second, identical call and against the reference formulation within
    the backward's 1e-5 bound at 128 x 96 (two runs differ there in the last bits by the blend's atomic
    order), bit for bit at the single-strip size; the unused frame and the masked rows exactly zero."""
    src, positions, sets, frames, ups, label, _, ref_grads = _case1()
    P, B = CASE1["P"], CASE1["B"]
    buf = torch.full((P, B, 3), float("nan"), device=DEV)
    run_window(src, positions, sets, frames, ups, label, call_kw=dict(grad_into={"means3D": buf}))
    _, returned, _ = run_window(src, positions, sets, frames, ups, label)
    print("grad_into vs returned: elements that differ:", int((buf != returned["means3D"]).sum()),
          "relative L2:", _rel(buf, returned["means3D"]))
    assert torch.isfinite(buf).all()  # every element was written
    assert _rel(buf, returned["means3D"]) <= TOL and _rel(buf, ref_grads["means3D"]) <= TOL
    assert torch.all(buf[:, 1] == 0) and torch.all(buf[label == 0] == 0)
    # and the same bits where two runs have the same bits (the note above cases 5 and 7)
    src1, pos1, sets1, frames1, ups1, label1, _, _ = _case(*SINGLE_STRIP[0])
    buf1 = torch.full((P, B, 3), float("nan"), device=DEV)
    run_window(src1, pos1, sets1, frames1, ups1, label1, call_kw=dict(grad_into={"means3D": buf1}))
    _, returned1, _ = run_window(src1, pos1, sets1, frames1, ups1, label1)
    assert (buf1 != 0).any(1).any(1).sum() >= 100 and torch.equal(buf1, returned1["means3D"])
    with pytest.raises(Exception, match="dmeans3D"):  # a (P, 3) destination is not the window's gradient
        run_window(src, positions, sets, frames, ups, label,
                   call_kw=dict(grad_into={"means3D": torch.empty(P, 3, device=DEV)}))


# ---- case 9: the CPU oracle as an anchor outside the package

def test_window_against_the_cpu_oracle():
    """B = 2, one camera per frame: each camera's image against oracle_forward on that frame's means at the
    SURVEY 8(c) tolerance of tests/test_gpu_parity.py (>= 99.9 % of pixels within 1e-5), and
    positions.grad[:, b] against oracle_backward's dL_dmeans3D for that camera within 1e-4 relative L2."""
    from tests import _harness as Hh
    P, W, H = 2000, 128, 96
    inps = [Hh.scene(P=P, F=0, W=W, H=H, cam_index=i) for i in (0, 5)]
    gen = torch.Generator().manual_seed(17)
    positions = torch.stack([inps[0]["means3D"], inps[0]["means3D"] + 0.04 * torch.randn(P, 3, generator=gen)], 1)
    sets = [GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=i["tan_fovx"], tanfovy=i["tan_fovy"], c_x=i["c_x"], c_y=i["c_y"],
        bg=i["bg"].to(DEV), viewmatrix=i["viewmatrix"].to(DEV), projmatrix=i["projmatrix"].to(DEV), sh_degree=0,
        campos=i["campos"].to(DEV), compat="reference") for i in inps]
    ups4 = [Hh.upstream_grads(H, W, 0, seed=1 + b) for b in range(2)]
    pos = positions.to(DEV).contiguous().requires_grad_(True)
    g = inps[0]
    im, radii, depth, alpha = GaussianRasterizerBatch(sets, camera_frames=[0, 1])(
        means3D=pos, means2D=torch.zeros(P, 3, device=DEV, requires_grad=True), opacities=g["opacity"].to(DEV),
        colors_precomp=g["colors"].to(DEV), scales=g["scales"].to(DEV), rotations=g["rotations"].to(DEV),
        label=torch.ones(P, device=DEV))
    torch.autograd.backward([im, depth, alpha], [torch.stack([u[0] for u in ups4]).to(DEV),
                                                 torch.stack([u[2] for u in ups4]).to(DEV),
                                                 torch.stack([u[3] for u in ups4]).to(DEV)])
    for b in range(2):
        inp = dict(inps[b], means3D=positions[:, b].contiguous())
        o = Hh.oracle_forward(inp)
        co, do = np.asarray(o[1]), np.asarray(o[3])
        cg, dg = im[b].detach().cpu().numpy(), depth[b].detach().cpu().numpy()
        np.testing.assert_array_equal(radii[b].cpu().numpy(), o[5])
        fc = np.mean(np.abs(cg - co) <= 1e-5)
        fd = np.mean(np.abs(dg - do) <= 1e-5 * max(1.0, np.abs(do).max()))
        ob = Hh.oracle_backward(inp, o, ups4[b])
        r = Hh.rel_l2(pos.grad[:, b].cpu().numpy(), np.asarray(ob[4]))
        print(f"frame {b}: colour within 1e-5 {fc:.5f}, depth {fd:.5f}, dL_dmeans3D rel L2 {r:.2e}")
        assert fc >= 0.999 and fd >= 0.999
        assert r <= 1e-4, (b, r)


# ---- case 10: end to end with the motion model

def test_motion_bases_through_a_window():
    """compute_means (K = 10, B = 3, softmax) -> the windowed batch (2 cameras per frame) -> backward: the
    gradients of means, coefs, rots and transls against the same chain through the reference formulation."""
    P, K, T, ts, frames, W, H = 3001, 10, 5, [0, 2, 4], [0, 0, 1, 1, 2, 2], 128, 96
    src, _ = _scene(P, 8, False, 1, seed=8)
    base = make_gaussians(P, seed=8, device=DEV)["means3D"]
    gen = torch.Generator(device=DEV).manual_seed(23)
    ident = torch.tensor([1.0, 0, 0, 0, 1.0, 0], device=DEV)
    rots0 = ident + 0.05 * torch.randn(K, T, 6, device=DEV, generator=gen)
    transls0 = 0.05 * torch.randn(K, T, 3, device=DEV, generator=gen)
    coefs0 = torch.randn(P, K, device=DEV, generator=gen)
    sets = _settings(camera_rig(len(frames), W, H), W, H, "reference")
    ups, label = _ups(len(frames), 8, W, H), _label(P)

    def chain(windowed):
        bases = MotionBases(rots0, transls0).to(DEV)
        means = base.clone().requires_grad_(True)
        coefs = coefs0.clone().requires_grad_(True)
        leaves = {k: v.clone().requires_grad_(True) for k, v in src.items()}
        m2 = torch.zeros(P, 3, device=DEV, requires_grad=True)
        positions = bases.compute_means(ts, means, coefs, softmax=True)
        assert positions.shape == (P, 3, 3) and positions.is_contiguous()
        if windowed:
            out = _call(GaussianRasterizerBatch(sets, camera_frames=frames), positions, leaves, label, m2, True)
            _backward(out, ups)
        else:
            outs, grs = [], []
            for b in sorted(set(frames)):
                idx = [c for c, f in enumerate(frames) if f == b]
                out = _call(GaussianRasterizerBatch([sets[c] for c in idx]), positions[:, b].contiguous(), leaves,
                            label, m2, True)
                for k in ("color", "depth", "alpha", "features"):
                    outs.append(out[k])
                    grs.append(ups[k][idx])
            torch.autograd.backward(outs, grs)
        return dict(means=means.grad, coefs=coefs.grad, rots=bases.params["rots"].grad,
                    transls=bases.params["transls"].grad, **{k: v.grad for k, v in leaves.items()})

    got, ref = chain(True), chain(False)
    rels = {k: _rel(got[k], ref[k]) for k in ref}
    print("relative L2 through the motion model:", {k: f"{v:.2e}" for k, v in rels.items()})
    for k in ("means", "coefs", "rots", "transls"):
        assert ref[k].abs().max() > 0 and rels[k] <= TOL, (k, rels[k])
