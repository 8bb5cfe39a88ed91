"""Camera gradients of the batch backward (include/gs_camera_grad.h;
GaussianRasterizerBatch.forward(viewmatrices=, projmatrices=, campos=)) on the
GPU, against

* torch autograd through the dense fp64 splat (oracle/torch_splat.py, on the
  CPU), which is differentiable in view, proj and -- through sh_colors --
  campos: the project's 1e-4 relative-L2 gradient bound, per
  camera and per tensor;
* the existing kernels at P = 20 000: the twist gradient of
  camera.PoseRefiner against the same twist applied to the scene's means and
  rotations in PyTorch;
* itself: bit-identical repeats, no effect on any other output or gradient,
  nothing launched when no camera tensor requires grad.

Scenes follow tests/_harness.scene (make_gaussians at scale_mult 3, the first
cameras of the 27-camera rig), opacity clamped to 0.9: test_autograd_oracle's
scene, free of alpha-clamp and frustum-clamp decisions."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from dynamic3dgaussians_amd import _C, PoseRefiner, pose_errors
from dynamic3dgaussians_amd.camera import camera_rig, intrinsics, look_at_w2c, setup_camera
from dynamic3dgaussians_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizerBatch
from dynamic3dgaussians_amd.scene import make_gaussians
from oracle import torch_splat as TS

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
TOL = 1e-4       # the project's gradient bound against fp64 autograd
TOL_SUM = 1e-5   # test_gpu_window.py's bound for re-ordered sums of the same terms
BG = (0.2, 0.4, 0.6)
CAM_NAMES = ("view", "proj", "campos")


# ---------------------------------------------------------------- scenes

@functools.lru_cache(maxsize=None)
def _case(P=800, W=80, H=64, C=3, F=8, seed=5, sh_degree=None, use_cov=False, pp=None, away=None):
    """CPU tensors of a scene and its C cameras.  `pp`: an off-centre principal
    point (cameras on a small arc instead of the rig); `away`: the index of a
    camera that is turned to look away from the scene."""
    g = make_gaussians(P, F=F, sh_degree=sh_degree or 0, seed=seed, scale_mult=3.0)
    g["opacities"] = g["opacities"].clamp(max=0.9)
    if pp is None:
        cams = camera_rig(27, W, H)[:C]
    else:
        eyes = [np.array([0.3 + 0.4 * c, -1.2, 2.2 - 0.3 * c]) for c in range(C)]
        cams = [setup_camera(W, H, intrinsics(W, H, 60.0, cx=pp[0], cy=pp[1]), look_at_w2c(e)) for e in eyes]
    if away is not None:
        eye = cams[away].campos.astype(np.float64)  # 2.5 from the origin, the scene within sqrt(3)
        cams[away] = setup_camera(W, H, intrinsics(W, H, 60.0), look_at_w2c(eye, target=3.0 * eye))  # facing out
    case = dict(P=P, W=W, H=H, C=C, F=F, cams=cams, degree=sh_degree or 0, use_sh=sh_degree is not None,
                use_cov=use_cov, **g)
    if use_cov:
        # a precomputed covariance R S^2 R^T of the normalised quaternion, fp64 -> fp32
        q = torch.nn.functional.normalize(g["rotations"].double(), dim=1)
        M = TS._quat_cols(q) * g["scales"].double()[:, None, :]
        S = M @ M.transpose(1, 2)
        case["cov3D"] = torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]],
                                    1).float().contiguous()
    return case


@functools.lru_cache(maxsize=None)
def _ups(C, F, W, H, seed=3, only_color=False):
    gen = torch.Generator().manual_seed(seed)
    ups = dict(color=torch.randn(C, 3, H, W, generator=gen), depth=0.1 * torch.randn(C, 1, H, W, generator=gen),
               alpha=torch.randn(C, 1, H, W, generator=gen), features=torch.randn(C, F, H, W, generator=gen))
    if only_color:
        ups = dict(color=ups["color"])
    return ups


def _rel(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


# ---------------------------------------------------------------- the fp64 oracle (CPU)

_ORACLE = {}


def oracle_camera_grads(case, ups):
    """Per camera, torch autograd's gradients of sum(output * upstream) with
    respect to view [16], proj [16] and campos [3] through the dense fp64
    splat.  Computed once per (case, upstream) and shared."""
    key = (id(case), id(ups))
    if key in _ORACLE:
        return _ORACLE[key][0]
    d64 = lambda t: t.double()  # noqa: E731
    out = dict(view=[], proj=[], campos=[])
    for c, cam in enumerate(case["cams"]):
        view = torch.from_numpy(cam.viewmatrix.copy()).double().reshape(-1).requires_grad_(True)
        proj = torch.from_numpy(cam.projmatrix.copy()).double().reshape(-1).requires_grad_(True)
        campos = torch.from_numpy(cam.campos.copy()).double().requires_grad_(True)
        m3 = d64(case["means3D"])
        if case["use_sh"]:
            col = TS.sh_colors(m3, d64(case["shs"]), case["degree"], campos)
        else:
            col = d64(case["colors"])
        # (a precomputed covariance is R S^2 R^T of the normalised quaternion: the same splat)
        rot = d64(case["rotations"])
        rot = torch.nn.functional.normalize(rot, dim=1) if case["use_cov"] else rot
        color, depth, feat, alpha = TS.render(
            m3, col, d64(case["opacities"]), d64(case["scales"]), rot, view, proj, cam.tanfovx, cam.tanfovy, cam.c_x,
            cam.c_y, case["W"], case["H"], torch.tensor(BG, dtype=torch.float64),
            features=d64(case["semantic_feature"]) if case["F"] else None)
        named = dict(color=color, depth=depth, alpha=alpha, features=feat)
        loss = sum((named[k] * ups[k][c].double()).sum() for k in ups if named[k] is not None)
        if loss.requires_grad:
            loss.backward()
        for k, t in (("view", view), ("proj", proj), ("campos", campos)):
            out[k].append((torch.zeros_like(t) if t.grad is None else t.grad).numpy().copy())
    _ORACLE[key] = ({k: np.stack(v) for k, v in out.items()}, case, ups)  # the keys' objects stay alive
    return _ORACLE[key][0]


# ---------------------------------------------------------------- the GPU call

def _settings(case, compat="fixed", windows=None):
    bg = torch.tensor(BG, device=DEV)
    return [GaussianRasterizationSettings(
        image_height=case["H"], image_width=case["W"], tanfovx=c.tanfovx, tanfovy=c.tanfovy, c_x=c.c_x, c_y=c.c_y,
        bg=bg, viewmatrix=torch.from_numpy(c.viewmatrix.copy()).to(DEV),
        projmatrix=torch.from_numpy(c.projmatrix.copy()).to(DEV), sh_degree=case["degree"],
        campos=torch.from_numpy(c.campos.copy()).to(DEV), compat=compat,
        tile_window=None if windows is None else windows[i]) for i, c in enumerate(case["cams"])]


def _camera_leaves(case, grad=True):
    cams = case["cams"]
    v = torch.from_numpy(np.stack([c.viewmatrix for c in cams])).to(DEV).requires_grad_(grad)
    p = torch.from_numpy(np.stack([c.projmatrix for c in cams])).to(DEV).requires_grad_(grad)
    cp = torch.from_numpy(np.stack([c.campos for c in cams])).to(DEV).requires_grad_(grad)
    return v, p, cp


def _gaussian_leaves(case, means=None, raw=False):
    leaves = dict(opacities=case["opacities"], scales=case["scales"], rotations=case["rotations"])
    if raw:  # logit_opacities, log_scales, unnorm_rotations (helpers.py:98-107)
        leaves = dict(opacities=torch.logit(case["opacities"]), scales=case["scales"].log(),
                      rotations=case["rotations"] * 1.7)
    if case["use_cov"]:
        leaves = dict(opacities=case["opacities"], cov3D_precomp=case["cov3D"])
    if case["F"]:
        leaves["semantic_feature"] = case["semantic_feature"]
    if case["use_sh"]:
        leaves["shs"] = case["shs"]
    else:
        leaves["colors_precomp"] = case["colors"]
    leaves["means3D"] = case["means3D"] if means is None else means
    return {k: v.to(DEV).clone().requires_grad_(True) for k, v in leaves.items()}


def run_gpu(case, ups, cam_grad=True, cam_tensors=True, label=None, ras=None, means=None, raw=False, **ras_kw):
    """One forward + backward; -> (outputs, per-Gaussian gradients, camera gradients [C, 16/16/3] or None)."""
    ras = GaussianRasterizerBatch(_settings(case), raw_params=raw, **ras_kw) if ras is None else ras
    leaves = _gaussian_leaves(case, means, raw)
    m2 = torch.zeros(case["P"], 3, device=DEV, requires_grad=True)
    cam = _camera_leaves(case, cam_grad) if cam_tensors else (None, None, None)
    kw = dict(zip(("viewmatrices", "projmatrices", "campos"), cam)) if cam_tensors else {}
    out = ras(means2D=m2, label=label, **leaves, **kw)
    if case["F"]:
        im, radii, feat, depth, alpha = out
    else:
        (im, radii, depth, alpha), feat = out, None
    named = dict(color=im, depth=depth, alpha=alpha, features=feat)
    ks = [k for k in ups if named[k] is not None]
    torch.autograd.backward([named[k] for k in ks], [ups[k].to(DEV) for k in ks])
    torch.cuda.synchronize()
    grads = {k: v.grad.detach().clone() for k, v in leaves.items()}
    grads["means2D"] = m2.grad.detach().clone()
    outs = {k: (None if v is None else v.detach().clone()) for k, v in dict(named, radii=radii).items()}
    cg = None
    if cam_tensors and cam_grad:
        cg = {k: t.grad.detach().reshape(case["C"], -1).cpu().numpy() for k, t in zip(CAM_NAMES, cam)}
        assert cam[0].grad.shape == (case["C"], 4, 4) and cam[2].grad.shape == (case["C"], 3)  # the given shapes
    return outs, grads, cg


def check_against_oracle(case, ups, cg, expect_campos=None, tol=TOL):
    """Per camera and tensor: relative L2 <= tol; the columns the forward does
    not read exactly 0; campos exactly 0 without SH.  Returns the worst figures."""
    ref = oracle_camera_grads(case, ups)
    worst = {}
    for k in CAM_NAMES:
        assert np.isfinite(cg[k]).all(), k
    assert np.all(cg["view"].reshape(-1, 4, 4)[:, :, 3] == 0.0)   # entries 4 i + 3
    assert np.all(cg["proj"].reshape(-1, 4, 4)[:, :, 2] == 0.0)   # entries 4 i + 2
    assert np.all(ref["view"].reshape(-1, 4, 4)[:, :, 3] == 0.0) and np.all(ref["proj"].reshape(-1, 4, 4)[:, :, 2] == 0.0)
    has_campos = case["use_sh"] and case["degree"] > 0 if expect_campos is None else expect_campos
    for c in range(case["C"]):
        for k in CAM_NAMES:
            if k == "campos" and not has_campos:
                assert np.all(cg[k][c] == 0.0) and np.all(ref[k][c] == 0.0)
                continue
            assert np.linalg.norm(ref[k][c]) > 0, (k, c)
            r = _rel(cg[k][c], ref[k][c])
            print(f"camera {c} {k}: rel L2 {r:.3e} (|ref| {np.linalg.norm(ref[k][c]):.3e})")
            worst[k] = max(worst.get(k, 0.0), r)
            assert r <= tol, (k, c, r)
    return worst


# ---------------------------------------------------------------- 1. against fp64 autograd

ORACLE_CASES = {
    "colors": dict(),
    "sh1": dict(sh_degree=1),
    "sh3": dict(sh_degree=3),
    "cov3d": dict(use_cov=True),
    "offcentre_75x50": dict(W=75, H=50, pp=(30.5, 29.25)),
}


@pytest.mark.parametrize("name", list(ORACLE_CASES))
def test_camera_gradients_match_fp64_autograd(name):
    """P = 800, 80 x 64 (75 x 50 off-centre: ragged tiles), F = 8, C = 3, random
    upstream gradients on all four outputs; per camera each of
    viewmatrices.grad, projmatrices.grad, campos.grad within 1e-4 relative L2
    of torch_splat's fp64 autograd.  Measured worst over the cameras (MI355X),
    view / proj / campos: colors 3.0e-6 / 2.3e-6 / 0; sh1 4.5e-6 / 2.3e-6 /
    4.1e-6; sh3 5.0e-6 / 3.0e-6 / 1.9e-6; cov3d 3.2e-6 / 2.5e-6 / 0;
    offcentre_75x50 3.4e-6 / 2.6e-6 / 0."""
    case = _case(**ORACLE_CASES[name])
    ups = _ups(case["C"], case["F"], case["W"], case["H"])
    _, _, cg = run_gpu(case, ups)
    check_against_oracle(case, ups, cg)


# ---------------------------------------------------------------- 2. reduction shapes

def test_less_than_one_wave_of_gaussians():
    case = _case(P=37)
    ups = _ups(3, 8, 80, 64)
    check_against_oracle(case, ups, run_gpu(case, ups)[2])


def test_several_records_per_camera_with_a_ragged_last_one():
    """P = 4000 at 128 x 96 (tests/_harness.scene's defaults: precomputed
    colours): two workgroup records per camera, the second of 1952 Gaussians;
    two cameras, so that camera 1's records sit behind camera 0's two.  Both
    cameras have Gaussians inside the frustum clamp (1 and 2): the exact
    derivative of the clamped Jacobian entry is what the oracle takes.
    Measured (MI355X): view 2.6e-5 / 3.2e-5, proj 4.9e-5 / 2.3e-5 for cameras
    0 / 1, ten times the P = 800 scenes' figures.  That is the records', not
    the reduction's: with SH degree 1 on the same Gaussians (view 1.8e-5 /
    7.0e-5, campos 9.5e-6 / 1.10e-4) the same formulas evaluated in fp64 on
    the host from the records read back were 5.4e-7 from the kernel and 7.0e-5
    from the oracle for camera 1 -- one near Gaussian (id 108, |term| 292 of
    |gradient| 313) covers thousands of pixels, and the blend's fp32 sums of
    random-sign upstream gradients carry an error relative to their absolute
    sum.  The position gradient is the blend's colour gradient times the
    direction Jacobian and inherits it, so this shape is checked with
    precomputed colours and the position gradient on the P = 800 scenes
    (DESIGN.md 9.13)."""
    case = _case(P=4000, W=128, H=96, C=2)
    ups = _ups(2, 8, 128, 96)
    check_against_oracle(case, ups, run_gpu(case, ups)[2])


def test_single_camera():
    case = _case(C=1, sh_degree=1)
    ups = _ups(1, 8, 80, 64)
    check_against_oracle(case, ups, run_gpu(case, ups)[2])


def test_a_camera_that_sees_nothing_gets_exact_zeros():
    """Camera 1 looks away: its three gradients are exactly zero and finite,
    the other cameras' are the oracle's."""
    case = _case(sh_degree=1, away=1)
    ups = _ups(3, 8, 80, 64)
    outs, _, cg = run_gpu(case, ups)
    assert int(outs["radii"][1].max()) == 0 and int(outs["radii"][0].max()) > 0  # it does see nothing
    for k in CAM_NAMES:
        assert np.all(cg[k][1] == 0.0), k
    ref = oracle_camera_grads(case, ups)
    for c in (0, 2):
        for k in CAM_NAMES:
            assert _rel(cg[k][c], ref[k][c]) <= TOL, (k, c)
    # and the others are what they are without it (cameras are reduced independently)
    sub = _case(sh_degree=1, C=1)
    cg0 = run_gpu(sub, {k: v[:1] for k, v in ups.items()})[2]
    for k in CAM_NAMES:
        assert _rel(cg[k][0], cg0[k][0]) <= TOL_SUM, k


def test_only_the_colour_output_has_an_upstream_gradient():
    case = _case(sh_degree=1)
    ups = _ups(3, 8, 80, 64, only_color=True)
    check_against_oracle(case, ups, run_gpu(case, ups)[2])


def test_empty_scene_gives_zero_camera_gradients():
    case = _case(P=0, F=0)
    ups = _ups(3, 0, 80, 64, only_color=True)
    calls = _C.camera_grad_calls
    _, _, cg = run_gpu(case, ups)
    assert cg["view"].shape == (3, 16) and cg["proj"].shape == (3, 16) and cg["campos"].shape == (3, 3)
    for k in CAM_NAMES:
        assert np.all(cg[k] == 0.0)
    assert _C.camera_grad_calls == calls  # answered before the binding, like the forward and the backward


# ---------------------------------------------------------------- 3. independence and determinism

def test_camera_gradients_change_nothing_else_and_repeat_bit_for_bit():
    """Whole calls compared bit for bit, so at the size where two runs of the
    SAME backward have the same bits: an 8 x 8 image is a single strip, every
    accumulation record gets one wave's sum (the note above cases 5 and 7 of
    tests/test_gpu_window.py; F = 0: a feature row would get one add per
    camera).  The camera kernels' own order is checked at 128 x 96 below."""
    case = _case(P=3001, W=8, H=8, F=0, sh_degree=1)
    ups = _ups(3, 0, 8, 8)
    ups = {k: ups[k] for k in ("color", "depth", "alpha")}
    calls = _C.camera_grad_calls
    outs0, grads0, _ = run_gpu(case, ups, cam_tensors=False)
    outs1, grads1, _ = run_gpu(case, ups, cam_grad=False)  # given, but none requires grad
    assert _C.camera_grad_calls == calls  # nothing extra was launched
    outs2, grads2, cg2 = run_gpu(case, ups)
    assert _C.camera_grad_calls == calls + 1
    outs3, grads3, cg3 = run_gpu(case, ups)
    for outs, grads in ((outs1, grads1), (outs2, grads2), (outs3, grads3)):
        for k, v in outs0.items():
            assert v is None or torch.equal(outs[k], v), k
        for k, v in grads0.items():
            assert torch.equal(grads[k], v), k
    assert int((outs0["radii"] > 0).sum()) >= 300
    for k in CAM_NAMES:
        assert np.array_equal(cg2[k], cg3[k]) and np.all(np.abs(cg2[k]).sum(1) > 0), k
    # a label masks per-Gaussian gradients only
    label = torch.ones(case["P"], device=DEV)
    label[::2] = 0.0
    _, grads4, cg4 = run_gpu(case, ups, label=label)
    for k in CAM_NAMES:
        assert np.array_equal(cg2[k], cg4[k]), k
    assert torch.all(grads4["means3D"][::2] == 0) and not torch.equal(grads4["means3D"], grads0["means3D"])


def test_camera_kernels_repeat_bit_for_bit_on_the_same_records():
    """P = 4000 at 128 x 96 (two records per camera): the binding's camera call
    twice on the scratch one backward left -- the new kernels' own sums have a
    fixed order (no atomics), whatever the blend's atomics did to the records
    -- and the result is the oracle's."""
    case = _case(P=4000, W=128, H=96, C=2)
    C, W, H = 2, 128, 96
    ups = {k: v.to(DEV) for k, v in _ups(C, 8, W, H).items()}
    d = lambda k: case[k].to(DEV)  # noqa: E731
    none = torch.Tensor([]).to(DEV)
    cams = case["cams"]
    v, p, cp = (t.detach() for t in _camera_leaves(case, grad=False))
    cam_scalars = ([c.c_x for c in cams], [c.c_y for c in cams], [c.tanfovx for c in cams], [c.tanfovy for c in cams])
    bg = torch.tensor(BG, device=DEV)
    NR, color, fmap, depth, alpha, radii, geom, binning, img, NI = _C.rasterize_gaussians_batch(
        bg, d("means3D"), d("colors"), d("semantic_feature"), d("opacities"), d("scales"), d("rotations"), 1.0, none,
        v, p, *cam_scalars, H, W, none, 0, cp, False, False, compat="fixed")
    scratch = _C.batch_backward_scratch(d("means3D"), d("semantic_feature"), C)
    _C.rasterize_gaussians_batch_backward(
        bg, d("means3D"), radii, d("colors"), d("semantic_feature"), d("scales"), d("rotations"), 1.0, none, v, p,
        *cam_scalars, ups["color"], ups["features"], ups["depth"], ups["alpha"], none, 0, cp, geom, NI, binning,
        img, alpha, False, compat="fixed", scratch=scratch)
    runs = [_C.rasterize_gaussians_batch_camera_grad(bg, d("means3D"), radii, none, v, p, *cam_scalars, H, W, none,
                                                     0, cp, geom, scratch, compat="fixed") for _ in range(3)]
    torch.cuda.synchronize()
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.equal(a, b)
    assert [tuple(t.shape) for t in runs[0]] == [(C, 16), (C, 16), (C, 3)]
    check_against_oracle(case, _ups(C, 8, W, H), {k: t.cpu().numpy() for k, t in zip(CAM_NAMES, runs[0])})


# ---------------------------------------------------------------- 4. composition

def test_camera_frames_window_matches_one_batch_per_frame():
    """camera_frames = [0, 0, 1] on (P, 2, 3) means against a batch of cameras
    0, 1 on frame 0 and a batch of camera 2 on frame 1: 1e-5 per camera."""
    case = _case(sh_degree=1)
    ups = _ups(3, 8, 80, 64)
    gen = torch.Generator().manual_seed(17)
    pos = torch.stack([case["means3D"], case["means3D"] + 0.04 * torch.randn(case["P"], 3, generator=gen)], 1).contiguous()
    _, gw, cgw = run_gpu(case, ups, means=pos, camera_frames=[0, 0, 1])
    assert gw["means3D"].shape == (case["P"], 2, 3)
    for frame, idx in ((0, [0, 1]), (1, [2])):
        sub = dict(case, cams=[case["cams"][c] for c in idx], C=len(idx))
        _, _, cg = run_gpu(sub, {k: v[idx] for k, v in ups.items()}, means=pos[:, frame].contiguous())
        for j, c in enumerate(idx):
            for k in CAM_NAMES:
                assert _rel(cgw[k][c], cg[k][j]) <= TOL_SUM, (k, c)


def test_raw_params_match_the_activated_call():
    case = _case(sh_degree=1)
    ups = _ups(3, 8, 80, 64)
    _, _, cg = run_gpu(case, ups)
    _, _, cgr = run_gpu(case, ups, raw=True)
    for k in CAM_NAMES:
        for c in range(3):
            assert _rel(cgr[k][c], cg[k][c]) <= TOL_SUM, (k, c)


def test_tile_window_gives_the_gradient_of_its_pixels():
    """grad_into, track_densify and a tile window next to the camera tensors:
    the window's camera gradient is the whole image's with the upstream
    gradients zeroed outside the window (the oracle's bound: another tile
    order of the same sums)."""
    case = _case(sh_degree=1, C=2)
    ups = _ups(2, 8, 80, 64)
    win = (1, 1, 4, 3)  # tiles [1, 4) x [1, 3) of the 5 x 4 grid
    cut = {k: torch.zeros_like(v) for k, v in ups.items()}
    for k, v in ups.items():
        cut[k][..., 16:48, 16:64] = v[..., 16:48, 16:64]
    _, _, cg_full = run_gpu(case, cut)
    ras = GaussianRasterizerBatch(_settings(case, windows=[win, win]))
    _, _, cg_win = run_gpu(case, ups, ras=ras)
    for k in CAM_NAMES:
        for c in range(2):
            assert _rel(cg_win[k][c], cg_full[k][c]) <= TOL, (k, c)
    # track_densify and grad_into keep working next to the camera tensors
    dest = torch.zeros(case["P"], 3, device=DEV)
    ras2 = GaussianRasterizerBatch(_settings(case), track_densify=True)
    leaves = _gaussian_leaves(case)
    cam = _camera_leaves(case)
    im, radii, feat, depth, alpha = ras2(means2D=torch.zeros(case["P"], 3, device=DEV), label=None, **leaves,
                                         viewmatrices=cam[0], projmatrices=cam[1], campos=cam[2],
                                         grad_into={"means3D": dest})
    (im * ups["color"].to(DEV)).sum().backward()
    assert leaves["means3D"].grad is None and float(dest.abs().sum()) > 0
    assert float(ras2.densify_stats["denom"].sum()) > 0 and float(cam[0].grad.abs().sum()) > 0


# ---------------------------------------------------------------- 5. against the existing kernels

def _quat_mul(a, b):
    """Hamilton product of (r, x, y, z) quaternions, broadcasting."""
    ar, ax, ay, az = a.unbind(-1)
    br, bx, by, bz = b.unbind(-1)
    return torch.stack([ar * br - ax * bx - ay * by - az * bz, ar * bx + ax * br + ay * bz - az * by,
                        ar * by - ax * bz + ay * br + az * bx, ar * bz + ax * by - ay * bx + az * br], -1)


def test_twist_gradient_matches_the_existing_means_and_rotations_path():
    """P = 20 000, 128 x 96, C = 4, precomputed colours, unit quaternions, a
    twist of ~1 degree and ~0.02 per camera.  (a) PoseRefiner -> camera tensors
    -> the new kernel; (b) the same twist as the world transform G = w2c^-1 T
    w2c of the means and of the rotations (G rotates by the twist's angle
    about R_w2c^T rot: a quaternion product), formed in PyTorch in fp64 on the
    host so that only the kernels' own fp32 error remains, one batch-of-one
    call per camera with the existing means3D / rotations gradients.  The
    bound is 1e-4 relative L2 on the 6 C vector; a correct implementation
    exceeds it here: measured (MI355X) 1.59e-4 between the two paths (per
    camera 2.4e-5, 2.5e-4, 4.5e-5, 5.9e-5).  Against (c), the fp64 run of the
    same chain, the camera path is at 1.17e-4 and the existing path at 1.73e-4
    (the scene has 7-15 pixels per camera with an undecided blend decision and
    ~200 Gaussians per camera inside the frustum clamp, where the per-Gaussian
    backward keeps the reference's factor 2 and the camera kernel the exact
    derivative), so the camera path is held to 10 x the existing path's own
    error, the envelope rule of tests/test_gpu_envelope.py."""
    case = _case(P=20000, W=128, H=96, C=4, F=0, seed=9)
    C, W, H = 4, 128, 96
    ups = _ups(C, 0, W, H, seed=21)
    ups = {k: ups[k].to(DEV) for k in ("color", "depth", "alpha")}
    gen = torch.Generator().manual_seed(5)
    twist = torch.randn(C, 6, generator=gen, dtype=torch.float64)
    twist = (0.0175 * twist / twist[:, :3].norm(dim=1, keepdim=True)).float().double()  # fp32 numbers, for every path
    w2c = np.stack([c.viewmatrix.T for c in case["cams"]])
    K = intrinsics(W, H, 60.0)
    sets = _settings(case)
    gauss = {k: case[k].to(DEV) for k in ("means3D", "opacities", "scales", "rotations", "colors")}
    m2 = torch.zeros(case["P"], 3, device=DEV)

    def loss_of(out):
        im, radii, depth, alpha = out
        return (im * ups["color"]).sum() + (depth * ups["depth"]).sum() + (alpha * ups["alpha"]).sum()

    # (a) the camera path
    ref = PoseRefiner(w2c, K, W, H).to(DEV)
    ref.rot.data, ref.trans.data = twist[:, :3].float().to(DEV), twist[:, 3:].float().to(DEV)
    v, p, cp = ref()
    ras = GaussianRasterizerBatch(sets)
    loss_of(ras(means3D=gauss["means3D"], means2D=m2, opacities=gauss["opacities"], colors_precomp=gauss["colors"],
                scales=gauss["scales"], rotations=gauss["rotations"], label=None, viewmatrices=v, projmatrices=p,
                campos=cp)).backward()
    ga = torch.cat([ref.rot.grad, ref.trans.grad], 1).double().cpu().numpy()  # [C, 6]

    # (b) the scene path, one camera at a time
    gb = np.zeros((C, 6))
    means64, rots64 = case["means3D"].double(), case["rotations"].double()
    for c in range(C):
        tw = twist[c].clone().requires_grad_(True)
        r, t = tw[:3], tw[3:]
        xi = torch.zeros(4, 4, dtype=torch.float64)
        xi[0, 1], xi[0, 2], xi[1, 2], xi[1, 0], xi[2, 0], xi[2, 1] = -r[2], r[1], -r[0], r[2], -r[1], r[0]
        xi[:3, 3] = t
        Wc = torch.from_numpy(w2c[c].astype(np.float64))
        G = torch.linalg.inv(Wc) @ torch.linalg.matrix_exp(xi) @ Wc  # world transform of the scene
        means = means64 @ G[:3, :3].T + G[:3, 3]
        th = r.norm()
        qG = torch.cat([torch.cos(th / 2)[None], torch.sin(th / 2) / th * (Wc[:3, :3].T @ r)])
        rots = _quat_mul(qG[None], rots64)
        one = GaussianRasterizerBatch([sets[c]])
        out = one(means3D=means.float().to(DEV), means2D=m2, opacities=gauss["opacities"],
                  colors_precomp=gauss["colors"], scales=gauss["scales"], rotations=rots.float().to(DEV), label=None)
        im, radii, depth, alpha = out
        ((im * ups["color"][c:c + 1]).sum() + (depth * ups["depth"][c:c + 1]).sum()
         + (alpha * ups["alpha"][c:c + 1]).sum()).backward()
        gb[c] = tw.grad.numpy()
    r = _rel(ga, gb)
    print(f"twist gradient: camera path vs scene path rel L2 {r:.3e}; per camera "
          f"{[f'{_rel(ga[c], gb[c]):.2e}' for c in range(C)]}; |g| {np.linalg.norm(gb):.3e}")

    # (c) the fp64 run of the same chain: torch_splat's camera gradients at the very matrices the
    # camera path rendered with, through PoseRefiner's fp64 Jacobian at the same twist
    from dynamic3dgaussians_amd.camera import CameraParams
    moved = dict(case, cams=[CameraParams(W=W, H=H, viewmatrix=v[c].detach().cpu().numpy(),
                                          projmatrix=p[c].detach().cpu().numpy(), campos=cp[c].detach().cpu().numpy(),
                                          c_x=k.c_x, c_y=k.c_y, tanfovx=k.tanfovx, tanfovy=k.tanfovy)
                             for c, k in enumerate(case["cams"])])
    og = oracle_camera_grads(moved, {k: u.cpu() for k, u in ups.items()})
    ref64 = PoseRefiner(w2c, K, W, H).double()
    ref64.rot.data, ref64.trans.data = twist[:, :3].clone(), twist[:, 3:].clone()
    v64, p64, _ = ref64()
    ((v64.reshape(C, 16) * torch.from_numpy(og["view"])).sum() + (p64.reshape(C, 16) * torch.from_numpy(og["proj"])).sum()
     ).backward()
    truth = torch.cat([ref64.rot.grad, ref64.trans.grad], 1).numpy()
    e_cam, e_exist = _rel(ga, truth), _rel(gb, truth)
    print(f"against the fp64 chain: camera path {e_cam:.3e}, existing means/rotations path {e_exist:.3e}")
    assert r <= TOL or e_cam <= 10.0 * e_exist, (r, e_cam, e_exist)


# ---------------------------------------------------------------- 6. errors

def test_errors_on_the_device():
    case = _case()
    leaves = _gaussian_leaves(case)
    m2 = torch.zeros(case["P"], 3, device=DEV)
    v, p, cp = _camera_leaves(case)
    ref_mode = GaussianRasterizerBatch(_settings(case, compat="reference"))
    with pytest.raises(ValueError, match='compat="fixed"'):
        ref_mode(means2D=m2, label=None, **leaves, viewmatrices=v)
    ref_mode(means2D=m2, label=None, **leaves, viewmatrices=v.detach())  # without a gradient it is a plain input
    ras = GaussianRasterizerBatch(_settings(case))
    with pytest.raises(ValueError, match="viewmatrices must have shape"):
        ras(means2D=m2, label=None, **leaves, viewmatrices=v[:2])
    with pytest.raises(ValueError, match="campos must have shape"):
        ras(means2D=m2, label=None, **leaves, campos=cp.reshape(-1))
    with pytest.raises(ValueError, match="projmatrices must be fp32"):
        ras(means2D=m2, label=None, **leaves, projmatrices=p.double())
    with pytest.raises(ValueError, match="campos must be a device tensor"):
        ras(means2D=m2, label=None, **leaves, campos=cp.detach().cpu())
    with pytest.raises(ValueError, match='compat="fixed"'):
        _C.rasterize_gaussians_batch_camera_grad(*([None] * 17), compat="reference")


# ---------------------------------------------------------------- 7. pose recovery

def test_pose_refinement_recovers_perturbed_cameras():
    """Targets rendered from 4 true cameras of a P = 5000, 128 x 96 scene; the
    poses start a seeded twist of 1 degree and 1 % of the scene radius (1.7)
    away; only PoseRefiner's parameters are trained (Adam, lr 5e-4, 40 steps,
    L1 image loss).  The loss, the ATE and the RPE rotation each end strictly
    below their start; with the three tensors detached the parameters do not
    move at all.  Measured before -> after (MI355X): loss 0.04346 -> 0.00547,
    ATE 0.01700 -> 0.01377, RPE translation 0.05281 -> 0.01597, RPE rotation
    1.089 -> 0.438 degrees."""
    P, W, H, C, STEPS = 5000, 128, 96, 4, 40
    case = _case(P=P, W=W, H=H, C=C, F=0, seed=11)
    w2c_true = np.stack([c.viewmatrix.T for c in case["cams"]]).astype(np.float64)
    K = intrinsics(W, H, 60.0)
    sets = _settings(case)
    g = {k: case[k].to(DEV) for k in ("means3D", "opacities", "scales", "rotations")}
    colors = case["colors"].to(DEV).requires_grad_(True)  # differentiable, never stepped: the backward always runs
    m2 = torch.zeros(P, 3, device=DEV)
    ras = GaussianRasterizerBatch(sets)

    def render(**cam):
        return ras(means3D=g["means3D"], means2D=m2, opacities=g["opacities"], colors_precomp=colors,
                   scales=g["scales"], rotations=g["rotations"], **cam)[0]

    with torch.no_grad():
        target = render()
    gen = torch.Generator().manual_seed(13)
    d = torch.randn(C, 6, generator=gen, dtype=torch.float64)
    rot0 = np.deg2rad(1.0) * d[:, :3] / d[:, :3].norm(dim=1, keepdim=True)
    trans0 = 0.017 * d[:, 3:] / d[:, 3:].norm(dim=1, keepdim=True)
    start = PoseRefiner(w2c_true, K, W, H).double()
    start.rot.data, start.trans.data = rot0, trans0
    w2c_start = start.refined_w2c().detach().numpy()
    c2w_true = np.linalg.inv(w2c_true)

    def train(detach):
        ref = PoseRefiner(w2c_start, K, W, H).to(DEV)
        opt = torch.optim.Adam(ref.parameters(), lr=5e-4)
        losses = []
        for _ in range(STEPS):
            v, p, cp = ref()
            if detach:
                v, p, cp = v.detach(), p.detach(), cp.detach()
            loss = (render(viewmatrices=v, projmatrices=p, campos=cp) - target).abs().mean()
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            losses.append(float(loss))
        with torch.no_grad():
            v, p, cp = ref()
            losses.append(float((render(viewmatrices=v, projmatrices=p, campos=cp) - target).abs().mean()))
        return ref, losses

    before = pose_errors(np.linalg.inv(w2c_start), c2w_true)
    ref, losses = train(detach=False)
    after = pose_errors(ref.poses(), c2w_true)
    print(f"loss {losses[0]:.5f} -> {losses[-1]:.5f}; ATE {before[0]:.5f} -> {after[0]:.5f}; "
          f"RPE_t {before[1]:.5f} -> {after[1]:.5f}; RPE_r {before[2]:.4f} -> {after[2]:.4f} deg")
    assert losses[-1] < losses[0]
    assert after[0] < before[0]
    assert after[2] < before[2]
    frozen, _ = train(detach=True)
    assert torch.all(frozen.rot == 0) and torch.all(frozen.trans == 0)
