"""Camera gradients (include/gs_camera_grad.h), the parts that need no GPU:
the exported symbols and the unchanged ABI, the host validator
gs_check_camera_grad through ctypes, the Python boundary's refusals before any
device work, camera.PoseRefiner against setup_camera and central differences,
and metrics.pose_errors against the reference's recorded values.  (The
validator's sanitizer program, tools/camera_grad_host_sanitize.c, is built and
run by hand on the CPU: DESIGN.md 9.13.)"""
from __future__ import annotations

import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import dynamic3dgaussians_amd as pkg
from dynamic3dgaussians_amd import _C, _lib
from dynamic3dgaussians_amd.camera import PoseRefiner, camera_rig, intrinsics, look_at_w2c, setup_camera
from dynamic3dgaussians_amd.metrics import pose_errors
from dynamic3dgaussians_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizerBatch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"gs_camera_grad_workspace_bytes", "gs_check_camera_grad", "gs_camera_grad_batch"}


def test_abi_is_still_13_and_the_new_header_is_exported():
    L = _lib.load()
    assert L.gs_version() == _lib.ABI_VERSION == 13  # a new header, no existing struct or entry point changed
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "gs_camera_grad.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(gs_[a-z_0-9]+)\s*\(", txt)) == NAMES
    for n in NAMES:
        assert hasattr(L, n) and n in _lib.PROTOTYPES, n
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.lib_path()], capture_output=True, text=True).stdout
    assert NAMES <= set(re.findall(r" T (gs_[a-z_0-9]+)", out))
    assert re.search(r"#define GS_CAMERA_GRAD_MAX_CAMS 64\b", txt) and _lib.GS_CAMERA_GRAD_MAX_CAMS == 64
    assert pkg.PoseRefiner is PoseRefiner and pkg.pose_errors is pose_errors


def test_workspace_is_one_record_per_camera_and_chunk():
    L = _lib.load()
    assert L.gs_camera_grad_workspace_bytes(0, 3) == 0
    assert L.gs_camera_grad_workspace_bytes(1, 1) == 256
    assert L.gs_camera_grad_workspace_bytes(2048, 2) == 512 and L.gs_camera_grad_workspace_bytes(2049, 2) == 1024
    assert L.gs_camera_grad_workspace_bytes(300000, 27) == 256 * 147 * 27
    assert L.gs_camera_grad_workspace_bytes(100, 0) == 0 and L.gs_camera_grad_workspace_bytes(100, 65) == 0


def _check(P=800, C=3, compat=1, short=0, ws=True, null_out=None):
    """gs_check_camera_grad on host buffers of the right sizes (it reads none of them)."""
    L = _lib.load()
    need = L.gs_camera_grad_workspace_bytes(P, C)
    buf = ctypes.create_string_buffer(max(need, 1) + 16)
    base = (ctypes.addressof(buf) + 15) & ~15
    outs = [ctypes.addressof(ctypes.create_string_buffer(4 * 16 * 64)) for _ in range(3)]
    held = [buf]  # keeps the workspace alive over the call
    if null_out is not None:
        outs[null_out] = None
    r = L.gs_check_camera_grad(P, C, compat, base if ws else None, need - short, *outs)
    del held
    return r, (L.gs_last_error() or b"").decode()


def test_validator_accepts_valid_arguments():
    assert _check()[0] == 0
    assert _check(P=1, C=1)[0] == 0
    assert _check(P=300000, C=64)[0] == 0
    assert _check(P=0, C=2, ws=False)[0] == 0  # no workspace needed, none checked


@pytest.mark.parametrize("kw,msg", [
    (dict(C=0), "camera batch size 0 outside 1..64"),
    (dict(C=65), "camera batch size 65 outside 1..64"),
    (dict(null_out=0), "dL_dview, dL_dproj and dL_dcampos are required"),
    (dict(null_out=1), "are required"),
    (dict(null_out=2), "are required"),
    (dict(short=1), "workspace of 767 bytes, 768 needed"),
    (dict(ws=False), "workspace is required"),
    (dict(compat=0), "compat 0 is refused"),
    (dict(P=-1), "P must be"),
])
def test_validator_rejects(kw, msg):
    r, err = _check(**kw)
    assert r != 0 and msg in err, err


def test_entry_point_runs_the_validator_before_anything_touches_a_device():
    L = _lib.load()
    g, cams = _lib.GsGaussians(P=10), (_lib.GsCamera * 2)()
    out = ctypes.create_string_buffer(4 * 32)
    a = ctypes.addressof(out)
    assert L.gs_camera_grad_batch(ctypes.byref(g), cams, 2, None, None, 0, None, None, None, 0, a, a, a, None) < 0
    assert b"compat 0 is refused" in L.gs_last_error()
    assert L.gs_camera_grad_batch(ctypes.byref(g), cams, 2, None, None, 1, None, None, None, 0, a, a, a, None) < 0
    assert b"workspace is required" in L.gs_last_error()
    assert L.gs_camera_grad_batch(None, cams, 2, None, None, 1, None, None, None, 0, a, a, a, None) < 0


def _cpu_settings(C, W=64, H=48, compat="fixed"):
    eye = torch.eye(4)
    return [GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=0.5, tanfovy=0.5, bg=torch.zeros(3),
                                          viewmatrix=eye, projmatrix=eye, campos=torch.zeros(3), compat=compat)
            for _ in range(C)]


def _cpu_call(ras, **cam):
    return ras(means3D=torch.zeros(5, 3), means2D=torch.zeros(5, 3), opacities=torch.ones(5, 1),
               colors_precomp=torch.ones(5, 3), scales=torch.ones(5, 3), rotations=torch.ones(5, 4), **cam)


def test_host_camera_tensors_raise_before_any_device_work():
    ras = GaussianRasterizerBatch(_cpu_settings(2))
    with pytest.raises(ValueError, match="viewmatrices must be a device tensor"):
        _cpu_call(ras, viewmatrices=torch.eye(4).repeat(2, 1, 1))
    with pytest.raises(ValueError, match="campos must be a device tensor"):
        _cpu_call(ras, campos=torch.zeros(2, 3, requires_grad=True))
    with pytest.raises(_lib.GsplatError):  # the binding itself: host tensors have no path
        _C.rasterize_gaussians_batch_camera_grad(
            torch.zeros(3), torch.zeros(5, 3), torch.ones(2, 5, dtype=torch.int32), None, torch.eye(4).repeat(2, 1, 1),
            torch.eye(4).repeat(2, 1, 1), [32, 32], [24, 24], [0.5, 0.5], [0.5, 0.5], 48, 64, None, 0,
            torch.zeros(2, 3), torch.zeros(8, dtype=torch.uint8), torch.zeros(8, dtype=torch.uint8), compat="fixed")


def test_wrong_shapes_and_dtypes_raise():
    ras = GaussianRasterizerBatch(_cpu_settings(2))
    with pytest.raises(ValueError, match=r"projmatrices must have shape \(2, 4, 4\) or \(2, 16\)"):
        _cpu_call(ras, projmatrices=torch.zeros(3, 4, 4))
    with pytest.raises(ValueError, match=r"campos must have shape \(2, 3\)"):
        _cpu_call(ras, campos=torch.zeros(2, 4))
    with pytest.raises(ValueError, match="viewmatrices must be fp32"):
        _cpu_call(ras, viewmatrices=torch.zeros(2, 16, dtype=torch.float64))
    with pytest.raises(TypeError, match="campos must be a tensor"):
        _cpu_call(ras, campos=[[0, 0, 0], [0, 0, 0]])


def test_reference_compat_with_a_camera_gradient_raises_and_names_fixed():
    ras = GaussianRasterizerBatch(_cpu_settings(2, compat="reference"))
    with pytest.raises(ValueError, match='compat="fixed"'):
        _cpu_call(ras, viewmatrices=torch.eye(4).repeat(2, 1, 1).requires_grad_(True))
    with pytest.raises(ValueError, match='compat="fixed"'):
        _C.rasterize_gaussians_batch_camera_grad(*([None] * 17), compat="reference")


# ---- camera.PoseRefiner

W, H = 80, 64


def _rig(C=3):
    cams = camera_rig(27, W, H)[:C]
    w2c = np.stack([c.viewmatrix.T for c in cams])
    return cams, w2c, intrinsics(W, H, 60.0)


def test_pose_refiner_at_zero_twist_reproduces_setup_camera():
    cams, w2c, K = _rig()
    view, proj, campos = PoseRefiner(w2c, K, W, H)()
    assert view.dtype == proj.dtype == campos.dtype == torch.float32
    assert view.shape == (3, 4, 4) and proj.shape == (3, 4, 4) and campos.shape == (3, 3)
    for c, cam in enumerate(cams):
        assert np.array_equal(view[c].detach().numpy(), cam.viewmatrix)  # exp(0) = I exactly
        # fp32 rounding of a 4-term dot product / of R^T t at |t| = 2.5
        np.testing.assert_allclose(proj[c].detach().numpy(), cam.projmatrix, rtol=0, atol=4 * 2.0 ** -23 * 3.0)
        np.testing.assert_allclose(campos[c].detach().numpy(), cam.campos, rtol=0, atol=4 * 2.0 ** -23 * 2.5)
    # an off-centre principal point and per-camera intrinsics
    K2 = np.stack([intrinsics(W, H, 50.0, cx=30.5, cy=40.25), intrinsics(W, H, 70.0), intrinsics(W, H, 60.0, cx=45.0)])
    _, proj2, _ = PoseRefiner(w2c, K2, W, H, near=0.1, far=50.0)()
    for c in range(3):
        ref = setup_camera(W, H, K2[c], w2c[c], near=0.1, far=50.0)
        np.testing.assert_allclose(proj2[c].detach().numpy(), ref.projmatrix, rtol=0, atol=4 * 2.0 ** -23 * 3.0)


@pytest.mark.parametrize("twist", [0.0, 0.1])
def test_pose_refiner_jacobian_equals_central_differences(twist):
    _, w2c, K = _rig(2)
    m = PoseRefiner(w2c, K, W, H).double()
    gen = torch.Generator().manual_seed(7)
    d = torch.randn(2, 6, generator=gen, dtype=torch.float64)
    x0 = twist * d / d.norm(dim=1, keepdim=True)  # a twist of `twist` rad / units per camera

    def f(x):
        m.rot.data, m.trans.data = x[:, :3].clone(), x[:, 3:].clone()
        return torch.cat([t.reshape(-1) for t in m()])

    m.rot.data, m.trans.data = x0[:, :3].clone(), x0[:, 3:].clone()
    out = torch.cat([t.reshape(-1) for t in m()])
    jac = torch.stack([torch.cat([g.reshape(-1) for g in torch.autograd.grad(o, (m.rot, m.trans), retain_graph=True)])
                       for o in out])  # [70, 12], columns: rot (2 x 3) then trans (2 x 3)
    h = 1e-6
    fd = torch.zeros_like(jac)
    for c in range(2):
        for k in range(6):
            e = torch.zeros_like(x0)
            e[c, k] = h
            col = (c * 3 + k) if k < 3 else (6 + c * 3 + k - 3)
            fd[:, col] = (f(x0 + e) - f(x0 - e)) / (2 * h)
    # central differences in fp64: truncation h^2 |f'''| ~ 1e-12, rounding eps |f| / h ~ 1e-9
    assert jac.abs().max() > 0.5
    assert (jac - fd).abs().max() < 1e-7, (jac - fd).abs().max()


def test_pose_refiner_poses_inverts_the_view():
    _, w2c, K = _rig()
    m = PoseRefiner(w2c, K, W, H).double()
    gen = torch.Generator().manual_seed(3)
    m.rot.data = 0.2 * torch.randn(3, 3, generator=gen, dtype=torch.float64)
    m.trans.data = 0.3 * torch.randn(3, 3, generator=gen, dtype=torch.float64)
    view, _, campos = m()
    c2w = m.poses()
    eye = torch.eye(4, dtype=torch.float64).expand(3, 4, 4)
    # the initial w2c and its stored inverse are fp32 numbers (rotations orthonormal to 2^-23 per entry,
    # translations of 2.5 + the twist rounded to 2^-23 x 3.5): products of four such terms
    fp32 = 4 * 2.0 ** -23 * 3.5
    assert (view.transpose(1, 2) @ c2w - eye).abs().max() < fp32  # view^T = w2c'
    assert (c2w[:, :3, 3] - campos).abs().max() < fp32  # the camera centre
    R = c2w[:, :3, :3]
    assert (R @ R.transpose(1, 2) - eye[:, :3, :3]).abs().max() < fp32  # still rigid
    assert (m.refined_w2c() - m.w2c).abs().max() > 0.05  # and moved


# ---- metrics.pose_errors

def test_pose_errors_equals_the_reference_fixture():
    z = np.load(os.path.join(REPO, "tests", "golden", "pose_errors.npz"))
    for name in ("perturbed", "identical", "pair"):
        got = pose_errors(torch.from_numpy(z[f"{name}.preds"]), z[f"{name}.targets"])
        # the same numpy fp64 operations on the same inputs
        np.testing.assert_allclose(got, z[f"{name}.errors"], rtol=1e-12, atol=1e-15)
    assert z["perturbed.preds"].shape == (6, 4, 4) and z["pair.preds"].shape == (2, 4, 4)
    assert np.all(z["identical.errors"] < 1e-14) and np.array_equal(z["identical.preds"], z["identical.targets"])
    assert np.all(z["perturbed.errors"] > 1e-2)
    with pytest.raises(ValueError):
        pose_errors(np.eye(4)[None], np.eye(4)[None])  # no relative pair
    with pytest.raises(ValueError):
        pose_errors(np.zeros((3, 3, 4)), np.zeros((3, 3, 4)))
