"""Temporal-window camera batches (include/gs_window.h), the parts that need
no GPU: the exported symbols, the ctypes mirror, the host validator
gs_check_window (through ctypes and in a stand-alone sanitizer program) and
GaussianRasterizerBatch's construction-time checks of `camera_frames`."""
from __future__ import annotations

import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

from dynamic3dgaussians_amd import _lib
from dynamic3dgaussians_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizerBatch
from tests._harness import run_host_sanitizer

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    txt = open(os.path.join(REPO, "include", "gs_window.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_library_exports_every_function_of_gs_window_h():
    L = _lib.load()
    names = sorted(set(re.findall(r"\b(gs_[a-z_0-9]+)\s*\(", _header())))
    assert set(names) == {"gs_check_window", "gs_forward_plan_batch_window", "gs_forward_batch_window",
                          "gs_backward_batch_window"}
    for n in names:
        assert hasattr(L, n), n
        assert n in _lib.PROTOTYPES, f"{n} has no ctypes prototype"
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.lib_path()], capture_output=True, text=True).stdout
    assert set(names) <= set(re.findall(r" T (gs_[a-z_0-9]+)", out))
    # the window forms take the batch calls' arguments plus the window
    for n in ("gs_forward_plan_batch", "gs_forward_batch", "gs_backward_batch"):
        base, win = _lib.PROTOTYPES[n][1], _lib.PROTOTYPES[n + "_window"][1]
        assert win == base[:-1] + [_lib.P_W] + base[-1:], n


def test_abi_version_is_unchanged():
    assert _lib.load().gs_version() == _lib.ABI_VERSION == 13  # a new header, no existing struct changed
    src = open(os.path.join(REPO, "include", "gsplat_hip.h")).read()
    assert re.search(r"#define GS_ABI_VERSION 13\b", src)


def test_ctypes_mirror_has_the_header_fields_in_order():
    src = _header()
    body = re.search(r"typedef struct gs_window \{(.*?)\} gs_window;", src, flags=re.S).group(1)
    names = [re.findall(r"[A-Za-z_]\w*", d)[-1] for d in filter(None, (d.strip() for d in body.split(";")))]
    assert names == ["B", "cam_frame"]
    assert [f for f, _ in _lib.GsWindow._fields_] == names
    assert ctypes.sizeof(_lib.GsWindow) == 16 and _lib.GsWindow.cam_frame.offset == 8
    assert _lib.GS_WINDOW_MAX_FRAMES == 64 and re.search(r"#define GS_WINDOW_MAX_FRAMES 64\b", src)


def _check(B, frames, C=None):
    L = _lib.load()
    arr = (ctypes.c_int32 * max(len(frames), 1))(*frames)
    w = _lib.GsWindow(B=B, cam_frame=arr)
    return L.gs_check_window(ctypes.byref(w), len(frames) if C is None else C)


def test_check_window_accepts_valid_windows():
    assert _check(1, [0]) == 0
    assert _check(3, [0, 0, 2, 2]) == 0
    assert _check(64, list(range(64))) == 0


@pytest.mark.parametrize("B,frames,msg", [
    (0, [0], b"B must be in [1, 64]"),
    (65, [0], b"B must be in [1, 64]"),
    (2, [0, 1, 2], b"cam_frame[2] = 2 is outside [0, 2)"),      # a frame equal to B
    (2, [-1, 0], b"cam_frame[0] = -1 is outside [0, 2)"),       # a negative frame
    (2, [0, 1, 0], b"non-decreasing"),                          # a decreasing pair
    (2, [1, 0], b"non-decreasing"),
    (1, [1], b"cam_frame[0] = 1 is outside [0, 1)"),            # C = 1, its frame out of range
])
def test_check_window_rejects_invalid_windows(B, frames, msg):
    L = _lib.load()
    assert _check(B, frames) != 0
    err = L.gs_last_error()
    assert err and msg in err, err


def test_check_window_rejects_null():
    L = _lib.load()
    assert L.gs_check_window(None, 1) != 0
    assert b"null window" in L.gs_last_error()
    w = _lib.GsWindow(B=2, cam_frame=None)
    assert L.gs_check_window(ctypes.byref(w), 1) != 0
    assert b"null cam_frame" in L.gs_last_error()
    assert _check(1, [0], C=0) != 0 and b"camera count" in L.gs_last_error()


def test_entry_points_run_the_validator_before_anything_touches_a_device():
    """A bad window is refused by the three *_window entry points with the
    validator's message; the other arguments are never looked at."""
    L = _lib.load()
    arr = (ctypes.c_int32 * 2)(1, 0)
    w = _lib.GsWindow(B=2, cam_frame=arr)
    g, cams = _lib.GsGaussians(), (_lib.GsCamera * 2)()
    one = ctypes.c_int64(0)
    fits = ctypes.c_int32(0)
    assert L.gs_forward_plan_batch_window(ctypes.byref(g), cams, 2, 0, 0, 0, None, None, None, ctypes.byref(one),
                                          None, ctypes.byref(w), None) < 0
    assert b"non-decreasing" in L.gs_last_error()
    assert L.gs_forward_batch_window(ctypes.byref(g), cams, 2, 0, 0, None, None, None, ctypes.byref(one), None, None,
                                     ctypes.byref(one), ctypes.byref(one), ctypes.byref(fits), None, None, None,
                                     None, ctypes.byref(w), None) < 0
    assert b"non-decreasing" in L.gs_last_error()
    assert L.gs_backward_batch_window(ctypes.byref(g), cams, 2, None, 0, 0, None, None, None, ctypes.byref(one),
                                      *([None] * 15), ctypes.byref(w), None) < 0
    assert b"non-decreasing" in L.gs_last_error()


def _cpu_settings(C, W=64, H=48):
    eye = torch.eye(4)
    return [GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=0.5, tanfovy=0.5, bg=torch.zeros(3),
                                          viewmatrix=eye, projmatrix=eye, campos=torch.zeros(3)) for _ in range(C)]


def test_rasterizer_validates_camera_frames_at_construction():
    sets = _cpu_settings(2)
    with pytest.raises(ValueError, match="3 entries for 2 cameras"):
        GaussianRasterizerBatch(sets, camera_frames=[0, 0, 1])
    with pytest.raises(ValueError, match=">= 0"):
        GaussianRasterizerBatch(sets, camera_frames=[-1, 0])
    with pytest.raises(ValueError, match="non-decreasing"):
        GaussianRasterizerBatch(sets, camera_frames=[1, 0])
    with pytest.raises(ValueError, match="at most 64 frames"):
        GaussianRasterizerBatch(sets, camera_frames=[0, 64])
    assert GaussianRasterizerBatch(sets, camera_frames=(0, 3)).camera_frames == [0, 3]
    assert GaussianRasterizerBatch(sets).camera_frames is None


def test_rasterizer_checks_the_means_of_a_window_before_any_device_work():
    ras = GaussianRasterizerBatch(_cpu_settings(2), camera_frames=[0, 2])
    kw = dict(means2D=torch.zeros(5, 3), opacities=torch.ones(5, 1), colors_precomp=torch.ones(5, 3),
              scales=torch.ones(5, 3), rotations=torch.ones(5, 4))
    with pytest.raises(ValueError, match=r"\(P, B, 3\) with B > 2"):
        ras(means3D=torch.zeros(5, 3), **kw)
    with pytest.raises(ValueError, match=r"\(P, B, 3\) with B > 2"):
        ras(means3D=torch.zeros(5, 2, 3), **kw)
    with pytest.raises(ValueError, match="contiguous"):
        ras(means3D=torch.zeros(3, 5, 3).transpose(0, 1), **kw)


@pytest.mark.skipif(shutil.which("gcc") is None or shutil.which("g++") is None, reason="gcc / g++ not available")
def test_validator_is_sanitizer_clean(tmp_path):
    """gs_window_host.cpp (with gs_host.cpp's error state) under ASan + UBSan in a plain CPU
    executable with its own main: nothing preloaded, nothing loaded into Python."""
    run_host_sanitizer(tmp_path, "window_host_sanitize.c", ["gs_window_host.cpp", "gs_host.cpp"],
                       "window host sanitize ok")
