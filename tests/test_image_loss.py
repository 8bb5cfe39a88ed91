"""CPU tests of the photometric loss (no GPU needed):
  * photometric_loss_torch in fp64 reproduces the reference's loss and gradients
    (fixture tests/golden/photometric_loss.npz, recorded from the reference's
    helpers.py / external.py by tests/golden/make_golden_loss.py);
  * the library exports every symbol include/gs_loss.h declares, each with a
    ctypes prototype, and the ctypes mirror of gs_photo_loss has the library's size
    and the header's fields;
  * the host validator refuses every bad argument block with a message;
  * the wrapper refuses what the kernels cannot take (no CPU fallback);
  * the validator runs clean under AddressSanitizer + UndefinedBehaviorSanitizer in
    a stand-alone program (tools/loss_host_sanitize.c).
"""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from dynamic3dgaussians_amd import _lib, image_loss
from dynamic3dgaussians_amd import photometric_image_loss, photometric_loss, photometric_loss_torch
from tests._harness import run_host_sanitizer

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden", "photometric_loss.npz")
CASES = ("small", "masked", "flat", "features")


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def test_fixture_is_small_and_complete(gold):
    assert os.path.getsize(GOLD) < 512 * 1024
    shapes = {"small": (3, 9, 7), "masked": (3, 37, 53), "flat": (3, 37, 53), "features": (32, 13, 23)}
    for name in CASES:
        assert gold[f"{name}.image"].shape == shapes[name] and gold[f"{name}.image"].dtype == np.float32
        assert gold[f"{name}.grad_image"].dtype == np.float64
    flat_i, flat_t = gold["flat.image"], gold["flat.target"]
    assert not flat_i[:, :18].any() and not flat_t[:, :18].any()
    assert flat_i[1, 30, 20] == flat_t[1, 30, 20] != 0
    assert 0.7 < gold["masked.mask"].mean() < 0.9


@pytest.mark.parametrize("name", CASES)
def test_torch_restatement_matches_the_reference_in_fp64(gold, name):
    """Both sides are fp64 torch on the CPU running the same operations: 1e-12 relative leaves
    four orders over fp64 rounding and catches any change of formula, window or padding."""
    im = torch.from_numpy(gold[f"{name}.image"]).double().requires_grad_(True)
    cam_m = torch.from_numpy(gold[f"{name}.cam_m"]).double().requires_grad_(True)
    cam_c = torch.from_numpy(gold[f"{name}.cam_c"]).double().requires_grad_(True)
    target = torch.from_numpy(gold[f"{name}.target"]).double()
    mask = torch.from_numpy(gold[f"{name}.mask"])  # uint8, as the reference multiplies by it
    loss = photometric_loss_torch(im, target, mask=mask, gain=torch.exp(cam_m), offset=cam_c)
    g_im, g_m, g_c = torch.autograd.grad(loss, (im, cam_m, cam_c))
    ref = float(gold[f"{name}.loss"])
    assert abs(loss.item() - ref) <= 1e-12 * abs(ref)
    assert _rel(g_im, gold[f"{name}.grad_image"]) <= 1e-12
    assert _rel(g_m, gold[f"{name}.grad_cam_m"]) <= 1e-12
    assert _rel(g_c, gold[f"{name}.grad_cam_c"]) <= 1e-12


def test_torch_restatement_batch_reduction_and_driver_form(gold):
    """The batched restatement is the per-image one stacked: reduction, [B, H, W] masks, the
    (images, features) tuple and the cam_m / cam_c chain of photometric_image_loss's contract."""
    im = torch.from_numpy(gold["masked.image"]).double()
    tg = torch.from_numpy(gold["masked.target"]).double()
    mask = torch.from_numpy(gold["masked.mask"])
    cam_m = torch.from_numpy(gold["masked.cam_m"]).double()
    cam_c = torch.from_numpy(gold["masked.cam_c"]).double()
    one = photometric_loss_torch(im, tg, mask=mask, gain=torch.exp(cam_m), offset=cam_c)
    plain = photometric_loss_torch(tg, im)
    ims, tgs = torch.stack([im, tg]), torch.stack([tg, im])
    masks = torch.stack([mask, torch.ones_like(mask)])
    gain = torch.stack([torch.exp(cam_m), torch.ones(3, dtype=torch.float64)])
    offset = torch.stack([cam_c, torch.zeros(3, dtype=torch.float64)])
    vec = photometric_loss_torch(ims, tgs, mask=masks, gain=gain, offset=offset, reduction="none")
    assert vec.shape == (2,)
    torch.testing.assert_close(vec, torch.stack([one, plain]), rtol=1e-13, atol=0)
    total = photometric_loss_torch(ims, tgs, mask=masks, gain=gain, offset=offset)
    torch.testing.assert_close(total, vec.sum(), rtol=1e-14, atol=0)
    with pytest.raises(ValueError):
        photometric_loss_torch(ims, tgs, reduction="mean")


def _declared_symbols():
    txt = open(os.path.join(REPO, "include", "gs_loss.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(gs_[a-z_0-9]+)\s*\(", txt)))


def test_library_exports_every_symbol_of_gs_loss_h():
    L = _lib.load()
    names = _declared_symbols()
    assert {"gs_photo_loss_workspace_bytes", "gs_photo_loss_forward", "gs_photo_loss_backward"} <= set(names)
    for n in names:
        assert hasattr(L, n), n
        assert n in _lib.PROTOTYPES, f"{n} has no ctypes prototype"
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.lib_path()], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (gs_[a-z_0-9]+)", out))
    assert set(names) <= exported
    assert L.gs_version() == _lib.ABI_VERSION == 13  # a new header, no existing struct changed


def test_ctypes_mirror_has_the_library_size_and_the_header_fields():
    L = _lib.load()
    assert ctypes.sizeof(_lib.GsPhotoLoss) == L.gs_photo_loss_struct_bytes()
    src = open(os.path.join(REPO, "include", "gs_loss.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    body = re.search(r"typedef struct gs_photo_loss \{(.*?)\} gs_photo_loss;", src, flags=re.S).group(1)
    names = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        names += [re.findall(r"[A-Za-z_]\w*", part)[-1] for part in decl.split(",")]
    assert [f for f, _ in _lib.GsPhotoLoss._fields_] == names


def test_workspace_bytes():
    L = _lib.load()
    n = 2 * 3 * 37 * 53
    ws = L.gs_photo_loss_workspace_bytes(2, 3, 37, 53)
    assert 3 * 4 * n <= ws <= 3 * 4 * n + 64 * 1024  # three planes and the partial sums
    assert L.gs_photo_loss_workspace_bytes(27, 32, 800, 800) >= 3 * 4 * 27 * 32 * 800 * 800
    for bad in [(0, 3, 8, 8), (1, -1, 8, 8), (1, 3, 0, 8), (1, 3, 8, -2)]:
        assert L.gs_photo_loss_workspace_bytes(*bad) == 0


def _good_block(keep):
    """A valid argument block over host arrays (the validator dereferences nothing)."""
    L = _lib.load()
    B, Ch, H, W = 2, 3, 9, 7
    ws_bytes = L.gs_photo_loss_workspace_bytes(B, Ch, H, W)
    bufs = {k: np.zeros(B * Ch * H * W, np.float32) for k in ("image", "target", "d_image")}
    bufs["losses"] = np.zeros(B, np.float32)
    bufs["up"] = np.zeros(B, np.float32)
    bufs["ws"] = np.zeros(ws_bytes // 4 + 64, np.float32)
    keep.append(bufs)
    p = {k: v.ctypes.data for k, v in bufs.items()}
    p["ws"] = (p["ws"] + 255) // 256 * 256
    a = _lib.GsPhotoLoss(B=B, Ch=Ch, H=H, W=W, image=p["image"], target=p["target"], l1_weight=0.8,
                         ssim_weight=0.2, losses=p["losses"], workspace=p["ws"], workspace_bytes=ws_bytes)
    return a, p


def test_validator_rejects_bad_arguments_without_gpu():
    L = _lib.load()
    keep = []
    v = lambda a, bwd=0, up=None, di=None, dg=None, do=None: L.gs_photo_loss_validate(  # noqa: E731
        ctypes.byref(a), bwd, up, di, dg, do)
    a, p = _good_block(keep)
    assert v(a) == 0
    assert v(a, 1, p["up"], p["d_image"]) == 0
    assert L.gs_photo_loss_validate(None, 0, None, None, None, None) < 0 and b"null argument" in L.gs_last_error()
    for field, value, msg in [("B", 0, b"must be > 0"), ("Ch", -1, b"must be > 0"), ("H", 0, b"must be > 0"),
                              ("W", -5, b"must be > 0"), ("image", None, b"required"), ("target", None, b"required"),
                              ("losses", None, b"required"), ("image", p["image"] + 2, b"4-byte aligned"),
                              ("target", p["target"] + 1, b"4-byte aligned"),
                              ("workspace", None, b"workspace is required"), ("workspace_bytes", 16, b"needed"),
                              ("l1_weight", float("nan"), b"finite"), ("ssim_weight", float("inf"), b"finite"),
                              ("l1_weight", float("-inf"), b"finite")]:
        bad, _ = _good_block(keep)
        setattr(bad, field, value)
        assert v(bad) < 0, (field, value)
        assert msg in L.gs_last_error(), (field, L.gs_last_error())
    assert v(a, 1, None, p["d_image"]) < 0 and b"dL_dloss" in L.gs_last_error()
    assert v(a, 1, p["up"], None) < 0 and b"dL_dimage" in L.gs_last_error()
    assert v(a, 1, p["up"], p["d_image"] + 1) < 0 and b"4-byte aligned" in L.gs_last_error()
    # the entry points run the validator before anything touches a device
    bad, _ = _good_block(keep)
    bad.W = 0
    assert L.gs_photo_loss_forward(ctypes.byref(bad), None) < 0 and b"must be > 0" in L.gs_last_error()
    assert L.gs_photo_loss_backward(ctypes.byref(bad), p["up"], p["d_image"], None, None, None) < 0


def test_wrapper_rejects_what_the_kernels_cannot_take():
    im, tg = torch.rand(2, 3, 9, 7), torch.rand(2, 3, 9, 7)
    with pytest.raises(_lib.GsplatError, match="device tensors"):
        photometric_loss(im, tg)
    with pytest.raises(_lib.GsplatError, match="device tensors"):
        photometric_image_loss(im, tg)
    # the dtype / layout / shape rules are checked before any device work; _DeviceClaim lets
    # them be reached where there is no GPU
    for dtype in (torch.float16, torch.float64):
        with pytest.raises(_lib.GsplatError, match="float32"):
            image_loss._need(_DeviceClaim(torch.rand(2, 3, 9, 7).to(dtype)), "image")
    with pytest.raises(_lib.GsplatError, match="contiguous"):
        image_loss._need(_DeviceClaim(torch.rand(2, 3, 7, 9).transpose(2, 3)), "image")
    with pytest.raises(_lib.GsplatError, match="shape"):
        image_loss._need(_DeviceClaim(torch.rand(2, 3, 9, 8)), "target", (2, 3, 9, 7))
    with pytest.raises(_lib.GsplatError, match="no gradient"):
        photometric_loss(_DeviceClaim(im), _DeviceClaim(tg.clone().requires_grad_(True)))
    with pytest.raises(_lib.GsplatError, match="shape"):
        photometric_loss(_DeviceClaim(im), _DeviceClaim(torch.rand(2, 3, 9, 8)))
    with pytest.raises(_lib.GsplatError, match="float32"):
        photometric_loss(_DeviceClaim(im.half()), _DeviceClaim(tg.half()))
    with pytest.raises(_lib.GsplatError, match="float32"):
        photometric_loss(_DeviceClaim(im.double()), _DeviceClaim(tg.double()))
    with pytest.raises(_lib.GsplatError, match="contiguous"):
        photometric_loss(_DeviceClaim(torch.rand(2, 3, 7, 9).transpose(2, 3)), _DeviceClaim(tg))
    with pytest.raises(ValueError):
        photometric_loss(_DeviceClaim(im), _DeviceClaim(tg), reduction="mean")


class _DeviceClaim(torch.Tensor):
    """A host tensor that reports is_cuda, so the wrapper's dtype / layout / shape rules (all
    checked before any device work) can be exercised where there is no GPU."""

    @staticmethod
    def __new__(cls, t):
        return torch.Tensor._make_subclass(cls, t, t.requires_grad)

    @property
    def is_cuda(self):
        return True


@pytest.mark.skipif(shutil.which("gcc") is None or shutil.which("g++") is None, reason="gcc / g++ not available")
def test_validator_is_sanitizer_clean(tmp_path):
    """gs_loss_host.cpp (with gs_host.cpp's error state) under ASan + UBSan in a plain CPU
    executable with its own main: nothing preloaded, nothing loaded into Python."""
    run_host_sanitizer(tmp_path, "loss_host_sanitize.c", ["gs_loss_host.cpp", "gs_host.cpp"],
                       "loss host sanitize ok")
