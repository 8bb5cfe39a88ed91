"""The feature decoder without a GPU: the PyTorch twins against F.conv2d + l1_loss + autograd
and against the reference-generated fixture, the module's state_dict contract, the host
validator (through ctypes and, under ASan + UBSan, as a stand-alone program), the build list
and the decoder argument of decoded_distillation_loss."""
from __future__ import annotations

import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dynamic3dgaussians_amd import (FeatureDecoder, _lib, bilinear_resize_torch, build, decode_features,
                                    decode_features_torch, decoded_distillation_loss, decoded_l1_loss,
                                    decoded_l1_loss_torch, distillation_image_loss, feature_distillation_loss)
from dynamic3dgaussians_amd._lib import GsplatError
from tests._harness import run_host_sanitizer
from tests.golden import make_golden_feature_decoder as gen

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "feature_decoder.npz")


def _inputs(B=2, F_in=5, C_out=7, h=6, w=9, seed=0, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, F_in, h, w, generator=g, dtype=dtype)
    W = torch.randn(C_out, F_in, generator=g, dtype=dtype)
    b = torch.randn(C_out, generator=g, dtype=dtype)
    t = torch.randn(B, C_out, h, w, generator=g, dtype=dtype)
    return x, W, b, t


@pytest.mark.parametrize("with_bias", [True, False])
def test_twins_are_conv2d_and_l1_loss(with_bias):
    x, W, b, t = _inputs()
    if not with_bias:
        b = None
    leaves = [v.clone().requires_grad_() for v in (x, W) + ((b,) if with_bias else ())]
    ref = [v.clone().requires_grad_() for v in (x, W) + ((b,) if with_bias else ())]
    y = decode_features_torch(leaves[0], leaves[1], leaves[2] if with_bias else None)
    y_ref = F.conv2d(ref[0], ref[1][:, :, None, None], ref[2] if with_bias else None)
    assert y.shape == y_ref.shape and float((y - y_ref).detach().abs().max()) <= 1e-13
    # one map, and the conv's own weight shape
    y1 = decode_features_torch(x[0], W[:, :, None, None], b)
    assert y1.shape == y_ref.shape[1:] and float((y1 - y_ref[0]).detach().abs().max()) <= 1e-13
    loss = decoded_l1_loss_torch(*leaves[:2], leaves[2] if with_bias else None, t)
    want = sum(F.l1_loss(y_ref[i], t[i]) for i in range(x.shape[0]))
    assert abs(loss.item() - want.item()) <= 1e-13
    for a, r in zip(torch.autograd.grad(loss, leaves), torch.autograd.grad(want, ref)):
        assert float((a - r).abs().max()) <= 1e-13 * max(1.0, float(r.abs().max()))
    per_cam = decoded_l1_loss_torch(x, W, b, t, reduction="none")
    assert per_cam.shape == (2,) and abs(per_cam.sum().item() - want.item()) <= 1e-13


def test_twin_mask_is_l1_loss_of_the_masked_maps():
    x, W, b, t = _inputs(seed=1)
    g = torch.Generator().manual_seed(2)
    for m in (torch.rand(6, 9, generator=g, dtype=torch.float64), torch.rand(2, 6, 9, generator=g, dtype=torch.float64)):
        m = torch.where(m < 0.3, torch.zeros((), dtype=torch.float64), m)
        y = F.conv2d(x, W[:, :, None, None], b)
        per_cam = [m[i][None] if m.dim() == 3 else m for i in range(2)]
        want = sum(F.l1_loss(y[i] * per_cam[i], t[i] * per_cam[i]) for i in range(2))
        assert abs(decoded_l1_loss_torch(x, W, b, t, mask=m).item() - want.item()) <= 1e-13


@pytest.mark.parametrize("name", list(gen.CASES))
def test_twin_reproduces_the_reference_fixture(name):
    """revise_train.py:101-104 with torch's own 1x1 conv as the decoder, all in fp64."""
    gold = np.load(GOLDEN)
    F_in, C_out, H, W_, h, w = gen.CASES[name]
    feat, target, weight, bias = gen.case_inputs(name)
    for k, v in (("feat", feat), ("target", target), ("weight", weight), ("bias", bias)):
        assert np.array_equal(gold[f"{name}.{k}"].astype(np.float32), v.numpy()), k  # the seeded inputs are the stored ones
    x = torch.from_numpy(gold[f"{name}.feat"].astype(np.float64)).requires_grad_()
    Wt = torch.from_numpy(gold[f"{name}.weight"].astype(np.float64)).requires_grad_()
    b = torch.from_numpy(gold[f"{name}.bias"].astype(np.float64)).requires_grad_()
    t = torch.from_numpy(gold[f"{name}.target"].astype(np.float64))
    resized = bilinear_resize_torch(x, (h, w), align_corners=True, axis_dtype=torch.float64)
    loss = decoded_l1_loss_torch(resized, Wt, b, t)
    want = float(gold[f"{name}.loss"])
    assert abs(loss.item() - want) <= 1e-12 * abs(want)
    for got, key in zip(torch.autograd.grad(loss, (x, Wt, b)), ("grad_feat", "grad_weight", "grad_bias")):
        ref = gold[f"{name}.{key}"]
        err = float(np.abs(got.numpy() - ref).max())
        print(f"{name}.{key}: max error {err:.3e} of max {np.abs(ref).max():.3e}")
        assert got.shape == ref.shape and err <= 1e-12 * float(np.abs(ref).max())


def test_fixture_is_small():
    assert os.path.getsize(GOLDEN) < 1 << 20


def test_module_contract():
    torch.manual_seed(0)
    dec = FeatureDecoder(6, 12)
    assert list(dec.state_dict()) == ["conv.weight", "conv.bias"]
    assert dec.conv.weight.shape == (12, 6, 1, 1) and len(list(dec.parameters())) == 2

    class Upstream(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.conv = torch.nn.Conv2d(6, 12, kernel_size=1)

        def forward(self, x):
            return self.conv(x)

    torch.manual_seed(0)
    up = Upstream()
    assert torch.equal(up.conv.weight, dec.conv.weight) and torch.equal(up.conv.bias, dec.conv.bias)  # torch's own init
    other = Upstream()
    other.load_state_dict(dec.state_dict())
    back = FeatureDecoder(6, 12)
    back.load_state_dict(other.state_dict())
    assert torch.equal(back.conv.weight, dec.conv.weight) and torch.equal(back.conv.bias, dec.conv.bias)
    x = torch.randn(6, 4, 5)
    y = decode_features_torch(x, dec.conv.weight, dec.conv.bias)
    assert y.shape == (12, 4, 5) and float((y - up(x)).detach().abs().max()) <= 1e-5
    with pytest.raises(GsplatError, match="_torch"):  # the HIP path has no CPU fallback
        dec(x)
    with pytest.raises(GsplatError, match="_torch"):
        dec.loss(x, torch.zeros(12, 4, 5))


def test_shape_and_argument_errors():
    x, W, b, t = _inputs(dtype=torch.float32)
    for call in (lambda: decode_features_torch(x, W[:, :4], b), lambda: decode_features_torch(x, W, b[:3]),
                 lambda: decode_features_torch(x[0, 0], W, b), lambda: decode_features_torch(x, W[None], b),
                 lambda: decoded_l1_loss_torch(x, W, b, t[:, :5]), lambda: decoded_l1_loss_torch(x, W, b, t[0]),
                 lambda: decoded_l1_loss_torch(x, W, b, t, mask=torch.ones(9, 6)),
                 lambda: decoded_l1_loss_torch(x, W, b, t, reduction="mean"),
                 lambda: decoded_l1_loss_torch(x, W, b, t.clone().requires_grad_()),
                 lambda: decoded_l1_loss(x, W, b, t.clone().requires_grad_()),
                 lambda: decoded_l1_loss(x, W, b, t), lambda: decode_features(x, W, b)):
        with pytest.raises(GsplatError):
            call()


def test_distillation_loss_checks_the_decoder_argument_on_the_cpu():
    feat, target = torch.zeros(2, 5, 8, 8), torch.zeros(2, 7, 4, 4)
    W, b = torch.zeros(7, 5), torch.zeros(7)
    with pytest.raises(GsplatError, match="FeatureDecoder or a"):
        decoded_distillation_loss(feat, target, W)
    with pytest.raises(GsplatError, match="5 -> 7 decoder"):
        decoded_distillation_loss(feat, torch.zeros(2, 5, 4, 4), (W, b))
    with pytest.raises(GsplatError, match="5 -> 7 decoder"):
        decoded_distillation_loss(torch.zeros(2, 7, 8, 8), target, FeatureDecoder(5, 7))
    with pytest.raises(GsplatError, match="weight must be"):
        decoded_distillation_loss(feat, target, (torch.zeros(7), b))
    with pytest.raises(GsplatError, match="on the CPU"):  # well-formed: it reaches the HIP resample, which refuses
        decoded_distillation_loss(feat, target, (W, b))
    with pytest.raises(GsplatError, match="agree in all but"):  # no decoder: the unchanged function and its check
        feature_distillation_loss(feat, target)
    import inspect
    assert "decoder" not in inspect.signature(feature_distillation_loss).parameters
    assert inspect.signature(distillation_image_loss).parameters["decoder"].default is None


def test_build_lists_the_new_sources():
    assert build.SOURCES["gs_feature_decoder.hip"] == ["-ffp-contract=off"]
    assert "gs_feature_decoder_host.cpp" in build.SOURCES
    for f in ("gs_feature_decoder.hip", "gs_feature_decoder_host.cpp", "gs_feature_decoder_layout.h", "gs_split_mfma.h"):
        assert os.path.exists(os.path.join(build.CSRC, f))
    with open(os.path.join(build.CSRC, "gs_render.hip")) as fh:
        render = fh.read()
    assert '#include "gs_split_mfma.h"' in render  # one home for the split helpers
    for definition in ("void split_bf16(", "struct bsplit", "struct hsplit"):
        assert definition not in render


def test_ctypes_mirror_and_documented_constants():
    L = _lib.load()
    assert ctypes.sizeof(_lib.GsFeatureDecoder) == L.gs_feature_decoder_struct_bytes()
    with open(os.path.join(REPO, "include", "gs_feature_decoder.h")) as fh:
        header = fh.read()
    for name, value in (("GS_FD_TILE_ROWS", _lib.FD_TILE_ROWS), ("GS_FD_TILE_PIXELS", _lib.FD_TILE_PIXELS),
                        ("GS_FD_GRID", _lib.FD_GRID), ("GS_FD_GRID_FORWARD", _lib.FD_GRID_FORWARD), ("GS_FD_MAX_F_IN", _lib.FD_MAX_F_IN),
                        ("GS_FD_MAX_C_OUT", _lib.FD_MAX_C_OUT), ("GS_FD_MAX_WEIGHTS", _lib.FD_MAX_WEIGHTS),
                        ("GS_FD_PASS_DECODE", 0), ("GS_FD_PASS_LOSS", 1), ("GS_FD_PASS_LOSS_BACKWARD", 2),
                        ("GS_FD_PASS_BACKWARD", 3)):
        assert f"#define {name} {value}\n" in header or f"#define {name} {value} " in header, name
    # the grid rule, n_t and n_acc as the header states them
    for B, h, w in ((1, 1, 1), (3, 72, 128), (27, 288, 512), (1, 288, 512), (300, 5, 9)):
        tiles = -(-h * w // _lib.FD_TILE_PIXELS)
        gx = min(tiles, max(1, _lib.FD_GRID // B))
        assert L.gs_feature_decoder_grid_x(B, h, w) == gx
        assert L.gs_feature_decoder_n_acc(B, h, w) == -(-tiles // gx) * _lib.FD_TILE_PIXELS
    for C in (1, 32, 33, 512):
        assert L.gs_feature_decoder_n_t(C) == 16 * -(-C // 32)
    # slabs by the grid, never by the pixels
    small = L.gs_feature_decoder_workspace_bytes(1, 32, 64, 288, 512, _lib.FD_PASS_LOSS_BACKWARD)
    assert L.gs_feature_decoder_workspace_bytes(1, 32, 64, 2880, 5120, _lib.FD_PASS_LOSS_BACKWARD) == small


def _block(**kw):
    buf = ctypes.create_string_buffer(4096)
    base = ctypes.addressof(buf) // 16 * 16 + 16
    a = _lib.GsFeatureDecoder(B=2, F_in=8, C_out=16, h=4, w=5, workspace=base, workspace_bytes=1 << 30)
    for k in ("x", "weight", "bias", "target", "mask", "up", "d_y", "y", "loss", "d_x", "d_weight", "d_bias"):
        setattr(a, k, base)
    for k, v in kw.items():
        setattr(a, k, v)
    a._keep = buf
    return a


@pytest.mark.parametrize("field,value,which,message", [
    ("B", 0, 0, "B must be in"), ("F_in", 0, 0, "F_in must be in"), ("F_in", 65, 1, "_torch"),
    ("C_out", 0, 0, "C_out must be in"), ("C_out", 513, 2, "_torch"), ("C_out", 2049, 3, "_torch"),
    ("h", 0, 0, "h, w must be"), ("w", 0, 0, "h, w must be"),
    ("x", None, 0, "x is required"), ("x", None, 3, "x is required"), ("weight", None, 1, "weight is required"),
    ("y", None, 0, "y is required"), ("target", None, 1, "target is required"), ("target", None, 2, "target is required"),
    ("loss", None, 1, "loss is required"), ("up", None, 2, "up is required"), ("d_y", None, 3, "d_y is required"),
    ("d_x", None, 2, "d_x is required"), ("d_x", None, 3, "d_x is required"),
    ("d_weight", None, 2, "d_weight is required"), ("d_weight", None, 3, "d_weight is required"),
    ("workspace", None, 0, "workspace is required"), ("workspace_bytes", 64, 2, "needed"),
])
def test_validator_refuses_with_a_message(field, value, which, message):
    L = _lib.load()
    for p in range(4):
        assert L.gs_feature_decoder_validate(ctypes.byref(_block()), p) == 0
    assert L.gs_feature_decoder_validate(ctypes.byref(_block(**{field: value})), which) != 0
    assert message in L.gs_last_error().decode()


def test_validator_refuses_the_weight_limit_and_names_the_twin():
    L = _lib.load()
    assert L.gs_feature_decoder_validate(ctypes.byref(_block(F_in=64, C_out=256)), 0) == 0
    assert L.gs_feature_decoder_validate(ctypes.byref(_block(F_in=32, C_out=512)), 0) == 0
    assert L.gs_feature_decoder_validate(ctypes.byref(_block(F_in=64, C_out=257)), 0) != 0
    msg = L.gs_last_error().decode()
    assert "16384" in msg and "decoded_l1_loss_torch" in msg and "decode_features_torch" in msg
    assert L.gs_feature_decoder_validate(None, 0) != 0 and "null argument block" in L.gs_last_error().decode()
    assert L.gs_feature_decoder_validate(ctypes.byref(_block()), 7) != 0 and "unknown pass" in L.gs_last_error().decode()


def test_validator_is_sanitizer_clean(tmp_path):
    """gs_feature_decoder_host.cpp (with gs_host.cpp's error state) under ASan + UBSan in a plain
    CPU executable with its own main: nothing preloaded, nothing loaded into Python."""
    run_host_sanitizer(tmp_path, "feature_decoder_host_sanitize.c", ["gs_feature_decoder_host.cpp", "gs_host.cpp"],
                       "feature decoder host sanitize ok")
