"""CPU tests of the bilinear resample and the feature-distillation loss (no GPU needed):
  * the host axis export (gs_resample_axis, the function the kernels share) and the Python
    rule (resample.axis_tables) give bit-identical i0, l1 and first over the edge sizes, and
    first is a non-decreasing partition of [0, O);
  * bilinear_resize_torch in fp32 against F.interpolate on the CPU in fp32, forward and
    backward, in two tiers (below);
  * the adjoint identity <resize(x), g> = <x, resize^T(g)> in fp64;
  * the restatement reproduces the fixture tests/golden/feature_loss.npz, recorded from the
    reference's own statements by tests/golden/make_golden_feature_loss.py;
  * the library exports every symbol include/gs_resample.h declares, the ctypes mirror has
    the library's size and the header's fields, the ABI version is unchanged;
  * the host validator refuses every bad argument block with a message naming the field;
  * the wrappers refuse what the kernels cannot take (no CPU fallback);
  * the host code runs clean under AddressSanitizer + UndefinedBehaviorSanitizer in a
    stand-alone program (tools/resample_host_sanitize.c).

Bounds against F.interpolate (fp32, CPU), with u = 2^-24:
  tight  16 u max|x|: both sides blend the same four taps with the same fp32 weights; three
         lerps of at most 2.5 roundings each on either side.  Holds where the source
         coordinate is computed identically whatever the host compiler did: every
         align_corners=True case, and half-pixel cases whose product scale * (o + 0.5) is exact
         (identity sizes, 16 <-> 8, 8 -> 32).
  loose  4 u (H + W) max|x|: one ulp of a source coordinate of magnitude up to H (or W) moves
         the two weights of that axis by up to 2 u H, each times a tap of at most max|x|.  A
         wrong tap or a wrong rule is an O(max|x|) error.  Holds for every case.
The backward's bounds are the same per term, times max|g| and the number of output pixels that
tap one input pixel (the fan-in).
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

from dynamic3dgaussians_amd import (_lib, bilinear_resize, bilinear_resize_torch, distillation_image_loss,
                                    feature_distillation_loss, photometric_loss_torch, resample)
from tests._harness import run_host_sanitizer

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden", "feature_loss.npz")
U = 2.0 ** -24
AXIS_IN = (1, 2, 3, 7, 16, 37, 800, 1080, 32768)
AXIS_OUT = (1, 2, 3, 8, 12, 288, 512, 801)
# (H, W, h, w, half-pixel product exact)
SHAPES = [(1, 1, 1, 1, True), (1, 5, 3, 1, False), (7, 9, 7, 9, True), (16, 16, 8, 8, True), (8, 8, 16, 16, True),
          (8, 8, 32, 32, True), (37, 53, 12, 31, False), (12, 31, 37, 53, False), (130, 75, 47, 48, False),
          (200, 200, 72, 128, False), (800, 800, 288, 512, False)]


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


# ------------------------------------------------------------ the axis rule

@pytest.mark.parametrize("align", [False, True])
def test_host_axis_export_equals_the_python_rule_bit_for_bit(align):
    L = _lib.load()
    for I in AXIS_IN:  # noqa: E741
        for O in AXIS_OUT:  # noqa: E741
            i0 = np.full(O, -7, np.int32)
            l1 = np.full(O, np.nan, np.float32)
            first = np.full(I + 1, -7, np.int32)
            assert L.gs_resample_axis(I, O, int(align), i0.ctypes.data, l1.ctypes.data, first.ctypes.data) == 0
            p0, p1, pl0, pl1, pfirst = resample.axis_tables(I, O, align)
            assert np.array_equal(i0, p0), (I, O)
            assert np.array_equal(l1.view(np.uint32), pl1.view(np.uint32)), (I, O)
            assert np.array_equal(first, pfirst), (I, O)
            # first: a non-decreasing partition of [0, O) by lower tap
            assert first[0] == 0 and first[I] == O and (np.diff(first) >= 0).all()
            for i in np.unique(i0):
                assert (i0[first[i]:first[i + 1]] == i).all() and first[i + 1] - first[i] == (i0 == i).sum()
            assert np.array_equal(p1, np.minimum(p0 + 1, I - 1)) and (0 <= pl1).all() and (pl1 < 1).all()
            assert np.array_equal(pl0, np.float32(1) - pl1)
            if I == O:
                assert np.array_equal(i0, np.arange(O)) and not l1.any()


def test_axis_rule_values():
    """A few values by hand: the corner rule, the half-pixel rule, the clamp at 0 and at I - 1."""
    i0, i1, l0, l1, first = resample.axis_tables(5, 3, True)   # scale 2: src 0, 2, 4
    assert i0.tolist() == [0, 2, 4] and i1.tolist() == [1, 3, 4] and not l1.any()
    assert first.tolist() == [0, 1, 1, 2, 2, 3]
    i0, i1, l0, l1, first = resample.axis_tables(8, 4, False)  # scale 2: src 0.5, 2.5, 4.5, 6.5
    assert i0.tolist() == [0, 2, 4, 6] and l1.tolist() == [0.5] * 4
    i0, i1, l0, l1, first = resample.axis_tables(2, 4, False)  # scale 0.5: src -0.25 -> 0, 0.25, 0.75, 1.25
    assert i0.tolist() == [0, 0, 0, 1] and i1.tolist() == [1, 1, 1, 1] and l1.tolist() == [0.0, 0.25, 0.75, 0.25]
    i0, i1, l0, l1, first = resample.axis_tables(800, 1, False)  # one output: src 399.5
    assert i0.tolist() == [399] and l1.tolist() == [0.5] and first[399] == 0 and first[400] == 1
    i0, _, _, l1, _ = resample.axis_tables(7, 1, True)
    assert i0.tolist() == [0] and l1.tolist() == [0.0]


# ------------------------------------------------------------ against F.interpolate

def _input(H, W, B=2, Ch=3, seed=0, dtype=torch.float32):
    gen = torch.Generator().manual_seed(1000 * H + W + seed)
    return torch.randn(B, Ch, H, W, generator=gen, dtype=torch.float64).to(dtype)


def _fan_in(I, O, align):  # noqa: E741
    """The largest number of outputs that tap one input of an axis."""
    i0, i1, _, _, _ = resample.axis_tables(I, O, align)
    return int((np.bincount(i0, minlength=I) + np.bincount(i1, minlength=I)).max())


@pytest.mark.parametrize("align", [False, True])
@pytest.mark.parametrize("H,W,h,w,exact", SHAPES)
def test_restatement_against_torch_interpolate_in_fp32(H, W, h, w, exact, align):
    B, Ch = (1, 2) if H * W > 100000 else (2, 3)
    x = _input(H, W, B, Ch).requires_grad_(True)
    g = _input(h, w, B, Ch, seed=5)
    want = F.interpolate(x, size=(h, w), mode="bilinear", align_corners=align)
    got = bilinear_resize_torch(x, (h, w), align_corners=align)
    assert got.shape == want.shape and got.dtype == torch.float32
    (gw,) = torch.autograd.grad(want, x, g)
    (gg,) = torch.autograd.grad(got, x, g)
    xm, gm = float(x.detach().abs().max()), float(g.abs().max())
    err, gerr = float((got - want).detach().abs().max()), float((gg - gw).abs().max())
    fan = _fan_in(H, h, align) * _fan_in(W, w, align)
    print(f"{H}x{W}->{h}x{w} align={align}: fwd {err / (U * xm):.2f} u max|x|, bwd {gerr / (U * gm):.2f} u max|g| "
          f"(fan-in {fan})")
    assert err <= 4 * U * (H + W) * xm
    assert gerr <= 4 * U * (H + W) * gm * fan
    if exact or align:
        assert err <= 16 * U * xm
        assert gerr <= 16 * U * gm * fan
    if (H, W) == (h, w):
        assert torch.equal(got, x) and torch.equal(gg, g)


def test_layouts_and_dtypes_of_the_restatement():
    x = _input(9, 11, 2, 3)
    y = bilinear_resize_torch(x, (5, 4))
    assert torch.equal(bilinear_resize_torch(x[0], (5, 4)), y[0])
    assert torch.equal(bilinear_resize_torch(x[1, 2], (5, 4)), y[1, 2])
    y64 = bilinear_resize_torch(x.double(), (5, 4))
    assert y64.dtype == torch.float64 and float((y64 - y).abs().max()) <= 8 * U * float(x.abs().max())
    for bad in ((5,), (0, 4), (5, 40000), "ab"):
        with pytest.raises(_lib.GsplatError):
            bilinear_resize_torch(x, bad)
    with pytest.raises(_lib.GsplatError):
        bilinear_resize_torch(torch.zeros(3), (2, 2))


@pytest.mark.parametrize("align", [False, True])
@pytest.mark.parametrize("H,W,h,w", [(37, 53, 12, 31), (12, 31, 37, 53), (1, 5, 3, 1), (7, 9, 7, 9)])
def test_adjoint_identity_in_fp64(H, W, h, w, align):
    x = _input(H, W, dtype=torch.float64).requires_grad_(True)
    g = _input(h, w, seed=3, dtype=torch.float64)
    y = bilinear_resize_torch(x, (h, w), align_corners=align)
    (gt,) = torch.autograd.grad(y, x, g)
    lhs, rhs = float((y * g).sum()), float((x * gt).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs), 1e-300)
    # untouched inputs get exact zeros
    rows = np.zeros(H, bool)
    y0, y1, _, _, _ = resample.axis_tables(H, h, align)
    rows[y0], rows[y1] = True, True
    assert not gt[:, :, ~torch.from_numpy(rows)].any()


# ------------------------------------------------------------ the fixture

CASES = ("l1", "l1_ssim", "depth")


def test_fixture_is_small_and_complete(gold):
    assert os.path.getsize(GOLD) < 512 * 1024
    shapes = {"l1": ((2, 4, 40, 56), (2, 4, 18, 32)), "l1_ssim": ((2, 4, 40, 56), (2, 4, 18, 32)),
              "depth": ((1, 1, 37, 53), (1, 1, 12, 31))}
    for name in CASES:
        assert gold[f"{name}.feat"].shape == shapes[name][0] and gold[f"{name}.feat"].dtype == np.float32
        assert gold[f"{name}.target"].shape == shapes[name][1] and gold[f"{name}.target"].dtype == np.float32
        assert gold[f"{name}.resized"].shape == shapes[name][1] and gold[f"{name}.resized"].dtype == np.float64
        assert gold[f"{name}.grad_feat"].shape == shapes[name][0] and gold[f"{name}.grad_feat"].dtype == np.float64
        assert bool(gold[f"{name}.align_corners"]) == (name != "depth")
    assert (float(gold["l1.l1_weight"]), float(gold["l1.ssim_weight"])) == (1.0, 0.0)
    assert (float(gold["l1_ssim.l1_weight"]), float(gold["l1_ssim.ssim_weight"])) == (0.8, 0.2)


def _restated(gold, name, dtype, axis_dtype=torch.float32):
    """(resized, loss, d loss / d feat) of the package's torch restatement on the fixture's inputs."""
    x = torch.from_numpy(gold[f"{name}.feat"]).to(dtype).requires_grad_(True)
    tg = torch.from_numpy(gold[f"{name}.target"]).to(dtype)
    r = bilinear_resize_torch(x, tg.shape[-2:], align_corners=bool(gold[f"{name}.align_corners"]),
                              axis_dtype=axis_dtype)
    loss = photometric_loss_torch(r, tg, l1_weight=float(gold[f"{name}.l1_weight"]),
                                  ssim_weight=float(gold[f"{name}.ssim_weight"]))
    (g,) = torch.autograd.grad(loss, x)
    return r.detach(), loss.detach(), g


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference_in_fp64(gold, name):
    """fp64 on both sides and the same operations: 1e-10.  The reference's statements run on
    fp64 tensors, where F.interpolate evaluates the axis rule in fp64 too, so the restatement does
    the same here (axis_dtype=torch.float64); with the kernels' fp32 weights a map of this size
    differs from the fp64 one by up to 2^-24 (H + W) max|x|, which the next test bounds."""
    r, loss, g = _restated(gold, name, torch.float64, axis_dtype=torch.float64)
    err = float((r - torch.from_numpy(gold[f"{name}.resized"])).abs().max())
    lerr = abs(float(loss) - float(gold[f"{name}.loss"]))
    gerr = float((g - torch.from_numpy(gold[f"{name}.grad_feat"])).abs().max())
    print(f"{name}: resized {err:.3e}, loss {lerr:.3e}, grad {gerr:.3e}")
    assert err <= 1e-10 and lerr <= 1e-10 and gerr <= 1e-10


@pytest.mark.parametrize("name", CASES)
def test_restatement_in_fp32_is_within_the_loose_bound_of_the_fixture(gold, name):
    r, loss, g = _restated(gold, name, torch.float32)
    H, W = gold[f"{name}.feat"].shape[-2:]
    xm = float(np.abs(gold[f"{name}.feat"]).max())
    assert float((r.double() - torch.from_numpy(gold[f"{name}.resized"])).abs().max()) <= 4 * U * (H + W) * xm
    assert abs(float(loss) - float(gold[f"{name}.loss"])) <= 1e-5 * max(1.0, abs(float(gold[f"{name}.loss"])))
    ref = torch.from_numpy(gold[f"{name}.grad_feat"])
    assert float((g.double() - ref).norm() / ref.norm()) <= 1e-4


# ------------------------------------------------------------ the C boundary

def _header():
    txt = open(os.path.join(REPO, "include", "gs_resample.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_library_exports_every_symbol_of_gs_resample_h():
    L = _lib.load()
    names = sorted(set(re.findall(r"\b(gs_[a-z_0-9]+)\s*\(", _header())))
    assert names == ["gs_resample_axis", "gs_resample_backward", "gs_resample_forward", "gs_resample_struct_bytes",
                     "gs_resample_validate", "gs_resample_workspace_bytes"]
    for n in names:
        assert hasattr(L, n), n
        assert n in _lib.PROTOTYPES, f"{n} has no ctypes prototype"
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.lib_path()], capture_output=True, text=True).stdout
    assert set(names) <= set(re.findall(r" T (gs_[a-z_0-9]+)", out))
    assert L.gs_version() == _lib.ABI_VERSION == 13  # a new header, no existing struct changed


def test_ctypes_struct_mirrors_the_header():
    L = _lib.load()
    body = re.search(r"typedef struct gs_resample \{(.*?)\} gs_resample;", _header(), flags=re.S).group(1)
    names = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        names += [re.findall(r"[A-Za-z_]\w*", part)[-1] for part in decl.split(",")]
    fields = [f for f, _ in _lib.GsResample._fields_]
    assert fields == names == ["B", "Ch", "H", "W", "h", "w", "align_corners", "x", "y", "workspace",
                               "workspace_bytes"]
    assert ctypes.sizeof(_lib.GsResample) == L.gs_resample_struct_bytes()


def test_workspace_bytes():
    ws = _lib.load().gs_resample_workspace_bytes
    assert ws(37, 53) == 160 + 224 and ws(1, 1) == 32 and ws(800, 800) == 2 * 3216
    assert ws(32768, 32768) == 2 * 131088
    for bad in [(0, 8), (8, -1), (32769, 8), (8, 32769)]:
        assert ws(*bad) == 0


def _good_block(keep):
    """A valid argument block over host arrays (the validator dereferences nothing)."""
    L = _lib.load()
    B, Ch, H, W, h, w = 2, 3, 9, 7, 4, 5
    ws_bytes = L.gs_resample_workspace_bytes(H, W)
    bufs = {"x": np.zeros(B * Ch * H * W, np.float32), "d_x": np.zeros(B * Ch * H * W, np.float32),
            "y": np.zeros(B * Ch * h * w, np.float32), "d_y": np.zeros(B * Ch * h * w, np.float32),
            "ws": np.zeros(ws_bytes // 4 + 128, np.float32)}
    keep.append(bufs)
    p = {k: v.ctypes.data for k, v in bufs.items()}
    p["ws"] = (p["ws"] + 255) // 256 * 256
    a = _lib.GsResample(B=B, Ch=Ch, H=H, W=W, h=h, w=w, align_corners=0, x=p["x"], y=p["y"], workspace=p["ws"],
                        workspace_bytes=ws_bytes)
    return a, p


def test_validator_rejects_bad_arguments_without_gpu():
    L = _lib.load()
    keep = []
    v = lambda a, bwd=0, dy=None, dx=None: L.gs_resample_validate(ctypes.byref(a), bwd, dy, dx)  # noqa: E731
    a, p = _good_block(keep)
    assert v(a) == 0 and v(a, 1, p["d_y"], p["d_x"]) == 0
    a.align_corners = 1
    a.workspace, a.workspace_bytes = None, 0  # the forward needs no workspace
    assert v(a) == 0
    a, p = _good_block(keep)
    a.x, a.y = None, None  # the backward needs neither x nor y
    assert v(a, 1, p["d_y"], p["d_x"]) == 0
    assert L.gs_resample_validate(None, 0, None, None) < 0 and b"null argument" in L.gs_last_error()
    for field, value, msg in [("B", 0, b"B, Ch must be > 0"), ("Ch", -1, b"B, Ch must be > 0"),
                              ("H", 0, b"H, W must be in [1, 32768]"), ("W", 32769, b"H, W must be in [1, 32768]"),
                              ("H", -5, b"H, W must be in [1, 32768]"), ("h", 0, b"h, w must be in [1, 32768]"),
                              ("w", 32769, b"h, w must be in [1, 32768]"), ("x", None, b"x is required"),
                              ("y", None, b"y is required"), ("x", p["x"] + 2, b"x and y must be 4-byte aligned"),
                              ("y", p["y"] + 1, b"x and y must be 4-byte aligned")]:
        bad, _ = _good_block(keep)
        setattr(bad, field, value)
        assert v(bad) < 0, (field, value)
        assert msg in L.gs_last_error(), (field, L.gs_last_error())
    for field, value, msg in [("workspace", None, b"workspace is required"), ("workspace_bytes", 16, b"needed"),
                              ("workspace", p["ws"] + 4, b"16-byte aligned"), ("H", 0, b"H, W must be in"),
                              ("w", 0, b"h, w must be in")]:
        bad, q = _good_block(keep)
        setattr(bad, field, value)
        assert v(bad, 1, q["d_y"], q["d_x"]) < 0, (field, value)
        assert msg in L.gs_last_error(), (field, L.gs_last_error())
    a, p = _good_block(keep)
    assert v(a, 1, None, p["d_x"]) < 0 and b"d_y is required" in L.gs_last_error()
    assert v(a, 1, p["d_y"], None) < 0 and b"d_x is required" in L.gs_last_error()
    assert v(a, 1, p["d_y"], p["d_x"] + 1) < 0 and b"gradient pointers must be 4-byte aligned" in L.gs_last_error()
    assert v(a, 1, p["d_y"] + 2, p["d_x"]) < 0 and b"gradient pointers must be 4-byte aligned" in L.gs_last_error()
    # the entry points run the validator before anything touches a device
    bad, q = _good_block(keep)
    bad.W = 0
    assert L.gs_resample_forward(ctypes.byref(bad), None) < 0 and b"H, W must be in" in L.gs_last_error()
    assert L.gs_resample_backward(ctypes.byref(bad), q["d_y"], q["d_x"], None) < 0
    assert L.gs_resample_axis(0, 3, 0, None, None, None) < 0 and b"I, O must be in" in L.gs_last_error()
    assert L.gs_resample_axis(3, 32769, 1, None, None, None) < 0


class _DeviceClaim(torch.Tensor):
    """A host tensor that reports is_cuda, so the wrapper's dtype / layout / shape rules (all
    checked before any device work) can be exercised where there is no GPU."""

    @staticmethod
    def __new__(cls, t):
        return torch.Tensor._make_subclass(cls, t, t.requires_grad)

    @property
    def is_cuda(self):
        return True


def test_wrappers_reject_what_the_kernels_cannot_take():
    x = torch.rand(2, 3, 9, 7)
    for t in (x, x[0], x[0, 0]):
        with pytest.raises(_lib.GsplatError, match="device tensors"):
            bilinear_resize(t, (4, 5))
    for dtype in (torch.float16, torch.float64):
        with pytest.raises(_lib.GsplatError, match="float32"):
            bilinear_resize(_DeviceClaim(x.to(dtype)), (4, 5))
    with pytest.raises(_lib.GsplatError, match="contiguous"):
        bilinear_resize(_DeviceClaim(torch.rand(2, 3, 7, 9).transpose(2, 3)), (4, 5))
    with pytest.raises(_lib.GsplatError, match=r"\[B, Ch, H, W\]"):
        bilinear_resize(_DeviceClaim(torch.rand(2, 2, 3, 9, 7)), (4, 5))
    with pytest.raises(_lib.GsplatError, match="not be empty"):
        bilinear_resize(_DeviceClaim(torch.rand(2, 0, 9, 7)), (4, 5))
    for size in ((4,), (0, 5), (4, 32769), None):
        with pytest.raises(_lib.GsplatError, match="size must be"):
            bilinear_resize(_DeviceClaim(x), size)
    # the loss wrappers: host tensors, disagreeing leading dimensions, a render that is not a pair
    tg = torch.rand(2, 3, 4, 5)
    with pytest.raises(_lib.GsplatError, match="device tensors"):
        feature_distillation_loss(x, tg)
    with pytest.raises(_lib.GsplatError, match="must agree"):
        feature_distillation_loss(_DeviceClaim(x), _DeviceClaim(torch.rand(2, 4, 4, 5)))
    with pytest.raises(_lib.GsplatError, match="must agree"):
        feature_distillation_loss(_DeviceClaim(x), _DeviceClaim(tg[0]))
    with pytest.raises(_lib.GsplatError, match=r"\(images, feature maps\)"):
        distillation_image_loss(x, tg)
    with pytest.raises(_lib.GsplatError, match="device tensors"):
        distillation_image_loss((torch.rand(2, 3, 9, 7), x), (torch.rand(2, 3, 9, 7), tg))
    import inspect
    sig = inspect.signature(feature_distillation_loss)
    assert [(k, p.default) for k, p in list(sig.parameters.items())[2:]] == [
        ("mask", None), ("l1_weight", 1.0), ("ssim_weight", 0.0), ("align_corners", True), ("reduction", "sum")]
    assert inspect.signature(bilinear_resize).parameters["align_corners"].default is False
    assert inspect.signature(distillation_image_loss).parameters["feature_weight"].default == 1.0


@pytest.mark.skipif(shutil.which("gcc") is None or shutil.which("g++") is None, reason="gcc / g++ not available")
def test_host_code_is_sanitizer_clean(tmp_path):
    """gs_resample_host.cpp (with gs_host.cpp's error state) under ASan + UBSan in a plain CPU
    executable with its own main: nothing preloaded, nothing loaded into Python."""
    run_host_sanitizer(tmp_path, "resample_host_sanitize.c", ["gs_resample_host.cpp", "gs_host.cpp"],
                       "resample host sanitize ok")
