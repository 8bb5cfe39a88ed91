"""CPU tests of the depth-correlation loss (no GPU needed):
  * depth_correlation_loss_torch in fp64 reproduces the reference's loss and gradient
    (fixture tests/golden/depth_loss.npz, recorded from the statements of the
    reference's dyn_train.py:256-265 by tests/golden/make_golden_depth_loss.py), in all
    three accepted layouts of the plane;
  * the closed-form gradient the kernel implements equals autograd through the
    restatement;
  * degenerate cameras, both ways of handling them;
  * the library exports every symbol include/gs_depth_loss.h declares, each with a
    ctypes prototype, and the ctypes mirror of gs_depth_loss has the library's size and
    the header's fields;
  * the host validator refuses every bad argument block with a message naming the field;
  * the wrapper refuses what the kernels cannot take (no CPU fallback);
  * the validator runs clean under AddressSanitizer + UndefinedBehaviorSanitizer in a
    stand-alone program (tools/depth_loss_host_sanitize.c);
  * TimestepDriver: unchanged without depth_loss, the hand-assembled sum with it.
"""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from dynamic3dgaussians_amd import _lib, depth_correlation_loss, depth_correlation_loss_torch, depth_loss
from dynamic3dgaussians_amd.timesteps import TimestepDriver, batch_renderer, l1_image_loss, params2rendervar
from tests._harness import run_host_sanitizer

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden", "depth_loss.npz")
CASES = ("tiny", "masked", "gated")
LAYOUTS = ("B1HW", "BHW", "HW")


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def test_fixture_is_small_and_complete(gold):
    assert os.path.getsize(GOLD) < 512 * 1024
    shapes = {"tiny": (3, 5), "masked": (37, 53), "gated": (37, 53)}
    for name in CASES:
        assert gold[f"{name}.depth"].shape == shapes[name] and gold[f"{name}.depth"].dtype == np.float32
        assert gold[f"{name}.target"].dtype == np.float32 and gold[f"{name}.mask"].dtype == np.uint8
        assert gold[f"{name}.grad_depth"].dtype == np.float64 and gold[f"{name}.grad_depth"].shape == shapes[name]
        assert float(gold[f"{name}.near"]) == 1e-7 and float(gold[f"{name}.far"]) == 50.0
    assert gold["tiny.mask"].all()
    assert 0.7 < gold["masked.mask"].mean() < 0.9 and 0.7 < gold["gated.mask"].mean() < 0.9
    d = gold["gated.depth"]
    assert 0.05 < (d == 80.0).mean() < 0.15 and 0.005 < (d == 0.0).mean() < 0.04
    assert 1.0 <= gold["masked.depth"].min() and gold["masked.depth"].max() <= 10.0


def _shaped(x, layout):
    return {"B1HW": x[None, None], "BHW": x[None], "HW": x}[layout]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", CASES)
def test_torch_restatement_matches_the_reference_in_fp64(gold, name, layout):
    """Both sides are fp64 torch on the CPU running the same operations: 1e-12 leaves four
    orders over fp64 rounding and catches any change of formula, order or gate."""
    d = _shaped(torch.from_numpy(gold[f"{name}.depth"]).double(), layout).clone().requires_grad_(True)
    g = _shaped(torch.from_numpy(gold[f"{name}.target"]).double(), layout)
    mask = None if name == "tiny" else torch.from_numpy(gold[f"{name}.mask"])
    loss = depth_correlation_loss_torch(d, g, mask=mask)
    (grad,) = torch.autograd.grad(loss, d)
    ref = float(gold[f"{name}.loss"])
    assert loss.dim() == 0 and grad.shape == d.shape
    assert abs(loss.item() - ref) <= 1e-12 * max(1.0, abs(ref))
    assert _rel(grad.reshape(gold[f"{name}.grad_depth"].shape), gold[f"{name}.grad_depth"]) <= 1e-12
    gated = (gold[f"{name}.mask"] == 0) | (gold[f"{name}.depth"] > 50.0) | (gold[f"{name}.depth"] < 1e-7)
    assert not grad.detach().numpy().reshape(gated.shape)[gated].any()


def closed_form(depth, target, mask, near, far, up):
    """The gradient of include/gs_depth_loss.h in plain tensor operations (one camera)."""
    m = torch.ones_like(depth, dtype=torch.bool) if mask is None else mask != 0
    p = 1 / torch.clamp(depth, near, far)
    pm, gm = p[m], target[m]
    pbar, gbar = pm.mean(), gm.mean()
    sxx, syy = ((pm - pbar) ** 2).sum(), ((gm - gbar) ** 2).sum()
    sxy = ((pm - pbar) * (gm - gbar)).sum()
    r = sxy / torch.sqrt(sxx * syy)
    grad = up * ((target - gbar) - (sxy / sxx) * (p - pbar)) / torch.sqrt(sxx * syy) / depth ** 2
    gate = m & (depth >= near) & (depth <= far) & (r.abs() <= 1)
    return torch.where(gate, grad, torch.zeros_like(grad)), 1 - r.clamp(-1, 1)


@pytest.mark.parametrize("name", CASES)
def test_closed_form_gradient_equals_autograd_in_fp64(gold, name):
    d = torch.from_numpy(gold[f"{name}.depth"]).double().requires_grad_(True)
    g = torch.from_numpy(gold[f"{name}.target"]).double()
    mask = torch.from_numpy(gold[f"{name}.mask"])
    up = -0.37
    loss = depth_correlation_loss_torch(d, g, mask=mask)
    (auto,) = torch.autograd.grad(loss * up, d)
    want, loss_cf = closed_form(d.detach(), g, mask, 1e-7, 50.0, up)
    assert abs(loss.item() - loss_cf.item()) <= 1e-12
    err = _rel(want, auto)
    print(f"{name}: closed form against autograd, rel L2 {err:.3e}")
    assert err <= 1e-10
    assert torch.equal(want == 0, auto == 0)  # the gates agree pixel for pixel


def test_batch_reduction_masks_and_stats(gold):
    """The batched restatement is the per-camera one stacked; [H, W] and [B, H, W] masks of any
    dtype; the statistics row."""
    d = torch.stack([torch.from_numpy(gold[f"{n}.depth"]).double() for n in ("masked", "gated")])
    g = torch.stack([torch.from_numpy(gold[f"{n}.target"]).double() for n in ("masked", "gated")])
    m = torch.stack([torch.from_numpy(gold[f"{n}.mask"]) for n in ("masked", "gated")])
    vec, stats = depth_correlation_loss_torch(d, g, mask=m, reduction="none", return_stats=True)
    assert vec.shape == (2,) and stats.shape == (2, 8)
    np.testing.assert_allclose(vec.numpy(), [gold["masked.loss"], gold["gated.loss"]], rtol=1e-12)
    np.testing.assert_allclose(stats[:, 0].numpy(), m.sum(dim=(1, 2)).numpy())
    np.testing.assert_allclose((1 - stats[:, 6]).numpy(), vec.numpy(), rtol=1e-10)
    assert stats[:, 7].tolist() == [1.0, 1.0]
    total = depth_correlation_loss_torch(d[:, None], g[:, None], mask=m.bool())
    torch.testing.assert_close(total, vec.sum(), rtol=1e-14, atol=0)
    shared = depth_correlation_loss_torch(d, g, mask=m[0].float() * 3.0, reduction="none")
    assert shared[0] == vec[0] and shared[1] != vec[1]
    with pytest.raises(ValueError):
        depth_correlation_loss_torch(d, g, reduction="mean")


def _degenerate(kind, dtype):
    """Three cameras of 6 x 7, camera 1 degenerate."""
    gen = torch.Generator().manual_seed(31)
    d = (2.0 + 3.0 * torch.rand(3, 6, 7, generator=gen)).to(dtype)
    g = (1.0 / d + 0.05 * torch.randn(3, 6, 7, generator=gen).to(dtype))
    m = torch.ones(3, 6, 7, dtype=torch.uint8)
    m[0, 0, :3] = 0
    if kind == "empty_mask":
        m[1] = 0
    elif kind == "one_pixel":
        m[1] = 0
        m[1, 2, 3] = 1
    elif kind == "constant_depth":
        d[1] = 2.0
    elif kind == "beyond_far":
        d[1] = 60.0 + 10.0 * torch.rand(6, 7, generator=gen).to(dtype)
    return d, g, m


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("kind", ["empty_mask", "one_pixel", "constant_depth", "beyond_far"])
def test_degenerate_cameras_both_ways(kind, dtype):
    d, g, m = _degenerate(kind, dtype)
    healthy = d.clone()
    healthy[1] = d[0].flip(0)
    hm = m.clone()
    hm[1] = 1
    want = depth_correlation_loss_torch(healthy, g, mask=hm, reduction="none")
    # default: the reference's NaN, in that camera only
    dd = d.clone().requires_grad_(True)
    vec, stats = depth_correlation_loss_torch(dd, g, mask=m, reduction="none", return_stats=True)
    assert torch.isnan(vec[1]) and torch.equal(vec[[0, 2]], want[[0, 2]])
    assert stats[:, 7].tolist() == [1.0, 0.0, 1.0]
    (grad,) = torch.autograd.grad(vec, dd, grad_outputs=torch.ones(3, dtype=dtype))
    assert torch.isfinite(grad[[0, 2]]).all() and grad[0].abs().sum() > 0
    open_ = (m[1] != 0) & (d[1] >= 1e-7) & (d[1] <= 50.0)
    assert not torch.isfinite(grad[1][open_]).any() and not grad[1][~open_].any()
    # skip_degenerate: loss 0, a zero gradient plane
    dd = d.clone().requires_grad_(True)
    vec, stats = depth_correlation_loss_torch(dd, g, mask=m, reduction="none", skip_degenerate=True,
                                              return_stats=True)
    assert vec[1] == 0 and torch.equal(vec[[0, 2]], want[[0, 2]]) and stats[1, 7] == 0
    (grad,) = torch.autograd.grad(vec.sum(), dd)
    assert not grad[1].any() and torch.isfinite(grad).all() and grad[2].abs().sum() > 0


# ------------------------------------------------------------ the C boundary

def _header():
    txt = open(os.path.join(REPO, "include", "gs_depth_loss.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_library_exports_every_symbol_of_gs_depth_loss_h():
    L = _lib.load()
    names = sorted(set(re.findall(r"\b(gs_[a-z_0-9]+)\s*\(", _header())))
    assert names == ["gs_depth_loss_backward", "gs_depth_loss_forward", "gs_depth_loss_struct_bytes",
                     "gs_depth_loss_validate", "gs_depth_loss_workspace_bytes"]
    for n in names:
        assert hasattr(L, n), n
        assert n in _lib.PROTOTYPES, f"{n} has no ctypes prototype"
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.lib_path()], capture_output=True, text=True).stdout
    assert set(names) <= set(re.findall(r" T (gs_[a-z_0-9]+)", out))
    assert L.gs_version() == _lib.ABI_VERSION  # a new header, no existing struct changed


def _header_struct_fields(name):
    """Field names of `typedef struct <name> { ... } <name>;` in the header, in order (the method
    of tests/test_boundary.py::test_ctypes_structs_mirror_the_header)."""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), _header(), flags=re.S).group(1)
    names = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        names += [re.findall(r"[A-Za-z_]\w*", part)[-1] for part in decl.split(",")]
    return names


def test_ctypes_struct_mirrors_the_header():
    L = _lib.load()
    fields = [f for f, _ in _lib.GsDepthLoss._fields_]
    assert fields == _header_struct_fields("gs_depth_loss")
    assert fields == ["B", "H", "W", "depth", "target", "mask", "mask_batch_stride", "near", "far",
                      "skip_degenerate", "losses", "stats", "workspace", "workspace_bytes"]
    assert ctypes.sizeof(_lib.GsDepthLoss) == L.gs_depth_loss_struct_bytes()


def test_workspace_bytes():
    L = _lib.load()
    ws = L.gs_depth_loss_workspace_bytes
    assert ws(1, 3, 5) == 24 and ws(2, 37, 53) == 2 * 2 * 24      # one 6-float record per workgroup
    assert ws(1, 257, 300) // 24 == 76 > 64                       # more records than a wave holds
    assert ws(1, 362, 362) == 128 * 24                            # 128 chunks: the last uncapped count
    assert ws(27, 800, 800) == 27 * 128 * 24                      # the workgroup count is capped
    assert ws(1, 4096, 4096) == 128 * 24
    for bad in [(0, 8, 8), (1, -1, 8), (1, 8, 0)]:
        assert ws(*bad) == 0


def _good_block(keep):
    """A valid argument block over host arrays (the validator dereferences nothing)."""
    L = _lib.load()
    B, H, W = 2, 9, 7
    ws_bytes = L.gs_depth_loss_workspace_bytes(B, H, W)
    bufs = {k: np.zeros(B * H * W, np.float32) for k in ("depth", "target", "d_depth")}
    bufs["mask"] = np.zeros(B * H * W + 4, np.uint8)
    bufs["losses"] = np.zeros(B, np.float32)
    bufs["stats"] = np.zeros(B * 8, np.float32)
    bufs["up"] = np.zeros(B, np.float32)
    bufs["ws"] = np.zeros(ws_bytes // 4 + 64, np.float32)
    keep.append(bufs)
    p = {k: v.ctypes.data for k, v in bufs.items()}
    p["ws"] = (p["ws"] + 255) // 256 * 256
    a = _lib.GsDepthLoss(B=B, H=H, W=W, depth=p["depth"], target=p["target"], near=1e-7, far=50.0,
                         losses=p["losses"], stats=p["stats"], workspace=p["ws"], workspace_bytes=ws_bytes)
    return a, p


def test_validator_rejects_bad_arguments_without_gpu():
    L = _lib.load()
    keep = []
    v = lambda a, bwd=0, up=None, dd=None: L.gs_depth_loss_validate(ctypes.byref(a), bwd, up, dd)  # noqa: E731
    a, p = _good_block(keep)
    assert v(a) == 0
    assert v(a, 1, p["up"], p["d_depth"]) == 0
    a.mask, a.mask_batch_stride = p["mask"] + 1, 0  # a byte mask at any address
    assert v(a) == 0
    a.mask_batch_stride = 9 * 7
    assert v(a) == 0 and v(a, 1, p["up"], p["d_depth"]) == 0
    a.losses, a.workspace, a.workspace_bytes = None, None, 0  # the backward needs only stats
    assert v(a, 1, p["up"], p["d_depth"]) == 0
    assert L.gs_depth_loss_validate(None, 0, None, None) < 0 and b"null argument" in L.gs_last_error()
    nan, inf = float("nan"), float("inf")
    for field, value, msg in [("B", 0, b"B, H, W must be > 0"), ("H", -1, b"B, H, W must be > 0"),
                              ("W", 0, b"B, H, W must be > 0"), ("depth", None, b"depth and target are required"),
                              ("target", None, b"depth and target are required"),
                              ("losses", None, b"losses is required"), ("stats", None, b"stats is required"),
                              ("depth", p["depth"] + 2, b"depth and target must be 4-byte aligned"),
                              ("target", p["target"] + 1, b"depth and target must be 4-byte aligned"),
                              ("stats", p["stats"] + 2, b"stats must be 4-byte aligned"),
                              ("losses", p["losses"] + 1, b"losses must be 4-byte aligned"),
                              ("workspace", None, b"workspace is required"), ("workspace_bytes", 16, b"needed"),
                              ("near", 50.0, b"near must be < far"), ("near", 60.0, b"near must be < far"),
                              ("far", 1e-8, b"near must be < far"), ("near", 0.0, b"near must be > 0"),
                              ("near", -1.0, b"near must be > 0"), ("near", nan, b"near and far must be finite"),
                              ("far", inf, b"near and far must be finite"),
                              ("far", nan, b"near and far must be finite"),
                              ("near", -inf, b"near and far must be finite")]:
        bad, _ = _good_block(keep)
        setattr(bad, field, value)
        assert v(bad) < 0, (field, value)
        assert msg in L.gs_last_error(), (field, L.gs_last_error())
    for stride in (1, 9 * 7 - 1, 2 * 9 * 7, -63):
        bad, q = _good_block(keep)
        bad.mask, bad.mask_batch_stride = q["mask"], stride
        assert v(bad) < 0 and b"mask_batch_stride must be 0 or H*W = 63" in L.gs_last_error(), stride
    a, p = _good_block(keep)
    assert v(a, 1, None, p["d_depth"]) < 0 and b"dL_dloss is required" in L.gs_last_error()
    assert v(a, 1, p["up"], None) < 0 and b"dL_ddepth is required" in L.gs_last_error()
    assert v(a, 1, p["up"], p["d_depth"] + 1) < 0 and b"gradient pointers must be 4-byte aligned" in L.gs_last_error()
    assert v(a, 1, p["up"] + 2, p["d_depth"]) < 0 and b"gradient pointers must be 4-byte aligned" in L.gs_last_error()
    # the entry points run the validator before anything touches a device
    bad, _ = _good_block(keep)
    bad.W = 0
    assert L.gs_depth_loss_forward(ctypes.byref(bad), None) < 0 and b"must be > 0" in L.gs_last_error()
    assert L.gs_depth_loss_backward(ctypes.byref(bad), p["up"], p["d_depth"], None) < 0


class _DeviceClaim(torch.Tensor):
    """A host tensor that reports is_cuda, so the wrapper's dtype / layout / shape rules (all
    checked before any device work) can be exercised where there is no GPU."""

    @staticmethod
    def __new__(cls, t):
        return torch.Tensor._make_subclass(cls, t, t.requires_grad)

    @property
    def is_cuda(self):
        return True


def test_wrapper_rejects_what_the_kernels_cannot_take():
    d, g = 1.0 + torch.rand(2, 1, 9, 7), torch.rand(2, 1, 9, 7)
    with pytest.raises(_lib.GsplatError, match="device tensors"):
        depth_correlation_loss(d, g)
    with pytest.raises(_lib.GsplatError, match="device tensors"):
        depth_correlation_loss(d[0, 0], g[0, 0], reduction="none")
    with pytest.raises(_lib.GsplatError, match="device tensors"):
        depth_correlation_loss(_DeviceClaim(d), g)
    for dtype in (torch.float16, torch.float64):
        with pytest.raises(_lib.GsplatError, match="float32"):
            depth_correlation_loss(_DeviceClaim(d.to(dtype)), _DeviceClaim(g.to(dtype)))
    with pytest.raises(_lib.GsplatError, match="contiguous"):
        depth_correlation_loss(_DeviceClaim(torch.rand(2, 7, 9).transpose(1, 2)), _DeviceClaim(g[:, 0]))
    with pytest.raises(_lib.GsplatError, match="shape"):
        depth_correlation_loss(_DeviceClaim(d), _DeviceClaim(g[:, 0]))
    with pytest.raises(_lib.GsplatError, match=r"\[B, 1, H, W\]"):
        depth_correlation_loss(_DeviceClaim(torch.rand(2, 3, 9, 7)), _DeviceClaim(torch.rand(2, 3, 9, 7)))
    with pytest.raises(_lib.GsplatError, match="no gradient"):
        depth_correlation_loss(_DeviceClaim(d), _DeviceClaim(g.clone().requires_grad_(True)))
    with pytest.raises(_lib.GsplatError, match="mask must be a device tensor"):
        depth_correlation_loss(_DeviceClaim(d), _DeviceClaim(g), mask=torch.ones(9, 7))
    with pytest.raises(_lib.GsplatError, match="mask must have shape"):
        depth_correlation_loss(_DeviceClaim(d), _DeviceClaim(g), mask=_DeviceClaim(torch.ones(7, 9)))
    for near, far in [(0.0, 50.0), (60.0, 50.0), (1e-7, float("inf")), (float("nan"), 50.0)]:
        with pytest.raises(_lib.GsplatError, match="near and far"):
            depth_correlation_loss(_DeviceClaim(d), _DeviceClaim(g), near=near, far=far)
    with pytest.raises(ValueError):
        depth_correlation_loss(_DeviceClaim(d), _DeviceClaim(g), reduction="mean")
    assert depth_loss.STATS[6:] == ("r", "valid")


@pytest.mark.skipif(shutil.which("gcc") is None or shutil.which("g++") is None, reason="gcc / g++ not available")
def test_validator_is_sanitizer_clean(tmp_path):
    """gs_depth_loss_host.cpp (with gs_host.cpp's error state) under ASan + UBSan in a plain CPU
    executable with its own main: nothing preloaded, nothing loaded into Python."""
    run_host_sanitizer(tmp_path, "depth_loss_host_sanitize.c", ["gs_depth_loss_host.cpp", "gs_host.cpp"],
                       "depth loss host sanitize ok")


# ------------------------------------------------------------ the driver

N_CAMS, HH, WW, P = 3, 6, 8, 40
LRS = {"means3D": 1e-3, "rgb_colors": 2e-3, "unnorm_rotations": 1e-3, "logit_opacities": 1e-2, "log_scales": 1e-3}


def _params():
    gen = torch.Generator().manual_seed(5)
    return {"means3D": torch.randn(P, 3, generator=gen), "rgb_colors": torch.rand(P, 3, generator=gen),
            "unnorm_rotations": torch.randn(P, 4, generator=gen), "logit_opacities": torch.randn(P, 1, generator=gen),
            "log_scales": torch.randn(P, 3, generator=gen) * 0.1}


def _stub_render(with_depth):
    """A differentiable stand-in for the rasterizer: every pixel a fixed mix of the Gaussians."""
    gen = torch.Generator().manual_seed(6)
    mix = torch.softmax(3.0 * torch.randn(N_CAMS, HH * WW, P, generator=gen), dim=-1)

    def render(rv, cams):
        col = rv["colors_precomp"] * rv["opacities"]
        ims = torch.stack([(mix[c] @ col).t().reshape(3, HH, WW) for c in cams])
        if not with_depth:
            return ims, None
        z = 3.0 + rv["means3D"][:, 2:3] + rv["scales"].sum(dim=1, keepdim=True)
        depth = torch.stack([(mix[c] @ z).reshape(1, HH, WW) for c in cams])
        return ims, None, depth
    return render


def _drive(steps=2, **kw):
    params = {k: torch.nn.Parameter(v.clone()) for k, v in _params().items()}
    opt = torch.optim.Adam([{"params": [params[k]], "name": k, "lr": lr} for k, lr in LRS.items()], lr=0.0, eps=1e-15)
    drv = TimestepDriver(params, {}, opt, N_CAMS, **kw)
    tg = torch.rand(N_CAMS, 3, HH, WW, generator=torch.Generator().manual_seed(7))
    losses = [drv.step(tg, 0, i) for i in range(steps)]
    return losses, {k: v.detach().clone() for k, v in drv.params.items()}, tg


def _depth_term(weight=0.001):
    gen = torch.Generator().manual_seed(8)
    prior = 0.3 + 0.1 * torch.rand(N_CAMS, 1, HH, WW, generator=gen)
    mask = torch.rand(HH, WW, generator=gen) < 0.8
    return lambda depth, cams: weight * depth_correlation_loss_torch(depth, prior[cams], mask=mask)


def test_driver_without_depth_loss_is_unchanged():
    """depth_loss=None: two steps are bit-identical to the run without the argument, also when the
    render hands a depth plane over that nobody asked for."""
    base = _drive(render=_stub_render(False))
    for kw in (dict(render=_stub_render(False), depth_loss=None), dict(render=_stub_render(True), depth_loss=None)):
        got = _drive(**kw)
        assert got[0] == base[0]
        for k in base[1]:
            assert torch.equal(got[1][k], base[1][k]), k


def test_driver_adds_the_depth_loss_over_n_cams():
    fn = _depth_term()
    losses, after, tg = _drive(steps=1, render=_stub_render(True), depth_loss=fn)
    # the same step by hand
    params = {k: torch.nn.Parameter(v.clone()) for k, v in _params().items()}
    ims, _, depth = _stub_render(True)(params2rendervar(params), list(range(N_CAMS)))
    image_term, depth_term = l1_image_loss(ims, tg) / N_CAMS, fn(depth, list(range(N_CAMS))) / N_CAMS
    want = image_term + depth_term
    assert depth_term.item() > 0 and losses[0] == pytest.approx(want.item(), rel=1e-6)
    opt = torch.optim.Adam([{"params": [params[k]], "name": k, "lr": lr} for k, lr in LRS.items()], lr=0.0, eps=1e-15)
    want.backward()
    opt.step()
    for k in after:
        torch.testing.assert_close(after[k], params[k].detach(), rtol=1e-6, atol=1e-9)
    without, _, _ = _drive(steps=1, render=_stub_render(True))
    assert without[0] == pytest.approx(image_term.item(), rel=1e-6) and without[0] != losses[0]
    with pytest.raises(ValueError, match="with_depth=True"):
        _drive(steps=1, render=_stub_render(False), depth_loss=fn)


def test_batch_renderer_keeps_its_default_signature():
    import inspect
    sig = inspect.signature(batch_renderer)
    assert list(sig.parameters) == ["settings_all", "with_depth"] and sig.parameters["with_depth"].default is False
