"""CPU tests of the quantile-trimmed losses (no GPU needed):
  * the `_torch` twins in fp64 reproduce the reference's losses and gradients (fixture
    tests/golden/robust_loss.npz, recorded from helpers.py:16-38 and ideaII.py:378-384 by
    tests/golden/make_golden_robust_loss.py), with integer and non-integer ranks;
  * the twins' threshold against the definition and against torch.quantile, ties, NaN, +inf;
  * the decision-robust cases of tests/_robust_loss_cases.py hold their margins;
  * the library exports every symbol include/gs_robust_loss.h declares, each with a ctypes
    prototype, and the ctypes mirror of gs_robust_loss has the library's size and the
    header's fields;
  * the host validator refuses every bad argument block with a message naming the field;
  * the wrappers refuse what the kernels cannot take (no CPU fallback);
  * the validator runs clean under AddressSanitizer + UndefinedBehaviorSanitizer in a
    stand-alone program (tools/robust_loss_host_sanitize.c).
"""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from dynamic3dgaussians_amd import (_lib, masked_trimmed_mse_loss, masked_trimmed_mse_loss_torch, plane_quantile,
                                    plane_quantile_torch, robust_loss, trimmed_mse_loss, trimmed_mse_loss_torch)
from tests import _robust_loss_cases as cases
from tests._harness import run_host_sanitizer
from tests.golden import make_golden_robust_loss as gen

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden", "robust_loss.npz")


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def test_fixture_is_small_and_complete(gold):
    assert os.path.getsize(GOLD) < 512 * 1024
    for size in gen.SIZES:
        key = f"mse.{size[0]}x{size[1]}"
        assert gold[f"{key}.pred"].shape == (3, *size) and gold[f"{key}.pred"].dtype == np.float32
        assert gold[f"{key}.gt"].dtype == np.float32 and gold[f"{key}.mask"].dtype == np.uint8
        assert 0.2 < 1 - gold[f"{key}.mask"].mean() < 0.4  # about 30 % zeros
        for normalize in (False, True):
            for q in gen.QUANTILES:
                g = gold[f"{gen.mse_name(size, normalize, q)}.grad_pred"]
                assert g.dtype == np.float64 and g.shape == (3, *size)
    assert gold["trim.flow.pred"].shape == gen.TRIM_SHAPE
    # ranks: integers at 37 x 53, not at 6 x 7
    assert all(float(q * (37 * 53 - 1)).is_integer() for q in gen.QUANTILES)
    assert not any(float(q * (6 * 7 - 1)).is_integer() for q in (0.9, 0.5))


@pytest.mark.parametrize("q", gen.QUANTILES)
@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("size", gen.SIZES)
def test_masked_twin_matches_the_reference_in_fp64(gold, size, normalize, q):
    """Both sides are fp64 torch on the CPU; the twin's threshold is the definition's, the
    reference's is torch.quantile's fp64 one: the same kept set, so 1e-12 relative."""
    key = f"mse.{size[0]}x{size[1]}"
    p = torch.from_numpy(gold[f"{key}.pred"]).double().requires_grad_(True)
    g = torch.from_numpy(gold[f"{key}.gt"]).double()
    m = torch.from_numpy(gold[f"{key}.mask"])
    name = gen.mse_name(size, normalize, q)
    for pp, gg, mm in ((p, g, m), (p[None], g[None], m[None])):
        loss = masked_trimmed_mse_loss_torch(pp, gg, mask=mm, quantile=q, normalize=normalize)
        (grad,) = torch.autograd.grad(loss, p)
        ref = float(gold[f"{name}.loss"])
        assert loss.dim() == 0 and abs(loss.item() - ref) <= 1e-12 * abs(ref)
        assert _rel(grad, gold[f"{name}.grad_pred"]) <= 1e-12


@pytest.mark.parametrize("q", gen.TRIM_QUANTILES)
def test_trimmed_twin_matches_the_reference_in_fp64(gold, q):
    p = torch.from_numpy(gold["trim.flow.pred"]).double().requires_grad_(True)
    g = torch.from_numpy(gold["trim.flow.gt"]).double()
    loss = trimmed_mse_loss_torch(p, g, q)
    (grad,) = torch.autograd.grad(loss, p)
    ref = float(gold[f"{gen.trim_name(q)}.loss"])
    assert abs(loss.item() - ref) <= 1e-12 * abs(ref)
    assert _rel(grad, gold[f"{gen.trim_name(q)}.grad_pred"]) <= 1e-12
    if q == 1.0:  # no special case: exactly the largest row is dropped
        assert int((grad.abs().sum(-1) == 0).sum()) == 1


def test_threshold_twin_is_the_definition():
    x = torch.tensor([[4.0, 0.0, 1.0, 9.0, 1.0], [0.0, 0.0, 0.0, 0.0, 7.0]])
    # n = 5: q = 0.5 -> rank 2; q = 0.9 -> rank 3.6
    assert plane_quantile_torch(x, 0.5).tolist() == [1.0, 0.0]
    got = plane_quantile_torch(x, 0.9)
    assert got.dtype == torch.float64 and got[0].item() == 4.0 + (0.9 * 4 - 3) * 5.0
    assert got[1].item() == 0.0 + (0.9 * 4 - 3) * 7.0
    assert plane_quantile_torch(x[0], 0.0).item() == 0.0 and plane_quantile_torch(x[0], 1.0).item() == 9.0
    assert plane_quantile_torch(torch.tensor([3.5]), 0.3).item() == 3.5  # n = 1
    y = x.clone()
    y[1, 2] = float("nan")
    got = plane_quantile_torch(y, 0.5)
    assert got[0].item() == 1.0 and torch.isnan(got[1])
    z = torch.tensor([1.0, float("inf"), 2.0])
    assert plane_quantile_torch(z, 0.25).item() == 1.5 and plane_quantile_torch(z, 0.75).item() == float("inf")
    assert torch.isnan(plane_quantile_torch(z, 0.5))  # w = 0 and v_hi = inf: the definition's 0 * inf
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(_lib.GsplatError, match="quantile"):
            plane_quantile_torch(x, bad)


def test_threshold_twin_against_torch_quantile():
    """torch.quantile's fp32 result differs from the definition by its fp32 rank only."""
    gen_ = torch.Generator().manual_seed(3)
    for n in (1, 2, 63, 1961):
        x = torch.rand(n, generator=gen_) ** 4
        for q in (0.0, 0.5, 0.9, 1.0):
            mine, theirs = plane_quantile_torch(x, q).item(), torch.quantile(x, q).item()
            v = torch.sort(x).values.double()
            lo = int(np.floor(q * (n - 1)))
            hi = min(lo + 1, n - 1)
            bound = (v[hi] - v[lo]).item() * n * 2.0 ** -23 + float(np.spacing(np.float32(v[hi].item())))
            assert abs(mine - theirs) <= bound, (n, q)


def test_twin_options():
    gen_ = torch.Generator().manual_seed(4)
    p, g = torch.rand(2, 3, 5, 6, generator=gen_).double(), torch.rand(2, 3, 5, 6, generator=gen_).double()
    m = torch.rand(2, 5, 6, generator=gen_) < 0.6
    vec, stats = masked_trimmed_mse_loss_torch(p, g, mask=m, quantile=0.7, reduction="none", return_stats=True)
    assert vec.shape == (2,) and stats.shape == (2, 4) and stats.dtype == torch.float64
    e = ((p - g) ** 2).mean(1)
    for b in range(2):
        thr = plane_quantile_torch(e[b].flatten(), 0.7)
        kept = e[b] < thr
        assert stats[b].tolist() == [thr.item(), kept.sum().item(), (kept & m[b]).sum().item(), 0.0]
        torch.testing.assert_close(vec[b], (e[b] * m[b])[kept].mean(), rtol=1e-13, atol=0)
    total = masked_trimmed_mse_loss_torch(p, g, mask=m.float() * 3, quantile=0.7)
    torch.testing.assert_close(total, vec.sum(), rtol=1e-14, atol=0)
    # quantile over the masked pixels only
    vec_m, stats_m = masked_trimmed_mse_loss_torch(p, g, mask=m, quantile=0.7, quantile_over="masked",
                                                   reduction="none", return_stats=True)
    for b in range(2):
        thr = plane_quantile_torch(e[b][m[b]], 0.7)
        kept = m[b] & (e[b] < thr)
        assert stats_m[b].tolist() == [thr.item(), kept.sum().item(), kept.sum().item(), 0.0]
        torch.testing.assert_close(vec_m[b], e[b][kept].mean(), rtol=1e-13, atol=0)
    # degenerate: q = 0 keeps nothing
    vec0 = masked_trimmed_mse_loss_torch(p, g, mask=m, quantile=0.0, reduction="none")
    assert torch.isnan(vec0).all()
    pz = p.clone().requires_grad_(True)
    vec0 = masked_trimmed_mse_loss_torch(pz, g, mask=m, quantile=0.0, reduction="none", skip_degenerate=True)
    assert not vec0.any() and not torch.autograd.grad(vec0.sum(), pz)[0].any()
    none_kept = masked_trimmed_mse_loss_torch(p, g, mask=torch.zeros(5, 6), quantile=0.9, normalize=True)
    assert none_kept.item() == 0.0
    with pytest.raises(ValueError):
        masked_trimmed_mse_loss_torch(p, g, reduction="mean")
    with pytest.raises(ValueError):
        masked_trimmed_mse_loss_torch(p, g, quantile_over="some")


def test_decision_robust_cases_hold_their_margins():
    """The builder asserts (it does not filter); here it runs for every case of the GPU tests."""
    names = [c.name for c in cases.image_cases()] + [cases.rows_case().name]
    assert len(names) == len(set(names)) == 7
    for c in cases.image_cases():
        assert c.pred.shape[0] == 3 and c.pred.dtype == torch.float32
    ranks = [0.9 * (37 * 53 - 1), 0.9 * (300 * 300 - 1)]
    assert float(ranks[0]).is_integer() and not float(ranks[1]).is_integer()


# ------------------------------------------------------------ the C boundary

def _header():
    txt = open(os.path.join(REPO, "include", "gs_robust_loss.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_library_exports_every_symbol_of_gs_robust_loss_h():
    L = _lib.load()
    names = sorted(set(re.findall(r"\b(gs_[a-z_0-9]+)\s*\(", _header())))
    assert names == ["gs_robust_loss_backward", "gs_robust_loss_forward", "gs_robust_loss_struct_bytes",
                     "gs_robust_loss_validate", "gs_robust_loss_workspace_bytes"]
    for n in names:
        assert hasattr(L, n), n
        assert n in _lib.PROTOTYPES, f"{n} has no ctypes prototype"
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.lib_path()], capture_output=True, text=True).stdout
    assert set(names) <= set(re.findall(r" T (gs_[a-z_0-9]+)", out))
    assert L.gs_version() == _lib.ABI_VERSION  # a new header, no existing struct changed


def test_ctypes_struct_mirrors_the_header():
    L = _lib.load()
    body = re.search(r"typedef struct gs_robust_loss \{(.*?)\} gs_robust_loss;", _header(), flags=re.S).group(1)
    names = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        names += [re.findall(r"[A-Za-z_]\w*", part)[-1] for part in decl.split(",")]
    fields = [f for f, _ in _lib.GsRobustLoss._fields_]
    assert fields == names
    assert fields == ["B", "R", "N", "layout", "pred", "gt", "mask", "mask_batch_stride", "quantile", "select",
                      "over_masked", "normalize", "norm_width", "skip_degenerate", "_pad", "losses", "stats",
                      "workspace", "workspace_bytes"]
    assert ctypes.sizeof(_lib.GsRobustLoss) == L.gs_robust_loss_struct_bytes()
    assert (robust_loss.CHANNELS, robust_loss.ROWS, robust_loss.VALUES) == (0, 1, 2)
    assert re.search(r"GS_ROBUST_CHANNELS = 0, GS_ROBUST_ROWS = 1, GS_ROBUST_VALUES = 2", _header())


def test_workspace_bytes():
    L = _lib.load()
    ws = L.gs_robust_loss_workspace_bytes
    head = (16 + 2048 + 2 * 1024 + 2 * 1024) * 4  # state and histograms of a plane
    assert ws(1, 5, 2) == head + 32 and ws(1, 5, 0) == head + 32 + 32  # one record; the plane, rounded to 16
    assert ws(3, 1961, 2) == 3 * (head + 2 * 32) and ws(3, 1961, 1) == (3 * (head + 2 * 32 + 1961 * 4) + 15) // 16 * 16
    assert ws(1, 128 * 1024, 2) == head + 128 * 32 == ws(1, 2 ** 31 - 1, 2)  # the workgroup count is capped
    assert ws(27, 640000, 0) == 27 * (head + 128 * 32 + 640000 * 4)
    for bad in [(0, 8, 0), (1, 0, 0), (1, -1, 2), (1, 8, 3), (1, 8, -1)]:
        assert ws(*bad) == 0


def _good_block(keep, layout=0):
    """A valid argument block over host arrays (the validator dereferences nothing)."""
    L = _lib.load()
    B, R, N = 2, 3, 63
    if layout == 2:
        R = 1
    ws_bytes = L.gs_robust_loss_workspace_bytes(B, N, layout)
    bufs = {k: np.zeros(B * R * N + 1, np.float32) for k in ("pred", "gt", "d_pred")}
    bufs["mask"] = np.zeros(B * N + 4, np.uint8)
    bufs["losses"] = np.zeros(B + 1, np.float32)
    bufs["stats"] = np.zeros(B * 4 + 1, np.float64)
    bufs["up"] = np.zeros(B + 1, np.float32)
    bufs["ws"] = np.zeros(ws_bytes // 4 + 64, np.float32)
    keep.append(bufs)
    p = {k: v.ctypes.data for k, v in bufs.items()}
    p["ws"] = (p["ws"] + 255) // 256 * 256
    a = _lib.GsRobustLoss(B=B, R=R, N=N, layout=layout, pred=p["pred"], gt=None if layout == 2 else p["gt"],
                          quantile=0.9, select=1, losses=p["losses"], stats=p["stats"], workspace=p["ws"],
                          workspace_bytes=ws_bytes)
    return a, p


def test_validator_rejects_bad_arguments_without_gpu():
    L = _lib.load()
    keep = []
    v = lambda a, bwd=0, up=None, dp=None: L.gs_robust_loss_validate(ctypes.byref(a), bwd, up, dp)  # noqa: E731
    for layout in (0, 1, 2):
        a, p = _good_block(keep, layout)
        assert v(a) == 0, L.gs_last_error()
    a, p = _good_block(keep)
    assert v(a, 1, p["up"], p["d_pred"]) == 0
    a.mask, a.mask_batch_stride, a.over_masked = p["mask"] + 1, 0, 1  # a byte mask at any address
    assert v(a) == 0
    a.mask_batch_stride, a.normalize, a.norm_width = 63, 1, 9
    assert v(a) == 0 and v(a, 1, p["up"], p["d_pred"]) == 0
    a.losses, a.workspace, a.workspace_bytes = None, None, 0  # the backward needs only stats
    assert v(a, 1, p["up"], p["d_pred"]) == 0
    assert L.gs_robust_loss_validate(None, 0, None, None) < 0 and b"null argument" in L.gs_last_error()
    nan, inf = float("nan"), float("inf")
    for field, value, msg in [("B", 0, b"B, R, N must be > 0"), ("R", -1, b"B, R, N must be > 0"),
                              ("N", 0, b"B, R, N must be > 0"), ("layout", 3, b"unknown layout"),
                              ("layout", -1, b"unknown layout"), ("N", 2 ** 30, b"does not fit int32"),
                              ("pred", None, b"pred is required"), ("gt", None, b"gt is required"),
                              ("losses", None, b"losses is required"), ("stats", None, b"stats is required"),
                              ("pred", p["pred"] + 2, b"pred and gt must be 4-byte aligned"),
                              ("gt", p["gt"] + 1, b"pred and gt must be 4-byte aligned"),
                              ("stats", p["stats"] + 4, b"stats must be 8-byte aligned"),
                              ("losses", p["losses"] + 1, b"losses must be 4-byte aligned"),
                              ("workspace", None, b"workspace is required"), ("workspace_bytes", 16, b"needed"),
                              ("quantile", nan, b"quantile must be in [0, 1]"),
                              ("quantile", inf, b"quantile must be in [0, 1]"),
                              ("quantile", -1e-12, b"quantile must be in [0, 1]"),
                              ("quantile", 1.0 + 1e-12, b"quantile must be in [0, 1]"),
                              ("over_masked", 1, b"over_masked needs a mask"),
                              ("normalize", 1, b"norm_width must be > 0")]:
        bad, _ = _good_block(keep)
        setattr(bad, field, value)
        assert v(bad) < 0, (field, value)
        assert msg in L.gs_last_error(), (field, L.gs_last_error())
    for stride in (1, 62, 126, -63):
        bad, q = _good_block(keep)
        bad.mask, bad.mask_batch_stride = q["mask"], stride
        assert v(bad) < 0 and b"mask_batch_stride must be 0 or N = 63" in L.gs_last_error(), stride
    vals, q = _good_block(keep, 2)
    vals.R = 2
    assert v(vals) < 0 and b"R must be 1" in L.gs_last_error()
    vals, q = _good_block(keep, 2)
    vals.select = 0
    assert v(vals) < 0 and b"needs select" in L.gs_last_error()
    vals, q = _good_block(keep, 2)
    assert v(vals, 1, q["up"], q["d_pred"]) < 0 and b"no backward" in L.gs_last_error()
    a, p = _good_block(keep)
    assert v(a, 1, None, p["d_pred"]) < 0 and b"dL_dloss is required" in L.gs_last_error()
    assert v(a, 1, p["up"], None) < 0 and b"dL_dpred is required" in L.gs_last_error()
    assert v(a, 1, p["up"], p["d_pred"] + 1) < 0 and b"gradient pointers must be 4-byte aligned" in L.gs_last_error()
    assert v(a, 1, p["up"] + 2, p["d_pred"]) < 0 and b"gradient pointers must be 4-byte aligned" in L.gs_last_error()
    # the entry points run the validator before anything touches a device
    bad, _ = _good_block(keep)
    bad.N = 0
    assert L.gs_robust_loss_forward(ctypes.byref(bad), None) < 0 and b"must be > 0" in L.gs_last_error()
    assert L.gs_robust_loss_backward(ctypes.byref(bad), p["up"], p["d_pred"], None) < 0


class _DeviceClaim(torch.Tensor):
    """A host tensor that reports is_cuda, so the wrappers' dtype / layout / shape rules (all
    checked before any device work) can be exercised where there is no GPU."""

    @staticmethod
    def __new__(cls, t):
        return torch.Tensor._make_subclass(cls, t, t.requires_grad)

    @property
    def is_cuda(self):
        return True


def test_wrappers_reject_what_the_kernels_cannot_take():
    p, g = torch.rand(2, 3, 9, 7), torch.rand(2, 3, 9, 7)
    D = _DeviceClaim
    for call in (lambda: masked_trimmed_mse_loss(p, g), lambda: masked_trimmed_mse_loss(p[0], g[0], quantile=0.9),
                 lambda: masked_trimmed_mse_loss(D(p), g), lambda: trimmed_mse_loss(p, g),
                 lambda: trimmed_mse_loss(D(p), g), lambda: plane_quantile(p.reshape(2, -1), 0.5),
                 lambda: plane_quantile(p.flatten(), 0.5)):
        with pytest.raises(_lib.GsplatError, match="device tensors"):
            call()
    for dtype in (torch.float16, torch.float64):
        with pytest.raises(_lib.GsplatError, match="float32"):
            masked_trimmed_mse_loss(D(p.to(dtype)), D(g.to(dtype)))
        with pytest.raises(_lib.GsplatError, match="float32"):
            trimmed_mse_loss(D(p.to(dtype)), D(g.to(dtype)))
        with pytest.raises(_lib.GsplatError, match="float32"):
            plane_quantile(D(p.reshape(2, -1).to(dtype)), 0.5)
    nc = torch.rand(2, 3, 7, 9).transpose(2, 3)
    with pytest.raises(_lib.GsplatError, match="contiguous"):
        masked_trimmed_mse_loss(D(nc), D(g))
    with pytest.raises(_lib.GsplatError, match="contiguous"):
        trimmed_mse_loss(D(nc), D(g))
    with pytest.raises(_lib.GsplatError, match="contiguous"):
        plane_quantile(D(torch.rand(9, 4).t()), 0.5)
    with pytest.raises(_lib.GsplatError, match="shape"):
        masked_trimmed_mse_loss(D(p), D(torch.rand(2, 2, 9, 7)))
    with pytest.raises(_lib.GsplatError, match="shape"):
        trimmed_mse_loss(D(p), D(g[0]))
    with pytest.raises(_lib.GsplatError, match=r"\[B, C, H, W\]"):
        masked_trimmed_mse_loss(D(p[0, 0]), D(g[0, 0]))
    with pytest.raises(_lib.GsplatError, match=r"\[B, N\] or \[N\]"):
        plane_quantile(D(p), 0.5)
    with pytest.raises(_lib.GsplatError, match="no gradient"):
        masked_trimmed_mse_loss(D(p), D(g.clone().requires_grad_(True)))
    with pytest.raises(_lib.GsplatError, match="no gradient"):
        trimmed_mse_loss(D(p), D(g.clone().requires_grad_(True)))
    with pytest.raises(_lib.GsplatError, match="mask must be a device tensor"):
        masked_trimmed_mse_loss(D(p), D(g), mask=torch.ones(9, 7))
    with pytest.raises(_lib.GsplatError, match="mask must have shape"):
        masked_trimmed_mse_loss(D(p), D(g), mask=D(torch.ones(7, 9)))
    for q in (-0.1, 1.1, float("nan"), float("inf")):
        with pytest.raises(_lib.GsplatError, match="quantile must be in"):
            masked_trimmed_mse_loss(D(p), D(g), quantile=q)
        with pytest.raises(_lib.GsplatError, match="quantile must be in"):
            trimmed_mse_loss(D(p), D(g), quantile=q)
        with pytest.raises(_lib.GsplatError, match="quantile must be in"):
            plane_quantile(D(p.reshape(2, -1)), q)
    with pytest.raises(ValueError):
        masked_trimmed_mse_loss(D(p), D(g), reduction="mean")
    with pytest.raises(ValueError):
        masked_trimmed_mse_loss(D(p), D(g), quantile_over="fg")
    assert robust_loss.STATS == ("thr", "kept", "kept_masked", "nan")


@pytest.mark.skipif(shutil.which("gcc") is None or shutil.which("g++") is None, reason="gcc / g++ not available")
def test_validator_is_sanitizer_clean(tmp_path):
    """gs_robust_loss_host.cpp (with gs_host.cpp's error state) under ASan + UBSan in a plain CPU
    executable with its own main: nothing preloaded, nothing loaded into Python."""
    run_host_sanitizer(tmp_path, "robust_loss_host_sanitize.c", ["gs_robust_loss_host.cpp", "gs_host.cpp"],
                       "robust loss host sanitize ok")
