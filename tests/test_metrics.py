"""CPU tests of the evaluation metrics (no GPU needed):
  * image_metrics_torch / mask_iou_torch in fp64 reproduce the reference's mSSIM, mPSNR,
    compute_psnr, calc_psnr, mask_iou, mIOU and MaskIoU (fixture tests/golden/eval_metrics.npz,
    recorded from the reference's metrics.py / external.py by tests/golden/make_golden_metrics.py),
    and the accumulators' compute() the recorded compute() values;
  * the library exports every symbol include/gs_metrics.h declares, each with a ctypes
    prototype, and the ctypes mirror of gs_image_metrics has the library's size and the
    header's fields;
  * the host validators refuse every bad argument with a message;
  * the wrappers refuse what the kernels cannot take (no CPU fallback);
  * the validators run clean under AddressSanitizer + UndefinedBehaviorSanitizer in a
    stand-alone program (tools/metrics_host_sanitize.c).
"""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import dynamic3dgaussians_amd as pkg
from dynamic3dgaussians_amd import _lib, metrics
from dynamic3dgaussians_amd.metrics import (MaskedPSNR, MaskedSSIM, MaskIoU, MeanIoU, image_metrics,
                                            image_metrics_torch, iou, mask_iou, mask_iou_torch, psnr_clamped,
                                            psnr_masked, psnr_plain)
from tests._harness import run_host_sanitizer

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden", "eval_metrics.npz")
SHAPES = {"one_window": (1, 3, 11, 11), "empty_windows": (2, 3, 13, 29), "ragged_masked": (2, 3, 45, 77),
          "flat": (1, 3, 37, 53), "features": (1, 32, 21, 40)}
CASES = tuple(SHAPES)
RGB_CASES = tuple(n for n in CASES if SHAPES[n][1] == 3)  # the reference's PSNR code hard-codes 3 channels
TOL = 1e-12  # both sides are fp64 torch on the CPU running the same operations
F32 = 2.0 ** -23  # mask_iou / MaskIoU divide their counts in fp32: the recorded ratios carry one fp32 rounding each


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def _close(got, want, tol=TOL):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.all(np.abs(got - want) <= tol * np.abs(want)), (got, want)


def _inputs(gold, name, dtype=torch.float64):
    pred = torch.from_numpy(gold[f"{name}.pred"]).to(dtype)
    target = torch.from_numpy(gold[f"{name}.target"]).to(dtype)
    mask = torch.from_numpy(gold[f"{name}.mask"]) if f"{name}.mask" in gold.files else None
    return pred, target, mask


def test_fixture_is_small_and_complete(gold):
    assert os.path.getsize(GOLD) < 512 * 1024
    for name in CASES:
        B = SHAPES[name][0]
        assert gold[f"{name}.pred"].shape == SHAPES[name] and gold[f"{name}.pred"].dtype == np.float32
        assert gold[f"{name}.target"].shape == SHAPES[name] and gold[f"{name}.target"].dtype == np.float32
        assert gold[f"{name}.ssim"].shape == (B,) and gold[f"{name}.ssim"].dtype == np.float64
        assert gold[f"{name}.calc_psnr"].shape == (B,)
    for name in RGB_CASES:
        for k in ("mpsnr_sse", "mpsnr_total", "mpsnr_compute", "mpsnr_compute_per_image", "compute_psnr"):
            assert f"{name}.{k}" in gold.files, (name, k)
    assert {n for n in CASES if f"{n}.mask" in gold.files} == {"empty_windows", "ragged_masked"}
    m = gold["empty_windows.mask"]
    assert m.shape == (2, 13, 29) and m.dtype == np.uint8 and not m[:, :, :12].any() and 0.7 < m[:, :, 12:].mean() < 0.9
    m = gold["ragged_masked.mask"]
    assert not m[1, 10:30, 25:55].any() and m[0, 10:30, 25:55].mean() > 0.6 and 0.7 < m[0].mean() < 0.9
    fp, ft = gold["flat.pred"], gold["flat.target"]
    assert not fp[:, :, :18].any() and not ft[:, :, :18].any() and np.all(fp[:, :, 18:] == np.float32(0.7))
    assert np.abs(gold["features.pred"]).mean() > 5
    assert gold["iou.pred"].shape == (3, 45, 77) and gold["iou.pred"].dtype == np.float32
    assert gold["iou.pred"][2].max() < 0.9 and gold["iou.target"][2].max() < 0.9  # an empty union at 0.9
    assert gold["iou.mask_iou"][2] == 1.0


@pytest.mark.parametrize("name", CASES)
def test_torch_restatement_matches_the_reference_in_fp64(gold, name):
    pred, target, mask = _inputs(gold, name)
    m = image_metrics_torch(pred, target, mask)
    assert m.ssim.dtype == torch.float64 and m.shape == SHAPES[name][1:]
    _close(m.ssim, gold[f"{name}.ssim"])
    _close(psnr_plain(image_metrics_torch(pred, target, ssim=False)), gold[f"{name}.calc_psnr"])
    hw = SHAPES[name][2] * SHAPES[name][3]
    want_mask = gold[f"{name}.mask"].reshape(SHAPES[name][0], -1).sum(1) if mask is not None else [hw] * SHAPES[name][0]
    assert m.mask_sum.tolist() == list(want_mask)
    if name in RGB_CASES:
        _close(psnr_clamped(m), gold[f"{name}.compute_psnr"])
        _close(m.sse.sum(), gold[f"{name}.mpsnr_sse"][0])
        assert float(m.mask_sum.sum()) * 3 == float(gold[f"{name}.mpsnr_total"][0])
        # every image as its own update: the mean of the per-image logs
        _close(psnr_masked(m).mean(), gold[f"{name}.mpsnr_compute_per_image"])
    one = image_metrics_torch(pred[0], target[0], mask[0] if mask is not None else None)  # a single image
    assert one.ssim.dim() == 0
    _close(one.ssim, gold[f"{name}.ssim"][0])
    _close(metrics.l1(m), (torch.abs(pred - target) * (mask[:, None] if mask is not None else 1)).mean(dim=(1, 2, 3)))


def test_shared_mask_is_the_per_image_mask_repeated(gold):
    pred, target, mask = _inputs(gold, "ragged_masked")
    shared = image_metrics_torch(pred, target, mask[0])
    stacked = image_metrics_torch(pred, target, torch.stack([mask[0], mask[0]]))
    for a, b in zip(shared[:4], stacked[:4]):
        assert torch.equal(a, b)


def test_accumulators_compute_the_recorded_values(gold):
    for name in RGB_CASES:
        pred, target, mask = _inputs(gold, name)
        acc = MaskedPSNR(image_metrics_torch)
        acc.update(pred, target, mask)  # one update of the whole batch
        _close(acc.compute(), gold[f"{name}.mpsnr_compute"])
        each = MaskedPSNR(image_metrics_torch)
        for i in range(pred.shape[0]):
            each.update(pred[i:i + 1], target[i:i + 1], mask[i:i + 1] if mask is not None else None)
        assert len(each) == pred.shape[0]
        _close(each.compute(), gold[f"{name}.mpsnr_compute_per_image"])
        filed = MaskedPSNR(image_metrics_torch)
        filed.update_images(image_metrics_torch(pred, target, mask, ssim=False))
        _close(filed.compute(), gold[f"{name}.mpsnr_compute_per_image"])
    for name in CASES:
        pred, target, mask = _inputs(gold, name)
        acc = MaskedSSIM(image_metrics_torch)
        acc.update(pred, target, mask)
        _close(acc.compute(), gold[f"{name}.ssim_compute"])
    # over several updates: the mean over all images, not over updates
    acc = MaskedSSIM(image_metrics_torch)
    for name in ("one_window", "ragged_masked"):
        acc.update(*_inputs(gold, name))
    _close(acc.compute(), np.concatenate([gold["one_window.ssim"], gold["ragged_masked.ssim"]]).mean(), 1e-14)
    with pytest.raises(_lib.GsplatError, match="before any update"):
        MaskedSSIM(image_metrics_torch).compute()


def test_mask_iou_restatement_and_accumulators(gold):
    sp, st = torch.from_numpy(gold["iou.pred"]), torch.from_numpy(gold["iou.target"])
    for a, b in ((sp, st), (sp.double(), st.double())):  # counts do not depend on the dtype
        i, u = mask_iou_torch(a, b, 0.9)
        assert i.dtype == torch.int64 and i.shape == (3,) and u[2] == 0 and i[0] > 0
        _close(iou(a, b, counts=mask_iou_torch), gold["iou.mask_iou"], F32)
    assert iou(sp, st, counts=mask_iou_torch)[2] == 1.0  # an empty union
    one = mask_iou_torch(sp[0], st[0], 0.9)
    assert one[0].dim() == 0 and one[0] == i[0] and one[1] == u[0]
    acc = MeanIoU(mask_iou_torch)
    for k in range(3):
        acc.update(sp[k], st[k])
    _close(acc.compute(), gold["iou.miou_compute"], 2 * F32)
    hp, ht = (sp > 0.5).float(), (st > 0.5).float()
    i0, u0 = mask_iou_torch(hp, ht, 0.0)
    assert i0.tolist() == gold["iou.maskiou_intersection"].tolist() and u0.tolist() == gold["iou.maskiou_union"].tolist()
    acc = MaskIoU(mask_iou_torch)
    for k in range(3):
        acc.update(hp[k], ht[k])
    # the reference's last line: the mean over the updates of intersection / union
    _close(acc.compute(), gold["iou.maskiou_compute"], 2 * F32)
    _close(acc.compute(), np.mean(gold["iou.maskiou_intersection"] / gold["iou.maskiou_union"]), 1e-15)
    empty = MaskIoU(mask_iou_torch)
    empty.update(torch.zeros(4, 4), torch.zeros(4, 4))
    assert empty.compute() == 0.0  # 0 / clamp(0, 1e-8), as the reference


def test_package_exports():
    for n in ("image_metrics", "image_metrics_torch", "mask_iou", "mask_iou_torch", "iou", "psnr_masked",
              "psnr_clamped", "psnr_plain", "MaskedPSNR", "MaskedSSIM", "MaskIoU", "MeanIoU", "ImageMetrics",
              "evaluate_cameras", "evaluate_sequence"):
        assert getattr(pkg, n) is getattr(metrics, n), n


def _declared_symbols():
    txt = open(os.path.join(REPO, "include", "gs_metrics.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(gs_[a-z_0-9]+)\s*\(", txt)))


def test_library_exports_every_symbol_of_gs_metrics_h():
    L = _lib.load()
    names = _declared_symbols()
    assert set(names) == {"gs_image_metrics_struct_bytes", "gs_image_metrics_workspace_bytes",
                          "gs_image_metrics_validate", "gs_image_metrics", "gs_mask_iou_validate", "gs_mask_iou"}
    for n in names:
        assert hasattr(L, n), n
        assert n in _lib.PROTOTYPES, f"{n} has no ctypes prototype"
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.lib_path()], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (gs_[a-z_0-9]+)", out))
    assert set(names) <= exported
    assert L.gs_version() == _lib.ABI_VERSION == 13  # a new header, no existing struct changed


def test_ctypes_mirror_has_the_library_size_and_the_header_fields():
    L = _lib.load()
    assert ctypes.sizeof(_lib.GsImageMetrics) == L.gs_image_metrics_struct_bytes()
    src = open(os.path.join(REPO, "include", "gs_metrics.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    body = re.search(r"struct gs_image_metrics \{(.*?)\};", src, flags=re.S).group(1)
    names = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        names += [re.findall(r"[A-Za-z_]\w*", part)[-1] for part in decl.split(",")]
    assert [f for f, _ in _lib.GsImageMetrics._fields_] == names


def test_workspace_bytes():
    L = _lib.load()
    ws = L.gs_image_metrics_workspace_bytes(2, 3, 45, 77)
    assert 2 * 3 * 2 * 3 * 16 <= ws <= 2 * 3 * 2 * 3 * 16 + 256  # four floats per 32 x 32 tile of H x W
    assert L.gs_image_metrics_workspace_bytes(27, 3, 800, 800) >= 27 * 3 * 25 * 25 * 16
    assert L.gs_image_metrics_workspace_bytes(1, 3, 9, 7) > 0  # the sums alone, below the window's size
    for bad in [(0, 3, 16, 16), (1, -1, 16, 16), (1, 3, 0, 16), (1, 3, 16, -2)]:
        assert L.gs_image_metrics_workspace_bytes(*bad) == 0


def _good_block(keep, H=13, W=29):
    """A valid argument block over host arrays (the validator dereferences nothing)."""
    L = _lib.load()
    B, Ch = 2, 3
    ws_bytes = L.gs_image_metrics_workspace_bytes(B, Ch, H, W)
    bufs = {k: np.zeros(B * Ch * H * W, np.float32) for k in ("pred", "target")}
    bufs["mask"] = np.zeros(B * H * W, np.float32)
    bufs["out"] = np.zeros(B * 4, np.float32)
    bufs["ws"] = np.zeros(ws_bytes // 4 + 64, np.float32)
    keep.append(bufs)
    p = {k: v.ctypes.data for k, v in bufs.items()}
    p["ws"] = (p["ws"] + 255) // 256 * 256
    a = _lib.GsImageMetrics(B=B, Ch=Ch, H=H, W=W, pred=p["pred"], target=p["target"], want_ssim=1, out=p["out"],
                            workspace=p["ws"], workspace_bytes=ws_bytes)
    return a, p


def test_validator_rejects_bad_arguments_without_gpu():
    L = _lib.load()
    keep = []
    v = lambda a: L.gs_image_metrics_validate(ctypes.byref(a))  # noqa: E731
    a, p = _good_block(keep)
    assert v(a) == 0
    a.mask, a.mask_batch_stride = p["mask"], 13 * 29
    assert v(a) == 0
    a.mask_batch_stride = 0
    assert v(a) == 0
    assert L.gs_image_metrics_validate(None) < 0 and b"null argument" in L.gs_last_error()
    for field, value, msg in [("B", 0, b"must be > 0"), ("Ch", -1, b"must be > 0"), ("H", 0, b"must be > 0"),
                              ("W", -5, b"must be > 0"), ("pred", None, b"required"), ("target", None, b"required"),
                              ("out", None, b"out is required"), ("pred", p["pred"] + 2, b"4-byte aligned"),
                              ("target", p["target"] + 1, b"4-byte aligned"),
                              ("workspace", None, b"workspace is required"), ("workspace_bytes", 16, b"needed"),
                              ("H", 10, b"no window fits"), ("W", 10, b"no window fits")]:
        bad, _ = _good_block(keep)
        setattr(bad, field, value)
        assert v(bad) < 0, (field, value)
        assert msg in L.gs_last_error(), (field, L.gs_last_error())
    bad, q = _good_block(keep)
    bad.mask, bad.mask_batch_stride = q["mask"], 7
    assert v(bad) < 0 and b"mask_batch_stride" in L.gs_last_error()
    small, _ = _good_block(keep, H=9, W=7)  # below the window: refused with SSIM, fine without
    assert v(small) < 0 and b"no window fits" in L.gs_last_error()
    small.want_ssim = 0
    assert v(small) == 0
    # the entry point runs the validator before anything touches a device
    bad, _ = _good_block(keep)
    bad.W = 0
    assert L.gs_image_metrics(ctypes.byref(bad), None) < 0 and b"must be > 0" in L.gs_last_error()

    n = 13 * 29
    counts = np.zeros(4, np.int64)
    keep.append(counts)
    iv = lambda B=2, n=n, pr=p["pred"], tg=p["target"], thr=0.9, out=counts.ctypes.data: (  # noqa: E731
        L.gs_mask_iou_validate(B, n, pr, tg, thr, out))
    assert iv() == 0 and iv(thr=0.0) == 0
    for kw, msg in [(dict(B=0), b"must be > 0"), (dict(n=0), b"must be > 0"), (dict(n=-3), b"must be > 0"),
                    (dict(B=1 << 20), b"too large"), (dict(pr=None), b"required"), (dict(tg=None), b"required"),
                    (dict(out=None), b"out is required"), (dict(thr=float("nan")), b"NaN"),
                    (dict(pr=p["pred"] + 1), b"4-byte aligned"), (dict(out=counts.ctypes.data + 4), b"8-byte aligned")]:
        assert iv(**kw) < 0, kw
        assert msg in L.gs_last_error(), (kw, L.gs_last_error())
    assert L.gs_mask_iou(0, n, p["pred"], p["target"], 0.9, counts.ctypes.data, None) < 0


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
    D = _DeviceClaim
    pr, tg = torch.rand(2, 3, 13, 29), torch.rand(2, 3, 13, 29)
    with pytest.raises(_lib.GsplatError, match="device tensors"):
        image_metrics(pr, tg)
    with pytest.raises(_lib.GsplatError, match="device tensors"):
        image_metrics(D(pr), tg)
    with pytest.raises(_lib.GsplatError, match="device tensors"):
        mask_iou(pr[:, 0], tg[:, 0])
    with pytest.raises(_lib.GsplatError, match="device tensors"):
        MaskedPSNR().update(pr, tg)
    for bad in (pr.half(), pr.double()):
        with pytest.raises(_lib.GsplatError, match="float32"):
            image_metrics(D(bad), D(bad))
        with pytest.raises(_lib.GsplatError, match="float32"):
            mask_iou(D(bad[:, 0].contiguous()), D(bad[:, 0].contiguous()))
    with pytest.raises(_lib.GsplatError, match="contiguous"):
        image_metrics(D(torch.rand(2, 3, 29, 13).transpose(2, 3)), D(tg))
    with pytest.raises(_lib.GsplatError, match="contiguous"):
        mask_iou(D(pr[:, 0]), D(tg[:, 0]))  # a channel slice
    with pytest.raises(_lib.GsplatError, match="shape"):
        image_metrics(D(pr), D(torch.rand(2, 3, 13, 28)))
    with pytest.raises(_lib.GsplatError, match="shape"):
        mask_iou(D(torch.rand(2, 13, 29)), D(torch.rand(2, 13, 28)))
    with pytest.raises(_lib.GsplatError, match="mask must have shape"):
        image_metrics(D(pr), D(tg), D(torch.ones(3, 13, 29)))
    with pytest.raises(_lib.GsplatError, match="mask must be a device tensor"):
        image_metrics(D(pr), D(tg), torch.ones(13, 29))
    with pytest.raises(_lib.GsplatError, match="no window fits"):
        image_metrics(D(torch.rand(1, 3, 9, 7)), D(torch.rand(1, 3, 9, 7)))
    with pytest.raises(_lib.GsplatError, match="no window fits"):
        image_metrics_torch(torch.rand(1, 3, 9, 7), torch.rand(1, 3, 9, 7))
    with pytest.raises(_lib.GsplatError, match=r"\[B, Ch, H, W\]"):
        image_metrics(D(torch.rand(13, 29)), D(torch.rand(13, 29)))
    with pytest.raises(_lib.GsplatError, match="empty"):
        image_metrics(D(torch.rand(0, 3, 13, 29)), D(torch.rand(0, 3, 13, 29)))
    with pytest.raises(_lib.GsplatError, match="NaN"):
        mask_iou(D(torch.rand(2, 13, 29)), D(torch.rand(2, 13, 29)), float("nan"))


@pytest.mark.skipif(shutil.which("gcc") is None or shutil.which("g++") is None, reason="gcc / g++ not available")
def test_validators_are_sanitizer_clean(tmp_path):
    """gs_metrics_host.cpp (with gs_host.cpp's error state) under ASan + UBSan in a plain CPU
    executable with its own main: nothing preloaded, nothing loaded into Python."""
    run_host_sanitizer(tmp_path, "metrics_host_sanitize.c", ["gs_metrics_host.cpp", "gs_host.cpp"],
                       "metrics host sanitize ok")
