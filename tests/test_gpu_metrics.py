"""The evaluation metrics (csrc/gs_metrics.hip) on the GPU against
image_metrics_torch / mask_iou_torch in fp64 on the CPU.

Bounds: sse and sae within 1e-5 relative (the project's loss bound, SURVEY.md
8(c)); mask_sum and the IoU counts exact; ssim within max(1e-5, 10 x the error
of the reference formulation itself in fp32: image_metrics_torch in fp32 on the
CPU against fp64, computed here, never the code under test), per image, the
margin tests/test_gpu_envelope.py and tests/test_gpu_image_loss.py give.  On
the flat case the formulation's own fp32 error (the E[z^2] - mu^2
cancellation) is above 1e-5, which is why the bound is an envelope.

The tile is 32 x 32 and the window 11, so the shapes are the fixture's small
ones: 11 x 11 (one output pixel), 13 x 29 (windows without an unmasked tap),
45 x 77 (2 x 3 tiles over the inputs, 2 x 3 ragged ones over the 35 x 67
outputs, halos across interior tile edges, masks per image and shared),
37 x 53 flat, 32 channels of 21 x 40, and 9 x 7 without the SSIM.
"""
from __future__ import annotations

import functools
import os

import numpy as np
import pytest
import torch

from dynamic3dgaussians_amd import metrics as M
from dynamic3dgaussians_amd.camera import camera_rig
from dynamic3dgaussians_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizerBatch
from dynamic3dgaussians_amd.scene import make_gaussians

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_metrics.npz")
SUM_TOL, SSIM_FLOOR, ENVELOPE = 1e-5, 1e-5, 10.0
CASES = ("one_window", "empty_windows", "ragged_masked", "shared_mask", "flat", "features")


@functools.lru_cache(maxsize=None)
def _case(name):
    """(pred, target, mask): fp32 CPU tensors of the fixture; None without a mask."""
    gold = np.load(GOLD)
    src = "ragged_masked" if name == "shared_mask" else name
    pred, target = torch.from_numpy(gold[f"{src}.pred"]), torch.from_numpy(gold[f"{src}.target"])
    mask = torch.from_numpy(gold[f"{src}.mask"]).float() if f"{src}.mask" in gold.files else None
    if name == "shared_mask":
        mask = mask[1]  # [H, W]: the one with the hole, for both images
    return pred, target, mask


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """The fp64 CPU oracle and the fp32 CPU reference formulation's own per-image ssim error."""
    pred, target, mask = _case(name)
    ref = M.image_metrics_torch(pred.double(), target.double(), mask)
    f32 = M.image_metrics_torch(pred, target, mask)
    return ref, ((f32.ssim.double() - ref.ssim).abs() / ref.ssim.abs())


def _device(name):
    return tuple(None if x is None else x.to(DEV) for x in _case(name))


def _rel(got, ref):
    return (got.double().cpu() - ref).abs() / ref.abs().clamp_min(1e-300)


@pytest.mark.parametrize("name", CASES)
def test_fixture_cases_against_the_fp64_restatement(name):
    ref, err32 = _oracle(name)
    got = M.image_metrics(*_device(name))
    torch.cuda.synchronize()
    assert got.shape == ref.shape and got.sse.shape == ref.sse.shape and got.sse.dtype == torch.float32
    e_sse, e_sae, e_ssim = _rel(got.sse, ref.sse), _rel(got.sae, ref.sae), _rel(got.ssim, ref.ssim)
    bound = torch.maximum(torch.full_like(err32, SSIM_FLOOR), ENVELOPE * err32)
    print(f"{name}: ssim {ref.ssim.tolist()} rel err {e_ssim.tolist()}; fp32 reference {err32.tolist()} "
          f"(ratio {(e_ssim / err32.clamp_min(1e-300)).tolist()}, bound {bound.tolist()}); "
          f"sse rel {e_sse.tolist()} sae rel {e_sae.tolist()}")
    assert torch.all(e_sse <= SUM_TOL) and torch.all(e_sae <= SUM_TOL)
    assert torch.equal(got.mask_sum.double().cpu(), ref.mask_sum)
    assert torch.all(e_ssim <= bound)
    # the derived PSNRs are the same sums
    for fn in (M.psnr_masked, M.psnr_clamped, M.psnr_plain, M.l1):
        assert torch.allclose(fn(got).cpu(), fn(ref), rtol=1e-4, atol=0), fn.__name__


def test_single_image_call_returns_scalars():
    pred, target, mask = _device("ragged_masked")
    ref, _ = _oracle("ragged_masked")
    got = M.image_metrics(pred[1], target[1], mask[1])
    whole = M.image_metrics(pred, target, mask)
    assert got.ssim.dim() == 0 and got.shape == ref.shape
    for a, b in zip(got[:4], whole[:4]):
        assert torch.equal(a, b[1])


def test_identical_images_score_exactly_one():
    """pred == target under the mask with empty windows: every map value is 1 exactly
    (numerator and denominator round alike), so is their mean; the error sums are 0."""
    pred, _, mask = _device("empty_windows")
    got = M.image_metrics(pred, pred.clone(), mask)
    assert torch.equal(got.ssim.cpu(), torch.ones(2)) and torch.equal(got.sse.cpu(), torch.zeros(2))
    assert torch.equal(got.sae.cpu(), torch.zeros(2))
    plain = M.image_metrics(pred, pred.clone())
    assert torch.equal(plain.ssim.cpu(), torch.ones(2))


def test_sums_alone_below_the_window_size():
    gen = torch.Generator().manual_seed(5)
    pred, target = torch.rand(1, 3, 9, 7, generator=gen), torch.rand(1, 3, 9, 7, generator=gen)
    mask = (torch.rand(1, 9, 7, generator=gen) < 0.8).float()
    ref = M.image_metrics_torch(pred.double(), target.double(), mask, ssim=False)
    got = M.image_metrics(pred.to(DEV), target.to(DEV), mask.to(DEV), ssim=False)
    assert torch.all(_rel(got.sse, ref.sse) <= SUM_TOL) and torch.all(_rel(got.sae, ref.sae) <= SUM_TOL)
    assert torch.equal(got.mask_sum.double().cpu(), ref.mask_sum)
    assert torch.equal(got.ssim.cpu(), torch.zeros(1))
    with pytest.raises(M.GsplatError, match="no window fits"):
        M.image_metrics(pred.to(DEV), target.to(DEV))
    # ssim=False on a shape that has windows: the same sums as with them
    pred, target, mask = _device("ragged_masked")
    a, b = M.image_metrics(pred, target, mask, ssim=False), M.image_metrics(pred, target, mask)
    assert all(torch.equal(x, y) for x, y in zip(a[:3], b[:3])) and torch.equal(a.ssim.cpu(), torch.zeros(2))


def test_two_runs_are_bit_identical():
    for name in ("ragged_masked", "features"):
        args = _device(name)
        a, b = M.image_metrics(*args), M.image_metrics(*args)
        assert all(torch.equal(x, y) for x, y in zip(a[:4], b[:4]))
    sp, st = _soft_masks()
    assert all(torch.equal(x, y) for x, y in zip(M.mask_iou(sp, st), M.mask_iou(sp, st)))


def _soft_masks():
    gold = np.load(GOLD)
    return torch.from_numpy(gold["iou.pred"]).to(DEV), torch.from_numpy(gold["iou.target"]).to(DEV)


def test_mask_iou_counts_are_exact():
    """2 x 45 x 77 soft masks at 0.9 and at 0, and a pair with an empty union (image 2 of the
    fixture stays below 0.9): the counts of the torch restatement, the ratio 1 for the empty one."""
    sp, st = _soft_masks()
    for pr, tg in ((sp[:2].contiguous(), st[:2].contiguous()), (sp, st)):
        for thr in (0.9, 0.0):
            i, u = M.mask_iou(pr, tg, thr)
            ri, ru = M.mask_iou_torch(pr.cpu(), tg.cpu(), thr)
            assert i.dtype == torch.int64 and i.is_cuda and i.shape == ri.shape
            assert torch.equal(i.cpu(), ri) and torch.equal(u.cpu(), ru), thr
    i, u = M.mask_iou(sp, st)
    assert u[2].item() == 0 and M.iou(sp, st)[2].item() == 1.0 and 0 < M.iou(sp, st)[0].item() < 1
    one = M.mask_iou(sp[0], st[0])
    assert one[0].dim() == 0 and one[0] == i[0] and one[1] == u[0]
    # more than one chunk of 16384 pixels per image, a ragged last one
    gen = torch.Generator().manual_seed(9)
    big_p, big_t = torch.rand(2, 150, 231, generator=gen), torch.rand(2, 150, 231, generator=gen)
    i, u = M.mask_iou(big_p.to(DEV), big_t.to(DEV), 0.5)
    ri, ru = M.mask_iou_torch(big_p, big_t, 0.5)
    assert torch.equal(i.cpu(), ri) and torch.equal(u.cpu(), ru)


def _settings(n, W, H):
    return [GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=c.tanfovx, tanfovy=c.tanfovy, c_x=c.c_x, c_y=c.c_y,
        bg=torch.zeros(3, device=DEV), viewmatrix=torch.from_numpy(c.viewmatrix.copy()).to(DEV),
        projmatrix=torch.from_numpy(c.projmatrix.copy()).to(DEV), sh_degree=0,
        campos=torch.from_numpy(c.campos.copy()).to(DEV), compat="reference") for c in camera_rig(27, W, H)[:n]]


def _scene(P=600, W=48, H=40, seed=3):
    """Two cameras of 48 x 40 over a small seeded scene, colours past 1 so that the clip acts
    (the render's maximum is 1.47 for both cameras)."""
    g = make_gaussians(P, seed=seed, scale_mult=6.0, device=DEV)
    rv = {"means3D": g["means3D"], "colors_precomp": g["colors"] * 1.6, "rotations": g["rotations"],
          "opacities": g["opacities"], "scales": g["scales"], "means2D": torch.zeros_like(g["means3D"])}
    rv = {k: v.clone().requires_grad_(True) for k, v in rv.items()}
    gen = torch.Generator().manual_seed(seed)
    targets = torch.rand(2, 3, H, W, generator=gen).to(DEV)
    masks = torch.ones(2, H, W)
    masks[0] = (torch.rand(H, W, generator=gen) < 0.8).float()  # a mask for camera 0 only
    seg, seg_t = torch.rand(2, H, W, generator=gen).to(DEV), torch.rand(2, H, W, generator=gen).to(DEV)
    return rv, _settings(2, W, H), targets, masks.to(DEV), seg, seg_t


def test_evaluate_cameras_scores_its_own_render():
    """Plumbing, clipping and mask routing (not renderer parity): every returned metric is the
    fp64 restatement of the call's own rendered images read back."""
    rv, sets, targets, masks, seg, seg_t = _scene()
    out = M.evaluate_cameras(rv, sets, targets, masks, seg=seg, seg_targets=seg_t)
    torch.cuda.synchronize()
    im = out["image"]
    assert im.shape == (2, 3, 40, 48) and float(im.max()) == 1.0 and float(im.min()) >= 0.0
    raw = GaussianRasterizerBatch(sets)(**{k: v.detach() for k, v in rv.items()})[0]
    assert float(raw.max()) > 1.0 and torch.equal(raw.clamp(0, 1), im)  # the clip acted, on this render
    ref = M.image_metrics_torch(im.double().cpu(), targets.double().cpu(), masks.cpu())
    f32 = M.image_metrics_torch(im.cpu(), targets.cpu(), masks.cpu())  # the formulation's own fp32 error
    ssim_tol = torch.clamp(ENVELOPE * (f32.ssim.double() - ref.ssim).abs() / ref.ssim.abs(), min=SSIM_FLOOR)
    for k, want, tol in (("sse", ref.sse, SUM_TOL), ("sae", ref.sae, SUM_TOL), ("ssim", ref.ssim, ssim_tol),
                         ("l1", M.l1(ref), SUM_TOL), ("psnr", M.psnr_plain(ref), SUM_TOL),
                         ("psnr_masked", M.psnr_masked(ref), SUM_TOL)):
        assert out[k].shape == (2,) and out[k].is_cuda, k
        assert torch.all(_rel(out[k], want) <= tol), (k, out[k], want)
    assert torch.equal(out["mask_sum"].double().cpu(), ref.mask_sum) and ref.mask_sum[1] == 40 * 48
    ri, ru = M.mask_iou_torch(seg.cpu(), seg_t.cpu(), 0.9)
    assert torch.equal(out["intersection"].cpu(), ri) and torch.equal(out["union"].cpu(), ru)
    assert torch.equal(out["iou"].cpu(), M.iou_ratio(ri, ru))
    assert all(v.grad is None for v in rv.values())
    assert not any(v.requires_grad for v in out.values() if isinstance(v, torch.Tensor))
    unclipped = M.evaluate_cameras(rv, sets, targets, clip=False)
    assert torch.equal(unclipped["image"], raw) and "psnr_masked" not in unclipped and "iou" not in unclipped


def test_evaluate_sequence_reports_the_means_of_its_timesteps():
    rv, sets, targets, masks, _, _ = _scene()
    g = {k: v.detach() for k, v in rv.items()}
    base = {"means3D": g["means3D"], "rgb_colors": g["colors_precomp"], "unnorm_rotations": g["rotations"],
            "logit_opacities": torch.logit(g["opacities"].clamp(1e-4, 1 - 1e-4)), "log_scales": torch.log(g["scales"])}
    steps = [base, {**base, "means3D": base["means3D"] + 0.01}]
    out = M.evaluate_sequence(steps, sets, lambda t: targets, lambda t: masks)
    assert out["images"] == 4 and set(out) == {"psnr", "l1", "mssim", "mpsnr", "images"}
    from dynamic3dgaussians_amd.timesteps import params2rendervar
    per = [M.evaluate_cameras(params2rendervar(p), sets, targets, masks) for p in steps]
    for key, src in (("psnr", "psnr"), ("l1", "l1"), ("mssim", "ssim"), ("mpsnr", "psnr_masked")):
        want = torch.cat([r[src].double() for r in per]).mean().item()
        assert abs(out[key] - want) <= 1e-12 * abs(want), key
    assert "mpsnr" not in M.evaluate_sequence(steps, sets, lambda t: targets)


def test_updates_and_evaluate_cameras_make_no_host_sync():
    """torch.cuda.set_sync_debug_mode("error") raises at every torch call that makes the host wait
    for the device.  Armed on an .item() first, which must raise.  compute() runs outside."""
    pred, target, mask = _device("ragged_masked")
    sp, st = _soft_masks()
    rv, sets, targets, masks, seg, seg_t = _scene()
    ras = GaussianRasterizerBatch(sets)
    # warm-ups outside the mode: the library is loaded, the rasterizer's plan is sized
    M.evaluate_cameras(rv, ras, targets, masks, seg=seg, seg_targets=seg_t)
    M.image_metrics(pred, target, mask)
    M.mask_iou(sp, st)
    accs = [M.MaskedPSNR(), M.MaskedSSIM(), M.MaskIoU(), M.MeanIoU()]
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode("error")
        try:
            pred.sum().item()
            armed = False
        except RuntimeError as e:
            armed = "synchroniz" in str(e)
        if armed:
            for _ in range(3):
                accs[0].update(pred, target, mask)
                accs[1].update(pred, target, mask)
                accs[2].update(sp, st)
                accs[3].update(sp, st)
            out = M.evaluate_cameras(rv, ras, targets, masks, seg=seg, seg_targets=seg_t)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert armed, "torch's sync debug mode did not raise at .item(): the guard checked nothing"
    ref, _ = _oracle("ragged_masked")
    ri, ru = M.mask_iou_torch(sp.cpu(), st.cpu(), 0.9)
    r0i, r0u = M.mask_iou_torch(sp.cpu(), st.cpu(), 0.0)
    want = [float(M.psnr_masked(ref._replace(sse=ref.sse.sum(), mask_sum=ref.mask_sum.sum()))), float(ref.ssim.mean()),
            float(r0i.sum()) / float(r0u.sum()), float(M.iou_ratio(ri, ru).mean())]
    for acc, w in zip(accs, want):
        assert len(acc) == 3 and abs(acc.compute() - w) <= 1e-4 * abs(w), type(acc).__name__
    assert torch.isfinite(out["psnr"]).all() and out["iou"].shape == (2,)
