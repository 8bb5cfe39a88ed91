"""The fused photometric loss (csrc/gs_loss.hip) on the GPU against
photometric_loss_torch in fp64 on the CPU.

Bounds: the loss within 1e-5 * max(1, |loss|), every gradient
within 1e-4 relative L2.  Envelope: the image gradient also stays within 10x
the error of the reference formulation itself in fp32 (photometric_loss_torch
in fp32 on the CPU against fp64, computed here; never the code under test),
the margin tests/test_gpu_envelope.py gives the render backward.

The tile is 32 x 32, so the shapes are the small ones: 9 x 7 (smaller than the
window), 37 x 53 (nothing divides the tile), 130 x 75 (five by three tiles,
ragged last ones, halos across interior tile edges), 32 channels of 21 x 70.
"""
from __future__ import annotations

import functools
import os

import numpy as np
import pytest
import torch

from dynamic3dgaussians_amd import photometric_image_loss, photometric_loss, photometric_loss_torch
from dynamic3dgaussians_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizerBatch
from tests import _harness as H

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "photometric_loss.npz")
LOSS_TOL, GRAD_TOL, ENVELOPE = 1e-5, 1e-4, 10.0


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def _smooth(gen, ch, h, w, amp=1.0):
    yy, xx = torch.meshgrid(torch.linspace(0, 1, h), torch.linspace(0, 1, w), indexing="ij")
    f = torch.rand(ch, 4, generator=gen) * 6.0
    base = 0.5 + 0.25 * torch.sin(f[:, 0, None, None] * xx + f[:, 1, None, None]) \
        * torch.cos(f[:, 2, None, None] * yy + f[:, 3, None, None])
    return (amp * (base + 0.05 * torch.randn(ch, h, w, generator=gen))).float()


@functools.lru_cache(maxsize=None)
def _case(name):
    """(image, target, mask, gain, offset): fp32 CPU tensors, batch first; None where absent."""
    gold = np.load(GOLD)
    t = lambda k: torch.from_numpy(gold[k])  # noqa: E731
    gen = torch.Generator().manual_seed(100 + len(name))
    if name in ("small", "flat"):  # the fixture's inputs; identity correction, so x == image exactly
        return (t(f"{name}.image")[None], t(f"{name}.target")[None], None,
                torch.exp(t(f"{name}.cam_m"))[None], t(f"{name}.cam_c")[None])
    if name == "two_cams":
        # camera 0: seeded, all-ones mask; camera 1: the fixture's masked case with its 80 % mask
        im0 = _smooth(gen, 3, 37, 53)
        tg0 = (im0 + 0.1 * torch.randn(3, 37, 53, generator=gen)).float()
        image = torch.stack([im0, t("masked.image")])
        target = torch.stack([tg0, t("masked.target")])
        mask = torch.stack([torch.ones(37, 53), t("masked.mask").float()])
        gain = torch.stack([torch.tensor([1.1, 0.9, 1.05]), torch.exp(t("masked.cam_m"))])
        offset = torch.stack([torch.tensor([-0.02, 0.03, 0.01]), t("masked.cam_c")])
        return image, target, mask, gain, offset
    if name == "tiles":
        im = _smooth(gen, 3, 130, 75)
        return im[None], (im + 0.1 * torch.randn(3, 130, 75, generator=gen)).float()[None], None, None, None
    if name == "features":
        im = (10.0 * torch.randn(2, 32, 21, 70, generator=gen)).float()
        return im, (im + 5.0 * torch.randn(2, 32, 21, 70, generator=gen)).float(), None, None, None
    raise KeyError(name)


def _run(fn, case, dtype, dev, upstream=None, reduction="sum", scale=None):
    """loss (or losses), d image, d gain, d offset of `fn` on copies of the case's tensors."""
    image, target, mask, gain, offset = case
    mv = lambda x, grad: None if x is None else x.to(device=dev, dtype=dtype).requires_grad_(grad)  # noqa: E731
    im, g, o = mv(image, True), mv(gain, True), mv(offset, True)
    out = fn(im, mv(target, False), mask=None if mask is None else mask.to(dev), gain=g, offset=o,
             reduction=reduction)
    wrt = [x for x in (im, g, o) if x is not None]
    if upstream is not None:
        grads = torch.autograd.grad(out, wrt, grad_outputs=torch.tensor(upstream, dtype=dtype, device=dev))
    else:
        grads = torch.autograd.grad(out * scale if scale is not None else out, wrt)
    grads = list(grads) + [None] * (3 - len(grads))
    return out.detach(), grads[0], grads[1], grads[2]


@functools.lru_cache(maxsize=None)
def _oracle(name, upstream=None, reduction="sum", scale=None):
    """The fp64 CPU oracle and the fp32 CPU reference formulation's own image-gradient error."""
    case = _case(name)
    ref = _run(photometric_loss_torch, case, torch.float64, "cpu", upstream, reduction, scale)
    f32 = _run(photometric_loss_torch, case, torch.float32, "cpu", upstream, reduction, scale)
    return ref, _rel(f32[1], ref[1])


def _check(name, upstream=None, reduction="sum", scale=None):
    ref, ref32_err = _oracle(name, upstream, reduction, scale)
    got = _run(photometric_loss, _case(name), torch.float32, DEV, upstream, reduction, scale)
    torch.cuda.synchronize()
    loss_err = float((got[0].double().cpu() - ref[0]).abs().max())
    loss_mag = max(1.0, float(ref[0].abs().max()))
    errs = [None if r is None else _rel(g, r) for g, r in zip(got[1:], ref[1:])]
    print(f"{name}: loss {ref[0].tolist()} err {loss_err:.3e}; rel L2 d_image {errs[0]:.3e} "
          f"d_gain {errs[1]} d_offset {errs[2]}; fp32 reference d_image {ref32_err:.3e} "
          f"(ratio {errs[0] / ref32_err:.2f})")
    assert loss_err <= LOSS_TOL * loss_mag
    for e in errs:
        assert e is None or e <= GRAD_TOL
    assert errs[0] <= ENVELOPE * ref32_err
    return got


def test_image_smaller_than_the_window():
    """B=1, 3 x 9 x 7: every window crosses every border."""
    _check("small")


def test_two_cameras_mask_and_colour_correction():
    """B=2, 3 x 37 x 53: nothing divides the tile, per-camera gain / offset, a [B, H, W] mask
    (all ones for camera 0, 80 % for camera 1)."""
    _check("two_cams")


def test_flat_image():
    """B=1, 3 x 37 x 53 flat: the sigma = E[x^2] - mu^2 cancellation, a fully zero region (m = 1,
    L1 derivative 0) and one pixel with x == y exactly in the non-zero half."""
    image, target, *_ = _case("flat")
    assert image[0, 1, 30, 20] == target[0, 1, 30, 20] != 0
    got = _check("flat")
    # rows 0..17 are zero in both inputs: the window sums vanish up to row 12, so P is exactly 0
    # there, and w * P, the only term that survives x = y = 0, is exactly 0 up to row 7
    assert not got[1][0, :, :8].any()


def test_several_tiles_with_ragged_edges():
    """B=1, 3 x 130 x 75: five by three tiles, halos across interior tile edges."""
    _check("tiles")


def test_feature_channels():
    """B=2, 32 x 21 x 70: values ~ +-10, no mask, no correction."""
    _check("features")


def test_upstream_gradient_is_read_per_image_on_the_device():
    """reduction="none" with upstream [0.25, -3.0]; reduction="sum" scaled by 1/27."""
    got = _check("two_cams", upstream=(0.25, -3.0), reduction="none")
    assert got[0].shape == (2,)
    _check("two_cams", scale=1.0 / 27.0)


def test_two_runs_are_bit_identical():
    a = _run(photometric_loss, _case("two_cams"), torch.float32, DEV)
    b = _run(photometric_loss, _case("two_cams"), torch.float32, DEV)
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_single_image_form_and_optional_inputs():
    """[Ch, H, W] input, a shared [H, W] uint8 mask, gain without offset."""
    image, target, mask, gain, _ = _case("two_cams")
    m = mask[1].to(torch.uint8)
    im = image[1].to(DEV).requires_grad_(True)
    g = gain[1].to(DEV).requires_grad_(True)
    loss = photometric_loss(im, target[1].to(DEV), mask=m.to(DEV), gain=g)
    d_im, d_g = torch.autograd.grad(loss, (im, g))
    im64 = image[1].double().requires_grad_(True)
    g64 = gain[1].double().requires_grad_(True)
    ref = photometric_loss_torch(im64, target[1].double(), mask=m, gain=g64)
    r_im, r_g = torch.autograd.grad(ref, (im64, g64))
    assert loss.dim() == 0 and abs(loss.item() - ref.item()) <= LOSS_TOL * max(1.0, abs(ref.item()))
    assert _rel(d_im, r_im) <= GRAD_TOL and _rel(d_g, r_g) <= GRAD_TOL


def _settings(inp):
    return GaussianRasterizationSettings(
        image_height=inp["image_height"], image_width=inp["image_width"], tanfovx=inp["tan_fovx"],
        tanfovy=inp["tan_fovy"], c_x=inp["c_x"], c_y=inp["c_y"], bg=torch.zeros(3, device=DEV),
        viewmatrix=inp["viewmatrix"].to(DEV), projmatrix=inp["projmatrix"].to(DEV), sh_degree=0,
        campos=inp["campos"].to(DEV))


def test_autograd_hand_over_from_the_batch_render():
    """A 2-camera GaussianRasterizerBatch render taken through photometric_image_loss and through
    photometric_loss_torch on the GPU: the Gaussian parameters' (and cam_m / cam_c's) gradients agree."""
    inps = [H.scene(P=500, W=64, H=48, cam_index=c) for c in (0, 1)]
    ras = GaussianRasterizerBatch([_settings(i) for i in inps])
    gen = torch.Generator().manual_seed(5)
    target = torch.rand(2, 3, 48, 64, generator=gen).to(DEV)
    mask = (torch.rand(48, 64, generator=gen) < 0.8).to(DEV)
    names = ("means3D", "colors", "opacity", "scales", "rotations")

    def grads(loss_fn):
        p = {k: inps[0][k].to(DEV).requires_grad_(True) for k in names}
        cam_m = torch.tensor([[0.05, -0.1, 0.0], [0.0, 0.1, -0.05]], device=DEV, requires_grad=True)
        cam_c = torch.tensor([[0.01, 0.0, -0.02], [0.02, -0.01, 0.0]], device=DEV, requires_grad=True)
        im, _radius, _depth = ras(means3D=p["means3D"], means2D=torch.zeros(500, 3, device=DEV),
                                  opacities=p["opacity"], colors_precomp=p["colors"], scales=p["scales"],
                                  rotations=p["rotations"])
        loss = loss_fn(im, cam_m, cam_c)
        loss.backward()
        return loss.detach(), [p[k].grad for k in names] + [cam_m.grad, cam_c.grad]

    fused = grads(lambda im, m, c: photometric_image_loss(im, target, cam_m=m, cam_c=c, mask=mask))
    plain = grads(lambda im, m, c: photometric_loss_torch(im, target, mask=mask, gain=torch.exp(m), offset=c))
    torch.cuda.synchronize()
    assert abs(fused[0].item() - plain[0].item()) <= LOSS_TOL * max(1.0, abs(plain[0].item()))
    for k, a, b in zip(names + ("cam_m", "cam_c"), fused[1], plain[1]):
        assert float(b.abs().sum()) > 0, k
        assert _rel(a, b) <= GRAD_TOL, (k, _rel(a, b))
