"""The bilinear resample (csrc/gs_resample.hip) and the feature-distillation loss on the GPU
against bilinear_resize_torch in fp64 on the CPU (the fp64 blend with the fp32 weights of the
axis rule, and its autograd adjoint); never the code under test.

Bounds, per element, with u = 2^-24:
  forward   |y - y64| <= 8 u max|its four taps|: three lerps of at most 2.5 roundings each give
            5; the margin to 8 allows for contraction in the blend.
  backward  |d_x - d64| <= (n + 4) u sum |w g| over the element's n terms (n = 0: exactly 0).
Each case prints its measured maxima in these units before it asserts; measured on an MI355X over
all shapes below and both modes: forward <= 2.76 u max|taps|, backward <= 0.45 of its bound.

A thread owns four consecutive x of one row of the side it writes; a workgroup has 256
threads.  Forward: gridDim.y = min(planes, 65535), a workgroup per plane and chunk.  Backward: a
thread takes four planes per step (p0, p0 + gridDim.y, ...; slots past the last plane store
nothing) and further steps with stride 4 gridDim.y, gridDim.y = min(ceil(planes / 4),
2048 / workgroups per plane).  The shapes are the smallest that reach each path:
  1x1 -> 1x1                 degenerate sizes
  1x5 -> 3x1                 an axis of size 1 on either side; untouched columns
  7x9 -> 7x9                 identity: bit-equal forward and backward
  16x16 -> 8x8, 8x8 -> 16x16 exact halves
  37x53 -> 12x31             odd planes (plane 1 unaligned, rows of 31 and 53: scalar stores and
                             tails); untouched rows in the backward: exact zeros; 9 planes: the
                             backward's last slot of four is past the end
  12x31 -> 37x53             upsample, fan-in up to 5 per axis
  130x75 -> 47x48            several workgroups and ragged tails
  200x200 -> 72x128, 2 x 32  the workload's ratios at a quarter of the size
  800x800 -> 288x512, 1 x 2  the real index magnitudes
  1x2 -> 2x1, 1 x 70000      (beyond the issue's list) more planes than gridDim.y holds: the
                             forward's plane walk (70000 > 65535), and in the backward nine steps of
                             4 x 2048 planes with a ragged last one, which no shape above reaches
"""
from __future__ import annotations

import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dynamic3dgaussians_amd import (bilinear_resize, bilinear_resize_torch, depth_correlation_loss,
                                    depth_correlation_loss_torch, distillation_image_loss, feature_distillation_loss,
                                    photometric_loss_torch, resample)
from dynamic3dgaussians_amd.camera import camera_rig
from dynamic3dgaussians_amd.rasterizer import GaussianRasterizationSettings
from dynamic3dgaussians_amd.scene import make_gaussians
from dynamic3dgaussians_amd.timesteps import TimestepDriver, batch_renderer, params2rendervar

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "feature_loss.npz")
U = 2.0 ** -24
LOSS_TOL, GRAD_TOL = 1e-5, 1e-4  # the bars of tests/test_gpu_image_loss.py

# (H, W, h, w, B, Ch)
SHAPES = [(1, 1, 1, 1, 1, 1), (1, 5, 3, 1, 3, 1), (7, 9, 7, 9, 1, 3), (16, 16, 8, 8, 3, 3), (8, 8, 16, 16, 1, 1),
          (37, 53, 12, 31, 3, 3), (12, 31, 37, 53, 1, 3), (130, 75, 47, 48, 1, 32), (200, 200, 72, 128, 2, 32),
          (800, 800, 288, 512, 1, 2), (1, 2, 2, 1, 1, 70000)]
IDS = ["%dx%d-%dx%d" % s[:4] for s in SHAPES]


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def _terms(I, O, align):  # noqa: E741
    """Number of outputs of an axis that tap each input (a clamped output counts twice)."""
    i0, i1, _, _, _ = resample.axis_tables(I, O, align)
    return torch.from_numpy(np.bincount(i0, minlength=I) + np.bincount(i1, minlength=I))


@functools.lru_cache(maxsize=None)
def _oracle(H, W, h, w, B, Ch, align):
    """x, g (fp32, CPU) and the fp64 oracle: y64, the largest tap magnitude per output, d64,
    sum |w g| per input and the number of terms n per input.  Computed once, never modified."""
    gen = torch.Generator().manual_seed(H * 7919 + W * 31 + h * 7 + w + int(align))
    x = torch.randn(B, Ch, H, W, generator=gen)
    g = torch.randn(B, Ch, h, w, generator=gen)
    x64 = x.double().requires_grad_(True)
    y64 = bilinear_resize_torch(x64, (h, w), align_corners=align)
    (d64,) = torch.autograd.grad(y64, x64, g.double())
    a64 = x.double().abs().requires_grad_(True)  # non-negative weights: the adjoint of |g| is sum |w g|
    (wg,) = torch.autograd.grad(bilinear_resize_torch(a64, (h, w), align_corners=align), a64, g.double().abs())
    y0, y1, _, _, _ = resample.axis_tables(H, h, align)
    x0, x1, _, _, _ = resample.axis_tables(W, w, align)
    ax = x.abs()
    y0, y1, x0, x1 = (torch.from_numpy(a.copy()) for a in (y0, y1, x0, x1))
    taps = torch.stack([ax[:, :, ys][..., xs] for ys in (y0, y1) for xs in (x0, x1)]).amax(dim=0)
    n = _terms(H, h, align)[:, None] * _terms(W, w, align)[None, :]
    return x, g, y64.detach(), taps.double(), d64, wg, n.double()


def _gpu(x, g, size, align):
    xd = x.to(DEV).requires_grad_(True)
    y = bilinear_resize(xd, size, align_corners=align)
    (d,) = torch.autograd.grad(y, xd, g.to(DEV))
    torch.cuda.synchronize()
    return y.detach().cpu(), d.cpu()


@pytest.mark.parametrize("align", [False, True])
@pytest.mark.parametrize("H,W,h,w,B,Ch", SHAPES, ids=IDS)
def test_forward_and_backward_against_the_fp64_oracle(H, W, h, w, B, Ch, align):
    x, g, y64, taps, d64, wg, n = _oracle(H, W, h, w, B, Ch, align)
    y, d = _gpu(x, g, (h, w), align)
    assert y.shape == (B, Ch, h, w) and d.shape == x.shape and y.dtype == d.dtype == torch.float32
    ferr = (y.double() - y64).abs()
    fmax = float((ferr / (U * taps).clamp_min(1e-300)).max())
    bound = (n + 4) * U * wg
    berr = (d.double() - d64).abs()
    bmax = float((berr / bound.clamp_min(1e-300))[n.expand_as(berr) > 0].max()) if float(n.max()) > 0 else 0.0
    print(f"{H}x{W}->{h}x{w} B{B} Ch{Ch} align={align}: forward {fmax:.2f} u max|taps| (bound 8), "
          f"backward {bmax:.3f} of (n + 4) u sum|w g| (n up to {int(n.max())})")
    assert bool((ferr <= 8 * U * taps).all())
    assert bool((berr <= bound).all())
    # inputs no output taps: exact zeros, written (not left over)
    untouched = (n == 0).expand_as(d)
    assert not d[untouched].any() and not d64[untouched].any()
    if (H, W) == (37, 53):
        # untouched rows; 53 -> 31 leaves no column untouched (1x5 -> 3x1 has the untouched columns)
        assert int((_terms(H, h, align) == 0).sum()) > 5
        assert (H * W) % 4 == 1 and (h * w) % 4 == 0 and w % 4 == 3  # plane 1 of x unaligned, ragged rows of y
    # the loose bound of tests/test_resample.py against F.interpolate on the CPU, same inputs
    xi = x.clone().requires_grad_(True)
    yi = F.interpolate(xi, size=(h, w), mode="bilinear", align_corners=align)
    (di,) = torch.autograd.grad(yi, xi, g)
    fan = float(n.max())
    assert float((y - yi.detach()).abs().max()) <= 4 * U * (H + W) * float(x.abs().max())
    assert float((d - di).abs().max()) <= 4 * U * (H + W) * float(g.abs().max()) * fan


@pytest.mark.parametrize("align", [False, True])
def test_identity_is_a_bit_exact_copy(align):
    x, g = _oracle(7, 9, 7, 9, 1, 3, align)[:2]
    y, d = _gpu(x, g, (7, 9), align)
    assert torch.equal(y, x) and torch.equal(d, g)
    big = torch.randn(2, 3, 130, 75, generator=torch.Generator().manual_seed(3))
    y, d = _gpu(big, big.flip(0), (130, 75), align)
    assert torch.equal(y, big) and torch.equal(d, big.flip(0))


def test_layouts_agree_bit_for_bit():
    x, g = _oracle(37, 53, 12, 31, 3, 3, False)[:2]
    y, _ = _gpu(x, g, (12, 31), False)
    y3 = bilinear_resize(x[1].to(DEV), (12, 31))
    y2 = bilinear_resize(x[2, 1].contiguous().to(DEV), (12, 31))
    assert y3.shape == (3, 12, 31) and y2.shape == (12, 31)
    assert torch.equal(y3.cpu(), y[1]) and torch.equal(y2.cpu(), y[2, 1])


def test_two_runs_are_bit_identical():
    for shape in (SHAPES[5], SHAPES[6], SHAPES[8]):
        H, W, h, w, B, Ch = shape
        x, g = _oracle(*shape, True)[:2]
        a, b = _gpu(x, g, (h, w), True), _gpu(x, g, (h, w), True)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_backward_overwrites_whatever_its_output_buffer_held():
    """The C entry point on a d_x buffer pre-filled with NaN (and a NaN workspace): every element
    is written, none accumulated."""
    from dynamic3dgaussians_amd import _lib
    L = _lib.load()
    for H, W, h, w, B, Ch in (SHAPES[5], SHAPES[7]):
        x, g, _, _, d64, _, _ = _oracle(H, W, h, w, B, Ch, False)
        gd = g.to(DEV)
        d_x = torch.full((B, Ch, H, W), float("nan"), device=DEV)
        ws = torch.full((L.gs_resample_workspace_bytes(H, W) // 4,), float("nan"), device=DEV)
        args = _lib.GsResample(B=B, Ch=Ch, H=H, W=W, h=h, w=w, align_corners=0, workspace=ws.data_ptr(),
                               workspace_bytes=ws.numel() * 4)
        _lib.check(L.gs_resample_backward(args, gd.data_ptr(), d_x.data_ptr(), _lib.stream(DEV)), "resample backward")
        torch.cuda.synchronize()
        assert not torch.isnan(d_x).any()
        assert torch.equal(d_x.cpu(), _gpu(x, g, (h, w), False)[1])


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.mark.parametrize("name", ["l1", "l1_ssim"])
def test_feature_distillation_loss_against_the_fixture_and_the_torch_composition(gold, name):
    feat = torch.from_numpy(gold[f"{name}.feat"])
    tg = torch.from_numpy(gold[f"{name}.target"])
    kw = dict(l1_weight=float(gold[f"{name}.l1_weight"]), ssim_weight=float(gold[f"{name}.ssim_weight"]))
    xd = feat.to(DEV).requires_grad_(True)
    loss = feature_distillation_loss(xd, tg.to(DEV), **kw)
    (grad,) = torch.autograd.grad(loss, xd)
    torch.cuda.synchronize()
    # the torch composition in fp64 on the CPU
    x64 = feat.double().requires_grad_(True)
    want = photometric_loss_torch(bilinear_resize_torch(x64, tg.shape[-2:], align_corners=True), tg.double(), **kw)
    (gwant,) = torch.autograd.grad(want, x64)
    ref = float(gold[f"{name}.loss"])
    print(f"{name}: loss {loss.item():.8f} fixture {ref:.8f} composition {want.item():.8f}; "
          f"grad rel L2 {_rel(grad, torch.from_numpy(gold[f'{name}.grad_feat'])):.3e} / {_rel(grad, gwant):.3e}")
    assert abs(loss.item() - ref) <= LOSS_TOL * max(1.0, abs(ref))
    assert abs(loss.item() - want.item()) <= LOSS_TOL * max(1.0, abs(want.item()))
    assert _rel(grad, torch.from_numpy(gold[f"{name}.grad_feat"])) <= GRAD_TOL
    assert _rel(grad, gwant) <= GRAD_TOL
    # per-camera vector and the single-map form
    vec = feature_distillation_loss(feat.to(DEV), tg.to(DEV), reduction="none", **kw)
    one = feature_distillation_loss(feat[1].to(DEV), tg[1].to(DEV), **kw)
    assert vec.shape == (2,) and abs(vec.sum().item() - loss.item()) <= 1e-6 and abs(one.item() - vec[1].item()) <= 1e-6


def test_depth_line_of_the_fixture(gold):
    """37 x 53 -> 12 x 31 with half-pixel centres, the reference's depth resample, against the
    recorded fp64 map: the forward bound plus the fp32 weights' distance from fp64 ones."""
    x = torch.from_numpy(gold["depth.feat"])
    y = bilinear_resize(x.to(DEV), (12, 31), align_corners=False).cpu()
    err = float((y.double() - torch.from_numpy(gold["depth.resized"])).abs().max())
    assert err <= (8 * U + 4 * U * (37 + 53)) * float(x.abs().max())


def test_distillation_image_loss_is_the_sum_of_its_two_terms(gold):
    gen = torch.Generator().manual_seed(17)
    feat, prior = torch.from_numpy(gold["l1.feat"]), torch.from_numpy(gold["l1.target"])
    im, gt = torch.rand(2, 3, 40, 56, generator=gen), torch.rand(2, 3, 40, 56, generator=gen)
    imd, fd = im.to(DEV).requires_grad_(True), feat.to(DEV).requires_grad_(True)
    loss = distillation_image_loss((imd, fd), (gt.to(DEV), prior.to(DEV)), feature_weight=0.5)
    g_im, g_f = torch.autograd.grad(loss, (imd, fd))
    torch.cuda.synchronize()
    i64, f64 = im.double().requires_grad_(True), feat.double().requires_grad_(True)
    want = photometric_loss_torch(i64, gt.double()) + 0.5 * photometric_loss_torch(
        bilinear_resize_torch(f64, (18, 32), align_corners=True), prior.double(), l1_weight=1.0, ssim_weight=0.0)
    w_im, w_f = torch.autograd.grad(want, (i64, f64))
    assert abs(loss.item() - want.item()) <= LOSS_TOL * max(1.0, abs(want.item()))
    assert _rel(g_im, w_im) <= GRAD_TOL and _rel(g_f, w_f) <= GRAD_TOL
    # the feature term of the oracle is the fixture's loss: fp64 on both sides once the axis rule is fp64 too
    f_term = photometric_loss_torch(bilinear_resize_torch(feat.double(), (18, 32), align_corners=True,
                                                          axis_dtype=torch.float64), prior.double(),
                                    l1_weight=1.0, ssim_weight=0.0)
    assert abs(float(gold["l1.loss"]) - f_term.item()) <= 1e-10


N_CAMS, WW, HH, P, NF = 2, 64, 48, 600, 32


def _settings():
    return [GaussianRasterizationSettings(
        image_height=HH, image_width=WW, tanfovx=c.tanfovx, tanfovy=c.tanfovy, c_x=c.c_x, c_y=c.c_y,
        bg=torch.zeros(3, device=DEV), viewmatrix=torch.from_numpy(c.viewmatrix.copy()).to(DEV),
        projmatrix=torch.from_numpy(c.projmatrix.copy()).to(DEV), sh_degree=0,
        campos=torch.from_numpy(c.campos.copy()).to(DEV)) for c in camera_rig(N_CAMS, WW, HH, seed=3)]


def _leaves(F_=NF):
    g = make_gaussians(P, F=F_, seed=4, scale_mult=3.0, device=DEV)
    p = {"means3D": g["means3D"], "rgb_colors": g["colors"], "unnorm_rotations": g["rotations"],
         "logit_opacities": torch.logit(g["opacities"].clamp(1e-4, 1 - 1e-4)), "log_scales": torch.log(g["scales"])}
    if F_:
        p["semantic_feature"] = g["semantic_feature"]
    return {k: torch.nn.Parameter(v.detach().clone().contiguous()) for k, v in p.items()}


def test_driver_step_with_the_distillation_loss():
    """A 2-camera G3 render (F = 32, 64 x 48) trained one step through TimestepDriver with
    image_loss=distillation_image_loss against priors of 24 x 32: the gradients reach
    semantic_feature and equal the per-camera autograd formulation over bilinear_resize_torch."""
    settings = _settings()
    gen = torch.Generator().manual_seed(12)
    tg = torch.rand(N_CAMS, 3, HH, WW, generator=gen).to(DEV)
    prior = torch.randn(N_CAMS, NF, 24, 32, generator=gen).to(DEV)
    params = _leaves()
    opt = torch.optim.SGD([{"params": [params[k]], "name": k, "lr": 0.0} for k in params], lr=0.0)
    drv = TimestepDriver(params, {}, opt, N_CAMS, batch_renderer(settings),
                         image_loss=functools.partial(distillation_image_loss, feature_weight=1.0))
    loss = drv.step((tg, prior))
    ref = _leaves()
    (im, feat), _stats = batch_renderer(settings)(params2rendervar(ref), list(range(N_CAMS)))
    assert feat.shape == (N_CAMS, NF, HH, WW)
    want = sum(photometric_loss_torch(im[c], tg[c])
               + photometric_loss_torch(bilinear_resize_torch(feat[c], (24, 32), align_corners=True), prior[c],
                                        l1_weight=1.0, ssim_weight=0.0) for c in range(N_CAMS)) / N_CAMS
    want.backward()
    torch.cuda.synchronize()
    assert abs(loss - want.item()) <= LOSS_TOL * max(1.0, abs(want.item()))
    for k in params:
        a, b = params[k].grad, ref[k].grad
        assert a is not None and torch.isfinite(a).all() and float(b.abs().sum()) > 0, k
        print(f"driver {k}: rel L2 {_rel(a, b):.3e}")
        assert _rel(a, b) <= GRAD_TOL, (k, _rel(a, b))


def test_depth_composition_reaches_the_means():
    """depth_correlation_loss(bilinear_resize(depth, (h, w), align_corners=False), prior_hw, mask=mask_hw),
    the reference's dyn_double.py:303 followed by its correlation loss, as a TimestepDriver
    depth_loss closure: equal to the torch composition, and the gradient reaches means3D."""
    settings = _settings()
    render = batch_renderer(settings, with_depth=True)
    gen = torch.Generator().manual_seed(13)
    with torch.no_grad():
        d0 = render(params2rendervar(_leaves(0)), [0, 1])[2]
    assert d0.shape == (N_CAMS, 1, HH, WW)
    small = bilinear_resize_torch(d0, (18, 32))
    mask = (small[:, 0] > 0.2) & (torch.rand(N_CAMS, 18, 32, generator=gen) < 0.8).to(DEV)
    assert int(mask[0].sum()) > 30 and int(mask[1].sum()) > 30
    prior = (1.0 / (1.3 * small.clamp_min(0.2)) + 0.05 * torch.randn(N_CAMS, 1, 18, 32, generator=gen).to(DEV)).contiguous()

    def grads(resize, corr):
        p = _leaves(0)
        depth = render(params2rendervar(p), [0, 1])[2]
        loss = corr(resize(depth, (18, 32), align_corners=False), prior, mask=mask)
        loss.backward()
        return loss.detach(), p["means3D"].grad

    fused = grads(bilinear_resize, depth_correlation_loss)
    plain = grads(bilinear_resize_torch, depth_correlation_loss_torch)
    torch.cuda.synchronize()
    assert abs(fused[0].item() - plain[0].item()) <= LOSS_TOL * max(1.0, abs(plain[0].item()))
    assert float(fused[1].abs().sum()) > 0 and torch.isfinite(fused[1]).all()
    print(f"depth composition means3D: rel L2 {_rel(fused[1], plain[1]):.3e}")
    assert _rel(fused[1], plain[1]) <= GRAD_TOL
