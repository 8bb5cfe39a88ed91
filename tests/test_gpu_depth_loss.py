"""The fused depth-correlation loss (csrc/gs_depth_loss.hip) on the GPU against
depth_correlation_loss_torch in fp64 on the CPU.

Bounds (as tests/test_gpu_image_loss.py): the loss within
1e-5 * max(1, |loss|), the depth gradient within 1e-4 relative L2.  Envelope:
the gradient also stays within 10x the error of the reference formulation
itself in fp32 (depth_correlation_loss_torch in fp32 on the CPU against fp64,
computed here; never the code under test).

A workgroup takes chunks of 1024 pixels, a wave 256, a thread 4, so the shapes
are the small ones: 3 x 5 (less than a wave), 37 x 53 (odd H*W: camera 1's
planes are unaligned), 64 x 64 (aligned, whole waves only), 130 x 75 (ten
workgroups and a ragged tail), 257 x 300 (76 workgroup records: more than a
wave of the finisher holds), and 363 x 401 (143 chunks: past the cap of 128
workgroups per camera, so some workgroups take a second chunk).
"""
from __future__ import annotations

import functools
import os

import numpy as np
import pytest
import torch

from dynamic3dgaussians_amd import _lib, depth_correlation_loss, depth_correlation_loss_torch
from dynamic3dgaussians_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizerBatch
from dynamic3dgaussians_amd.timesteps import TimestepDriver, batch_renderer, l1_image_loss, params2rendervar
from tests import _harness as H

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "depth_loss.npz")
LOSS_TOL, GRAD_TOL, ENVELOPE = 1e-5, 1e-4, 10.0
NEAR, FAR = 1e-7, 50.0


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def _field(gen, b, h, w):
    """Depths of about 1 to 10 (a smooth field plus 0.3 |N(0, 1)|) and the prior 1 / (s d) plus
    0.05 N(0, 1), one scale s per camera."""
    yy, xx = torch.meshgrid(torch.linspace(0, 1, h), torch.linspace(0, 1, w), indexing="ij")
    f = torch.rand(b, 4, generator=gen) * 5.0
    base = 0.5 + 0.45 * torch.sin(f[:, 0, None, None] * xx + f[:, 1, None, None]) \
        * torch.cos(f[:, 2, None, None] * yy + f[:, 3, None, None])
    depth = (1.0 + 8.5 * base + 0.3 * torch.randn(b, h, w, generator=gen).abs()).float()
    s = 0.5 + 2.0 * torch.rand(b, 1, 1, generator=gen)
    target = (1.0 / (s * depth) + 0.05 * torch.randn(b, h, w, generator=gen)).float()
    return depth, target


@functools.lru_cache(maxsize=None)
def _case(name):
    """(depth [B, H, W], target [B, H, W], mask or None): fp32 / uint8 CPU tensors, never modified."""
    gold = np.load(GOLD)
    t = lambda k: torch.from_numpy(gold[k])  # noqa: E731
    gen = torch.Generator().manual_seed(200 + len(name))
    if name == "tiny":
        return t("tiny.depth")[None], t("tiny.target")[None], None
    if name == "two_cams":
        return (torch.stack([t("masked.depth"), t("gated.depth")]), torch.stack([t("masked.target"), t("gated.target")]),
                torch.stack([t("masked.mask"), t("gated.mask")]))
    if name == "aligned":
        return (*_field(gen, 3, 64, 64), None)
    if name == "shared_mask":
        d, g = _field(gen, 3, 130, 75)
        u = torch.rand(3, 130, 75, generator=gen)
        d[u < 0.10] = 80.0  # beyond far
        d[u > 0.98] = 0.0   # below near
        return d, g, (torch.rand(130, 75, generator=gen) < 0.6).to(torch.uint8)
    if name == "large":
        return (*_field(gen, 1, 257, 300), (torch.rand(1, 257, 300, generator=gen) < 0.6).to(torch.uint8))
    if name == "looped":
        return (*_field(gen, 1, 363, 401), (torch.rand(1, 363, 401, generator=gen) < 0.6).to(torch.uint8))
    if name == "half_segments":
        # every thread's four pixels half masked: the first two (camera 0), every second one (camera 1)
        m = torch.stack([torch.tensor([1, 1, 0, 0], dtype=torch.uint8).repeat(64 * 16).reshape(64, 64),
                         torch.tensor([0, 1, 0, 1], dtype=torch.uint8).repeat(64 * 16).reshape(64, 64)])
        return (*_field(gen, 2, 64, 64), m)
    if name == "row_bands":
        # 96 x 64 = six workgroups of 16 rows: rows 4..7 of each are masked out (the whole of the
        # workgroup's second wave: an empty wave record), and so is all of workgroup 2 (rows
        # 32..47: an empty workgroup record), and three of the four pixels of row 0's threads
        m = torch.ones(1, 96, 64, dtype=torch.uint8)
        for wg in range(6):
            m[0, 16 * wg + 4:16 * wg + 8] = 0
        m[0, 32:48] = 0
        m[0, 0].view(16, 4)[:, 1:] = 0
        return (*_field(gen, 1, 96, 64), m)
    if name in ("empty_mask", "constant_depth", "healthy"):
        # three cameras of 20 x 23 (odd H*W); camera 1 is degenerate in the first two
        d, g = _field(torch.Generator().manual_seed(77), 3, 20, 23)
        m = (torch.rand(3, 20, 23, generator=torch.Generator().manual_seed(78)) < 0.8).to(torch.uint8)
        if name == "empty_mask":
            m[1] = 0
        if name == "constant_depth":
            d[1] = 2.0  # 1 / 2 and its sums are exact: Sxx is 0 in any precision and order
        return d, g, m
    raise KeyError(name)


def _run(fn, case, dtype, dev, upstream=None, reduction="sum", scale=None, layout="BHW", **kw):
    """(loss or losses, d depth as [B, H, W]) of `fn` on copies of the case's tensors."""
    depth, target, mask = case
    shape = {"BHW": depth.shape, "B1HW": (depth.shape[0], 1, *depth.shape[1:]), "HW": depth.shape[1:]}[layout]
    d = depth.to(device=dev, dtype=dtype).reshape(shape).clone().requires_grad_(True)
    g = target.to(device=dev, dtype=dtype).reshape(shape)
    out = fn(d, g, mask=None if mask is None else mask.to(dev), reduction=reduction, **kw)
    stats = None
    if isinstance(out, tuple):
        out, stats = out
    if upstream is not None:
        (grad,) = torch.autograd.grad(out, d, grad_outputs=torch.tensor(upstream, dtype=dtype, device=dev))
    else:
        (grad,) = torch.autograd.grad(out * scale if scale is not None else out, d)
    return out.detach(), grad.reshape(depth.shape), stats


@functools.lru_cache(maxsize=None)
def _oracle(name, upstream=None, reduction="sum", scale=None):
    """The fp64 CPU oracle and the fp32 CPU reference formulation's own gradient error."""
    ref = _run(depth_correlation_loss_torch, _case(name), torch.float64, "cpu", upstream, reduction, scale)
    f32 = _run(depth_correlation_loss_torch, _case(name), torch.float32, "cpu", upstream, reduction, scale)
    return ref, _rel(f32[1], ref[1])


def _check(name, upstream=None, reduction="sum", scale=None):
    ref, ref32_err = _oracle(name, upstream, reduction, scale)
    got = _run(depth_correlation_loss, _case(name), torch.float32, DEV, upstream, reduction, scale)
    torch.cuda.synchronize()
    loss_err = float((got[0].double().cpu() - ref[0]).abs().max())
    loss_mag = max(1.0, float(ref[0].abs().max()))
    err = _rel(got[1], ref[1])
    print(f"{name}: loss {ref[0].tolist()} err {loss_err:.3e}; rel L2 d_depth {err:.3e}; "
          f"fp32 reference d_depth {ref32_err:.3e} (ratio {err / ref32_err:.2f})")
    assert loss_err <= LOSS_TOL * loss_mag
    assert err <= GRAD_TOL
    assert err <= ENVELOPE * ref32_err
    depth, _, mask = _case(name)
    closed = (depth < NEAR) | (depth > FAR)
    if mask is not None:
        closed = closed | (mask.expand_as(depth) == 0)
    # exactly 0.0 outside the mask and where the clamp is active, as in the oracle
    assert not got[1].cpu()[closed].any() and not ref[1][closed].any()
    return got


def test_less_than_a_wave():
    """1 x 3 x 5, the fixture's plane: one workgroup, the scalar path only."""
    _check("tiny")


def test_fixture_planes_stacked_with_unaligned_second_camera():
    """2 x 37 x 53 with a [B, H, W] mask: H*W = 1961 is odd, so camera 1's planes start 4 bytes
    off a 16-byte boundary; the gated plane has depths beyond far and at 0."""
    depth, _, mask = _case("two_cams")
    assert (depth.shape[1] * depth.shape[2]) % 4 == 1
    assert (depth[1] > FAR).sum() > 100 and (depth[1] < NEAR).sum() > 10 and (mask == 0).sum() > 500
    _check("two_cams")


def test_aligned_whole_segments_without_mask():
    """3 x 64 x 64: every plane 16-byte aligned, four whole chunks each, no mask."""
    _check("aligned")


def test_several_workgroups_shared_mask_ragged_tail():
    """3 x 130 x 75 with one [H, W] mask: ten workgroups per camera, the last one ragged (9750 =
    9 * 1024 + 534), camera 1 unaligned (9750 % 4 = 2), clamp gates on both sides."""
    _check("shared_mask")


def test_more_records_than_a_wave_holds():
    """1 x 257 x 300: the finisher merges 76 workgroup records (its threads 0..75, two waves)."""
    records = _lib.load().gs_depth_loss_workspace_bytes(1, 257, 300) // (6 * 4)
    assert records == 76 and records > 64
    _check("large")


def test_workgroups_that_walk_several_chunks():
    """1 x 363 x 401, 143 chunks of 1024 pixels (the last one of 155): past the cap of 128
    workgroups per camera, so workgroups 0..14 take a second chunk in both passes and the others
    do not.  The one plane here that is larger than 257 x 300: up to 128 chunks no workgroup loops."""
    L = _lib.load()
    assert L.gs_depth_loss_workspace_bytes(1, 363, 401) // (6 * 4) == 128 and -(-363 * 401 // 1024) == 143
    _check("looped")


def test_half_masked_segments():
    """2 x 64 x 64, each thread's 16-byte segment half masked in a fixed pattern."""
    _check("half_segments")


def test_empty_partial_records_inside_a_valid_camera():
    """1 x 96 x 64: empty thread, wave and workgroup records (n = 0) meet the pairwise merge."""
    got = _check("row_bands")
    stats = _run(depth_correlation_loss, _case("row_bands"), torch.float32, DEV, return_stats=True)[2]
    assert stats[0, 0].item() == float(_case("row_bands")[2].sum()) and stats[0, 7].item() == 1.0
    assert torch.isfinite(got[1]).all()


@pytest.mark.parametrize("kind", ["empty_mask", "constant_depth"])
def test_degenerate_camera_in_a_batch(kind):
    case, healthy = _case(kind), _case("healthy")
    ones = (1.0, 1.0, 1.0)
    want = _run(depth_correlation_loss, healthy, torch.float32, DEV, ones, "none", return_stats=True)
    # default: NaN as the reference, the neighbours untouched bit for bit
    loss, grad, stats = _run(depth_correlation_loss, case, torch.float32, DEV, ones, "none", return_stats=True)
    torch.cuda.synchronize()
    assert torch.isnan(loss[1]) and stats[1, 7] == 0 and stats[:, 7].tolist() == [1.0, 0.0, 1.0]
    assert torch.equal(loss[[0, 2]], want[0][[0, 2]]) and torch.equal(grad[[0, 2]], want[1][[0, 2]])
    assert torch.equal(stats[[0, 2]], want[2][[0, 2]])
    depth, _, mask = case
    open_ = ((mask[1] != 0) & (depth[1] >= NEAR) & (depth[1] <= FAR)).to(DEV)
    assert not torch.isfinite(grad[1][open_]).any() and not grad[1][~open_].any()
    assert int(open_.sum()) == (0 if kind == "empty_mask" else int(mask[1].sum()))
    ref = _run(depth_correlation_loss_torch, case, torch.float64, "cpu", ones, "none")
    assert torch.isnan(ref[0][1]) and torch.equal(torch.isfinite(ref[1]), torch.isfinite(grad).cpu())
    # skip_degenerate: loss 0, an all-zero gradient plane, valid = 0
    loss, grad, stats = _run(depth_correlation_loss, case, torch.float32, DEV, ones, "none", return_stats=True,
                             skip_degenerate=True)
    torch.cuda.synchronize()
    assert loss[1] == 0 and not grad[1].any() and stats[1, 7] == 0
    assert torch.equal(loss[[0, 2]], want[0][[0, 2]]) and torch.equal(grad[[0, 2]], want[1][[0, 2]])
    total = _run(depth_correlation_loss, case, torch.float32, DEV, skip_degenerate=True)[0]
    assert torch.isfinite(total) and abs(total.item() - want[0][[0, 2]].sum().item()) <= 1e-6


def test_upstream_gradient_is_read_per_camera_on_the_device():
    """reduction="none" with upstream [0.25, -3.0]; reduction="sum" scaled by 0.001 / 27."""
    got = _check("two_cams", upstream=(0.25, -3.0), reduction="none")
    assert got[0].shape == (2,)
    _check("two_cams", scale=0.001 / 27.0)


def test_layouts_agree_bit_for_bit():
    base = _run(depth_correlation_loss, _case("two_cams"), torch.float32, DEV, (0.5, 2.0), "none")
    four = _run(depth_correlation_loss, _case("two_cams"), torch.float32, DEV, (0.5, 2.0), "none", layout="B1HW")
    assert torch.equal(base[0], four[0]) and torch.equal(base[1], four[1])
    depth, target, mask = _case("two_cams")
    one = _run(depth_correlation_loss, (depth[:1], target[:1], mask[0]), torch.float32, DEV, 0.5, "none", layout="HW")
    torch.cuda.synchronize()
    assert one[0].dim() == 0 and one[0] == base[0][0] and torch.equal(one[1][0], base[1][0])


def test_mask_dtypes_give_identical_bits():
    depth, target, mask = _case("two_cams")
    runs = [_run(depth_correlation_loss, (depth, target, m), torch.float32, DEV, (1.0, -2.0), "none")
            for m in (mask, mask.bool(), mask.float() * 0.25, mask.to(torch.int32) * -7)]
    torch.cuda.synchronize()
    for r in runs[1:]:
        assert torch.equal(r[0], runs[0][0]) and torch.equal(r[1], runs[0][1])


def test_two_runs_are_bit_identical():
    for name in ("shared_mask", "large"):
        a = _run(depth_correlation_loss, _case(name), torch.float32, DEV, return_stats=True)
        b = _run(depth_correlation_loss, _case(name), torch.float32, DEV, return_stats=True)
        torch.cuda.synchronize()
        for x, y in zip(a, b):
            assert torch.equal(x, y)


def _settings(inp):
    return GaussianRasterizationSettings(
        image_height=inp["image_height"], image_width=inp["image_width"], tanfovx=inp["tan_fovx"],
        tanfovy=inp["tan_fovy"], c_x=inp["c_x"], c_y=inp["c_y"], bg=torch.zeros(3, device=DEV),
        viewmatrix=inp["viewmatrix"].to(DEV), projmatrix=inp["projmatrix"].to(DEV), sh_degree=0,
        campos=inp["campos"].to(DEV))


def test_autograd_hand_over_from_the_batch_render():
    """A 2-camera GaussianRasterizerBatch render whose depth plane goes through
    depth_correlation_loss and through depth_correlation_loss_torch on the GPU: the Gaussian
    parameters' gradients agree within the render backward's own bound."""
    inps = [H.scene(P=600, W=64, H=64, cam_index=c) for c in (0, 1)]
    ras = GaussianRasterizerBatch([_settings(i) for i in inps])
    names = ("means3D", "opacity", "scales", "rotations")

    def render(p):
        _im, _radius, depth = ras(means3D=p["means3D"], means2D=torch.zeros(600, 3, device=DEV),
                                  opacities=p["opacity"], colors_precomp=inps[0]["colors"].to(DEV),
                                  scales=p["scales"], rotations=p["rotations"])
        return depth

    with torch.no_grad():
        d0 = render({k: inps[0][k].to(DEV) for k in names})
    assert d0.shape == (2, 1, 64, 64)
    gen = torch.Generator().manual_seed(9)
    covered = d0[:, 0] > 0.2  # a prior exists where the scene is
    mask = covered & (torch.rand(2, 64, 64, generator=gen) < 0.8).to(DEV)
    assert int(mask[0].sum()) > 50 and int(mask[1].sum()) > 50
    prior = (1.0 / (1.3 * d0.clamp_min(0.2)) + 0.05 * torch.randn(2, 1, 64, 64, generator=gen).to(DEV)).contiguous()

    def grads(loss_fn):
        p = {k: inps[0][k].to(DEV).requires_grad_(True) for k in names}
        loss = loss_fn(render(p))
        loss.backward()
        return loss.detach(), [p[k].grad for k in names]

    fused = grads(lambda d: depth_correlation_loss(d, prior, mask=mask))
    plain = grads(lambda d: depth_correlation_loss_torch(d, prior, mask=mask))
    torch.cuda.synchronize()
    assert abs(fused[0].item() - plain[0].item()) <= LOSS_TOL * max(1.0, abs(plain[0].item()))
    for k, a, b in zip(names, fused[1], plain[1]):
        print(f"hand-over {k}: rel L2 {_rel(a, b):.3e}")
        assert float(b.abs().sum()) > 0, k
        assert _rel(a, b) <= GRAD_TOL, (k, _rel(a, b))


def test_driver_step_with_the_depth_loss():
    """One TimestepDriver step over batch_renderer(..., with_depth=True) with a depth loss: the
    step's loss is image_loss / n_cams + depth_loss / n_cams of the same render."""
    inps = [H.scene(P=600, W=64, H=64, cam_index=c) for c in (0, 1)]
    settings = [_settings(i) for i in inps]
    base = {"means3D": inps[0]["means3D"], "rgb_colors": inps[0]["colors"], "unnorm_rotations": inps[0]["rotations"],
            "logit_opacities": torch.logit(inps[0]["opacity"].clamp(1e-4, 1 - 1e-4)),
            "log_scales": torch.log(inps[0]["scales"])}
    leaf = lambda: {k: torch.nn.Parameter(v.to(DEV).clone()) for k, v in base.items()}  # noqa: E731
    gen = torch.Generator().manual_seed(10)
    tg = torch.rand(2, 3, 64, 64, generator=gen).to(DEV)
    prior = (0.1 + 0.3 * torch.rand(2, 1, 64, 64, generator=gen)).to(DEV)
    mask = (torch.rand(64, 64, generator=gen) < 0.8).to(DEV)
    cam_ids = torch.arange(2, device=DEV)

    def depth_term(depth, cams):
        assert depth.shape == (len(cams), 1, 64, 64) and list(cams) == [0, 1]
        return 0.001 * depth_correlation_loss(depth, prior[cam_ids[cams]], mask=mask)

    params = leaf()
    opt = torch.optim.SGD([{"params": [params[k]], "name": k, "lr": 0.0} for k in base], lr=0.0)
    drv = TimestepDriver(params, {}, opt, 2, batch_renderer(settings, with_depth=True), depth_loss=depth_term)
    loss = drv.step(tg)
    ref = leaf()
    im, _stats, depth = batch_renderer(settings, with_depth=True)(params2rendervar(ref), [0, 1])
    image_term, dterm = l1_image_loss(im, tg) / 2, depth_term(depth, [0, 1]) / 2
    torch.cuda.synchronize()
    assert np.isfinite(loss) and dterm.item() > 0
    np.testing.assert_allclose(loss, (image_term + dterm).item(), rtol=1e-6)
    assert abs(loss - image_term.item()) > 1e-7  # the depth term is in
    for k in base:
        assert params[k].grad is not None and torch.isfinite(params[k].grad).all(), k
