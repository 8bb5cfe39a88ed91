"""GPU tests of the quantile-trimmed losses (csrc/gs_robust_loss.hip).

Exact selection: plane_quantile on the device equals plane_quantile_torch (fp32 sort, fp64 lerp)
bit for bit on the float64 thresholds -- the order statistics are exact and the lerp is the same
fp64 expression -- and torch.quantile's fp32 result differs from it by at most
(v_hi - v_lo) n 2^-23 plus one fp32 ulp of v_hi, the rank error of its fp32 q (n - 1).

Loss parity on the decision-robust cases of tests/_robust_loss_cases.py: the kept set equals the
fp64 formulation's on every pixel, the kept count and sum kept m exactly, and the loss and every
gradient element lie within ENVELOPE = 4 x the fp32 twin's own deviation from the fp64
formulation (per element at least one fp32 ulp of the value), the bar of the depth-geometry and
motion-init tests.  With GS_PARITY_JSON set to a path, the measured deviations and their bounds
are written there at the end of the module (profiles/robust_loss/parity.json is such a record).

Shapes are the smallest that reach every branch: planes of 1, 2, 63, 64, 65 and 1961 values (one
lane, below / at / above a wave, two chunks with a ragged end), 300 x 300 (88 workgroups) and
133001 values (130 chunks on 128 workgroups: the strided walk).
"""
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

from dynamic3dgaussians_amd import (masked_trimmed_mse_loss, masked_trimmed_mse_loss_torch, plane_quantile,
                                    plane_quantile_torch, trimmed_mse_loss, trimmed_mse_loss_torch)
from dynamic3dgaussians_amd.robust_loss import _residual_torch
from tests import _robust_loss_cases as C

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ENVELOPE = 4.0
QS = (0.0, 1e-7, 0.5, 0.9, 1 - 1e-7, 1.0)
RECORD = {}


@pytest.fixture(scope="module", autouse=True)
def _write_parity_record():
    yield
    path = os.environ.get("GS_PARITY_JSON")
    if path and RECORD:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            json.dump({"envelope": ENVELOPE, "cases": RECORD}, fh, indent=1, sort_keys=True)


def _ulp32(v: torch.Tensor) -> torch.Tensor:
    return torch.from_numpy(np.asarray(np.spacing(v.abs().float().cpu().numpy()))).double()


def _check(name, got, ref64, twin32):
    """got (device, fp32) within ENVELOPE x max|twin32 - ref64| of ref64, per element at least one
    fp32 ulp of the value."""
    got, ref64, twin32 = got.detach().cpu().double(), ref64.detach().cpu().double(), twin32.detach().cpu().double()
    assert got.shape == ref64.shape, (got.shape, ref64.shape)
    own = (twin32 - ref64).abs().max().item()
    err = (got - ref64).abs()
    bound = torch.maximum(torch.full_like(err, ENVELOPE * own), _ulp32(ref64))
    RECORD[name] = {"hip_deviation": err.max().item(), "fp32_formulation_deviation": own,
                    "ratio": err.max().item() / own if own > 0 else 0.0}
    print(f"{name}: hip {err.max().item():.3e} fp32 formulation {own:.3e}")
    assert torch.all(err <= bound), RECORD[name]


def _same_bits(a, b):
    """Equal float64 values, NaN where the other has NaN."""
    a, b = a.cpu(), b.cpu()
    return a.dtype == b.dtype == torch.float64 and a.shape == b.shape and \
        torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a[~torch.isnan(a)], b[~torch.isnan(b)])


# ---- 1. exact selection

def _three_planes(n, seed):
    """Three distributions: u^4 (dense near 0), log-normal over many decades, exponential."""
    gen = torch.Generator().manual_seed(seed)
    return torch.stack([torch.rand(n, generator=gen) ** 4, torch.exp(4.0 * torch.randn(n, generator=gen)),
                        -torch.log(1 - torch.rand(n, generator=gen))]).float()


def _check_selection(x, qs=QS, against_torch=True):
    xd = x.to(DEV).contiguous()
    n = x.shape[-1]
    for q in qs:
        want = plane_quantile_torch(x, q)
        got = plane_quantile(xd, q)
        assert _same_bits(got, want), (n, q, got.cpu().tolist(), want.tolist())
        if not against_torch:
            continue
        theirs = torch.quantile(xd, q, dim=-1).cpu().double()
        v = torch.sort(x, dim=-1).values.double()
        lo = math.floor(q * (n - 1))
        hi = min(lo + 1, n - 1)
        bound = (v[..., hi] - v[..., lo]) * n * 2.0 ** -23 + _ulp32(v[..., hi])
        assert torch.all((theirs - want).abs() <= bound), (n, q, (theirs - want).abs().max().item())


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1961])
def test_selection_is_exact_small_planes(n):
    x = _three_planes(n, 100 + n)
    _check_selection(x)
    assert _same_bits(plane_quantile(x[1].to(DEV).contiguous(), 0.9), plane_quantile_torch(x[1], 0.9))  # one [N] plane


@pytest.mark.parametrize("n", [300 * 300, 133001])
def test_selection_is_exact_across_workgroups(n):
    _check_selection(_three_planes(n, n)[: 3 if n == 300 * 300 else 2])


def test_selection_with_shared_upper_bits():
    """Plane 0: all values agree in the top 21 bits and differ in the low 10 only; plane 1: they
    agree in the top 11 bits; plane 2: two level-1 bins, the rank's neighbours across the edge."""
    gen = torch.Generator().manual_seed(7)
    n = 1500
    low10 = torch.randint(0, 1024, (n,), generator=gen, dtype=torch.int32)
    low20 = torch.randint(0, 1 << 20, (n,), generator=gen, dtype=torch.int32)
    edge = torch.where(torch.arange(n) < n // 2, 0x3F7FFFFF - low10, 0x3F800000 + low10).int()
    x = torch.stack([0x3F800000 + low10, 0x3F800000 + low20, edge]).int().view(torch.float32)
    assert (x[0] >= 1).all() and (x[0] < 1.0002).all() and (x[1] < 1.13).all()
    _check_selection(x)
    _check_selection(x, qs=(0.4993, 0.4997, 0.5003))  # plane 2: lo and hi on either side of 1.0


def test_selection_inside_a_run_of_ties():
    """60 % exact zeros: the rank inside the run, on its last element (v_hi the smallest value above
    it) and on its first non-zero."""
    gen = torch.Generator().manual_seed(8)
    n = 1000
    x = torch.rand(3, n, generator=gen)
    x[:, torch.randperm(n, generator=gen)[:600]] = 0.0
    assert int((x[0] == 0).sum()) == 600
    qs = (0.3, 598.5 / 999, 599.5 / 999, 600.5 / 999, 0.0, 1.0)
    assert [math.floor(q * 999) for q in qs[:4]] == [299, 598, 599, 600]
    _check_selection(x, qs=qs)
    assert plane_quantile(x.to(DEV), qs[1])[0].item() == 0.0 and plane_quantile(x.to(DEV), qs[2])[0].item() > 0.0
    big = torch.zeros(2, 70000)  # ties across workgroups, every lane of a wave on one bin
    big[:, ::5] = torch.rand(2, 14000, generator=gen)
    _check_selection(big, qs=(0.5, 0.8, 0.80001, 0.9))


def test_selection_over_the_whole_range_and_nan():
    """1e-30 .. 1e30 with denormals and one +inf are ordinary values; one NaN makes its own plane's
    threshold NaN and leaves the others alone."""
    gen = torch.Generator().manual_seed(9)
    n = 777
    x = (10.0 ** (60.0 * torch.rand(3, n, generator=gen) - 30.0)).float()
    x[:, :5] = torch.tensor([1e-45, 3e-42, 1e-39, 0.0, 1.1754944e-38])
    x[:, 5] = float("inf")
    _check_selection(x, against_torch=False)
    # rank n - 1.5: between the largest finite value and +inf; at q = 1 the definition's lerp is
    # inf + 0 * (inf - inf) = NaN, on the device as in the twin (checked above)
    assert plane_quantile(x.to(DEV), (n - 1.5) / (n - 1))[0].item() == float("inf")
    assert torch.isnan(plane_quantile(x.to(DEV), 1.0)).all()
    y = x.clone()
    y[1, 400] = float("nan")
    for q in QS:
        got = plane_quantile(y.to(DEV), q).cpu()
        assert torch.isnan(got[1]) and _same_bits(got[[0, 2]], plane_quantile_torch(x[[0, 2]], q)), q
    z = x.clone()
    z[2, 3] = -0.0  # a negative zero is a zero
    assert _same_bits(plane_quantile(z.to(DEV), 0.001), plane_quantile_torch(x, 0.001))


# ---- 2. loss parity on decision-robust cases

# (mask, quantile_over, normalize)
ALL_CONFIGS = [(m, o, n) for m in ("none", "hw", "b") for o in ("all", "masked") for n in (False, True)
               if not (m == "none" and o == "masked")]
SOME_CONFIGS = [("none", "all", False), ("hw", "all", True), ("b", "masked", False), ("hw", "masked", True),
                ("b", "all", True)]
PARITY = [(s, c) for s in C.SHAPES for c in (ALL_CONFIGS if s == (3, 37, 53) else SOME_CONFIGS)]
UP = torch.tensor([0.7, -1.3, 2.1])  # distinct, one negative


def _mask_of(case, which):
    return {"none": None, "hw": case.mask_hw, "b": case.mask_b}[which]


@functools.lru_cache(maxsize=None)
def _device_case(shape):
    case = C.image_case(shape)
    return case, case.pred.to(DEV), case.gt.to(DEV)


def _run(fn, pred, gt, mask, dtype, **kw):
    p = pred.to(dtype).requires_grad_(True)
    vec, stats = fn(p, gt.to(dtype), mask=mask, reduction="none", return_stats=True, **kw)
    (grad,) = torch.autograd.grad((vec * UP.to(vec)).sum(), p)
    return vec.detach(), stats, grad


@pytest.mark.parametrize("shape,config", PARITY, ids=lambda v: "-".join(str(x) for x in v))
def test_masked_loss_parity(shape, config):
    which, over, normalize = config
    case, pred, gt = _device_case(shape)
    mask = None if which == "none" else _mask_of(case, which).to(DEV)
    kw = dict(quantile=C.Q, normalize=normalize, quantile_over=over)
    ref = _run(masked_trimmed_mse_loss_torch, pred, gt, mask, torch.float64, **kw)
    f32 = _run(masked_trimmed_mse_loss_torch, pred, gt, mask, torch.float32, **kw)
    hip = _run(masked_trimmed_mse_loss, pred, gt, mask, torch.float32, **kw)
    name = f"{case.name}.{which}.{over}.n{int(normalize)}"
    assert hip[1].dtype == torch.float64 and hip[1].shape == (C.B, 4)
    # the kept count and sum kept m, exactly; no NaN
    assert torch.equal(hip[1][:, 1:], ref[1][:, 1:]), (hip[1].cpu(), ref[1].cpu())
    # the kept set on every pixel: the kernel's threshold on the fp32 residual (the twin's rounds as
    # the kernel's) against the fp64 formulation's
    e32 = _residual_torch(pred, gt, 1)
    e64 = _residual_torch(pred.double(), gt.double(), 1)
    part = torch.ones_like(e32, dtype=torch.bool) if over == "all" else (mask != 0).expand_as(e32)
    kept_hip = part & (e32.double() < hip[1][:, 0].reshape(-1, 1, 1))
    kept_ref = part & (e64 < ref[1][:, 0].reshape(-1, 1, 1))
    assert torch.equal(kept_hip, kept_ref)
    assert torch.equal(kept_hip.sum((1, 2)).double(), hip[1][:, 1])
    assert _same_bits(hip[1][:, 0], f32[1][:, 0])  # and the threshold is the fp32 twin's, bit for bit
    assert torch.equal(hip[2] == 0, ref[2] == 0)  # kept and masked, from the gradient
    _check(name + ".loss", hip[0], ref[0], f32[0])
    _check(name + ".grad", hip[2], ref[2], f32[2])


def test_rows_loss_parity():
    case = C.rows_case()
    pred, gt = case.pred.to(DEV), case.gt.to(DEV)

    def run(fn, dtype):
        p = pred.to(dtype).requires_grad_(True)
        loss = fn(p, gt.to(dtype), C.Q)
        (grad,) = torch.autograd.grad(loss * -1.3, p)
        return loss.detach(), grad
    ref, f32, hip = run(trimmed_mse_loss_torch, torch.float64), run(trimmed_mse_loss_torch, torch.float32), \
        run(trimmed_mse_loss, torch.float32)
    assert hip[0].dim() == 0 and hip[1].shape == pred.shape
    assert torch.equal(hip[1] == 0, ref[1] == 0)  # the kept rows
    assert int((ref[1].abs().sum(-1) != 0).sum()) == math.floor(C.Q * 287) + 1
    _check(case.name + ".loss", hip[0], ref[0], f32[0])
    _check(case.name + ".grad", hip[1], ref[1], f32[1])
    # q = 1: no special case, exactly the largest row is dropped
    p = pred.clone().requires_grad_(True)
    (g1,) = torch.autograd.grad(trimmed_mse_loss(p, gt, 1.0), p)
    e = _residual_torch(pred, gt, -1)
    assert torch.equal(g1.abs().sum(-1) == 0, e == e.max())


# ---- 3. further checks

def _small():
    case, pred, gt = _device_case((3, 37, 53))
    return pred, gt, case.mask_b.to(DEV)


def test_two_runs_are_bit_identical():
    for shape in ((3, 37, 53), (3, 300, 300)):
        case, pred, gt = _device_case(shape)
        mask = case.mask_b.to(DEV)
        runs = [_run(masked_trimmed_mse_loss, pred, gt, mask, torch.float32, quantile=C.Q, normalize=True)
                for _ in range(2)]
        for a, b in zip(*runs):
            assert torch.equal(a, b)


def test_sum_is_the_sum_of_none_and_a_batch_is_its_cameras():
    pred, gt, mask = _small()
    for kw in (dict(quantile=C.Q), dict(quantile=0.5, normalize=True, quantile_over="masked"), dict(quantile=1.0)):
        vec, stats, grad = _run(masked_trimmed_mse_loss, pred, gt, mask, torch.float32, **kw)
        total = masked_trimmed_mse_loss(pred, gt, mask=mask, **kw)
        assert total.dim() == 0 and torch.equal(total, vec.sum())
        for b in range(C.B):
            p = pred[b].clone().requires_grad_(True)
            one, st = masked_trimmed_mse_loss(p, gt[b], mask=mask[b], reduction="none", return_stats=True, **kw)
            (g,) = torch.autograd.grad(one * UP[b].item(), p)
            assert one.dim() == 0 and torch.equal(one, vec[b]) and _same_bits(st[0], stats[b])
            assert torch.equal(g, grad[b])


@pytest.mark.parametrize("shape", [(3, 37, 53), (32, 300, 300)], ids=str)
def test_quantile_one_is_the_plain_masked_mean(shape):
    case, pred, gt = _device_case(shape)
    mask = case.mask_hw.to(DEV)
    for normalize in (False, True):
        kw = dict(quantile=1.0, normalize=normalize)
        hip = _run(masked_trimmed_mse_loss, pred, gt, mask, torch.float32, **kw)
        e64 = ((pred.double() - gt.double()) ** 2).mean(1) * mask
        H, W = mask.shape
        want = e64.sum((1, 2)) / (W * mask.sum() + 1e-8) if normalize else e64.mean((1, 2))
        f32 = _run(masked_trimmed_mse_loss_torch, pred, gt, mask, torch.float32, **kw)
        ref = _run(masked_trimmed_mse_loss_torch, pred, gt, mask, torch.float64, **kw)
        torch.testing.assert_close(ref[0], want, rtol=1e-12, atol=0)
        assert hip[1][:, 0].tolist() == [float("inf")] * C.B and hip[1][:, 1].tolist() == [float(H * W)] * C.B
        _check(f"{case.name}.q1.n{int(normalize)}.loss", hip[0], want, f32[0])
        _check(f"{case.name}.q1.n{int(normalize)}.grad", hip[2], ref[2], f32[2])


def test_degenerate_cameras():
    pred, gt, mask = _small()
    healthy = masked_trimmed_mse_loss(pred, gt, mask=mask, quantile=C.Q, reduction="none")
    # q = 0 keeps nothing: NaN, or 0 with a zero gradient under skip_degenerate
    vec, stats = masked_trimmed_mse_loss(pred, gt, mask=mask, quantile=0.0, reduction="none", return_stats=True)
    assert torch.isnan(vec).all() and not stats[:, 1:].any()
    p = pred.clone().requires_grad_(True)
    vec = masked_trimmed_mse_loss(p, gt, mask=mask, quantile=0.0, reduction="none", skip_degenerate=True)
    assert not vec.any() and not torch.autograd.grad(vec.sum(), p)[0].any()
    # a NaN pixel in camera 1: its threshold is NaN, nothing is kept; cameras 0 and 2 are unaffected
    bad = pred.clone()
    bad[1, 2, 5, 7] = float("nan")
    p = bad.clone().requires_grad_(True)
    vec, stats = masked_trimmed_mse_loss(p, gt, mask=mask, quantile=C.Q, reduction="none", return_stats=True)
    assert torch.isnan(vec[1]) and torch.equal(vec[[0, 2]], healthy[[0, 2]])
    assert torch.isnan(stats[1, 0]) and stats[1, 1:].tolist() == [0.0, 0.0, 1.0] and stats[0, 3] == 0
    (g,) = torch.autograd.grad(vec[[0, 2]].sum(), p)
    assert not g[1].any() and g[0].abs().sum() > 0
    twin = masked_trimmed_mse_loss_torch(bad, gt, mask=mask, quantile=C.Q, reduction="none")
    assert torch.isnan(twin[1])
    # an all-zero mask with normalize: 0 through the 1e-8; one camera's mask only
    m = mask.clone()
    m[1] = 0
    for over in ("all", "masked"):
        vec = masked_trimmed_mse_loss(pred, gt, mask=m, quantile=C.Q, normalize=True, quantile_over=over,
                                      reduction="none")
        want = masked_trimmed_mse_loss(pred, gt, mask=mask, quantile=C.Q, normalize=True, quantile_over=over,
                                       reduction="none")
        assert vec[1].item() == 0.0 and torch.equal(vec[[0, 2]], want[[0, 2]])
    vec = masked_trimmed_mse_loss(pred, gt, mask=torch.zeros_like(mask[0]), quantile=C.Q, normalize=True,
                                  reduction="none")
    assert vec.tolist() == [0.0, 0.0, 0.0]
    # over the masked pixels with an empty mask there is no quantile: NaN without normalize
    vec = masked_trimmed_mse_loss(pred, gt, mask=m, quantile=C.Q, quantile_over="masked", reduction="none")
    assert torch.isnan(vec[1]) and torch.isfinite(vec[[0, 2]]).all()
