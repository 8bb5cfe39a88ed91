"""Decision-robust inputs for the quantile-trimmed losses' parity tests
(tests/test_gpu_robust_loss.py; checked on the CPU by tests/test_robust_loss.py).

A case is decision-robust when the kept set cannot hang on fp32 rounding: in the fp64
formulation (the fp32 inputs cast to fp64), for every threshold the tests use -- the quantile
over all pixels of a camera, over the pixels of the shared [H, W] mask and over those of the
camera's own [B, H, W] mask -- apart from the elements equal to v_lo or v_hi no residual lies
within

    margin = 4 (R + 2) 2^-24 thr

of thr, and v_hi - v_lo is either 0 or larger than that margin.  (R + 2) 2^-24 bounds the
relative rounding error of a residual of R terms in fp32: R products, R - 1 additions, one
division, half an ulp each; the factor 4 is headroom.)  The builder ASSERTS this for the pinned
seeds; it filters nothing, and no element is excluded from any comparison.

The residual scale is log-normal per pixel (three e-folds), so the residuals span many decades
-- every level of the radix select sees populated and empty bins -- and are sparse around the
0.9 quantile, which is what makes a seed search for a 300 x 300 plane short.  `python -m
tests._robust_loss_cases` runs that search and prints the seeds to pin.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from functools import lru_cache

import torch

Q = 0.9
B = 3
SHAPES = ((1, 37, 53), (3, 37, 53), (32, 37, 53), (1, 300, 300), (3, 300, 300), (32, 300, 300))
ROWS_SHAPE = (4, 2, 36, 64)
# pinned by the search below
SEEDS = {(1, 37, 53): 0, (3, 37, 53): 0, (32, 37, 53): 0, (1, 300, 300): 0, (3, 300, 300): 0, (32, 300, 300): 2,
         ROWS_SHAPE: 0}


@dataclass(frozen=True)
class Case:
    name: str
    pred: torch.Tensor      # fp32
    gt: torch.Tensor        # fp32
    mask_hw: torch.Tensor   # uint8 [H, W], about 80 % ones (None for the rows case)
    mask_b: torch.Tensor    # uint8 [B, H, W]


def margin(R: int, thr: float) -> float:
    return 4.0 * (R + 2) * 2.0 ** -24 * thr


def check_robust(e64: torch.Tensor, q: float, R: int, what: str):
    """Assert the module's condition for the 1-D fp64 residuals e64; returns (thr, kept count)."""
    n = e64.numel()
    assert n > 1, what
    v = torch.sort(e64).values
    r = q * (n - 1)
    lo = math.floor(r)
    hi = min(lo + 1, n - 1)
    v_lo, v_hi = v[lo].item(), v[hi].item()
    thr = v_lo + (r - lo) * (v_hi - v_lo)
    m = margin(R, thr)
    assert v_hi == v_lo or v_hi - v_lo > m, f"{what}: v_hi - v_lo = {v_hi - v_lo:.3e} within the margin {m:.3e}"
    near = ((e64 - thr).abs() <= m) & (e64 != v_lo) & (e64 != v_hi)
    assert not near.any(), f"{what}: {int(near.sum())} residuals within {m:.3e} of thr = {thr:.6e}"
    return thr, int((e64 < thr).sum())


def _image_inputs(shape, seed):
    C, H, W = shape
    gen = torch.Generator().manual_seed(seed)
    pred = torch.rand(B, C, H, W, generator=gen)
    scale = 0.02 * torch.exp(1.5 * torch.randn(B, 1, H, W, generator=gen))
    gt = (pred + scale * torch.randn(B, C, H, W, generator=gen)).float()
    mask_hw = (torch.rand(H, W, generator=gen) < 0.8).to(torch.uint8)
    mask_b = (torch.rand(B, H, W, generator=gen) < 0.8).to(torch.uint8)
    return pred.float(), gt, mask_hw, mask_b


def _check_image(shape, pred, gt, mask_hw, mask_b):
    C = shape[0]
    e = ((pred.double() - gt.double()) ** 2).mean(1)  # [B, H, W]
    for b in range(B):
        check_robust(e[b].flatten(), Q, C, f"{shape} camera {b}, all pixels")
        check_robust(e[b][mask_hw != 0], Q, C, f"{shape} camera {b}, [H, W] mask")
        check_robust(e[b][mask_b[b] != 0], Q, C, f"{shape} camera {b}, [B, H, W] mask")


@lru_cache(maxsize=None)
def image_case(shape) -> Case:
    pred, gt, mask_hw, mask_b = _image_inputs(shape, SEEDS[shape])
    _check_image(shape, pred, gt, mask_hw, mask_b)
    return Case("c%d_%dx%d" % shape, pred, gt, mask_hw, mask_b)


def image_cases():
    return [image_case(s) for s in SHAPES]


def _rows_inputs(seed):
    gen = torch.Generator().manual_seed(seed)
    pred = torch.randn(*ROWS_SHAPE, generator=gen).float()
    scale = 0.05 * torch.exp(1.5 * torch.randn(*ROWS_SHAPE[:-1], 1, generator=gen))
    gt = (pred + scale * torch.randn(*ROWS_SHAPE, generator=gen)).float()
    return pred, gt


@lru_cache(maxsize=None)
def rows_case() -> Case:
    pred, gt = _rows_inputs(SEEDS[ROWS_SHAPE])
    e = ((pred.double() - gt.double()) ** 2).mean(-1).flatten()
    check_robust(e, Q, ROWS_SHAPE[-1], f"rows {ROWS_SHAPE}")
    return Case("rows_%dx%dx%dx%d" % ROWS_SHAPE, pred, gt, None, None)


def _search():
    for shape in SHAPES:
        for seed in range(10000):
            try:
                _check_image(shape, *_image_inputs(shape, seed))
            except AssertionError:
                continue
            print(f"{shape}: {seed},")
            break
    for seed in range(10000):
        pred, gt = _rows_inputs(seed)
        try:
            check_robust(((pred.double() - gt.double()) ** 2).mean(-1).flatten(), Q, ROWS_SHAPE[-1], "rows")
        except AssertionError:
            continue
        print(f"{ROWS_SHAPE}: {seed},")
        break


if __name__ == "__main__":
    _search()
