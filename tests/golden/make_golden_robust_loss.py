#!/usr/bin/env python3
"""Generate tests/golden/robust_loss.npz from the REFERENCE's own functions (run where the
reference checkout exists; the fixture -- data only -- is committed, the reference never
travels).

The two functions, helpers.py:16-38 (masked_mse_loss) and ideaII.py:378-384
(trimmed_mse_loss), are read out of the checkout at run time, after checking that the slices
begin and end where expected, and executed in a namespace that supplies torch, F and a `print`
that does nothing (masked_mse_loss prints shapes).  Nothing of the reference's text is stored
here.

As written, masked_mse_loss raises an IndexError for quantile < 1: the kept mask loses its
leading axis (a `.squeeze(0)` after the comparison) while the tensor it indexes keeps it.  For
those cases this script drops that one call from the text in memory, which gives the kept mask
the shape the quantile >= 1 branch already has; the cases with quantile = 1 run the text as it
stands.

Everything runs in fp64 on the CPU, so the threshold is torch.quantile's fp64 one; the inputs
are stored as the fp32 values they were drawn as.  Recorded per case: pred, gt, (mask), the
loss and the autograd gradient with respect to pred.

Cases (all seeded):
  mse.<H>x<W>.n<0|1>.q<q>   C = 3, a mask with about 30 % zeros, normalize both ways,
                            q in {1.0, 0.9, 0.5}; 37 x 53 (n = 1961: q (n - 1) is an integer
                            for 0.9 and 0.5) and 6 x 7 (n = 42: it is not)
  trim.<name>.q<q>          the flow layout [N, 2, H, W], the mean over the last axis:
                            [3, 2, 6, 8] at q = 0.9 (36 rows, rank 31.5), q = 0.5 and q = 1.0
                            (an integer rank; the largest row is dropped)

Usage: python tests/golden/make_golden_robust_loss.py --reference <reference checkout>
"""
from __future__ import annotations

import argparse
import os

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
MSE_FIRST, MSE_LAST = 16, 38  # helpers.py, 1-based, inclusive
TRIM_FIRST, TRIM_LAST = 378, 384  # ideaII.py
SIZES = ((37, 53), (6, 7))
QUANTILES = (1.0, 0.9, 0.5)
TRIM_SHAPE = (3, 2, 6, 8)
TRIM_QUANTILES = (0.9, 0.5, 1.0)


def mse_name(size, normalize, q):
    return f"mse.{size[0]}x{size[1]}.n{int(normalize)}.q{q}"


def trim_name(q):
    return f"trim.flow.q{q}"


def mse_inputs(size):
    gen = torch.Generator().manual_seed(1000 + size[0])
    pred = torch.rand(3, *size, generator=gen).float()
    gt = (pred + 0.1 * torch.randn(3, *size, generator=gen) * torch.rand(1, *size, generator=gen) ** 3).float()
    mask = (torch.rand(*size, generator=gen) < 0.7).to(torch.uint8)
    return pred, gt, mask


def trim_inputs():
    gen = torch.Generator().manual_seed(2000)
    pred = torch.randn(*TRIM_SHAPE, generator=gen).float()
    gt = (pred + 0.2 * torch.randn(*TRIM_SHAPE, generator=gen)).float()
    return pred, gt


def _slice(path, first, last):
    with open(path) as fh:
        return fh.read().splitlines()[first - 1:last]


def reference_functions(reference):
    mse = _slice(os.path.join(reference, "helpers.py"), MSE_FIRST, MSE_LAST)
    assert mse[0].startswith("def masked_mse_loss(pred, gt, mask=None, normalize=False, quantile"), mse[0]
    assert mse[-1].strip().startswith("return torch.mean((sum_loss * mask)[quantile_mask])"), mse[-1]
    trim = _slice(os.path.join(reference, "ideaII.py"), TRIM_FIRST, TRIM_LAST)
    assert trim[0].startswith("def trimmed_mse_loss(pred, gt, quantile=0.9):"), trim[0]
    assert trim[-1].strip() == "return trimmed_loss", trim[-1]
    text = "\n".join(mse)
    cmp_line = [s for s in mse if "torch.quantile(sum_loss, quantile)" in s]
    assert len(cmp_line) == 1 and cmp_line[0].count(".squeeze(0)") == 1, cmp_line
    indexable = text.replace(cmp_line[0], cmp_line[0].replace(".squeeze(0)", ""))

    def load(src, name, what):
        ns = {"torch": torch, "F": F, "print": lambda *a, **k: None}
        exec(compile(src, what, "exec"), ns)
        return ns[name]
    where = "helpers.py:%d-%d" % (MSE_FIRST, MSE_LAST)
    return (load(text, "masked_mse_loss", where), load(indexable, "masked_mse_loss", where),
            load("\n".join(trim), "trimmed_mse_loss", "ideaII.py:%d-%d" % (TRIM_FIRST, TRIM_LAST)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference (helpers.py, ideaII.py)")
    a = ap.parse_args()
    mse_as_written, mse_indexable, trim = reference_functions(a.reference)
    out = {}
    for size in SIZES:
        pred, gt, mask = mse_inputs(size)
        key = f"mse.{size[0]}x{size[1]}"
        out[f"{key}.pred"], out[f"{key}.gt"], out[f"{key}.mask"] = pred.numpy(), gt.numpy(), mask.numpy()
        for normalize in (False, True):
            for q in QUANTILES:
                p = pred.double().requires_grad_(True)
                fn = mse_as_written if q >= 1 else mse_indexable
                loss = fn(p, gt.double(), mask.double()[None], normalize, q)  # the mask as [1, H, W]
                (grad,) = torch.autograd.grad(loss, p)
                name = mse_name(size, normalize, q)
                out[f"{name}.loss"], out[f"{name}.grad_pred"] = loss.detach().numpy(), grad.numpy()
                print(f"{name}: rank {q * (size[0] * size[1] - 1)!r}  loss {loss.item():.12g}  |grad| {grad.norm():.6g}")
    pred, gt = trim_inputs()
    out["trim.flow.pred"], out["trim.flow.gt"] = pred.numpy(), gt.numpy()
    for q in TRIM_QUANTILES:
        p = pred.double().requires_grad_(True)
        loss = trim(p, gt.double(), q)
        (grad,) = torch.autograd.grad(loss, p)
        out[f"{trim_name(q)}.loss"], out[f"{trim_name(q)}.grad_pred"] = loss.detach().numpy(), grad.numpy()
        print(f"{trim_name(q)}: rank {q * (pred.numel() // pred.shape[-1] - 1)!r}  loss {loss.item():.12g}")
    path = os.path.join(HERE, "robust_loss.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
