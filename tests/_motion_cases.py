"""Shared builders of the motion-warp tests (tests/test_motion.py on the CPU,
tests/test_gpu_motion.py on the device) and of the fixture's generator
(tests/golden/make_golden_motion.py): seeded cases of one recipe, and the
conditioning margin every case must keep.

Recipe: a basis 6-vector is 0.6 * (1, 0, 0, 0, 1, 0) + 0.4 * (the first two
columns of a random rotation) + 0.05 * noise, so every blend with weights that
sum to about one stays well away from a zero vector and from parallel halves;
logits are 2 * randn; the given coefficients (mode 0) are the logits' softmax
times a per-Gaussian factor in [1, 1.5], so that they do not sum to one.
Every value is rounded to fp32 and returned in fp64: the fp32 kernels and the
fp64 oracle see the same numbers.

Margin (asserted by `margins_ok`): every blended |x1| and |y1 - (y1 . x) x| is
at least 0.2 and the sine of the angle between the blended x1 and y1 at least
0.25: off the clamp of the normalisation and off the Gram-Schmidt singularity.
"""
from __future__ import annotations

import os

import numpy as np
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "motion_bases.npz")
FIXTURE_CASES = {"c200": (200, 7, 12, 3), "c64": (64, 1, 9, 2)}  # name: (G, K, T, seed)
FIXTURE_TS = tuple(range(9))  # what the reference's compute_transforms uses whatever it is given
MODES = {"given": False, "softmax": True}  # name: softmax
MIN_NORM, MIN_SINE = 0.2, 0.25
GRADS = ("means", "coefs", "rots", "transls")


def _round32(t: torch.Tensor) -> torch.Tensor:
    return t.float().double()


def make_case(G: int, K: int, T: int, seed: int) -> dict:
    """means (G, 3), logits and coefs (G, K), rots (K, T, 6), transls (K, T, 3): fp64 tensors of
    fp32-representable values."""
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)  # noqa: E731
    q, r = torch.linalg.qr(rn(K, T, 3, 3))
    q = q * torch.sign(torch.diagonal(r, dim1=-2, dim2=-1))[..., None, :]  # a fixed sign convention
    ident = torch.tensor([1.0, 0, 0, 0, 1.0, 0], dtype=torch.float64)
    rots = 0.6 * ident + 0.4 * torch.cat([q[..., :, 0], q[..., :, 1]], dim=-1) + 0.05 * rn(K, T, 6)
    transls = 0.5 * rn(K, T, 3)
    logits = 2.0 * rn(G, K)
    scale = 1.0 + 0.5 * torch.rand(G, 1, generator=gen, dtype=torch.float64)
    coefs = torch.softmax(_round32(logits), dim=-1) * scale
    means = rn(G, 3)
    return {"means": _round32(means), "logits": _round32(logits), "coefs": _round32(coefs),
            "rots": _round32(rots), "transls": _round32(transls)}


def weights(G: int, B: int, seed: int, transforms: bool = False) -> torch.Tensor:
    """The fixed upstream weights of sum(w * output)."""
    gen = torch.Generator().manual_seed(1000 + seed)
    shape = (G, B, 3, 4) if transforms else (G, B, 3)
    return _round32(torch.randn(*shape, generator=gen, dtype=torch.float64))


def margins(case: dict, ts, softmax: bool):
    """(min |x1|, min |y1 - (y1 . x) x|, min sine between x1 and y1) over every (g, b)."""
    c = torch.softmax(case["logits"], -1) if softmax else case["coefs"]
    r = torch.einsum("pk,kni->pni", c.double(), case["rots"].double()[:, list(ts)])
    x1, y1 = r[..., :3], r[..., 3:]
    nx = x1.norm(dim=-1)
    x = x1 / nx[..., None]
    u = y1 - (y1 * x).sum(-1, keepdim=True) * x
    nu = u.norm(dim=-1)
    sine = nu / y1.norm(dim=-1)
    if r.numel() == 0:
        return 1.0, 1.0, 1.0
    return float(nx.min()), float(nu.min()), float(sine.min())


def margins_ok(case: dict, ts, softmax: bool) -> bool:
    a, b, s = margins(case, ts, softmax)
    return a >= MIN_NORM and b >= MIN_NORM and s >= MIN_SINE


def conditioned_case(G: int, K: int, T: int, ts, seed: int):
    """(case, seed used): the first of seed, seed + 1, ... whose case keeps the margin at the frames
    ts in both coefficient modes.  Deterministic; the recipe fails the margin at roughly half of
    the seeds at K = 7, so the search is short."""
    for s in range(seed, seed + 64):
        case = make_case(G, K, T, s)
        if margins_ok(case, ts, False) and margins_ok(case, ts, True):
            return case, s
    raise AssertionError(f"no seed in [{seed}, {seed + 64}) keeps the margin at G {G}, K {K}, T {T}")


def rel_l2(a, b) -> float:
    a = np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a, np.float64)
    b = np.asarray(b.detach().cpu() if isinstance(b, torch.Tensor) else b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))
