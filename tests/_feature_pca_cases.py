"""What tests/test_feature_pca.py and tests/test_gpu_feature_pca.py share: the shapes, the seeded
inputs, a numpy statement of the mathematics and the derived error bounds (u = 2^-24)."""
from __future__ import annotations

import functools

import numpy as np
import torch

U = 2.0 ** -24
SHAPES = [(1, 1, 1, 1), (2, 3, 5, 9), (1, 20, 9, 65), (1, 32, 37, 53), (2, 33, 12, 31), (1, 64, 37, 53),
          (1, 128, 12, 31), (3, 32, 72, 128), (1, 8, 288, 512)]
MASKS = ("none", "hw", "bhw")
SIGMA = (8.0, 6.0, 4.0, 2.0, 1.0)  # then 0.5, 0.5, ...


def shape_id(s):
    return "x".join(map(str, s))


@functools.lru_cache(maxsize=None)
def spectrum(B, C, H, W, seed=0):
    """x = Z diag(sigma) Q^T + mu, float32 [B, C, H, W]: sigma = (8, 6, 4, 2, 1, 0.5, ...), Q a random
    orthogonal matrix, |mu| = 4, so the shift matters and the top eigengaps are wide."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * C + H)
    Z = torch.randn(B * H * W, C, generator=g, dtype=torch.float64)
    sigma = torch.tensor((SIGMA + (0.5,) * C)[:C], dtype=torch.float64)
    Q = torch.linalg.qr(torch.randn(C, C, generator=g, dtype=torch.float64)).Q
    mu = torch.randn(C, generator=g, dtype=torch.float64)
    mu = 4.0 * mu / mu.norm()
    X = (Z * sigma) @ Q.T + mu
    return X.reshape(B, H, W, C).permute(0, 3, 1, 2).to(torch.float32).contiguous()


@functools.lru_cache(maxsize=None)
def mask_of(kind, B, H, W, seed=0):
    """None, [H, W] or [B, H, W] float32 with about 30 % zeros; pixel 0 of every image takes part."""
    if kind == "none":
        return None
    g = torch.Generator().manual_seed(seed + 31 * H + W)
    shape = (H, W) if kind == "hw" else (B, H, W)
    m = (torch.rand(shape, generator=g) >= 0.3).to(torch.float32)
    m[..., 0, 0] = 1.0
    return m


def ddof_of(shape):
    return 0 if shape[0] * shape[2] * shape[3] == 1 else 1


def k_of(shape):
    return min(shape[1], 3)


# ------------------------------------------------------------------ numpy, fp64

def np_xhat(x, normalize):
    if not normalize:
        return x
    return x / np.maximum(np.sqrt((x * x).sum(axis=1, keepdims=True)), 1e-12)


def np_fit_set(B, H, W, mask, stride):
    take = np.broadcast_to((np.arange(H * W) % stride == 0)[None], (B, H * W))
    if mask is None:
        return take
    return take & (np.asarray(mask).reshape(-1, H * W) != 0)


def np_samples(x, mask, normalize, stride):
    B, C, H, W = x.shape
    rows = np_xhat(x, normalize).transpose(0, 2, 3, 1).reshape(B, H * W, C)
    return rows[np_fit_set(B, H, W, mask, stride)]


def np_sign_rule(vec_rows):
    idx = np.abs(vec_rows).argmax(axis=1)  # the first maximum
    s = np.where(vec_rows[np.arange(len(idx)), idx] < 0, -1.0, 1.0)
    return vec_rows * s[:, None]


def np_pca(x, mask, normalize, stride, ddof, k):
    """(mean, cov, eigenvalues descending, components [k, C]) of float64 x [B, C, H, W]."""
    X = np_samples(x, mask, normalize, stride)
    n = X.shape[0]
    mean = X.mean(axis=0)
    D = X - mean
    cov = D.T @ D / (n - ddof)
    lam, vec = np.linalg.eigh(cov)
    lam, rows = lam[::-1], vec[:, ::-1].T
    return mean, cov, lam, np_sign_rule(rows)[:k]


def np_project(x, comp, mean, mask, normalize):
    B, C, H, W = x.shape
    t = np.einsum("bchw,kc->bkhw", np_xhat(x, normalize) - mean[None, :, None, None], comp)
    if mask is not None:
        t = np.where((np.asarray(mask).reshape(-1, 1, H, W) != 0), t, 0.0)
    return t


def np_part(B, H, W, mask):
    """The pixels that take part in a transform, bool [B, H * W]."""
    return np_fit_set(B, H, W, mask, 1)


def np_range(t, mask):
    B, k, H, W = t.shape
    part = np_part(B, H, W, mask)
    flat = t.reshape(B, k, H * W)
    lo = np.stack([flat[b][:, part[b]].min(axis=1) for b in range(B)])
    hi = np.stack([flat[b][:, part[b]].max(axis=1) for b in range(B)])
    return lo, hi


def np_colour(t, lo, hi, mask, clamp=False):
    """v [B, 3, H, W] in fp64: (t - lo) / (hi - lo), 0 where hi == lo and off the mask."""
    B, k, H, W = t.shape
    lo, hi = np.broadcast_to(lo, (B, k))[:, :, None, None], np.broadcast_to(hi, (B, k))[:, :, None, None]
    span = hi - lo
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.where(span == 0, 0.0, (t.astype(np.float64) - lo) / np.where(span == 0, 1.0, span))
    if mask is not None:
        v = np.where(np.asarray(mask).reshape(-1, 1, H, W) != 0, v, 0.0)
    return np.clip(v, 0.0, 1.0) if clamp else v


def np_quantile(u, q):
    """robust_loss's threshold of the planes u [N, n]: exact order statistics, the lerp in fp64."""
    n = u.shape[1]
    r = q * (n - 1)
    lo = int(np.floor(r))
    hi = min(lo + 1, n - 1)
    s = np.sort(u, axis=1).astype(np.float64)
    return s[:, lo] + (r - lo) * (s[:, hi] - s[:, lo])


# ------------------------------------------------------------------ derived bounds

def moment_bounds(xh, xp, sel, n_acc, C, normalize):
    """Elementwise bounds on S and M of the device against the fp64 sums of the same x' (xh, xp
    float64 [B, HW, C]: x_hat and x' = x_hat - shift; sel bool [B, HW]).  A slab's fp32 accumulator
    adds at most n_acc terms ((n_acc - 1) u), each factor is one fp32 rounding of x_hat - shift (u
    each) and the three-piece split drops under u of a product: (n_acc + 4) u sum |x'_i x'_j|.
    Under normalize every factor carries x_hat's own error, (C + 6) u |x_hat| (C squares and
    C - 1 additions, the root, the maximum, the division)."""
    a, h = np.abs(xp[sel]), np.abs(xh[sel])
    bS = (n_acc + 4) * U * a.sum(axis=0)
    bM = (n_acc + 4) * U * (a.T @ a)
    if normalize:
        bS = bS + (C + 6) * U * h.sum(axis=0)
        cross = h.T @ a
        bM = bM + (C + 6) * U * (cross + cross.T)
    return bS, bM


def projection_bound(xh, comp, mean, normalize):
    """E [B, k, H, W]: u sum_c |V_jc| ((C + 6) |x_hat_c| + (C + 4) |x_hat_c - mean_c|), the first term
    under normalize only (x_hat's error; then one rounding of the difference, one of the product
    and C - 1 additions, with slack for second-order terms)."""
    C = xh.shape[1]
    d = np.abs(xh - mean[None, :, None, None])
    E = (C + 4) * np.einsum("bchw,kc->bkhw", d, np.abs(comp))
    if normalize:
        E = E + (C + 6) * np.einsum("bchw,kc->bkhw", np.abs(xh), np.abs(comp))
    return U * E


def colour_bound(E, lo, hi, shared):
    """Per image and component: (2 max E + u (hi - lo)) / (hi - lo); inf where hi == lo.  `shared`:
    one lo and hi per image over all components (the min / max range), so max E is over them all."""
    B, k = E.shape[:2]
    span = np.broadcast_to(hi, (B, k)) - np.broadcast_to(lo, (B, k))
    emax = E.reshape(B, k, -1).max(axis=2)
    if shared:
        emax = emax.max(axis=1, keepdims=True)
    with np.errstate(divide="ignore"):
        return np.where(span > 0, (2 * emax + U * span) / np.where(span > 0, span, 1.0), np.inf)


def check_uint8(img, v64, bound, part):
    """img [B, H, W, 3] against trunc(255 v) with v = v64 [B, 3, H, W] (not clamped) limited to
    [0, 1]: equal wherever 255 v is further than 255 * bound from an integer, within 1 elsewhere.
    A pixel whose v64 lies further than the bound outside [0, 1] is clamped whatever the error: its
    byte (0 or 255) is decided and compared exactly.  Returns the excluded share of the (pixel,
    component) pairs that take part."""
    v = np.clip(v64, 0.0, 1.0) * 255.0
    want = np.floor(v).astype(np.int64)
    got = np.asarray(img).astype(np.int64).transpose(0, 3, 1, 2)
    bnd = np.broadcast_to(bound[:, :, None, None], v.shape)
    near = (np.abs(v - np.round(v)) <= 255.0 * bnd) & ~((v64 < -bnd) | (v64 > 1.0 + bnd))
    assert np.array_equal(got[~near], want[~near])
    assert np.abs(got - want).max(initial=0) <= 1
    sel = np.broadcast_to(part.reshape(part.shape[0], 1, *v.shape[2:]), v.shape)
    return float(near[sel].mean()) if sel.any() else 0.0
