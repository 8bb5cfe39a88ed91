"""PCA colouring of rendered feature maps, on the HIP kernels of csrc/gs_feature_pca.hip (C ABI
and arithmetic: include/gs_feature_pca.h): channel moments with the Gram matrix on the matrix
cores, a one-workgroup fp64 Jacobi eigensolve (csrc/gs_sym_eig.h), and fused project / range /
colour passes.  Nothing is read back to the host, there are no float atomics, and two runs give
the same bits.

What the reference does to look at a 32-channel `semantic_feature` map, always the same way:

    utils/image_utils.py:27-58 feature_map        normalize, fit on [::3], first call freezes mean
                                                   and vectors, 1 % / 99 % quantile range, clamp
    sanity_feature.py:570-591, sanity_visuals.py:80-108, sanity_get_pca_feat*.py
                                                   sklearn PCA(3) on the masked pixels, one min / max
                                                   over the three components, (x * 255).astype(uint8)
    sanity_visuals_along_temporal*.py:56-129      one PCA over 300 frames, every frame transformed

becomes

    pca = FeaturePCA(32).update(maps, mask).fit()           # or fit_sequence(frames, masks)
    rgb = pca.colourise(maps, mask)                          # [B, H, W, 3] uint8, min / max range
    img = feature_map(feature, pca)                          # feature_map's semantics, [3, H, W]

Conventions: x is [B, C, H, W] or [C, H, W]; mask is None, [H, W] or [B, H, W] and a pixel takes
part iff its value is non-zero; normalize is F.normalize(dim=1); sample_stride s makes only the
pixels whose flat index within the image is a multiple of s take part in a fit (transforms
always cover every pixel).

Every function has a `_torch` twin in PyTorch operations for any device and dtype (FeaturePCA:
`FeaturePCATorch`): the parity oracle, the CPU path and the benchmark's baseline.  The HIP path
takes contiguous float32 device tensors and has no CPU fallback: host tensors raise.
"""
from __future__ import annotations

import functools
from typing import Iterable, Optional

import torch

from . import _args, _lib, robust_loss
from ._lib import GsplatError

MAX_C, MAX_K, MAX_SWEEPS = _lib.FPCA_MAX_C, _lib.FPCA_MAX_K, _lib.FPCA_MAX_SWEEPS
EPS = 1e-12  # F.normalize's
STATUS = {0: "ok", 1: "no more samples than ddof", 2: "the eigensolve's sweep cap was reached",
          3: "the covariance is not finite (a NaN or infinite pixel took part)"}

_need = functools.partial(_args.need, op="feature PCA needs", twin="the _torch twins run")


# ------------------------------------------------------------------ shared checks

def _images(x, what="x", C=None):
    """[B, C, H, W] or [C, H, W] -> the [B, C, H, W] view."""
    if not isinstance(x, torch.Tensor) or x.dim() not in (3, 4):
        raise GsplatError(f"{what} must be a [B, C, H, W] or [C, H, W] tensor")
    x4 = x[None] if x.dim() == 3 else x
    if min(x4.shape) < 1:
        raise GsplatError(f"{what} must not be empty (got {tuple(x.shape)})")
    if C is not None and x4.shape[1] != C:
        raise GsplatError(f"{what} must have {C} channels (got {tuple(x.shape)})")
    return x4


def _check_mask(mask, B, H, W, need_device):
    if mask is not None:
        _args.check_mask(mask, B, H, W, need_device=need_device)


def _check_k(C, k):
    if not (isinstance(k, int) and 1 <= k <= min(C, MAX_K)):
        raise GsplatError(f"n_components must be in [1, min(C, {MAX_K})] (got {k} with C = {C})")


def _check_components(components, mean, C=None):
    if not isinstance(components, torch.Tensor) or components.dim() != 2:
        raise GsplatError("components must be a [k, C] tensor")
    k, Cc = components.shape
    if C is not None and Cc != C:
        raise GsplatError(f"components [k, C] must match x's {C} channels (got {tuple(components.shape)})")
    if not 1 <= k <= MAX_K:
        raise GsplatError(f"components must have 1 to {MAX_K} rows (got {k})")
    if not isinstance(mean, torch.Tensor) or tuple(mean.shape) != (Cc,):
        raise GsplatError(f"mean must be [C] = [{Cc}]")
    return k


def _check_q(q):
    try:
        q0, q1 = q
    except (TypeError, ValueError):
        raise GsplatError("q must be a pair (q_lo, q_hi)") from None
    return robust_loss._check_q(q0), robust_loss._check_q(q1)


def _check_out(out):
    if out not in (torch.uint8, torch.float32):
        raise GsplatError(f"out must be torch.uint8 or torch.float32 (got {out})")


def _check_limits(C):
    if not 1 <= C <= MAX_C:
        raise GsplatError(f"the HIP feature PCA takes 1 <= C <= {MAX_C} channels (got {C}); the _torch twins take "
                          "any size")


def _bounds(lo, hi, B, k, device):
    """(lo, hi) broadcast to contiguous float64 [B, k] on `device`."""
    out = []
    for name, v in (("lo", lo), ("hi", hi)):
        v = torch.as_tensor(v, dtype=torch.float64, device=device)
        try:
            v = v.broadcast_to(B, k)
        except RuntimeError:
            raise GsplatError(f"{name} must broadcast to [B, k] = {(B, k)} (got {tuple(v.shape)})") from None
        out.append(v.contiguous())
    return out


def _mask_b(mask, B, H, W):
    """The mask as booleans [B or 1, H * W], or None."""
    if mask is None:
        return None
    return (mask != 0).reshape(-1, H * W)


# ------------------------------------------------------------------ the PyTorch twins

def _xhat_torch(x4, normalize):
    if not normalize:
        return x4
    return x4 / x4.pow(2).sum(dim=1, keepdim=True).sqrt().clamp_min(EPS)


def _fit_set_torch(B, H, W, mask, stride, device):
    """The pixels of a fit, bool [B, H * W]."""
    take = (torch.arange(H * W, device=device) % stride == 0)[None].expand(B, -1)
    m = _mask_b(mask, B, H, W)
    return take if m is None else take & m


def pca_moments_torch(x, mask=None, normalize=False, sample_stride=1, shift=None):
    """One call's moments (n, S [C], M [C, C], shift [C]): float64 sums over the fit set of
    x' = x_hat - shift in x's dtype; shift (x's dtype) defaults to the fit set's channel mean."""
    x4 = _images(x)
    B, C, H, W = x4.shape
    _check_mask(mask, B, H, W, need_device=False)
    if not (isinstance(sample_stride, int) and sample_stride >= 1):
        raise GsplatError(f"sample_stride must be an integer >= 1 (got {sample_stride})")
    sel = _fit_set_torch(B, H, W, mask, sample_stride, x4.device)
    X = _xhat_torch(x4, normalize).permute(0, 2, 3, 1).reshape(B, H * W, C)[sel]  # [n, C]
    n = X.shape[0]
    if shift is None:
        shift = (X.double().sum(0) / n).to(x4.dtype) if n else torch.zeros(C, dtype=x4.dtype, device=x4.device)
    elif not isinstance(shift, torch.Tensor) or tuple(shift.shape) != (C,):
        raise GsplatError(f"shift must be [C] = [{C}]")
    Xd = (X - shift.to(x4.dtype)).double()
    return torch.tensor(float(n), dtype=torch.float64, device=x4.device), Xd.sum(0), Xd.T @ Xd, shift


def pca_covariance_torch(n, S, M, shift, ddof=1):
    """(mean [C], cov [C, C]) in float64 of the moments; zeros (mean = shift) when n <= ddof."""
    n, S, M = n.double(), S.double(), M.double()
    ok = n > ddof
    d = torch.where(n > 0, S / n.clamp_min(1.0), torch.zeros_like(S))
    cov = (M - (n * d)[:, None] * d[None, :]) / torch.where(ok, n - ddof, torch.ones_like(n))
    return shift.double() + d, torch.where(ok, cov, torch.zeros_like(cov))


def pca_eig_torch(cov):
    """(eigenvalues [C] descending, eigenvectors [C, C] in rows) of a symmetric matrix with fit's
    sign rule: every row's entry of largest magnitude is positive, the lowest index on a tie."""
    lam, vec = torch.linalg.eigh(cov.double())
    lam, vec = lam.flip(0), vec.flip(1).T.contiguous()
    idx = vec.abs().argmax(dim=1, keepdim=True)
    sign = torch.where(vec.gather(1, idx) < 0, -1.0, 1.0).to(vec.dtype)
    return lam, vec * sign


def pca_project_torch(x, components, mean, mask=None, normalize=False, return_range=False):
    """pca_project in PyTorch operations, any device and dtype (x's)."""
    x4 = _images(x)
    B, C, H, W = x4.shape
    k = _check_components(components, mean, C)
    _check_mask(mask, B, H, W, need_device=False)
    d = _xhat_torch(x4, normalize) - mean.to(x4.dtype)[None, :, None, None]
    t = torch.einsum("bchw,kc->bkhw", d, components.to(x4.dtype))
    m = _mask_b(mask, B, H, W)
    if m is not None:
        t = torch.where(m.reshape(-1, 1, H, W), t, torch.zeros_like(t))
    t = t.reshape(*x.shape[:-3], k, H, W)
    if not return_range:
        return t
    return (t, *pca_range_torch(t, mask))


def pca_range_torch(t, mask=None):
    """(tmin, tmax) [B, k] of t [B, k, H, W] over the pixels that take part; 0 / 0 for none."""
    t4 = _images(t, "t")
    B, k, H, W = t4.shape
    m = _mask_b(mask, B, H, W)
    flat = t4.reshape(B, k, H * W)
    if m is None:
        return flat.amin(2), flat.amax(2)
    m = m[:, None].expand(B, k, H * W)
    inf = torch.full((), float("inf"), dtype=t4.dtype, device=t4.device)
    lo, hi = torch.where(m, flat, inf).amin(2), torch.where(m, flat, -inf).amax(2)
    none = ~m.any(2)
    return torch.where(none, torch.zeros_like(lo), lo), torch.where(none, torch.zeros_like(hi), hi)


def pca_colour_torch(t, lo, hi, mask=None, out=torch.uint8, clamp=False):
    """pca_colour in PyTorch operations, any device and dtype."""
    t4 = _images(t, "t")
    B, k, H, W = t4.shape
    if k != 3:
        raise GsplatError(f"colour needs k = 3 components (got {k})")
    _check_out(out)
    _check_mask(mask, B, H, W, need_device=False)
    lo, hi = _bounds(lo, hi, B, k, t4.device)
    span = (hi - lo)[:, :, None, None]
    flat = span == 0
    v = (t4.double() - lo[:, :, None, None]) / torch.where(flat, torch.ones_like(span), span)
    v = torch.where(flat, torch.zeros_like(v), v)
    m = _mask_b(mask, B, H, W)
    if m is not None:
        v = torch.where(m.reshape(-1, 1, H, W), v, torch.zeros_like(v))
    if clamp or out == torch.uint8:
        v = torch.where(v > 0, v.clamp_max(1.0), torch.zeros_like(v))  # NaN -> 0
    if out == torch.uint8:
        img = (255.0 * v).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
        return img[0] if t.dim() == 3 else img
    return v.to(torch.float32).reshape(t.shape)


# ------------------------------------------------------------------ the HIP path

def _struct(L, which, ws_dims, device, **fields):
    """The argument block of one pass with its workspace (kept alive by the caller through `ws`)."""
    n = L.gs_feature_pca_workspace_bytes(*ws_dims, which)
    ws = torch.empty(max(n, 16), dtype=torch.uint8, device=device)
    vals = {k: (_args.ptr(v) if isinstance(v, torch.Tensor) or v is None else v) for k, v in fields.items()}
    return _lib.GsFeaturePca(workspace=ws.data_ptr(), workspace_bytes=ws.numel(), **vals), ws


def _mask_bytes(mask, B, H, W):
    m = _args.mask_u8(mask, B, H, W)
    return m, int(m is not None and m.dim() == 3)


def pca_project(x: torch.Tensor, components: torch.Tensor, mean: torch.Tensor, mask: Optional[torch.Tensor] = None,
                normalize: bool = False, return_range: bool = False):
    """t [B, k, H, W] ([k, H, W] for one map), t[j] = sum_c fl32(x_hat[c] - mean[c]) components[j, c] in
    float32 in channel order, 0 where the mask is 0.  components [k, C] and mean [C] are float32
    (FeaturePCA.components_f32_ / mean_f32_).  return_range: also (tmin, tmax) [B, k], the minima
    and maxima of t over the pixels that take part.  Contiguous float32 device tensors only."""
    x4 = _images(x)
    B, C, H, W = x4.shape
    k = _check_components(components, mean, C)
    _need(x, "x")
    _need(components, "components")
    _need(mean, "mean")
    _check_limits(C)
    _check_k(C, k)
    m, per_image = _mask_bytes(mask, B, H, W)
    L = _lib.load()
    dev = x.device
    t = torch.empty(B, k, H, W, dtype=torch.float32, device=dev)
    tmin = torch.empty(B, k, dtype=torch.float32, device=dev)
    tmax = torch.empty(B, k, dtype=torch.float32, device=dev)
    s, ws = _struct(L, _lib.FPCA_PASS_PROJECT, (B, C, H, W, k), dev, B=B, C=C, H=H, W=W, k=k, mask_per_image=per_image,
                    normalize=int(bool(normalize)), x=x4, mask=m, proj_components=components, proj_mean=mean, t=t,
                    tmin=tmin, tmax=tmax)
    _lib.check(L.gs_feature_pca_project(s, _lib.stream(dev)), "feature pca project")
    t = t.reshape(*x.shape[:-3], k, H, W)
    return (t, tmin, tmax) if return_range else t


def _offset(t4, sub):
    """u = fl32(t - sub[b, j]) per plane."""
    B, k, H, W = t4.shape
    L = _lib.load()
    u = torch.empty_like(t4)
    s, ws = _struct(L, _lib.FPCA_PASS_OFFSET, (B, k, H, W, k), t4.device, B=B, C=k, H=H, W=W, k=k, t=t4, sub=sub, u=u)
    _lib.check(L.gs_feature_pca_offset(s, _lib.stream(t4.device)), "feature pca offset")
    return u


def pca_colour(t: torch.Tensor, lo, hi, mask: Optional[torch.Tensor] = None, out: torch.dtype = torch.uint8,
               clamp: bool = False) -> torch.Tensor:
    """The colours of t [B, 3, H, W] ([3, H, W]): v = (t - lo) / (hi - lo) in float64 with lo, hi
    broadcastable to [B, 3], 0 where hi == lo and where the mask is 0.  out=torch.uint8:
    [B, H, W, 3] holding trunc(255 v) with v limited to [0, 1]; out=torch.float32: [B, 3, H, W]
    holding fl32(v), limited to [0, 1] with clamp.  Contiguous float32 device tensors only."""
    t4 = _images(t, "t")
    B, k, H, W = t4.shape
    if k != 3:
        raise GsplatError(f"colour needs k = 3 components (got {k})")
    _check_out(out)
    _need(t, "t")
    lo, hi = _bounds(lo, hi, B, k, t.device)
    m, per_image = _mask_bytes(mask, B, H, W)
    L = _lib.load()
    u8 = out == torch.uint8
    img = torch.empty((B, H, W, 3) if u8 else (B, 3, H, W), dtype=out, device=t.device)
    s, ws = _struct(L, _lib.FPCA_PASS_COLOUR, (B, k, H, W, k), t.device, B=B, C=k, H=H, W=W, k=k,
                    mask_per_image=per_image, out_uint8=int(u8), clamp=int(bool(clamp)), t=t4, mask=m, lo=lo, hi=hi,
                    out=img)
    _lib.check(L.gs_feature_pca_colour(s, _lib.stream(t.device)), "feature pca colour")
    return img[0] if t.dim() == 3 else img


class FeaturePCA:
    """A PCA over the channels of feature maps, accumulated on the device.

    update(x, mask) adds a call's pixels to the float64 moments n, S = sum x', M = sum x' x'^T of
    x' = fl32(x_hat - shift); the float32 shift is the first update's masked channel mean (or the
    caller's), which keeps the centred second moment free of cancellation, so accumulating over
    frames needs no merge formulas.  covariance() -> (mean, cov, n); fit() diagonalises it on the
    device and sets components_ [k, C] (float64) and components_f32_, explained_variance_ [C],
    mean_ [C] and mean_f32_, eigenvectors_ [C, C] (rows) and the int32 status, none of which is
    read back; check() reads the status and raises unless it is 0 (1: no more samples than ddof,
    2: the sweep cap was reached, 3: the covariance is not finite, as after a NaN pixel; the
    components are zeros then, never NaN)."""

    _hip = True

    def __init__(self, C: int, normalize: bool = False, sample_stride: int = 1, ddof: int = 1, n_components: int = 3):
        if not (isinstance(C, int) and C >= 1):
            raise GsplatError(f"C must be an integer >= 1 (got {C})")
        if self._hip:
            _check_limits(C)
        _check_k(C, n_components)
        if not (isinstance(sample_stride, int) and sample_stride >= 1):
            raise GsplatError(f"sample_stride must be an integer >= 1 (got {sample_stride})")
        if not (isinstance(ddof, int) and ddof >= 0):
            raise GsplatError(f"ddof must be an integer >= 0 (got {ddof})")
        self.C, self.normalize, self.sample_stride, self.ddof, self.n_components = C, bool(normalize), sample_stride, ddof, n_components
        self.state = None   # float64 [1 + C + C*C]: n, S, M
        self.shift = None   # [C]
        self.fitted = False

    # -- moments
    def _begin(self, x, shift):
        dev = x.device
        self.state = torch.zeros(1 + self.C + self.C * self.C, dtype=torch.float64, device=dev)
        if shift is not None:
            if not isinstance(shift, torch.Tensor) or tuple(shift.shape) != (self.C,):
                raise GsplatError(f"shift must be [C] = [{self.C}]")
            self.shift = shift.detach().to(device=dev, dtype=torch.float32 if self._hip else x.dtype).clone()
        return shift is None

    def update(self, x: torch.Tensor, mask: Optional[torch.Tensor] = None, shift: Optional[torch.Tensor] = None):
        """Add the fit set of x [B, C, H, W] to the moments.  `shift` [C] can be given to the first update
        only: the moments of one object are about one shift, so a later one raises."""
        x4 = _images(x, C=self.C)
        B, C, H, W = x4.shape
        if self._hip:
            _need(x, "x")
        _check_mask(mask, B, H, W, need_device=self._hip)
        if self.state is not None and self.state.device != x.device:
            raise GsplatError(f"x is on {x.device}, the moments are on {self.state.device}")
        first = self.state is None
        if shift is not None and not first:
            raise GsplatError("shift can be given to the first update only: the moments so far are about the first one")
        compute = self._begin(x4, shift) if first else False
        if not self._hip:
            n, S, M, sh = pca_moments_torch(x4.detach(), mask, self.normalize, self.sample_stride,
                                            None if compute else self.shift)
            self.shift = sh
            self.state += torch.cat([n.reshape(1), S, M.reshape(-1)])
            return self
        if compute:
            self.shift = torch.empty(C, dtype=torch.float32, device=x.device)
        m, per_image = _mask_bytes(mask, B, H, W)
        L = _lib.load()
        s, ws = _struct(L, _lib.FPCA_PASS_UPDATE, (B, C, H, W, 0), x.device, B=B, C=C, H=H, W=W, mask_per_image=per_image,
                        normalize=int(self.normalize), sample_stride=self.sample_stride, compute_shift=int(compute),
                        x=x4.detach(), mask=m, shift=self.shift, state=self.state)
        _lib.check(L.gs_feature_pca_update(s, _lib.stream(x.device)), "feature pca update")
        return self

    def _moments(self):
        if self.state is None:
            raise GsplatError("no update() yet")
        C = self.C
        return self.state[0], self.state[1:1 + C], self.state[1 + C:].view(C, C)

    @property
    def n(self):
        return self._moments()[0]

    def covariance(self):
        """(mean [C], cov [C, C], n), float64 on the device."""
        n, S, M = self._moments()
        if not self._hip:
            return (*pca_covariance_torch(n, S, M, self.shift, self.ddof), n)
        C, dev = self.C, self.state.device
        mean = torch.empty(C, dtype=torch.float64, device=dev)
        cov = torch.empty(C, C, dtype=torch.float64, device=dev)
        L = _lib.load()
        s, ws = _struct(L, _lib.FPCA_PASS_COVARIANCE, (1, C, 1, 1, 0), dev, C=C, ddof=self.ddof, shift=self.shift,
                        state=self.state, mean=mean, cov=cov)
        _lib.check(L.gs_feature_pca_covariance(s, _lib.stream(dev)), "feature pca covariance")
        return mean, cov, n

    # -- eigensolve
    def fit(self):
        """Diagonalise the covariance of everything added so far."""
        n, S, M = self._moments()
        C, k, dev = self.C, self.n_components, self.state.device
        if not self._hip:
            mean, cov = pca_covariance_torch(n, S, M, self.shift, self.ddof)
            finite = torch.isfinite(cov).all()
            lam, vec = pca_eig_torch(torch.where(finite, cov, torch.zeros_like(cov)))
            ok = (n > self.ddof) & finite
            self.status = torch.where(n > self.ddof, torch.where(finite, 0, 3), 1).to(torch.int32).reshape(1)
            self.explained_variance_, self.eigenvectors_ = lam * ok, vec * ok
            self.mean_ = mean
        else:
            f64 = functools.partial(torch.empty, dtype=torch.float64, device=dev)
            self.mean_, self.explained_variance_, self.eigenvectors_, self.components_ = f64(C), f64(C), f64(C, C), f64(k, C)
            self.mean_f32_ = torch.empty(C, dtype=torch.float32, device=dev)
            self.components_f32_ = torch.empty(k, C, dtype=torch.float32, device=dev)
            self.status = torch.empty(1, dtype=torch.int32, device=dev)
            L = _lib.load()
            s, ws = _struct(L, _lib.FPCA_PASS_FIT, (1, C, 1, 1, k), dev, C=C, k=k, ddof=self.ddof, shift=self.shift,
                            state=self.state, mean=self.mean_, mean_f32=self.mean_f32_, evals=self.explained_variance_,
                            evecs=self.eigenvectors_, components=self.components_, components_f32=self.components_f32_,
                            status=self.status)
            _lib.check(L.gs_feature_pca_fit(s, _lib.stream(dev)), "feature pca fit")
            self._ws = ws  # the eigensolve's matrices above the LDS order: alive until the next fit
        if not self._hip:
            self.components_ = self.eigenvectors_[:k].contiguous()
            self.mean_f32_ = self.mean_.to(torch.float32)
            self.components_f32_ = self.components_.to(torch.float32)
        self.fitted = True
        return self

    def check(self):
        """Read the status back; raise unless the fit succeeded."""
        self._fitted()
        st = int(self.status.item())
        if st:
            raise GsplatError(f"feature PCA fit: status {st} ({STATUS.get(st, 'unknown')})")
        return self

    def _fitted(self):
        if not self.fitted:
            raise GsplatError("no fit() yet")

    # -- transform and colour
    def transform(self, x: torch.Tensor, mask: Optional[torch.Tensor] = None, return_range: bool = False):
        """pca_project with the fitted components and mean (their float32 roundings on the HIP path)."""
        self._fitted()
        _images(x, C=self.C)
        if self._hip:
            return pca_project(x, self.components_f32_, self.mean_f32_, mask, self.normalize, return_range)
        return pca_project_torch(x, self.components_.to(x.dtype), self.mean_.to(x.dtype), mask, self.normalize, return_range)

    def colourise(self, x: torch.Tensor, mask: Optional[torch.Tensor] = None, range="minmax",
                  out: torch.dtype = torch.uint8, q=(0.01, 0.99), return_range: bool = False):
        """Project x and colour it.  range: "minmax" (per image one lo = min and one hi = max over
        the three components and the pixels that take part: the reference's sklearn scripts),
        "quantile" (per image and component the q quantiles of u = t - min t, clamped: feature_map;
        needs mask=None) or a pair (lo, hi) broadcastable to [B, 3] for colours that stay fixed over a
        sequence.  out=torch.uint8 -> [B, H, W, 3]; torch.float32 -> [B, 3, H, W].  return_range: also the
        float64 (lo, hi) [B, 3] that were used (for the quantile range: of u)."""
        self._fitted()
        _check_out(out)
        if self.n_components != 3:
            raise GsplatError(f"colour needs k = 3 components (got {self.n_components})")
        quantile = isinstance(range, str) and range == "quantile"
        if isinstance(range, str) and range not in ("minmax", "quantile"):
            raise GsplatError(f"range must be 'minmax', 'quantile' or a pair (lo, hi) (got {range!r})")
        if quantile:
            q0, q1 = _check_q(q)
            if mask is not None:
                raise GsplatError("range='quantile' needs mask=None: the quantile's values layout has no mask")
        elif not isinstance(range, str):
            try:
                lo, hi = range
            except (TypeError, ValueError):
                raise GsplatError("range must be 'minmax', 'quantile' or a pair (lo, hi)") from None
        colour = pca_colour if self._hip else pca_colour_torch
        t, tmin, tmax = self.transform(x, mask, return_range=True)
        t4 = _images(t, "t")
        B, k, H, W = t4.shape
        single = x.dim() == 3
        if quantile:
            u = _offset(t4, tmin) if self._hip else t4 - tmin[:, :, None, None]
            quant = robust_loss.plane_quantile if self._hip else robust_loss.plane_quantile_torch
            planes = u.reshape(B * k, H * W)
            lo, hi = quant(planes, q0).reshape(B, k), quant(planes, q1).reshape(B, k)
            img = colour(u, lo, hi, None, out, clamp=True)
        elif isinstance(range, str):
            lo = tmin.amin(dim=1, keepdim=True).double().expand(B, k)
            hi = tmax.amax(dim=1, keepdim=True).double().expand(B, k)
            img = colour(t4, lo, hi, mask, out)
        else:
            lo, hi = _bounds(lo, hi, B, k, t4.device)
            img = colour(t4, lo, hi, mask, out)
        img = img[0] if single else img
        return (img, lo, hi) if return_range else img


class FeaturePCATorch(FeaturePCA):
    """FeaturePCA in PyTorch operations, any device and dtype: the moments are float64 sums of x'
    in x's dtype, the eigensolve is torch.linalg.eigh in float64."""
    _hip = False


def fit_sequence(maps: Iterable[torch.Tensor], masks: Optional[Iterable] = None, pca: Optional[FeaturePCA] = None,
                 **kw) -> FeaturePCA:
    """The temporal scripts' flow: one update per element of `maps` ([B, C, H, W] or [C, H, W],
    with the matching element of `masks`), then one fit.  `pca` (default: a new FeaturePCA of the
    first map's channel count, **kw its arguments) is returned."""
    return _fit_sequence(FeaturePCA, maps, masks, pca, kw)


def fit_sequence_torch(maps, masks=None, pca=None, **kw) -> FeaturePCA:
    """fit_sequence in PyTorch operations, any device and dtype."""
    return _fit_sequence(FeaturePCATorch, maps, masks, pca, kw)


def _fit_sequence(cls, maps, masks, pca, kw):
    masks = iter(masks) if masks is not None else None
    seen = False
    for x in maps:
        if pca is None:
            pca = cls(_images(x).shape[1], **kw)
        try:
            mask = next(masks) if masks is not None else None
        except StopIteration:
            raise GsplatError("masks ended before maps") from None
        pca.update(x, mask)
        seen = True
    if not seen:
        raise GsplatError("maps must not be empty")
    return pca.fit()


def feature_map(feature: torch.Tensor, pca: Optional[FeaturePCA] = None) -> torch.Tensor:
    """The reference's feature_map (utils/image_utils.py:27-58) of one map [C, H, W] (or a batch):
    normalized features, a fit on every third pixel, the 1 % / 99 % quantile range, float colours
    [3, H, W] in [0, 1].  The first call with a given `pca` (feature_map_pca(C)) fits it and thereby
    freezes mean and components for the later calls; without one every call fits its own."""
    return _feature_map(FeaturePCA, feature, pca)


def feature_map_torch(feature: torch.Tensor, pca: Optional[FeaturePCA] = None) -> torch.Tensor:
    """feature_map in PyTorch operations, any device and dtype."""
    return _feature_map(FeaturePCATorch, feature, pca)


def feature_map_pca(C: int, torch_twin: bool = False) -> FeaturePCA:
    """The FeaturePCA that feature_map fits: normalize, every third pixel, ddof 1, three components."""
    return (FeaturePCATorch if torch_twin else FeaturePCA)(C, normalize=True, sample_stride=3)


def _feature_map(cls, feature, pca):
    x4 = _images(feature, "feature")
    if pca is None:
        pca = cls(x4.shape[1], normalize=True, sample_stride=3)
    if not pca.fitted:
        pca.update(feature).fit()
    return pca.colourise(feature, None, "quantile", torch.float32)
