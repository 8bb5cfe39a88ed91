"""The feature-map PCA (include/gs_feature_pca.h) on the GPU against float64 statements on the
CPU (numpy, tests/_feature_pca_cases.py, and the float64 twin), never against the code under test.

Bounds, with u = 2^-24, derived and not measured (n_acc and the sweep cap S are read from the
library; the derivations are in tests/_feature_pca_cases.py):

    shift        u |m| + (n 2^-53 + (C + 6) u) mean |x_hat|  of the fit set's mean m: one fp32 rounding, fp64
                 sums of n terms, and under normalize x_hat's own error
    S, M         (n_acc + 4) u sum |x'|, (n_acc + 4) u sum |x'_i x'_j|, under normalize plus
                 (C + 6) u sum |x_hat| and (C + 6) u sum (|x_hat_i x'_j| + |x'_i x_hat_j|);
                 against the fp64 sums of x' = x_hat - (the device's own fp32 shift)
    covariance   1e-12 relative: the same fp64 formula on the device's own state
    eigensolve   |AV - V L|_F <= S C 2^-52 |A|_F,  |V^T V - I|_F <= S C 2^-52,  eigenvalues against
                 eigh within S C 2^-52 |A|_F;  A the device's own covariance
    projection   E = u sum_c |V_jc| ((C + 6) |x_hat_c| + (C + 4) |x_hat_c - mean_c|), the first term under
                 normalize only; against the fp64 projection with the device's own fp32 components
    min / max    within max E over the pixels that take part
    quantile     lo, hi equal plane_quantile_torch of the device's own u, bit for bit
    colours      float: (2 max E + u (hi - lo)) / (hi - lo) from the fp64 v of the device's t, lo, hi;
                 uint8: trunc(255 v64) wherever 255 v64 is further than 255 * that from an integer,
                 within 1 elsewhere, the excluded share <= 5 %; a pixel whose v64 lies further than
                 that outside [0, 1] is clamped whatever the error: decided, compared exactly
    subspace     |V^T V - V64^T V64|_F <= 2 |cov - cov64|_F / gap + S C 2^-52  (Davis-Kahan)

Each comparison prints its measured maximum as a fraction of its bound before asserting.  Measured
on an MI355X over all cases (profiles/feature_pca/parity.json), largest error / bound: shift 0.98
(the one fp32 rounding), S 0.004, M 0.04, residual 0.03, orthogonality 0.55, eigenvalues 0.02,
projection 0.35, min / max 0.27, colours 0.06, subspace 0.13; uint8 excluded share at most 2.2 %
(min / max range) and 1.3 % (quantile range).
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

from dynamic3dgaussians_amd import (FeaturePCA, FeaturePCATorch, _lib, feature_map, feature_map_pca, fit_sequence,
                                    pca_colour, pca_covariance_torch, pca_project, pca_project_torch,
                                    plane_quantile_torch)
from dynamic3dgaussians_amd._lib import GsplatError
from tests import _feature_pca_cases as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = K.U

FRACTIONS = []  # (quantity, max error / bound) of every comparison made (tools/feature_pca_bench.py --parity)


def _np(t):
    return t.detach().cpu().numpy()


def _frac(name, got, want, bound):
    err = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64))
    bound = np.broadcast_to(np.asarray(bound, np.float64), err.shape)
    frac = float((err / np.maximum(bound, 1e-300)).max(initial=0.0))
    print(f"{name}: max error / bound = {frac:.3f}")
    FRACTIONS.append((name, frac))
    assert (err <= bound).all(), (name, frac)
    return frac


def _dev(t):
    return None if t is None else t.to(DEV)


def _eigen_checks(A, lam, rows, S, tag):
    C = A.shape[0]
    V, nA, b = rows.T, np.linalg.norm(A), S * C * 2.0 ** -52
    _frac(f"{tag} residual", np.linalg.norm(A @ V - V * lam), 0.0, b * nA)
    _frac(f"{tag} orthogonality", np.linalg.norm(V.T @ V - np.eye(C)), 0.0, b)
    _frac(f"{tag} eigenvalues", lam, np.linalg.eigvalsh((A + A.T) / 2)[::-1], b * nA)
    assert np.all(np.diff(lam) <= 0)
    assert np.array_equal(K.np_sign_rule(rows), rows)  # the sign rule, on every component


@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("normalize", [False, True], ids=["raw", "normalized"])
@pytest.mark.parametrize("kind", K.MASKS)
@pytest.mark.parametrize("shape", K.SHAPES, ids=K.shape_id)
def test_against_fp64(shape, kind, normalize, stride):
    B, C, H, W = shape
    L = _lib.load()
    n_acc, S_cap = L.gs_feature_pca_n_acc(B, H, W), L.gs_feature_pca_max_sweeps()
    assert n_acc > 0 and S_cap == _lib.FPCA_MAX_SWEEPS
    x, mask = K.spectrum(*shape), K.mask_of(kind, B, H, W)
    ddof, k = K.ddof_of(shape), K.k_of(shape)
    xd, md = _dev(x), _dev(mask)
    tag = f"{K.shape_id(shape)} {kind} {'normalized' if normalize else 'raw'} stride {stride}:"

    # ---- moments
    pca = FeaturePCA(C, normalize=normalize, sample_stride=stride, ddof=ddof, n_components=k).update(xd, md)
    shift, state = _np(pca.shift).astype(np.float64), _np(pca.state)
    n, Sd, Md = state[0], state[1:1 + C], state[1 + C:].reshape(C, C)
    x64 = x.double().numpy()
    xh = K.np_xhat(x64, normalize)
    rows_h = xh.transpose(0, 2, 3, 1).reshape(B, H * W, C)
    rows_p = rows_h - shift
    sel = K.np_fit_set(B, H, W, mask, stride)
    assert n == sel.sum() and n > ddof
    m64 = rows_h[sel].mean(axis=0)
    mabs = np.abs(rows_h[sel]).mean(axis=0)  # one fp32 rounding of the mean, fp64 sums of n terms in some order
    _frac(f"{tag} shift", shift, m64, U * np.abs(m64) + (n * 2.0 ** -53 + (C + 6) * U * normalize) * mabs)
    bS, bM = K.moment_bounds(rows_h, rows_p, sel, n_acc, C, normalize)
    _frac(f"{tag} S", Sd, rows_p[sel].sum(axis=0), bS)
    _frac(f"{tag} M", Md, rows_p[sel].T @ rows_p[sel], bM)
    assert np.array_equal(Md, Md.T)  # stored symmetric

    # ---- covariance: the documented fp64 formula on the device's own state
    mean_d, cov_d, n_d = pca.covariance()
    mean_t, cov_t = pca_covariance_torch(pca.state[0].cpu(), torch.from_numpy(Sd), torch.from_numpy(Md), pca.shift.cpu(), ddof)
    A = _np(cov_d)
    _frac(f"{tag} cov", A, cov_t.numpy(), 1e-12 * np.abs(cov_t.numpy()).max())
    _frac(f"{tag} mean", _np(mean_d), mean_t.numpy(), 1e-12 * np.abs(mean_t.numpy()).max())
    assert float(n_d) == n

    # ---- eigensolve
    pca.fit()
    assert int(pca.status.item()) == 0
    pca.check()
    lam, rows = _np(pca.explained_variance_), _np(pca.eigenvectors_)
    _eigen_checks(A, lam, rows, S_cap, tag)
    assert torch.equal(pca.components_, pca.eigenvectors_[:k]) and torch.equal(pca.mean_, mean_d)
    assert torch.equal(pca.components_f32_, pca.components_.float()) and torch.equal(pca.mean_f32_, pca.mean_.float())

    # ---- projection
    comp, mean = _np(pca.components_f32_).astype(np.float64), _np(pca.mean_f32_).astype(np.float64)
    t, tmin, tmax = pca.transform(xd, md, return_range=True)
    assert t.shape == (B, k, H, W) and t.dtype == torch.float32
    t_dev = _np(t)
    t64 = K.np_project(x64, comp, mean, mask, normalize)
    E = K.projection_bound(xh, comp, mean, normalize)
    _frac(f"{tag} t", t_dev, t64, E)
    part = K.np_part(B, H, W, mask)
    off = ~part.reshape(B, 1, H, W)
    assert not t_dev[np.broadcast_to(off, t_dev.shape)].any()  # exactly 0 where masked out
    Emax = np.stack([E.reshape(B, k, -1)[b][:, part[b]].max(axis=1) for b in range(B)])
    lo64, hi64 = K.np_range(t64, mask)
    _frac(f"{tag} tmin", _np(tmin), lo64, Emax)
    _frac(f"{tag} tmax", _np(tmax), hi64, Emax)
    flat = t_dev.reshape(B, k, -1)
    for b in range(B):  # and exactly the extrema of the device's own t
        assert np.array_equal(_np(tmin)[b], flat[b][:, part[b]].min(axis=1))
        assert np.array_equal(_np(tmax)[b], flat[b][:, part[b]].max(axis=1))
    if k != 3:
        with pytest.raises(GsplatError, match="k = 3"):
            pca.colourise(xd, md)
        return

    # ---- min / max colours
    img, lo, hi = pca.colourise(xd, md, "minmax", torch.uint8, return_range=True)
    vf = pca.colourise(xd, md, "minmax", torch.float32)
    assert img.shape == (B, H, W, 3) and img.dtype == torch.uint8 and vf.shape == (B, 3, H, W)
    lo_d, hi_d = _np(lo), _np(hi)
    assert np.array_equal(lo_d, np.broadcast_to(_np(tmin).min(axis=1, keepdims=True).astype(np.float64), (B, 3)))
    assert np.array_equal(hi_d, np.broadcast_to(_np(tmax).max(axis=1, keepdims=True).astype(np.float64), (B, 3)))
    v64 = K.np_colour(t_dev, lo_d, hi_d, mask)
    bound = K.colour_bound(E, lo_d, hi_d, shared=True)
    _frac(f"{tag} colours", _np(vf), v64, bound[:, :, None, None])
    share = K.check_uint8(_np(img), v64, bound, part)
    print(f"{tag} uint8 excluded share {share:.4f}")
    FRACTIONS.append((f"{tag} uint8 excluded share / 0.05", share / 0.05))
    assert share <= 0.05
    off_img = np.broadcast_to(~part.reshape(B, H, W, 1), (B, H, W, 3))
    assert not _np(img)[off_img].any() and not _np(vf)[np.broadcast_to(off, (B, 3, H, W))].any()

    # ---- quantile colours
    if kind != "none":
        with pytest.raises(GsplatError, match="mask=None"):
            pca.colourise(xd, md, "quantile")
        return
    vq, qlo, qhi = pca.colourise(xd, None, "quantile", torch.float32, return_range=True)
    u = t.cpu() - tmin.cpu()[:, :, None, None]  # fl32(t - tmin), as the device's
    planes = u.reshape(B * 3, H * W)
    assert torch.equal(qlo.cpu().reshape(-1), plane_quantile_torch(planes, 0.01))
    assert torch.equal(qhi.cpu().reshape(-1), plane_quantile_torch(planes, 0.99))
    vq_raw = K.np_colour(u.numpy(), _np(qlo), _np(qhi), None)  # before the clamp
    qbound = K.colour_bound(E, _np(qlo), _np(qhi), shared=False)
    _frac(f"{tag} quantile colours", _np(vq), np.clip(vq_raw, 0.0, 1.0), qbound[:, :, None, None])
    imq = pca.colourise(xd, None, "quantile", torch.uint8)
    share = K.check_uint8(_np(imq), vq_raw, qbound, part)
    print(f"{tag} quantile uint8 excluded share {share:.4f}")
    FRACTIONS.append((f"{tag} quantile uint8 excluded share / 0.05", share / 0.05))
    assert share <= 0.05


def _integers(shape, seed=0):
    g = torch.Generator().manual_seed(77 + seed + sum(shape))
    return torch.randint(-8, 9, shape, generator=g).to(torch.float32)


@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("kind", K.MASKS)
@pytest.mark.parametrize("shape", K.SHAPES, ids=K.shape_id)
def test_exact_layout_and_reruns(shape, kind, stride):
    """Integers in [-8, 8] with shift 0: every piece product and every partial sum is exact below
    2^24, so n, S and M are the integer sums bit for bit, whatever the order; so is a projection
    onto integer components.  And two runs of every function give the same bits."""
    B, C, H, W = shape
    x, mask = _integers(shape), K.mask_of(kind, B, H, W)
    xd, md = _dev(x), _dev(mask)
    k = min(C, 8)

    def moments():
        return FeaturePCA(C, sample_stride=stride, ddof=K.ddof_of(shape), n_components=K.k_of(shape)).update(
            xd, md, shift=torch.zeros(C))
    pca = moments()
    rows = x.double().numpy().transpose(0, 2, 3, 1).reshape(B, H * W, C)[K.np_fit_set(B, H, W, mask, stride)]
    state = _np(pca.state)
    assert state[0] == rows.shape[0] and not _np(pca.shift).any()
    assert np.array_equal(state[1:1 + C], rows.sum(axis=0))
    assert np.array_equal(state[1 + C:].reshape(C, C), rows.T @ rows)
    twice = moments().update(xd, md)  # accumulation: the same call again doubles every sum
    assert np.array_equal(_np(twice.state), 2 * state)

    g = torch.Generator().manual_seed(5)
    comp = torch.randint(-4, 5, (k, C), generator=g).to(torch.float32)
    mean = torch.randint(-2, 3, (C,), generator=g).to(torch.float32)
    t, tmin, tmax = pca_project(xd, _dev(comp), _dev(mean), md, return_range=True)
    t64, lo64, hi64 = pca_project_torch(x.double(), comp.double(), mean.double(), mask, return_range=True)
    assert torch.equal(t.cpu().double(), t64) and torch.equal(tmin.cpu().double(), lo64) and torch.equal(tmax.cpu().double(), hi64)

    # reruns
    again = moments()
    assert torch.equal(again.state, pca.state)
    auto = [FeaturePCA(C, normalize=True, sample_stride=stride, ddof=K.ddof_of(shape), n_components=K.k_of(shape))
            .update(xd + 0.25, md).fit() for _ in range(2)]
    for name in ("state", "shift", "mean_", "explained_variance_", "eigenvectors_", "components_", "components_f32_",
                 "mean_f32_", "status"):
        assert torch.equal(getattr(auto[0], name), getattr(auto[1], name)), name
    assert int(auto[0].status.item()) == 0
    t2, tmin2, tmax2 = pca_project(xd, _dev(comp), _dev(mean), md, return_range=True)
    assert torch.equal(t, t2) and torch.equal(tmin, tmin2) and torch.equal(tmax, tmax2)
    if C >= 3:
        for how, m in (("minmax", md), ("quantile", None)):
            for out in (torch.uint8, torch.float32):
                a, b = (auto[0].colourise(xd + 0.25, m, how, out) for _ in range(2))
                assert torch.equal(a, b)


SUBSPACE = [s for s in K.SHAPES if s[1] >= 4]


@pytest.mark.parametrize("shape", SUBSPACE, ids=K.shape_id)
def test_top3_subspace_matches_the_fp64_twin(shape):
    B, C, H, W = shape
    x = K.spectrum(*shape)
    S_cap = _lib.load().gs_feature_pca_max_sweeps()
    dev = FeaturePCA(C).update(_dev(x)).fit().check()
    twin = FeaturePCATorch(C).update(x.double()).fit().check()
    cov, cov64 = _np(dev.covariance()[1]), twin.covariance()[1].numpy()
    lam64 = twin.explained_variance_.numpy()
    gap = lam64[2] - lam64[3]
    assert gap > 0.05 * lam64[0]
    V, V64 = _np(dev.components_), twin.components_.numpy()
    bound = 2 * np.linalg.norm(cov - cov64) / gap + S_cap * C * 2.0 ** -52
    _frac(f"{K.shape_id(shape)} top-3 subspace", np.linalg.norm(V.T @ V - V64.T @ V64), 0.0, bound)


def test_feature_map_and_fit_sequence_are_their_compositions():
    frames = [_dev(K.spectrum(1, 32, 37, 53, seed=s)[0]) for s in range(3)]
    masks = [_dev(K.mask_of("hw", 1, 37, 53, seed=s)) for s in range(3)]
    pca = fit_sequence(frames, masks)
    step = FeaturePCA(32)
    for f, m in zip(frames, masks):
        step.update(f, m)
    step.fit()
    for name in ("state", "shift", "components_", "components_f32_", "mean_", "explained_variance_", "status"):
        assert torch.equal(getattr(pca, name), getattr(step, name)), name
    assert int(pca.status.item()) == 0 and float(pca.n) == sum(float((m != 0).sum()) for m in masks)
    # every frame coloured with the sequence's PCA and one fixed range
    lo, hi = -20.0, 20.0
    for f, m in zip(frames, masks):
        t = pca.transform(f, m)
        assert torch.equal(pca.colourise(f, m, (lo, hi)), pca_colour(t, lo, hi, m))

    holder = feature_map_pca(32)
    first = feature_map(frames[0], holder)
    ref = FeaturePCA(32, normalize=True, sample_stride=3).update(frames[0]).fit()
    assert first.shape == (3, 37, 53) and first.dtype == torch.float32
    assert torch.equal(first, ref.colourise(frames[0], None, "quantile", torch.float32))
    second = feature_map(frames[1], holder)  # frozen by the first call
    assert torch.equal(holder.components_, ref.components_) and torch.equal(holder.mean_, ref.mean_)
    assert torch.equal(second, ref.colourise(frames[1], None, "quantile", torch.float32))
    assert float(first.min()) == 0.0 and float(first.max()) == 1.0
    batch = feature_map(torch.stack(frames[:2]), holder)
    assert torch.equal(batch[0], first) and torch.equal(batch[1], second)


def test_status_and_degenerate_inputs():
    x = _dev(K.spectrum(1, 3, 1, 1))
    pca = FeaturePCA(3).update(x).fit()  # one sample, ddof 1
    assert int(pca.status.item()) == 1
    for name in ("components_", "components_f32_", "explained_variance_", "eigenvectors_"):
        v = getattr(pca, name)
        assert not v.any() and not torch.isnan(v).any(), name
    with pytest.raises(GsplatError, match="status 1"):
        pca.check()
    empty = FeaturePCA(3).update(_dev(K.spectrum(1, 3, 4, 5)), torch.zeros(4, 5, device=DEV)).fit()
    assert int(empty.status.item()) == 1 and float(empty.n) == 0 and not empty.shift.any() and not torch.isnan(empty.mean_).any()
    t, tmin, tmax = empty.transform(_dev(K.spectrum(1, 3, 4, 5)), torch.zeros(4, 5, device=DEV), return_range=True)
    assert not t.any() and not tmin.any() and not tmax.any()
    # a NaN or infinite pixel in the fit set: a status of its own, zeros and no NaN in what fit writes
    for C, bad in ((3, float("nan")), (32, float("inf")), (128, float("nan"))):
        xb = K.spectrum(1, C, 12, 31).clone()
        xb[0, C // 2, 5, 7] = bad
        pca = FeaturePCA(C).update(_dev(xb)).fit()
        assert int(pca.status.item()) == 3
        for name in ("components_", "components_f32_", "explained_variance_", "eigenvectors_"):
            v = getattr(pca, name)
            assert not v.any() and not torch.isnan(v).any(), (C, name)
        with pytest.raises(GsplatError, match="status 3"):
            pca.check()
        mask = torch.ones(12, 31)
        mask[5, 7] = 0  # the same pixel masked out takes no part
        assert int(FeaturePCA(C).update(_dev(xb), _dev(mask)).fit().status.item()) == 0
    const = torch.full((2, 3, 9, 17), 2.0, device=DEV)
    pca = FeaturePCA(3).update(const).fit().check()  # a zero covariance: every projection is 0
    for how in ("minmax", "quantile", (1.5, 1.5)):
        for out in (torch.uint8, torch.float32):
            img = pca.colourise(const, None, how, out)
            assert not img.any() and not torch.isnan(img.float()).any()  # hi == lo


def test_device_argument_checks():
    x = _dev(K.spectrum(2, 7, 11, 13))
    V, mu, t = torch.eye(3, 7, device=DEV), torch.zeros(7, device=DEV), torch.zeros(2, 3, 11, 13, device=DEV)
    for call in (lambda: FeaturePCA(7).update(x.double()), lambda: FeaturePCA(7).update(x.transpose(2, 3)),
                 lambda: FeaturePCA(7).update(x, torch.ones(11, 13)), lambda: pca_project(x, V.double(), mu),
                 lambda: pca_project(x, V, mu.cpu()), lambda: pca_project(x[:, :, :, ::2], V, mu),
                 lambda: pca_colour(t.double(), 0.0, 1.0), lambda: pca_colour(t[:, :, ::2], 0.0, 1.0),
                 lambda: pca_colour(t, 0.0, 1.0, mask=torch.ones(11, 13)),
                 lambda: FeaturePCA(7).update(x).update(x.cpu()),
                 lambda: FeaturePCA(7).update(x).update(x, shift=torch.zeros(7))):
        with pytest.raises(GsplatError):
            call()
