"""The feature-map PCA without a GPU: the PyTorch twins against a numpy fp64 statement of the same
mathematics and against sklearn, the host build of the Jacobi eigensolver (csrc/gs_sym_eig.h)
through the library's host entry, the host validator (through ctypes and, under ASan + UBSan, as
a stand-alone program), the build list, the ctypes mirror, and the argument checks of both
paths."""
from __future__ import annotations

import ctypes
import os

import numpy as np
import pytest
import torch

from dynamic3dgaussians_amd import (FeaturePCA, FeaturePCATorch, _lib, build, feature_map, feature_map_pca,
                                    feature_map_torch, fit_sequence, fit_sequence_torch, pca_colour, pca_colour_torch,
                                    pca_project, pca_project_torch, pca_range_torch, plane_quantile_torch)
from dynamic3dgaussians_amd import feature_pca as fp
from dynamic3dgaussians_amd._lib import GsplatError
from tests import _feature_pca_cases as K
from tests._harness import run_host_sanitizer

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-10


def _close(got, want, what, scale=None):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = float(np.abs(want).max(initial=0.0)) if scale is None else scale
    err = float(np.abs(got - want).max(initial=0.0))
    print(f"{what}: max error {err:.3e} of scale {scale:.3e}")
    assert got.shape == want.shape and err <= RTOL * max(scale, 1e-300), what


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("kind", K.MASKS)
@pytest.mark.parametrize("stride", [1, 3])
def test_twins_against_numpy(normalize, kind, stride):
    B, C, H, W = 2, 7, 11, 13
    x = K.spectrum(B, C, H, W).double()
    mask = K.mask_of(kind, B, H, W)
    xn = x.numpy()
    mean, cov, lam, comp = K.np_pca(xn, mask, normalize, stride, 1, 3)
    pca = FeaturePCATorch(C, normalize=normalize, sample_stride=stride).update(x, mask).fit().check()
    m, c, n = pca.covariance()
    assert int(n) == int(K.np_fit_set(B, H, W, mask, stride).sum())
    _close(m, mean, "mean")
    _close(c, cov, "cov")
    _close(pca.mean_, mean, "mean_")
    _close(pca.explained_variance_, lam, "eigenvalues", scale=lam[0])
    _close(pca.components_, comp, "components", scale=1.0)
    # two updates accumulate to the same moments as one (the shift is the first call's)
    two = FeaturePCATorch(C, normalize=normalize, sample_stride=stride)
    two.update(x[:1], mask if kind != "bhw" else mask[:1]).update(x[1:], mask if kind != "bhw" else mask[1:])
    _close(two.covariance()[1], cov, "cov of two updates")
    # projection, ranges and colours with the twin's own components
    cn, mn = pca.components_.numpy(), pca.mean_.numpy()
    t, tmin, tmax = pca.transform(x, mask, return_range=True)
    t_np = K.np_project(xn, cn, mn, mask, normalize)
    tscale = float(np.abs(t_np).max())
    _close(t, t_np, "t")
    lo_np, hi_np = K.np_range(t_np, mask)
    _close(tmin, lo_np, "tmin", scale=tscale)
    _close(tmax, hi_np, "tmax", scale=tscale)
    lo1, hi1 = lo_np.min(axis=1, keepdims=True), hi_np.max(axis=1, keepdims=True)
    v_np = K.np_colour(t_np, lo1, hi1, mask)
    vf, lo, hi = pca.colourise(x, mask, "minmax", torch.float32, return_range=True)
    _close(lo, np.broadcast_to(lo1, (B, 3)), "lo", scale=tscale)
    _close(hi, np.broadcast_to(hi1, (B, 3)), "hi", scale=tscale)
    assert vf.dtype == torch.float32 and vf.shape == (B, 3, H, W)
    assert np.abs(vf.numpy() - v_np).max() <= 2.0 ** -24 + RTOL
    img = pca.colourise(x, mask, "minmax", torch.uint8)
    assert img.dtype == torch.uint8 and img.shape == (B, H, W, 3)
    share = K.check_uint8(img.numpy(), v_np, np.full((B, 3), 1e-9 / 255), K.np_part(B, H, W, mask))
    # by construction every image's minimum and maximum sit on the integers 0 and 255: two pairs an image
    assert share * 3 * K.np_part(B, H, W, mask).sum() <= 2 * B + 0.5
    if mask is not None:
        off = np.broadcast_to((mask.numpy() == 0).reshape(-1, H, W), (B, H, W))
        assert not img.numpy()[off].any() and not t.numpy().transpose(0, 2, 3, 1)[off].any()
    # an explicit pair is the same formula
    pair = pca.colourise(x, mask, (lo[:, :1], hi), torch.float32)
    assert torch.equal(pair, vf)
    if kind == "none":
        u_np = (t_np - lo_np[:, :, None, None]).reshape(B * 3, H * W)
        qlo, qhi = K.np_quantile(u_np, 0.01).reshape(B, 3), K.np_quantile(u_np, 0.99).reshape(B, 3)
        vq, lo, hi = pca.colourise(x, None, "quantile", torch.float32, return_range=True)
        _close(lo, qlo, "quantile lo", scale=tscale)
        _close(hi, qhi, "quantile hi", scale=tscale)
        want = K.np_colour(u_np.reshape(B, 3, H, W), qlo, qhi, None, clamp=True)
        assert np.abs(vq.numpy() - want).max() <= 2.0 ** -24 + 10 * RTOL
        assert float(vq.min()) == 0.0 and float(vq.max()) == 1.0


def test_twin_against_sklearn():
    skd = pytest.importorskip("sklearn.decomposition")
    B, C, H, W = 2, 7, 11, 13
    x = K.spectrum(B, C, H, W).double()
    mask = K.mask_of("bhw", B, H, W)
    X = K.np_samples(x.numpy(), mask, False, 1)
    sk = skd.PCA(3, svd_solver="full").fit(X)
    pca = FeaturePCATorch(C).update(x, mask).fit().check()
    err = float(np.abs(pca.components_.numpy() - sk.components_).max())
    print(f"components against sklearn: max error {err:.3e}")
    assert err <= 1e-8
    assert np.abs(pca.explained_variance_.numpy()[:3] - sk.explained_variance_).max() <= 1e-8 * sk.explained_variance_[0]
    assert np.abs(pca.mean_.numpy() - sk.mean_).max() <= 1e-10
    t = pca.transform(x, mask).numpy().transpose(0, 2, 3, 1).reshape(-1, 3)[K.np_part(B, H, W, mask).reshape(-1)]
    assert np.abs(t - sk.transform(X)).max() <= 1e-8 * np.abs(t).max()


def _eig_host(A):
    L = _lib.load()
    C = A.shape[0]
    A = np.ascontiguousarray(A, np.float64)
    lam, vec = np.empty(C), np.empty((C, C))
    sweeps, rot = ctypes.c_int32(-1), ctypes.c_int64(-1)
    st = L.gs_feature_pca_eig_host(C, A.ctypes.data, lam.ctypes.data, vec.ctypes.data, ctypes.byref(sweeps), ctypes.byref(rot))
    return st, lam, vec, sweeps.value, rot.value


def _eig_cases():
    for C in (1, 2, 3, 31, 32, 33, 64, 128):
        rng = np.random.default_rng(C)
        X = rng.standard_normal((C, C + 3))
        yield f"random{C}", X @ X.T - 0.5 * np.eye(C)
    Q = np.linalg.qr(np.random.default_rng(5).standard_normal((12, 12)))[0]
    yield "repeated", (Q * np.array([3.0] * 5 + [1.0] * 4 + [-2.0] * 3)) @ Q.T
    yield "diagonal", np.diag(np.array([4.0, -1.0, 4.0, 0.0, 2.5, 2.5, 7.0]))
    yield "zero", np.zeros((5, 5))


@pytest.mark.parametrize("name,A", list(_eig_cases()), ids=[n for n, _ in _eig_cases()])
def test_host_eigensolver(name, A):
    """The three checks with S the sweep cap: each rotation is orthogonal to a few ulps and a sweep
    has fewer than C^2 of them on C-vectors, so S sweeps stay within S * C * 2^-52."""
    A = (A + A.T) / 2
    C, S = A.shape[0], _lib.load().gs_feature_pca_max_sweeps()
    assert S == _lib.FPCA_MAX_SWEEPS
    st, lam, vec, sweeps, rot = _eig_host(A)
    assert st == 0 and 0 <= sweeps <= S and 0 <= rot < max(sweeps, 1) * C * C
    V, nA, b = vec.T, np.linalg.norm(A), S * C * 2.0 ** -52
    res, orth = np.linalg.norm(A @ V - V * lam), np.linalg.norm(V.T @ V - np.eye(C))
    ev = np.abs(lam - np.linalg.eigvalsh(A)[::-1]).max()
    print(f"{name}: {sweeps} sweeps, {rot} rotations; residual / bound {res / (b * nA) if nA else 0.0:.3e}, "
          f"orthogonality / bound {orth / b:.3e}, eigenvalues / bound {ev / (b * nA) if nA else 0.0:.3e}")
    assert res <= b * nA and orth <= b and ev <= b * nA
    assert np.all(np.diff(lam) <= 0)
    assert np.array_equal(K.np_sign_rule(vec), vec)  # the sign rule holds on every component
    if name == "diagonal":  # ties by index: the permutation is the stable descending sort
        assert np.array_equal(lam, np.array([7.0, 4.0, 4.0, 2.5, 2.5, 0.0, -1.0]))
        assert np.array_equal(vec.argmax(axis=1), np.array([6, 0, 2, 4, 5, 3, 1])) and sweeps == 0


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), 1e200])
def test_host_eigensolver_gives_non_finite_input_a_status(bad):
    """A NaN or infinite entry, or one whose square overflows: status 3, zeros, nothing rotated."""
    A = np.diag(np.arange(1.0, 6.0))
    A[1, 3] = A[3, 1] = bad
    st, lam, vec, sweeps, rot = _eig_host(A)
    assert st == 3 and sweeps == 0 and rot == 0 and not lam.any() and not vec.any()


def test_validator_and_host_eigensolver_are_sanitizer_clean(tmp_path):
    """gs_feature_pca_host.cpp (with gs_host.cpp's error state) under ASan + UBSan in a plain CPU
    executable with its own main: nothing preloaded, nothing loaded into Python."""
    run_host_sanitizer(tmp_path, "feature_pca_host_sanitize.c", ["gs_feature_pca_host.cpp", "gs_host.cpp"],
                       "feature pca host sanitize ok")


def test_build_lists_the_new_sources():
    assert build.SOURCES["gs_feature_pca.hip"] == ["-ffp-contract=off"]
    assert "gs_feature_pca_host.cpp" in build.SOURCES
    for f in ("gs_feature_pca.hip", "gs_feature_pca_host.cpp", "gs_feature_pca_layout.h", "gs_sym_eig.h"):
        assert os.path.exists(os.path.join(build.CSRC, f))
    with open(os.path.join(build.CSRC, "gs_feature_pca.hip")) as fh:
        text = fh.read()
    assert '#include "gs_split_mfma.h"' in text and '#include "gs_sym_eig.h"' in text
    assert "asm" not in text and "atomic" not in text.replace("No atomics", "")


def test_ctypes_mirror_and_documented_constants():
    L = _lib.load()
    assert ctypes.sizeof(_lib.GsFeaturePca) == L.gs_feature_pca_struct_bytes()
    with open(os.path.join(REPO, "include", "gs_feature_pca.h")) as fh:
        header = fh.read()
    for name, value in (("GS_FPCA_MAX_C", _lib.FPCA_MAX_C), ("GS_FPCA_MAX_K", _lib.FPCA_MAX_K),
                        ("GS_FPCA_MAX_SWEEPS", _lib.FPCA_MAX_SWEEPS), ("GS_FPCA_TILE_PIXELS", _lib.FPCA_TILE_PIXELS),
                        ("GS_FPCA_CHUNK", _lib.FPCA_CHUNK), ("GS_FPCA_SLAB_GROUP", _lib.FPCA_SLAB_GROUP),
                        ("GS_FPCA_LDS_MAX_C", _lib.FPCA_LDS_MAX_C), ("GS_FPCA_PASS_UPDATE", 0),
                        ("GS_FPCA_PASS_COVARIANCE", 1), ("GS_FPCA_PASS_FIT", 2), ("GS_FPCA_PASS_PROJECT", 3),
                        ("GS_FPCA_PASS_OFFSET", 4), ("GS_FPCA_PASS_COLOUR", 5)):
        assert f"#define {name} {value}\n" in header or f"#define {name} {value} " in header, name
    assert L.gs_feature_pca_max_sweeps() == _lib.FPCA_MAX_SWEEPS
    for B, H, W in ((1, 1, 1), (3, 72, 128), (27, 800, 800), (1, 12, 31)):
        assert L.gs_feature_pca_n_acc(B, H, W) == min(_lib.FPCA_CHUNK, -(-H * W // 128) * 128)
    # the LDS of one compute unit holds both fp64 matrices up to the documented order only
    assert 2 * _lib.FPCA_LDS_MAX_C * (_lib.FPCA_LDS_MAX_C + 1) * 8 <= 160 << 10 < 2 * _lib.FPCA_MAX_C ** 2 * 8
    assert L.gs_feature_pca_workspace_bytes(1, 64, 1, 1, 3, _lib.FPCA_PASS_FIT) == 0
    assert L.gs_feature_pca_workspace_bytes(1, 128, 1, 1, 3, _lib.FPCA_PASS_FIT) == 2 * 128 * 129 * 8


def _block(**kw):
    buf = ctypes.create_string_buffer(4096)
    base = ctypes.addressof(buf) // 16 * 16 + 16
    a = _lib.GsFeaturePca(B=2, C=8, H=4, W=5, k=3, sample_stride=1, ddof=1, out_uint8=1, workspace=base,
                          workspace_bytes=1 << 30)
    for name, _ in _lib.GsFeaturePca._fields_[12:-2]:
        setattr(a, name, base)
    for name, v in kw.items():
        setattr(a, name, v)
    a._keep = buf
    return a


@pytest.mark.parametrize("field,value,which,message", [
    ("C", 0, 0, "C must be in"), ("C", 129, 0, "_torch"), ("C", 129, 2, "C must be in"), ("B", 0, 3, "B must be in"),
    ("H", 0, 0, "H, W must be"), ("W", 0, 5, "H, W must be"), ("k", 0, 2, "k must be in"), ("k", 9, 3, "k must be in"),
    ("k", 2, 5, "colour needs k = 3"), ("sample_stride", 0, 0, "sample_stride"), ("ddof", -1, 1, "ddof"),
    ("x", None, 0, "x is required"), ("x", None, 3, "x is required"), ("state", None, 0, "state is required"),
    ("shift", None, 2, "shift is required"), ("cov", None, 1, "cov is required"), ("status", None, 2, "status is required"),
    ("proj_components", None, 3, "proj_components"), ("t", None, 3, "t is required"), ("t", None, 5, "t is required"),
    ("sub", None, 4, "sub is required"), ("lo", None, 5, "lo and hi"), ("out", None, 5, "out is required"),
    ("workspace", None, 0, "workspace is required"), ("workspace_bytes", 64, 0, "needed"),
])
def test_validator_refuses_with_a_message(field, value, which, message):
    L = _lib.load()
    for p in range(6):
        assert L.gs_feature_pca_validate(ctypes.byref(_block()), p) == 0, L.gs_last_error().decode()
    assert L.gs_feature_pca_validate(ctypes.byref(_block(**{field: value})), which) != 0
    assert message in L.gs_last_error().decode()
    assert L.gs_feature_pca_validate(None, 0) != 0 and "null argument block" in L.gs_last_error().decode()
    assert L.gs_feature_pca_validate(ctypes.byref(_block()), 6) != 0 and "unknown pass" in L.gs_last_error().decode()


def test_argument_checks_of_both_paths():
    x = K.spectrum(2, 7, 11, 13)
    V, mu = torch.eye(3, 7), torch.zeros(7)
    t = torch.zeros(2, 3, 11, 13)
    fitted = FeaturePCATorch(7).update(x).fit()
    for cls in (FeaturePCA, FeaturePCATorch):
        for call in (lambda: cls(0), lambda: cls(7, n_components=9), lambda: cls(2, n_components=3),
                     lambda: cls(7, sample_stride=0), lambda: cls(7, ddof=-1), lambda: cls(7).covariance(),
                     lambda: cls(7).fit(), lambda: cls(7).transform(x), lambda: cls(7).check(),
                     lambda: cls(7).update(x[0, 0]), lambda: cls(7).update(x[:, :5]), lambda: cls(8).update(x),
                     lambda: cls(7).update(x, mask=torch.ones(13, 11)), lambda: cls(7).update(x, shift=torch.zeros(6))):
            with pytest.raises(GsplatError):
                call()
    with pytest.raises(GsplatError, match="128"):
        FeaturePCA(129)
    assert FeaturePCATorch(129).C == 129  # the twins take any size
    for project in (pca_project, pca_project_torch):
        for call in (lambda: project(x[0, 0], V, mu), lambda: project(x, V[:, :6], mu), lambda: project(x, V, mu[:6]),
                     lambda: project(x, torch.zeros(9, 7), mu), lambda: project(x, V[0], mu),
                     lambda: project(x, V, mu, mask=torch.ones(2, 13, 11))):
            with pytest.raises(GsplatError):
                call()
    for colour in (pca_colour, pca_colour_torch):
        for call in (lambda: colour(t[:, :2], 0.0, 1.0), lambda: colour(t[0, 0], 0.0, 1.0),
                     lambda: colour(t, 0.0, 1.0, out=torch.float64), lambda: colour(t, torch.zeros(5), 1.0),
                     lambda: colour(t, 0.0, 1.0, mask=torch.ones(13, 11))):
            with pytest.raises(GsplatError):
                call()
    for call in (lambda: fitted.colourise(x, torch.ones(11, 13), "quantile"), lambda: fitted.colourise(x, None, "quantile", q=(0.1, 1.5)),
                 lambda: fitted.colourise(x, None, "quantile", q=(-0.1, 0.9)), lambda: fitted.colourise(x, None, "quantile", q=0.5),
                 lambda: fitted.colourise(x, None, "median"), lambda: fitted.colourise(x, None, (0.0,)),
                 lambda: fitted.colourise(x, None, "minmax", torch.int32),
                 lambda: FeaturePCATorch(7, n_components=2).update(x).fit().colourise(x),
                 lambda: fit_sequence_torch([]), lambda: fit_sequence_torch([x, x], [None])):
        with pytest.raises(GsplatError):
            call()
    with pytest.raises(GsplatError, match="mask=None"):
        fitted.colourise(x, torch.ones(11, 13), "quantile")
    # the HIP path has no CPU fallback: host tensors raise and name the twins
    for call in (lambda: FeaturePCA(7).update(x), lambda: pca_project(x, V, mu), lambda: pca_colour(t, 0.0, 1.0),
                 lambda: feature_map(x[0]), lambda: fit_sequence([x]), lambda: feature_map(x[0], feature_map_pca(7))):
        with pytest.raises(GsplatError, match="_torch"):
            call()


def test_status_and_degenerate_inputs_of_the_twin():
    x = K.spectrum(1, 3, 1, 1)
    pca = FeaturePCATorch(3).update(x).fit()  # one sample, ddof 1
    assert int(pca.status) == 1 and not pca.components_.any() and not torch.isnan(pca.components_).any()
    with pytest.raises(GsplatError, match="status 1"):
        pca.check()
    with pytest.raises(GsplatError, match="first update only"):  # one object, one shift
        FeaturePCATorch(3).update(K.spectrum(1, 3, 4, 5)).update(K.spectrum(1, 3, 4, 5), shift=torch.zeros(3))
    bad = K.spectrum(1, 3, 4, 5).clone()
    bad[0, 1, 2, 3] = float("nan")
    pca = FeaturePCATorch(3).update(bad).fit()  # a status of its own, zeros and no NaN
    assert int(pca.status) == 3 and not pca.components_.any() and not torch.isnan(pca.eigenvectors_).any()
    with pytest.raises(GsplatError, match="status 3"):
        pca.check()
    mask = torch.ones(4, 5)
    mask[2, 3] = 0
    assert int(FeaturePCATorch(3).update(bad, mask).fit().status) == 0
    const = torch.full((1, 3, 4, 5), 2.0)
    pca = FeaturePCATorch(3).update(const).fit().check()  # a zero covariance: every projection is 0
    for how in ("minmax", "quantile", (1.5, 1.5)):
        img = pca.colourise(const, None, how, torch.float32)
        assert not img.any() and not torch.isnan(img).any()  # hi == lo


def test_feature_map_and_fit_sequence_are_their_compositions():
    frames = [K.spectrum(1, 6, 9, 10, seed=s)[0].double() for s in range(3)]
    pca = fit_sequence_torch(frames, normalize=True)
    step = FeaturePCATorch(6, normalize=True)
    for f in frames:
        step.update(f)
    step.fit()
    assert torch.equal(pca.components_, step.components_) and torch.equal(pca.mean_, step.mean_)
    holder = feature_map_pca(6, torch_twin=True)
    first = feature_map_torch(frames[0], holder)
    ref = FeaturePCATorch(6, normalize=True, sample_stride=3).update(frames[0]).fit()
    assert torch.equal(first, ref.colourise(frames[0], None, "quantile", torch.float32))
    assert first.shape == (3, 9, 10) and first.dtype == torch.float32
    second = feature_map_torch(frames[1], holder)  # frozen by the first call
    assert torch.equal(holder.components_, ref.components_)
    assert torch.equal(second, ref.colourise(frames[1], None, "quantile", torch.float32))
    assert not torch.equal(feature_map_torch(frames[1]), second)  # without a holder every call fits its own


@pytest.mark.parametrize("normalize", [False, True], ids=["raw", "normalized"])
@pytest.mark.parametrize("shape", [s for s in K.SHAPES if s[1] >= 3], ids=K.shape_id)
def test_uint8_decisions_of_the_gpu_cases_stay_under_the_excluded_share(shape, normalize):
    """The GPU test excludes a uint8 comparison where 255 v is within 255 * bound of an integer and
    asserts that share <= 5 %: here, on the CPU, the float32 twin against the float64 one on the
    same inputs and with the same bounds, for every GPU shape that has colours (C >= 3), both
    ranges.  The masks only remove pixels of the same distribution, and the GPU test asserts its
    own share in every masked case."""
    B, C, H, W = shape
    x32 = K.spectrum(*shape)
    x64 = x32.double().numpy()
    p64 = FeaturePCATorch(C, normalize=normalize).update(x32.double()).fit()
    comp, mean = p64.components_.float(), p64.mean_.float()
    cn, mn = comp.double().numpy(), mean.double().numpy()
    t32, tmin, tmax = pca_project_torch(x32, comp, mean, None, normalize, return_range=True)
    E = K.projection_bound(K.np_xhat(x64, normalize), cn, mn, normalize)
    frac = float((np.abs(t32.numpy() - K.np_project(x64, cn, mn, None, normalize)) / E).max())
    part = K.np_part(B, H, W, None)
    lo, hi = tmin.amin(1, keepdim=True).double().numpy(), tmax.amax(1, keepdim=True).double().numpy()
    share = K.check_uint8(pca_colour_torch(t32, lo, hi).numpy(), K.np_colour(t32.numpy(), lo, hi, None),
                          K.colour_bound(E, lo, hi, shared=True), part)
    u = t32 - tmin[:, :, None, None]
    planes = u.reshape(B * 3, H * W)
    qlo = plane_quantile_torch(planes, 0.01).reshape(B, 3).numpy()
    qhi = plane_quantile_torch(planes, 0.99).reshape(B, 3).numpy()
    qshare = K.check_uint8(pca_colour_torch(u, qlo, qhi, clamp=True).numpy(), K.np_colour(u.numpy(), qlo, qhi, None),
                           K.colour_bound(E, qlo, qhi, shared=False), part)
    print(f"{K.shape_id(shape)} normalize={normalize}: projection error / bound {frac:.3f}, excluded share "
          f"{share:.4f} (min / max), {qshare:.4f} (quantile)")
    assert frac <= 1.0 and share <= 0.05 and qshare <= 0.05


def test_check_uint8_counts_clamped_pixels_as_decided():
    v = np.array([-0.5, -1e-9, 0.0, 0.3, 1.0, 1.0 + 1e-9, 1.5]).reshape(1, 1, 1, 7).repeat(3, axis=1)
    img = np.floor(np.clip(v, 0, 1) * 255).astype(np.uint8).transpose(0, 2, 3, 1)
    part = np.ones((1, 7), bool)
    # -0.5 and 1.5 are decided; the four values within the bound of 0 or 1 are not; 0.3 is decided
    assert K.check_uint8(img, v, np.full((1, 3), 1e-6), part) == pytest.approx(4 / 7)
    wrong = img.copy()
    wrong[0, 0, 0, 0] = 1  # a clamped pixel is compared exactly
    with pytest.raises(AssertionError):
        K.check_uint8(wrong, v, np.full((1, 3), 1e-6), part)


def test_range_twin_of_an_empty_mask():
    t = torch.randn(2, 3, 4, 5)
    mask = torch.zeros(2, 4, 5)
    mask[1, 2, 3] = 1
    lo, hi = pca_range_torch(t, mask)
    assert not lo[0].any() and not hi[0].any() and torch.equal(lo[1], t[1, :, 2, 3]) and torch.equal(hi[1], t[1, :, 2, 3])
    assert fp.STATUS[0] == "ok"
