"""CPU tests of the motion-basis initialisation (no GPU needed):
  * the _torch twins against independent statements: kmeans_torch against scikit-learn's Lloyd
    (when it is installed), solve_procrustes_bases_torch against an SVD Kabsch with the
    determinant fix written here, cluster_medians_torch against torch.median per cluster;
  * the Procrustes walk: recovery of known SE(3) trajectories, det R = +1 under mirrored noise,
    the skip / copy rule, the visiting order, the quaternion double cover, labels of -1, T = 1;
  * the host layer: the validators refuse bad arguments (also under ASan + UBSan in a stand-alone
    program, tools/motion_init_host_sanitize.c), build.SOURCES lists the new files, the ctypes
    mirrors have the library's sizes and the header's fields.

Parity unpinned: dyn_som.py is a fragment that cannot be imported, so there is no golden record;
the twins are the specification.

Bounds.  Everything here is fp64 on the CPU.  Two fp64 routes to the same optimum (Horn's
eigenvector, the SVD) differ by the conditioning of the eigenvector, at most 1e3 here, times
2^-53: 1e-10 is generous and still 1e3 below the fp32 envelope the GPU tests apply.
"""
import ctypes
import math
import os
import re
import shutil

import numpy as np
import pytest
import torch

import dynamic3dgaussians_amd as pkg
from dynamic3dgaussians_amd import _lib, build, motion_init as mi
from dynamic3dgaussians_amd.motion import MotionBases, cont_6d_to_rmat
from tests import _motion_init_cases as C
from tests._harness import run_host_sanitizer

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-10
MIRRORS = {"gs_kmeans_assign": _lib.GsKmeansAssign, "gs_kmeans_update": _lib.GsKmeansUpdate,
           "gs_coefs_from_centers": _lib.GsCoefsFromCenters, "gs_procrustes": _lib.GsProcrustes}


# ---- the twins against independent statements

@pytest.mark.parametrize("name", ["km_257x3_k5_s0", "km_1000x24_k20_s0"])
def test_kmeans_twin_against_scikit_learn(name):
    """Neither case ends with an empty cluster (scikit-learn relocates those: the documented
    difference).  scikit-learn re-assigns once after its last update, the twin does not: its
    labels are compared with the assignment to the twin's final centres."""
    cluster = pytest.importorskip("sklearn.cluster")
    x, init, run, _ = C.kmeans_case(name)
    assert (run["counts"] > 0).all()
    km = cluster.KMeans(n_clusters=init.shape[0], init=init.double().numpy(), n_init=1, max_iter=C.ITERS, tol=0,
                        algorithm="lloyd").fit(x.double().numpy())
    ours = mi.kmeans_torch(x.double(), init=init.double(), iters=C.ITERS)
    assert torch.equal(ours.labels, run["labels"][-1]) and torch.equal(ours.moved, run["moved"])
    assert np.abs(km.cluster_centers_ - ours.centers.numpy()).max() < TOL
    final = mi.kmeans_assign_torch(x.double(), ours.centers)
    assert np.array_equal(km.labels_.astype(np.int64), final.numpy())
    assert torch.equal(ours.counts, torch.bincount(ours.labels, minlength=init.shape[0]))


def test_kmeans_twin_rules():
    x = torch.tensor([[0.0], [1.0], [2.0], [10.0]], dtype=torch.float64)
    c = torch.tensor([[1.0], [1.0], [50.0]], dtype=torch.float64)
    assert mi.kmeans_assign_torch(x, c).tolist() == [0, 0, 0, 0]  # ties go to the lowest k
    new, counts = mi.kmeans_update_torch(x, torch.tensor([0, 0, 2, -1]), c)
    assert counts.tolist() == [2, 0, 1] and new[:, 0].tolist() == [0.5, 1.0, 2.0]  # empty keeps its centre
    r = mi.kmeans(x, 2, iters=3, seed=4)
    rows = torch.randperm(4, generator=torch.Generator().manual_seed(4))[:2]
    assert torch.equal(mi.kmeans(x, 2, iters=0, seed=4).centers, x[rows])
    assert r.moved.shape == (3,) and r.moved[0] == 4 and r.labels.dtype == torch.int64
    with pytest.raises(ValueError, match="at least as many points"):
        mi.kmeans(x, 5)
    with pytest.raises(ValueError, match=r"in \[1, 64\]"):
        mi.kmeans(torch.zeros(100, 2), 65)
    with pytest.raises(ValueError, match="num_clusters or init"):
        mi.kmeans(x)
    empty = mi.kmeans(x[:0], 3, iters=2)
    assert empty.labels.shape == (0,) and empty.centers.shape == (3, 1) and empty.counts.tolist() == [0, 0, 0]
    valid = torch.tensor([True, False, True, True])
    m = mi.kmeans(x, init=x[[0, 3]], iters=2, valid=valid)
    assert m.labels.tolist() == [0, -1, 0, 1] and m.counts.tolist() == [2, 1] and m.moved.tolist() == [3, 0]
    v = mi.velocity_directions(torch.tensor([[[0.0, 0, 0], [3.0, 4, 0], [3.0, 4, 0]]], dtype=torch.float64))
    assert v.shape == (1, 6) and abs(v[0, 0] - 3 / (5 + 1e-5)) < 1e-15 and not v[0, 3:].any()


def test_cluster_medians_twin_against_torch_median():
    gen = torch.Generator().manual_seed(2)
    for dtype in (torch.float64, torch.float32):
        pts = torch.randn(1001, 3, generator=gen, dtype=dtype)
        labels = torch.randint(0, 4, (1001,), generator=gen)
        labels[labels == 2] = 0
        labels[:1] = 5
        labels[1:11] = 4
        labels[11:20] = -1
        got = mi.cluster_medians_torch(pts, labels, 6)
        for k in (0, 1, 3, 4, 5):
            assert torch.equal(got[k], pts[labels == k].median(dim=0).values), k  # bit for bit
        assert torch.isnan(got[2]).all() and (labels == 4).sum() % 2 == 0 and (labels == 5).sum() == 1
    assert torch.isnan(mi.cluster_medians_torch(torch.zeros(0, 3), torch.zeros(0, dtype=torch.int64), 2)).all()


def test_coefs_twin():
    means = torch.tensor([[0.0, 0, 0], [3.0, 4, 0]], dtype=torch.float64)
    got = mi.coefs_from_centers(means, torch.tensor([[0.0, 0, 0]], dtype=torch.float64))
    assert got.shape == (2, 1) and got[0, 0] == 10 and abs(got[1, 0] - 10 * math.exp(-5)) < 1e-15


def _kabsch(src, tgt, w):
    """The weighted SVD solution with the determinant fix: (R, t, err_after, err_before)."""
    cs, cg = (w[:, None] * src).sum(0) / w.sum(), (w[:, None] * tgt).sum(0) / w.sum()
    H = ((src - cs) * w[:, None]).T @ (tgt - cg)
    U, _, Vt = torch.linalg.svd(H)
    d = torch.sign(torch.linalg.det(Vt.T @ U.T))
    R = Vt.T @ torch.diag(torch.tensor([1.0, 1.0, d], dtype=src.dtype)) @ U.T
    t = cg - R @ cs
    ea = torch.sqrt((w * ((src @ R.T + t - tgt) ** 2).sum(-1)).sum() / w.sum())
    eb = torch.sqrt((w * ((src - tgt) ** 2).sum(-1)).sum() / w.sum())
    return R, t, ea, eb


def test_procrustes_twin_against_an_svd_kabsch():
    p = C.procrustes_case()
    out = mi.solve_procrustes_bases_torch(p["tracks"], p["labels"], p["K"], p["cano_t"], visibles=p["visibles"],
                                          confidences=p["confidences"],
                                          min_mean_weight=C.PROCRUSTES_MIN_MEAN_WEIGHT)
    vis, conf, c = p["visibles"].double(), p["confidences"].double(), p["cano_t"]
    R_all = cont_6d_to_rmat(out.rots)
    assert out.skipped.sum() == 1 and out.skipped[C.PROCRUSTES_SKIP]
    for k in C.PROCRUSTES_FULL_RANK:
        m = p["labels"] == k
        for t in range(p["tracks"].shape[1]):
            if out.skipped[k, t]:
                continue
            w = vis[m, c] * vis[m, t] * (conf[m, c] + conf[m, t]) / 2
            R, tr, ea, eb = _kabsch(p["tracks"][m, c], p["tracks"][m, t], w)
            assert (R_all[k, t] - R).abs().max() < TOL and (out.transls[k, t] - tr).abs().max() < TOL
            assert abs(out.err_after[k, t] - ea) < TOL and abs(out.err_before[k, t] - eb) < TOL
            Rp, tp = p["poses"][k, t]
            assert (R - Rp).abs().max() < 5e-3 and ea < 0.03  # and both are the pose behind the noise


# ---- the Procrustes walk

def _rigid_tracks(poses, pts):
    return torch.stack([pts @ R.T + t for R, t in poses], 1)


def test_noise_free_recovery_quaternions_past_180_degrees_and_the_double_cover():
    gen = torch.Generator().manual_seed(1)
    pts = torch.randn(50, 3, generator=gen, dtype=torch.float64)
    T = 13
    poses = [(C.rotation((0.3, 1.0, -0.2), 0.6 * t), torch.tensor([0.1 * t, -0.2 * t, 0.05 * t * t], dtype=torch.float64))
             for t in range(T)]  # 7.2 rad in all: past 180 and past 360 degrees
    tracks = _rigid_tracks(poses, pts)
    labels = torch.zeros(50, dtype=torch.int64)
    out = mi.solve_procrustes_bases_torch(tracks, labels, 1, 0, rot_type="quat")
    R = mi._quat_to_rmat(out.rots[0])
    for t in range(T):
        assert (R[t] - poses[t][0]).abs().max() < TOL and (out.transls[0, t] - poses[t][1]).abs().max() < TOL
    assert out.err_after.max() < 1e-12 and not out.skipped.any()
    assert abs(out.err_before[0, 1] - (tracks[:, 0] - tracks[:, 1]).norm(dim=-1).pow(2).mean().sqrt()) < 1e-12
    q = out.rots[0]
    assert torch.all((q[1:] * q[:-1]).sum(-1) >= 0) and q[0].tolist() == [1.0, 0.0, 0.0, 0.0]
    assert q[:, 0].min() < -0.5  # the cover really is followed past w = 0: no snap back to w >= 0
    six = mi.solve_procrustes_bases(tracks, labels, 1, 0)  # the default: 6-D, what MotionBases takes
    assert six.rots.shape == (1, T, 6) and (cont_6d_to_rmat(six.rots)[0] - R).abs().max() < TOL
    assert six.rots[0, 0].tolist() == [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]


def test_near_planar_cluster_with_mirrored_noise_keeps_det_plus_one():
    gen = torch.Generator().manual_seed(3)
    pts = torch.randn(200, 3, generator=gen, dtype=torch.float64)
    pts[:, 2] *= 1e-3
    R0 = C.rotation((1.0, 2.0, 0.5), 0.7)
    tgt = pts @ R0.T
    tgt = tgt - 2 * (tgt @ R0[:, 2])[:, None] * R0[:, 2]  # the thin axis mirrored: the best orthogonal map reflects
    tracks = torch.stack([pts, tgt], 1)
    out = mi.solve_procrustes_bases_torch(tracks, torch.zeros(200, dtype=torch.int64), 1, 0)
    R = cont_6d_to_rmat(out.rots)[0, 1]
    raw = torch.stack([out.rots[0, 1, :3], out.rots[0, 1, 3:]], -1)
    assert (raw.T @ raw - torch.eye(2, dtype=torch.float64)).abs().max() < 1e-12
    assert abs(torch.linalg.det(R) - 1) < 1e-12
    Rk = _kabsch(pts, tgt, torch.ones(200, dtype=torch.float64))[0]
    assert (R - Rk).abs().max() < TOL and (R - R0).abs().max() < 1e-3  # the proper optimum, next to R0


def test_skip_copy_rule_visiting_order_and_ignored_labels():
    gen = torch.Generator().manual_seed(5)
    N, T, cano = 60, 7, 3
    pts = torch.randn(N, 3, generator=gen, dtype=torch.float64)
    poses = [(C.rotation((0.0, 0.0, 1.0), 0.3 * (t - cano)), torch.tensor([0.5 * (t - cano), 0.0, 0.0], dtype=torch.float64))
             for t in range(T)]
    tracks = _rigid_tracks(poses, pts)
    labels = torch.zeros(N, dtype=torch.int64)
    labels[40:] = -1
    tracks[40:] = torch.randn(20, T, 3, generator=gen, dtype=torch.float64)  # ignored, or they would spoil the fit
    vis = torch.ones(N, T, dtype=torch.bool)
    vis[:, 1] = False  # frame 1 (visited after 2): copies frame 2
    vis[:, 5] = False  # frame 5 (visited after 4): copies frame 4
    out = mi.solve_procrustes_bases_torch(tracks, labels, 2, cano, visibles=vis)  # basis 1 has no point at all
    assert out.skipped[0].tolist() == [False, True, False, False, False, True, False]
    assert out.skipped[1].all() and torch.all(out.err_after[1] == -1)
    assert torch.equal(out.rots[1], torch.tensor([1.0, 0, 0, 0, 1, 0], dtype=torch.float64).expand(T, 6))
    assert torch.equal(out.rots[0, 1], out.rots[0, 2]) and torch.equal(out.transls[0, 1], out.transls[0, 2])
    assert torch.equal(out.rots[0, 5], out.rots[0, 4]) and torch.equal(out.transls[0, 5], out.transls[0, 4])
    assert out.err_after[0, 1] == -1 and out.err_before[0, 5] == -1 and out.err_after[0].max() < 1e-12
    R = cont_6d_to_rmat(out.rots[0])
    for t in (0, 2, 3, 4, 6):
        assert (R[t] - poses[t][0]).abs().max() < TOL
    # the canonical frame itself under the threshold: it is visited after frame 0 and copies frame 0
    vis = torch.ones(N, T, dtype=torch.bool)
    conf = torch.ones(N, T, dtype=torch.float64)
    conf[:, cano] = 1e-3  # w = (1e-3 + 1) / 2 elsewhere, 1e-3 at the canonical frame: 40 x 1e-3 < 0.1 x 7
    out = mi.solve_procrustes_bases_torch(tracks, labels, 1, cano, visibles=vis, confidences=conf)
    assert out.skipped[0].tolist() == [False, False, False, True, False, False, False]
    assert torch.equal(out.rots[0, cano], out.rots[0, 0]) and torch.equal(out.transls[0, cano], out.transls[0, 0])
    assert (cont_6d_to_rmat(out.rots[0, 0]) - poses[0][0]).abs().max() < TOL
    # explicit weights replace the visibilities
    w = torch.ones(N, T, dtype=torch.float64)
    w[:, 6] = 0.0
    out = mi.solve_procrustes_bases_torch(tracks, labels, 1, cano, visibles=vis, weights=w)
    assert out.skipped[0].tolist() == [False] * 6 + [True] and torch.equal(out.rots[0, 6], out.rots[0, 5])


def test_one_frame_and_argument_errors():
    pts = torch.randn(10, 1, 3, dtype=torch.float64)
    out = mi.solve_procrustes_bases_torch(pts, torch.zeros(10, dtype=torch.int64), 1, 0, rot_type="quat")
    assert out.rots.shape == (1, 1, 4) and (out.rots[0, 0] - torch.tensor([1.0, 0, 0, 0])).abs().max() < 1e-12
    assert out.transls.abs().max() < 1e-12 and out.err_before[0, 0] == 0 and not out.skipped.any()
    lab = torch.zeros(10, dtype=torch.int64)
    with pytest.raises(ValueError, match="cano_t"):
        mi.solve_procrustes_bases(pts, lab, 1, 1)
    with pytest.raises(ValueError, match="num_bases"):
        mi.solve_procrustes_bases(pts, lab, 65, 0)
    with pytest.raises(ValueError, match="rot_type"):
        mi.solve_procrustes_bases(pts, lab, 1, 0, rot_type="euler")
    with pytest.raises(ValueError, match="visibles must be"):
        mi.solve_procrustes_bases(pts, lab, 1, 0, visibles=torch.ones(10, 2, dtype=torch.bool))
    with pytest.raises(ValueError, match="int64"):
        mi.solve_procrustes_bases(pts, lab.int(), 1, 0)


def test_composed_calls_on_the_twins():
    case = C.bodies_case()
    out = case["ref"]
    assert isinstance(out, mi.MotionInit) and isinstance(out.bases, MotionBases)
    assert out.motion_coefs.shape == (1200, 4) and out.labels.shape == (1200,) and out.centers.shape == (4, 3)
    assert out.valid_mask.sum() == 1140 and torch.all(out.labels[~out.valid_mask] == -1)
    pos = out.bases.compute_means(range(12), out.means_cano.float(), out.motion_coefs.float(), softmax=True)
    assert pos.shape == (1200, 12, 3) and torch.isfinite(pos).all()
    quat = mi.init_motion_bases_from_tracks(case["tracks"], num_bases=4, cano_t=3, seed=case["seed"], rot_type="quat")
    assert quat.bases is None and quat.procrustes.rots.shape == (4, 12, 4)
    with pytest.raises(ValueError, match="no cluster"):
        mi.init_motion_bases_from_tracks(case["tracks"], num_bases=4, cano_t=3, min_cluster_size=5000)
    dropped = mi.init_motion_bases_from_tracks(case["tracks"], num_bases=4, cano_t=3, seed=case["seed"],
                                               min_cluster_size=int(out.labels[out.labels >= 0].bincount().min()))
    assert dropped.centers.shape == (3, 3) and dropped.motion_coefs.shape == (1200, 3)
    assert (dropped.labels == -1).sum() > (out.labels == -1).sum() and dropped.labels.max() == 2
    means, feats, run = C.feature_case()
    bases, coefs, labels, centers = mi.init_motion_coefs_from_features(means.double(), feats.double(), 49, num_frames=5)
    assert torch.equal(labels, run["labels"][-1]) and coefs.shape == (4097, 49) and centers.shape == (49, 3)
    assert bases.params["rots"].shape == (49, 5, 6)


def test_package_exports_and_docs():
    for n in ("kmeans", "kmeans_assign", "kmeans_update", "cluster_medians", "coefs_from_centers",
              "solve_procrustes_bases"):
        assert getattr(pkg, n) is getattr(mi, n) and getattr(pkg, n + "_torch") is getattr(mi, n + "_torch"), n
    for n in ("velocity_directions", "init_motion_bases_from_tracks", "init_motion_coefs_from_features",
              "KMeansResult", "ProcrustesInit", "MotionInit"):
        assert getattr(pkg, n) is getattr(mi, n), n
    assert "Parity unpinned" in mi.__doc__
    assert "Parity unpinned" in open(os.path.join(REPO, "DESIGN.md")).read().split("### 9.16 ")[1]


# ---- the host layer

def test_build_lists_the_new_sources():
    assert build.SOURCES["gs_motion_init.hip"] == ["-ffp-contract=off"]
    assert "gs_motion_init_host.cpp" in build.SOURCES


def _header():
    txt = open(os.path.join(REPO, "include", "gs_motion_init.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_library_exports_every_symbol_of_the_header():
    L = _lib.load()
    names = sorted(set(re.findall(r"\b(gs_[a-z_0-9]+)\s*\(", _header())))
    want = {s + suffix for s in MIRRORS for suffix in ("", "_validate", "_struct_bytes")}
    assert set(names) == want | {"gs_kmeans_workspace_bytes", "gs_procrustes_workspace_bytes"}
    for n in names:
        assert hasattr(L, n) and n in _lib.PROTOTYPES, n
    assert L.gs_version() == _lib.ABI_VERSION  # a new header, no existing struct changed


@pytest.mark.parametrize("struct", tuple(MIRRORS))
def test_ctypes_mirrors_have_the_library_sizes_and_the_header_fields(struct):
    L = _lib.load()
    mirror = MIRRORS[struct]
    assert ctypes.sizeof(mirror) == getattr(L, struct + "_struct_bytes")()
    body = re.search(r"struct %s \{(.*?)\};" % struct, _header(), flags=re.S).group(1)
    names = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        names += [re.findall(r"[A-Za-z_]\w*", part)[-1] for part in decl.split(",")]
    assert [f for f, _ in mirror._fields_] == names


def _blocks(keep):
    L = _lib.load()
    N, D, K, T = 100, 40, 7, 9
    km, pr = L.gs_kmeans_workspace_bytes(N, K, D), L.gs_procrustes_workspace_bytes(K, T)
    bufs = {"f": np.zeros(N * max(D, T * 3), np.float32), "i": np.zeros(N + K + 1, np.int64),
            "u8": np.zeros(N + K * T, np.uint8), "ws": np.zeros(max(km, pr) // 4 + 64, np.float32)}
    keep.append(bufs)
    p = {k: v.ctypes.data for k, v in bufs.items()}
    p["ws"] = (p["ws"] + 255) // 256 * 256
    return {
        "gs_kmeans_assign": _lib.GsKmeansAssign(N=N, D=D, K=K, x=p["f"], centers=p["f"], labels=p["i"]),
        "gs_kmeans_update": _lib.GsKmeansUpdate(N=N, D=D, K=K, x=p["f"], labels=p["i"], centers=p["f"], counts=p["i"],
                                                workspace=p["ws"], workspace_bytes=km),
        "gs_coefs_from_centers": _lib.GsCoefsFromCenters(N=N, K=K, means=p["f"], centers=p["f"], coefs=p["f"]),
        "gs_procrustes": _lib.GsProcrustes(N=N, T=T, K=K, cano_t=4, rot_dim=6, min_weight_sum=0.9, tracks=p["f"],
                                           order=p["i"], offsets=p["i"], rots=p["f"], transls=p["f"],
                                           err_after=p["f"], err_before=p["f"], skipped=p["u8"], workspace=p["ws"],
                                           workspace_bytes=pr),
    }


BAD = {
    "gs_kmeans_assign": [("K", 65, b"K must be"), ("K", 0, b"K must be"), ("D", 0, b"D must be"), ("N", -1, b"N must be"),
                         ("x", None, b"x is required"), ("centers", None, b"centers are required"),
                         ("labels", None, b"labels are required")],
    "gs_kmeans_update": [("K", 65, b"K must be"), ("D", -1, b"D must be"), ("x", None, b"x and labels"),
                         ("labels", None, b"x and labels"), ("centers", None, b"centers are required"),
                         ("counts", None, b"counts are required"), ("workspace", None, b"workspace is required"),
                         ("workspace_bytes", 8, b"needed")],
    "gs_coefs_from_centers": [("K", 0, b"K must be"), ("N", -1, b"N must be"), ("means", None, b"means and coefs"),
                              ("coefs", None, b"means and coefs"), ("centers", None, b"centers are required")],
    "gs_procrustes": [("K", 65, b"K must be"), ("K", 0, b"K must be"), ("T", 0, b"T must be"), ("cano_t", 9, b"outside"),
                      ("cano_t", -1, b"outside"), ("rot_dim", 3, b"rot_dim"), ("min_weight_sum", float("nan"), b"NaN"),
                      ("tracks", None, b"tracks and order"), ("order", None, b"tracks and order"),
                      ("offsets", None, b"offsets are required"), ("rots", None, b"rots and transls"),
                      ("transls", None, b"rots and transls"), ("err_after", None, b"skipped are required"),
                      ("skipped", None, b"skipped are required"), ("workspace", None, b"workspace is required"),
                      ("workspace_bytes", 16, b"needed")],
}


@pytest.mark.parametrize("entry", tuple(BAD))
def test_validators_reject_bad_arguments_without_gpu(entry):
    L = _lib.load()
    keep = []
    validate, call = getattr(L, entry + "_validate"), getattr(L, entry)
    assert validate(ctypes.byref(_blocks(keep)[entry])) == 0, L.gs_last_error()
    assert validate(None) < 0 and b"null argument" in L.gs_last_error()
    for field, value, msg in BAD[entry]:
        bad = _blocks(keep)[entry]
        setattr(bad, field, value)
        assert validate(ctypes.byref(bad)) < 0, (field, value)
        assert msg in L.gs_last_error(), (field, L.gs_last_error())
        # the entry point runs the validator before anything touches a device
        assert call(ctypes.byref(bad), None) < 0 and msg in L.gs_last_error(), field
    bytewise = ("workspace", "valid", "skipped")  # byte arrays have no alignment rule; the workspace has its own
    for field in [f for f, t in MIRRORS[entry]._fields_ if t is ctypes.c_void_p and f not in bytewise]:
        bad = _blocks(keep)[entry]
        if getattr(bad, field):
            setattr(bad, field, getattr(bad, field) + 2)
            assert validate(ctypes.byref(bad)) < 0 and b"aligned" in L.gs_last_error(), field


def test_workspace_bytes():
    L = _lib.load()
    assert L.gs_kmeans_workspace_bytes(4097, 49, 32) >= 9 * 49 * 32 * 8 + 9 * 49 * 8  # nine slices of 512 points
    assert L.gs_kmeans_workspace_bytes(10 ** 6, 64, 447) <= 1024 * 64 * 447 * 8 + 1024 * 64 * 8 + 512
    assert L.gs_procrustes_workspace_bytes(49, 150) >= 49 * 150 * 19 * 8
    for bad in [(-1, 4, 4), (10, 0, 4), (10, 65, 4), (10, 4, 0)]:
        assert L.gs_kmeans_workspace_bytes(*bad) == 0
    assert L.gs_procrustes_workspace_bytes(65, 3) == 0 and L.gs_procrustes_workspace_bytes(3, 0) == 0


@pytest.mark.skipif(shutil.which("gcc") is None or shutil.which("g++") is None, reason="gcc / g++ not available")
def test_validators_are_sanitizer_clean(tmp_path):
    """gs_motion_init_host.cpp (with gs_host.cpp's error state) under ASan + UBSan in a plain CPU
    executable with its own main: nothing preloaded, nothing loaded into Python."""
    run_host_sanitizer(tmp_path, "motion_init_host_sanitize.c", ["gs_motion_init_host.cpp", "gs_host.cpp"],
                       "motion init host sanitize ok")
