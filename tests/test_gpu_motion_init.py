"""The motion-initialisation kernels (csrc/gs_motion_init.hip) on the GPU against the fp64 _torch
twins of motion_init.py on the CPU, never against the HIP code's own output.  Parity unpinned:
dyn_som.py cannot be imported, so the twins (checked against scikit-learn, an SVD Kabsch and
torch.median in tests/test_motion_init.py) are the measuring stick.

Values follow the _check convention of tests/test_gpu_depth_geometry.py: within 4 x the deviation
of the fp32 twin from the fp64 twin on the same inputs, computed here, with a floor of one fp32 ulp
of the value.  Decisions (labels, moved, counts, skipped) must be exact on every point: the cases
of tests/_motion_init_cases.py are built so that none hangs on rounding.

Shapes are the smallest at which the kernels can go wrong: N = 257 (two assign workgroups, the
second with one point), D = 3, 24, 32 and 447 (below, at and above the 32-dimension LDS chunk
and the 64-dimension update chunk, neither a multiple), K = 1, 5, 20, 49 and 64 (every register
tier of the assign kernel), N = 63 (less than a wave), 4097 points (nine update slices of 512, the
last with one point), clusters of 1, 2, 257 and 300 tracks (a moments workgroup's 32 point lanes:
fewer, and a ragged multiple), T = 9 and 12 (two frame chunks of 8, the second ragged).
"""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from dynamic3dgaussians_amd import motion_init as mi
from dynamic3dgaussians_amd.motion import cont_6d_to_rmat
from tests import _motion_init_cases as C

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ENVELOPE = 4.0


def _ulp32(v: torch.Tensor) -> torch.Tensor:
    return torch.from_numpy(np.spacing(v.abs().float().numpy())).double()


def _check(name, got, ref64, twin32):
    """got (device, fp32) within ENVELOPE x max|twin32 - ref64| of ref64, per element at least one
    fp32 ulp of the value."""
    got, ref64, twin32 = got.detach().cpu().double(), ref64.double(), twin32.double()
    assert got.shape == ref64.shape, (got.shape, ref64.shape)
    own = (twin32 - ref64).abs().max().item() if ref64.numel() else 0.0
    err = (got - ref64).abs()
    bound = torch.maximum(torch.full_like(err, ENVELOPE * own), _ulp32(ref64))
    print(f"{name}: hip {err.max().item() if err.numel() else 0.0:.3e} fp32 formulation {own:.3e}")
    assert torch.all(err <= bound), (name, err.max().item(), own)


def _dev(t):
    return None if t is None else t.to(DEV).contiguous()


# ---- 1. assign

@pytest.mark.parametrize("name", tuple(C.KMEANS_CASES))
def test_assign_matches_the_twin_at_every_iteration(name):
    x, _, run, _ = C.kmeans_case(name)
    d_x = _dev(x)
    for it, (centres, labels) in enumerate(zip(run["centres"], run["labels"])):
        got = mi.kmeans_assign(d_x, _dev(centres.float()))
        assert got.dtype == torch.int64 and torch.equal(got.cpu(), labels), (name, it)


def test_assign_with_one_centre_one_point_per_centre_and_less_than_a_wave():
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(300, 7, generator=gen)
    assert torch.equal(mi.kmeans_assign(_dev(x), _dev(x[:1])).cpu(), torch.zeros(300, dtype=torch.int64))  # K = 1
    pts = 2.0 * torch.randn(64, 3, generator=gen)  # N = K = 64: every point is its own centre, distance 0
    assert torch.cdist(pts.double(), pts.double()).fill_diagonal_(9.0).min() > 1e-2
    assert torch.equal(mi.kmeans_assign(_dev(pts), _dev(pts)).cpu(), torch.arange(64))
    x63 = C.blobs(63, 5, 4, 0)  # N = 63: below one wave
    c = x63[:4]
    ref = mi.kmeans_assign_torch(x63.double(), c.double())
    assert C.margins(x63.double(), c.double()).min() > C.TAU
    assert torch.equal(mi.kmeans_assign(_dev(x63), _dev(c)).cpu(), ref)
    assert mi.kmeans_assign(_dev(x63[:0]), _dev(c)).shape == (0,)


# ---- 2. the tie rule

def test_identical_centres_give_the_lower_index():
    x = C.blobs(500, 24, 6, 4)
    c = x[:6].clone()
    c[4] = c[1]  # centres 1 and 4 coincide: bit-identical distances
    c = torch.cat([c, c[2:3]])  # and 6 coincides with 2
    x = x[C.margins(x.double(), c[[0, 1, 2, 3, 5]].double()) > C.TAU]  # the ties apart, every decision is robust
    assert x.shape[0] > 400
    ref = mi.kmeans_assign_torch(x.double(), c.double())
    got = mi.kmeans_assign(_dev(x), _dev(c)).cpu()
    assert (ref == 1).any() and (ref == 2).any()
    assert not (got == 4).any() and not (got == 6).any()
    assert torch.equal(got, ref)


# ---- 3. update

@pytest.mark.parametrize("name", tuple(C.KMEANS_CASES))
def test_update_matches_the_twin(name):
    x, _, run, _ = C.kmeans_case(name)
    empties = 0
    for it in (0, C.ITERS - 1):
        prev, labels = run["centres"][it].float(), run["labels"][it]
        ref, ref_counts = mi.kmeans_update_torch(x.double(), labels, prev.double())
        f32, _ = mi.kmeans_update_torch(x, labels, prev)
        got, counts = mi.kmeans_update(_dev(x), _dev(labels), _dev(prev))
        assert torch.equal(counts.cpu(), ref_counts)
        _check(f"update {name} it{it}", got, ref, f32)
        empty = ref_counts == 0
        empties += int(empty.sum())
        assert torch.equal(got.cpu()[empty], prev[empty])  # an empty cluster's centre: bit for bit
        again, _ = mi.kmeans_update(_dev(x), _dev(labels), _dev(prev))
        assert torch.equal(got, again)
    if name in ("km_4097x32_k49_s0", "km_1000x447_k20_s1"):
        assert empties > 0


def test_update_ignores_labels_outside_the_clusters():
    x = C.blobs(700, 5, 3, 2)
    labels = torch.randint(-2, 5, (700,), generator=torch.Generator().manual_seed(1))
    prev = x[:3].clone()
    ref, ref_counts = mi.kmeans_update_torch(x.double(), labels, prev.double())
    got, counts = mi.kmeans_update(_dev(x), _dev(labels), _dev(prev))
    assert torch.equal(counts.cpu(), ref_counts) and ref_counts.sum() < 700
    _check("update with ignored labels", got, ref, mi.kmeans_update_torch(x, labels, prev)[0])


# ---- 4. the whole loop

@pytest.mark.parametrize("name", tuple(C.KMEANS_CASES))
def test_kmeans_matches_the_twin_and_reruns_bit_identically(name):
    x, init, run, f32 = C.kmeans_case(name)
    got = mi.kmeans(_dev(x), init=_dev(init), iters=C.ITERS)
    assert got.moved.is_cuda and got.moved.dtype == torch.int64
    assert torch.equal(got.labels.cpu(), run["labels"][-1])
    assert torch.equal(got.moved.cpu(), run["moved"])
    assert torch.equal(got.counts.cpu(), run["counts"])
    _check(f"kmeans {name}", got.centers, run["final_centres"], f32.centers)
    again = mi.kmeans(_dev(x), init=_dev(init), iters=C.ITERS)
    for a, b in zip(got, again):
        assert torch.equal(a, b)


def test_kmeans_draws_its_initial_rows_and_honours_the_mask():
    x, _, _, _ = C.kmeans_case("km_1000x24_k20_s0")
    K = 20
    rows = torch.randperm(x.shape[0], generator=torch.Generator().manual_seed(7))[:K]
    assert torch.equal(mi.kmeans(_dev(x), K, iters=0, seed=7).centers.cpu(), x[rows])  # the documented draw
    one = mi.kmeans(_dev(x), K, iters=1, seed=7)
    assert torch.equal(one.moved.cpu(), torch.tensor([x.shape[0]])) and one.counts.sum().item() == x.shape[0]
    valid = torch.rand(x.shape[0], generator=torch.Generator().manual_seed(8)) < 0.7
    init = x[valid][:K].clone()
    ref = mi.kmeans_torch(x.double(), init=init.double(), iters=3, valid=valid)
    got = mi.kmeans(_dev(x), init=_dev(init), iters=3, valid=_dev(valid))
    assert torch.all(got.labels.cpu()[~valid] == -1) and got.counts.sum().item() == int(valid.sum())
    sub = mi.kmeans_torch(x[valid].double(), init=init.double(), iters=3)
    assert torch.equal(ref.labels[valid], sub.labels)  # the mask is the compacted problem
    assert got.moved.cpu()[0] == int(valid.sum())  # a masked point stays at -1: it never moves
    empty = mi.kmeans(_dev(x[:0]), 4, iters=2)
    assert empty.labels.shape == (0,) and empty.centers.shape == (4, 24) and not empty.moved.any()


# ---- 5. medians

def test_cluster_medians_bit_for_bit():
    gen = torch.Generator().manual_seed(2)
    pts = torch.randn(1001, 3, generator=gen)
    labels = torch.randint(0, 4, (1001,), generator=gen)
    labels[labels == 2] = 0  # cluster 2 is empty
    labels[:1] = 5           # cluster 5 has a single member
    labels[1:11] = 4         # cluster 4 an even count
    labels[11:20] = -1
    got = mi.cluster_medians(_dev(pts), _dev(labels), 6).cpu()
    ref = mi.cluster_medians_torch(pts.double(), labels, 6)
    assert torch.equal(got.double()[[0, 1, 3, 4, 5]], ref[[0, 1, 3, 4, 5]])
    assert torch.isnan(got[2]).all() and torch.isnan(ref[2]).all()
    for k in (0, 1, 3, 4, 5):
        assert torch.equal(got[k], pts[labels == k].median(dim=0).values)
    assert (labels == 4).sum() % 2 == 0 and (labels == 5).sum() == 1


# ---- 6. coefficients

@pytest.mark.parametrize("N,K", [(1000, 49), (257, 1)])
def test_coefs_from_centers(N, K):
    gen = torch.Generator().manual_seed(N)
    means = 1.5 * torch.randn(N, 3, generator=gen)
    centers = 1.5 * torch.randn(K, 3, generator=gen)
    got = mi.coefs_from_centers(_dev(means), _dev(centers))
    assert got.shape == (N, K) and got.dtype == torch.float32
    _check(f"coefs {N}x{K}", got, mi.coefs_from_centers_torch(means.double(), centers.double()),
           mi.coefs_from_centers_torch(means, centers))


# ---- 7. Procrustes

@functools.lru_cache(maxsize=None)
def _procrustes_refs(rot_type):
    p = C.procrustes_case()
    kw = dict(visibles=p["visibles"], confidences=p["confidences"], min_mean_weight=C.PROCRUSTES_MIN_MEAN_WEIGHT,
              rot_type=rot_type)
    ref = mi.solve_procrustes_bases_torch(p["tracks"], p["labels"], p["K"], p["cano_t"], **kw)
    f32 = mi.solve_procrustes_bases_torch(p["tracks"].float(), p["labels"], p["K"], p["cano_t"], **kw)
    assert torch.equal(ref.skipped, f32.skipped)
    return ref, f32


@pytest.mark.parametrize("rot_type", ["6d", "quat"])
def test_procrustes_matches_the_twin(rot_type):
    p = C.procrustes_case()
    ref, f32 = _procrustes_refs(rot_type)
    full = list(C.PROCRUSTES_FULL_RANK)
    k, t = C.PROCRUSTES_SKIP
    assert ref.skipped[k, t] and ref.skipped.sum() == 1

    def run():
        return mi.solve_procrustes_bases(_dev(p["tracks"].float()), _dev(p["labels"]), p["K"], p["cano_t"],
                                         visibles=_dev(p["visibles"]), confidences=_dev(p["confidences"]),
                                         min_mean_weight=C.PROCRUSTES_MIN_MEAN_WEIGHT, rot_type=rot_type)
    got = run()
    assert torch.equal(got.skipped.cpu(), ref.skipped)
    for field in ("rots", "transls", "err_after", "err_before"):
        _check(f"procrustes {rot_type} {field}", getattr(got, field)[full], getattr(ref, field)[full],
               getattr(f32, field)[full])
    assert got.err_after[k, t] == -1 and got.err_before[k, t] == -1
    assert torch.equal(got.rots[k, t], got.rots[k, t - 1])  # frame 6 is visited after frame 5: a copy
    # the clusters of one and two points: finite, a proper rotation, the centroid mapped
    tracks, w_vis, conf = p["tracks"], p["visibles"].double(), p["confidences"].double()
    for small in (0, 1):
        m = p["labels"] == small
        rots, transls = got.rots[small].cpu().double(), got.transls[small].cpu().double()
        assert torch.isfinite(rots).all() and torch.isfinite(transls).all()
        assert torch.isfinite(got.err_after[small]).all() and torch.isfinite(got.err_before[small]).all()
        R = cont_6d_to_rmat(rots) if rot_type == "6d" else mi._quat_to_rmat(rots)
        if rot_type == "6d":  # the raw columns, before cont_6d_to_rmat's Gram-Schmidt
            c0, c1 = rots[:, :3], rots[:, 3:]
            raw = torch.stack([c0, c1, torch.linalg.cross(c0, c1)], -1)
            assert (raw.transpose(1, 2) @ raw - torch.eye(3, dtype=torch.float64)).abs().max() <= 1e-6
        assert (R.transpose(1, 2) @ R - torch.eye(3, dtype=torch.float64)).abs().max() <= 1e-6
        assert torch.all(torch.linalg.det(R) > 0.999)
        for f in range(tracks.shape[1]):
            w = w_vis[m, p["cano_t"]] * w_vis[m, f] * (conf[m, p["cano_t"]] + conf[m, f]) / 2
            cs = (w[:, None] * tracks[m, p["cano_t"]]).sum(0) / w.sum()
            cg = (w[:, None] * tracks[m, f]).sum(0) / w.sum()
            # R and t are rounded to fp32, 2^-24 of each term of R cs + t, and cont_6d_to_rmat
            # renormalises the rounded columns (three more roundings per entry): 4 x 2^-23 of the terms
            bound = 2.0 ** -21 * (cs.abs().sum() + transls[f].abs().max() + cg.abs().max())
            assert (R[f] @ cs + transls[f] - cg).abs().max() <= bound
    again = run()
    for a, b in zip(got, again):
        assert torch.equal(a, b)


# ---- 8. end to end

def test_init_from_tracks_end_to_end():
    case = C.bodies_case()
    tracks, body, ref = case["tracks"], case["body"], case["ref"]
    kw = dict(num_bases=4, cano_t=case["cano_t"], seed=case["seed"])
    f32 = mi.init_motion_bases_from_tracks(tracks.float(), **kw)
    got = mi.init_motion_bases_from_tracks(_dev(tracks.float()), **kw)
    assert torch.equal(got.valid_mask.cpu(), ref.valid_mask) and torch.equal(got.labels.cpu(), ref.labels)
    assert torch.equal(f32.labels, ref.labels)
    labels = got.labels.cpu()
    assert torch.all(labels[~ref.valid_mask] == -1) and ref.valid_mask.sum() == 1140
    for b in range(4):  # the partition is the bodies
        mine = labels[(body == b) & ref.valid_mask]
        assert (mine == mine[0]).all() and (labels == mine[0]).sum() == mine.numel()
    assert torch.equal(got.means_cano.cpu().double(), ref.means_cano)
    assert torch.equal(got.centers.cpu().double(), ref.centers)  # medians: a selection, exact
    _check("e2e coefs", got.motion_coefs, ref.motion_coefs, f32.motion_coefs)
    for field in ("rots", "transls", "err_after", "err_before"):
        _check(f"e2e {field}", getattr(got.procrustes, field), getattr(ref.procrustes, field),
               getattr(f32.procrustes, field))
    assert not got.procrustes.skipped.any() and not ref.procrustes.skipped.any()

    def moved(pro, dtype):  # every basis applied to its own cluster's canonical points
        keep = labels >= 0
        R = cont_6d_to_rmat(pro.rots.cpu().to(dtype))[labels[keep]]  # (n, T, 3, 3)
        t = pro.transls.cpu().to(dtype)[labels[keep]]
        return (R * tracks[keep, case["cano_t"]].to(dtype)[:, None, None, :]).sum(-1) + t
    want = moved(ref.procrustes, torch.float64)
    _check("e2e mapped points", moved(got.procrustes, torch.float32), want, moved(f32.procrustes, torch.float32))
    assert (want - tracks[labels >= 0]).abs().max() < 1e-5  # and they are the tracks (noise-free bodies)
    out = got.bases.to(DEV).compute_means(range(12), got.means_cano, got.motion_coefs, softmax=True)
    assert out.shape == (1200, 12, 3) and out.is_cuda and torch.isfinite(out).all()


# ---- 9. from features

def test_init_from_features():
    means, feats, run = C.feature_case()
    K = 49
    bases, coefs, labels, centers = mi.init_motion_coefs_from_features(_dev(means), _dev(feats), K, num_frames=7)
    assert torch.equal(labels.cpu(), run["labels"][-1])
    ref = mi.init_motion_coefs_from_features(means.double(), feats.double(), K, num_frames=7)
    f32 = mi.init_motion_coefs_from_features(means, feats, K, num_frames=7)
    assert torch.equal(ref[2], labels.cpu())
    live = ~torch.isnan(ref[3]).any(dim=1)
    assert torch.equal(torch.isnan(centers.cpu()).any(dim=1), ~live)
    assert torch.equal(centers.cpu()[live].double(), ref[3][live])
    _check("features coefs", coefs[:, live], ref[1][:, live], f32[1][:, live])
    ident = torch.tensor([1.0, 0, 0, 0, 1, 0])
    assert bases.params["rots"].shape == (K, 7, 6) and torch.all(bases.params["rots"].cpu() == ident)
    assert bases.params["transls"].shape == (K, 7, 3) and not bases.params["transls"].any()
