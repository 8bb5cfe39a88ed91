"""Neighbour losses (csrc/gs_neighbor.hip) against float64, per Gaussian, on
every dispatch path: the lane-per-pair kernels at G = 64 // K in {64, 9, 3,
2, 1}, the thread-per-Gaussian kernels (K > 64), the forward's grid-stride
second trip, K = 0, non-unit quaternions (the normalisation Jacobian of
rotation_bwd), a hub (a reverse row of length N), self / repeated neighbours
and zero weights.  Cases and their branches: tests/_neighbor_cases.py.

Reference: oracle.neighbor.torch_reference on the CPU on .double() copies of
the same fp32 inputs (autograd gradients), its forward pinned to the float64
numpy restatement here.

Metric: per gradient tensor, max over rows of
|g_i - h_i|_inf / max(|h_i|_inf, 1e-3 max_j |h_j|_inf); per loss, the relative
error.  Bound: the same figure of the fp32 torch_reference on the CPU against
float64 (e_ref) is the yardstick of fp32 rounding on that case, and the kernel
may differ from it by summation order only (its own share over K lanes
through LDS, its reverse row in 4 strided partials, torch through index-add):
e_hip <= 8 e_ref + 4e-6 for gradients, rel_hip <= 8 rel_ref + 1e-6 for
losses.  The measured table is in DESIGN.md section 9.2."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from oracle import neighbor as ON
from tests import _neighbor_cases as NC

DEV = "cuda"
gpu = pytest.mark.gpu
case_param = pytest.mark.parametrize("case", NC.CASES, ids=[c.id for c in NC.CASES])


# ------------------------------------------------------------------- CPU

def test_knn_graph_blocks_equal_oracle():
    """The builder's row-blocked k-NN is the oracle's, bit for bit, ties at the
    k-th distance included (a grid cloud: most distances repeat)."""
    g = np.random.default_rng(0)
    grid = np.stack([g.integers(0, 12, 2100) * 0.05, g.integers(0, 12, 2100) * 0.05, g.integers(0, 3, 2100) * 0.05], 1)
    for p, k in ((grid, 20), (grid, 1), (g.random((2100, 3)), 7)):
        d, i = NC.knn_graph(p, k, rows=500)
        od, oi = ON.knn(p, k)
        np.testing.assert_array_equal(d, od)
        np.testing.assert_array_equal(i, oi)


@case_param
def test_case_structures_and_float64_reference(case):
    """The builder makes what it claims, the float64 reference is finite and
    equals numpy_losses, and the fp32 reference is well conditioned."""
    pts, rot, v, meta = NC.build(case)
    N, K = case.N, case.K
    nbr, w = v["neighbor_indices"].numpy(), v["neighbor_weight"].numpy()
    assert nbr.shape == (N, K) and w.shape == (N, K) and v["prev_offset"].shape == (N, K, 3)
    rows = np.arange(N)[:, None]
    hub = N // 2
    if "hub" in case.flags:
        ptr, _ = ON.reverse_csr(nbr)
        assert ptr[hub + 1] - ptr[hub] >= N
        # the hub's row is not a row of zeros: rows near it keep a real weight
        assert (w[:, 0] > 1e-6).sum() >= 20
    n_self = int((nbr == rows).sum())
    if "selfdup" in case.flags:
        assert (nbr[::7, K // 2] == rows[::7, 0]).all() and (nbr[::5, K - 1] == nbr[::5, 0]).all()
        # the hub's own row names itself through column 0 (and through its copy in the last column)
        extra = int("hub" in case.flags) * (1 + int(hub % 5 == 0))
        assert n_self == meta["self_rows"] + extra and meta["self_rows"] == -(-N // 7)
        assert meta["dup_rows"] == -(-N // 5)
        self_w = w[::7, K // 2]
        assert (self_w == 1.0).all()  # zero offset: the 1e-20 terms carry everything
    else:
        assert n_self == int("hub" in case.flags)
    if "zero_w" in case.flags:
        assert (w[::11, 1] == 0).all() and meta["zero_w"] == -(-N // 11)
        # off the hub column (whose far rows underflow exp(-2000 d^2)) exactly the built zeros
        assert int((w[:, 1:] == 0).sum()) == meta["zero_w"]
    elif "hub" not in case.flags:
        assert int((w == 0).sum()) == 0
    for q in (rot, v["prev_inv_rot_fg"]):
        n = q.norm(dim=1)
        if "nonunit" in case.flags:
            assert 0.4999 <= n.min() <= 0.5001 and 1.9999 <= n.max() <= 2.0001
        else:
            assert (n - 1).abs().max() <= 1e-6
    if K > 0:
        assert float(w.max()) > 0.01  # weights not all vanishing

    r64 = NC.reference(case, torch.float64)
    r32 = NC.reference(case, torch.float32)
    if K == 0:
        assert np.isnan(r64.losses).all() and np.isnan(r32.losses).all()
        for r in (r64, r32):
            assert not np.any(r.d_pts) and not np.any(r.d_rot)  # zeros, not NaN
        return
    assert np.isfinite(r64.losses).all() and np.isfinite(r64.d_pts).all() and np.isfinite(r64.d_rot).all()
    n = ON.numpy_losses(pts.numpy(), rot.numpy(), nbr, w, v["neighbor_dist"].numpy(), v["prev_offset"].numpy(),
                        v["prev_inv_rot_fg"].numpy())
    for a, b in zip(r64.losses, n):
        assert abs(a - b) <= 1e-12 * abs(b)
    terms = (None, 0, 1, 2) if case.id in NC.EACH_TERM else (None,)
    for term in terms:
        a, b = NC.reference(case, torch.float32, term), NC.reference(case, torch.float64, term)
        e = (NC.row_error(a.d_pts, b.d_pts), NC.row_error(a.d_rot, b.d_rot))
        rel = [NC.rel_error(x, y) for x, y in zip(a.losses, b.losses)]
        print(f"NBREF {case.id} term={term} e_ref d_pts={e[0]:.3e} d_rot={e[1]:.3e} rel_ref={max(rel):.3e}")
        # above this the fp32 reference itself is ill conditioned on the case
        assert max(e) < 1e-3 and max(rel) < 1e-3, (term, e, rel)


# ------------------------------------------------------------------- GPU

def _hip(case, term=None):
    from dynamic3dgaussians_amd.neighbor import neighbor_losses
    pts, rot, v, _ = NC.build(case)
    return NC.run(neighbor_losses, pts.to(DEV), rot.to(DEV), {k: t.to(DEV) for k, t in v.items()}, term)


def _check(case, term):
    hip = _hip(case, term)
    r64 = NC.reference(case, torch.float64, term)
    r32 = NC.reference(case, torch.float32, term)
    bad = []
    for name, x, y, z in zip(("rigid", "rot", "iso"), hip.losses, r32.losses, r64.losses):
        e_hip, e_ref = NC.rel_error(x, z), NC.rel_error(y, z)
        msg = (f"NBCASE {case.id} term={term} {name}: rel_hip={e_hip:.3e} rel_ref={e_ref:.3e} "
               f"ratio={e_hip / max(e_ref, 1e-30):.2f}")
        print(msg)
        if not e_hip <= 8 * e_ref + 1e-6:
            bad.append(msg)
    for name, g, f, h in (("d_pts", hip.d_pts, r32.d_pts, r64.d_pts), ("d_rot", hip.d_rot, r32.d_rot, r64.d_rot)):
        e_hip, e_ref = NC.row_error(g, h), NC.row_error(f, h)
        msg = (f"NBCASE {case.id} term={term} {name}: e_hip={e_hip:.3e} e_ref={e_ref:.3e} "
               f"ratio={e_hip / max(e_ref, 1e-30):.2f}")
        print(msg)
        if not e_hip <= 8 * e_ref + 4e-6:
            bad.append(msg)
    assert not bad, "\n".join(bad)


@gpu
@case_param
def test_neighbor_losses_match_float64(case):
    if case.K == 0:
        # NaN losses and the gradients of torch_reference (zeros), exactly
        hip = _hip(case)
        for ref in (NC.reference(case, torch.float64), NC.reference(case, torch.float32)):
            assert np.array_equal(hip.losses, ref.losses, equal_nan=True)
            assert np.array_equal(hip.d_pts, ref.d_pts, equal_nan=True)
            assert np.array_equal(hip.d_rot, ref.d_rot, equal_nan=True)
        return
    _check(case, None)


@gpu
@pytest.mark.parametrize("term", [0, 1, 2], ids=["rigid", "rot", "iso"])
@pytest.mark.parametrize("cid", NC.EACH_TERM)
def test_neighbor_losses_each_term_alone_float64(cid, term):
    """G = 1 with idle lanes and the thread-per-Gaussian kernels with the other
    two upstream gradients absent; an input the term does not reach gets an
    exactly zero gradient."""
    _check(NC.BY_ID[cid], term)


@gpu
@pytest.mark.parametrize("cid", NC.DETERMINISM)
def test_neighbor_backward_bit_identical(cid):
    """No atomics: two backward runs agree bit for bit on the hub (one reverse
    row of 4100 in nb_gather_kernel) and in nb_bwd_kernel."""
    a, b = _hip(NC.BY_ID[cid]), _hip(NC.BY_ID[cid])
    assert np.array_equal(a.losses, b.losses)
    assert np.array_equal(a.d_pts, b.d_pts) and np.array_equal(a.d_rot, b.d_rot)


@gpu
@pytest.mark.parametrize("N,K,hub", [
    (255, 1, False), (256, 1, False), (257, 1, False),  # keys <= N: 8 bits at N = 255, 9 from 256: one pass, then two
    (65535, 1, False), (65536, 1, False),               # 16 bits | 17: two passes | three (the other ping-pong buffer)
    (300, 65, False), (40, 0, False),                   # the loss tests' K > 64 and K = 0 graphs
    (257, 3, True), (4100, 64, True),                   # column 0 constant: one reverse row of N
])
def test_reverse_csr_bitexact_radix_passes(N, K, hub):
    from dynamic3dgaussians_amd.neighbor import reverse_csr
    g = torch.Generator().manual_seed(7 * N + K)
    nbr = torch.randint(0, N, (N, K), generator=g)
    if hub:
        nbr[:, 0] = N // 2
    ptr, pair, pos = reverse_csr(nbr.to(DEV))
    optr, opair = ON.reverse_csr(nbr.numpy())
    np.testing.assert_array_equal(ptr.cpu().numpy(), optr)
    np.testing.assert_array_equal(pair.cpu().numpy(), opair)
    opos = np.empty_like(opair)
    opos[opair] = np.arange(opair.size, dtype=np.int32)
    np.testing.assert_array_equal(pos.cpu().numpy(), opos)
    if hub:
        assert optr[N // 2 + 1] - optr[N // 2] >= N
