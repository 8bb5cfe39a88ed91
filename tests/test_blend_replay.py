"""The fp64 replay of the blend (oracle/gs_oracle.c or_render_fwd64 /
or_render_bwd64) and the decision-robust scenes built on it (tests/_robust.py)
-- CPU only.

* the replay's gradients equal torch autograd through the dense fp64 splat
  (oracle/torch_splat.py), element by element, at fp64 rounding level;
* every scene of _robust.ALL_SCENES becomes decision-robust within 8 rounds;
* on each of them, in both compat modes, the fp32 C oracle takes the
  replay's decisions at every pixel and passes the per-element check at
  1.5 x K_ORACLE (direct tensors) and 10 x K_DOWN (behind preprocess_bwd):
  the numbers the HIP kernels are then held to (tests/test_gpu_elementwise.py)
  cannot drift unnoticed;
* four small corruptions that the aggregate criteria of
  tests/test_gpu_parity.py accept and the per-element check refuses.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

from oracle import oracle as O
from oracle import torch_splat as TS
from tests import _harness as H
from tests import _robust as R
from tests.test_autograd_oracle import _autograd, _scene

U64 = 2.0 ** -53


# ------------------------------------------------ replay == fp64 autograd

def _autograd_on_records(inp, st, grads, monkeypatch):
    """torch autograd through torch_splat's blend, fed the oracle's fp32
    per-Gaussian records (widened to float64) as leaves: gradients with
    respect to exactly what the replay differentiates."""
    leaf = lambda a: torch.from_numpy(np.asarray(a, np.float64).copy()).requires_grad_(True)  # noqa: E731
    rec = dict(px=leaf(st.means2D[:, 0]), py=leaf(st.means2D[:, 1]), depth=leaf(st.depths),
               conic=leaf(st.conic_opacity[:, :3]))
    orig = TS.preprocess

    def on_records(*a, **k):
        pre = orig(*a, **k)
        np.testing.assert_array_equal(pre["visible"].numpy(), st.radii > 0)
        pre.update(rec)
        return pre
    monkeypatch.setattr(TS, "preprocess", on_records)
    d64 = lambda t: t.double().clone().requires_grad_(True)  # noqa: E731
    op, col, sem = d64(inp["opacity"]), d64(inp["colors"]), d64(inp["semantic_feature"])
    color, depth, feat, alpha = TS.render(
        inp["means3D"].double(), col, op, inp["scales"].double(), inp["rotations"].double(),
        inp["viewmatrix"].double(), inp["projmatrix"].double(), inp["tan_fovx"], inp["tan_fovy"], inp["c_x"],
        inp["c_y"], inp["image_width"], inp["image_height"], inp["bg"].double(), features=sem)
    dc, df, dd, da = [t.double() for t in grads]
    ((color * dc).sum() + (depth * dd).sum() + (feat * df).sum() + (alpha * da).sum()).backward()
    W, Hh = inp["image_width"], inp["image_height"]
    g = lambda t: t.grad.numpy()  # noqa: E731
    conic = g(rec["conic"]) * np.array([1.0, 0.5, 1.0])   # the blend's dconic b slot holds half of dL/db
    return dict(dmean2D=np.stack([g(rec["px"]) * 0.5 * W, g(rec["py"]) * 0.5 * Hh], 1), dconic=conic,
                dopacity=g(op).reshape(-1), dcolors=g(col), dsemantic=g(sem), ddepth=g(rec["depth"])), \
        (color, depth, feat, alpha)


def test_replay_gradients_equal_fp64_autograd_per_element(monkeypatch):
    """Both sides are float64 evaluations of the same sums over the same
    records, in different orders (autograd: cumulative products and dense
    matrix products per tile; the replay: the reference's reverse walk, whose
    T is recovered by dividing 1 - alpha back up the list).  A term of a list
    of length L passes through at most ~4 L roundings on either side, so the
    two differ by at most 8 L 2^-53 times the element's absolute sum; L is
    the scene's longest list."""
    inp = _scene()
    grads = H.upstream_grads(inp["image_height"], inp["image_width"], 8)
    o = H.oracle_forward(inp, "fixed")
    st = o[6]
    W, Hh = inp["image_width"], inp["image_height"]
    ag, (color, depth, feat, alpha) = _autograd_on_records(inp, st, grads, monkeypatch)
    f64 = O.render_forward64(st, W, Hh, inp["colors"], inp["semantic_feature"], inp["bg"], "fixed")
    lens = st.ranges.reshape(-1, 2).astype(np.int64)
    L = int((lens[:, 1] - lens[:, 0]).max())
    worst = {}
    for name, img in (("color", color), ("depth", depth), ("feature", feat), ("alpha", alpha)):
        got, ref, A = f64[name], img.detach().numpy(), f64["A_" + name]
        assert not np.any(got[A == 0]) and not np.any(ref[A == 0]), name
        worst[name] = R.normalised_error(got, ref, A) * R.U / U64
        assert worst[name] <= 8 * L, (name, worst[name])
    b64 = O.render_backward64(st, W, Hh, inp["colors"], inp["semantic_feature"], inp["bg"], f64["alpha"], grads,
                              "fixed")
    for name, ref in ag.items():
        got, A = b64[name], b64["A_" + name]
        assert got.shape == ref.shape, name
        assert not np.any(got[A == 0]) and not np.any(ref[A == 0]), name
        nz = A > 0
        assert nz.sum() > 0.5 * nz.size, name    # the scene reaches most Gaussians
        worst[name] = float((np.abs(got - ref)[nz] / (U64 * A[nz])).max())
        assert worst[name] <= 8 * L, (name, worst[name], L)
    print("replay vs fp64 autograd, worst |diff| / (2^-53 A):", {k: round(v, 1) for k, v in worst.items()}, "L =", L)


def test_k_down_against_autograd():
    """K_DOWN: the C oracle's gradients behind preprocess_bwd against torch
    autograd through the whole fp64 splat (fixed mode), per element in units
    of u s; pinned at 1.5 x the recorded value."""
    worst = {}
    for sh_degree in (None, 3):
        inp = _scene(sh_degree=sh_degree)
        grads = H.upstream_grads(inp["image_height"], inp["image_width"], 8)
        ag, _ = _autograd(inp, grads)
        o = H.oracle_forward(inp, "fixed")
        ob = dict(zip(R.GRAD_NAMES, H.oracle_backward(inp, o, grads, "fixed")))
        ref = dict(inp=inp, st=o[6], grads=grads)
        b64 = R.replay_backward(ref, "fixed", o[4])
        _, scale = R.downstream(ref, "fixed", b64)
        for k in ("dmeans3D", "dscales", "drotations") + (("dsh",) if sh_degree is not None else ()):
            w = R.normalised_error(ob[k], ag[k].numpy().reshape(ob[k].shape), scale[k])
            worst[k] = max(worst.get(k, 0.0), w)
    print("K_down per tensor:", {k: round(v, 1) for k, v in worst.items()})
    assert max(worst.values()) <= 1.5 * R.K_DOWN, worst


# --------------------------------------------------- robust scenes, oracle

def test_margin_factor_is_capped():
    assert O.MARGIN_FACTOR <= 64


@pytest.mark.parametrize("name", R.ALL_SCENES)
def test_robust_scene_converges(name):
    inps, rounds = R.robust_scene(name)
    assert rounds <= R.MAX_ROUNDS
    for cam in range(len(inps)):
        f64 = R.reference(name, "fixed", cam)["fwd64"]
        assert not f64["flag"].any()
        assert f64["closeness"].min() > 1.0


def test_scenes_reach_what_they_are_for():
    """The stacks' lists have exactly n records, pixels stop inside them, the
    centre pixel clamps at 0.99 and odd and even survivor counts occur; the
    SH scene has clamped channels; the frustum scene has Gaussians past the
    clamp that still receive gradient; the long-list scenes pass 512."""
    for n in R.STACKS:
        ref = R.reference(f"stack{n}", "fixed")
        st, f64 = ref["st"], ref["fwd64"]
        assert st.ranges.tolist() == [0, n]
        stopped = (f64["alpha"].reshape(-1) > 1 - 2e-4) & (f64["last_pos"] < n)
        assert stopped.any(), n
        co = st.conic_opacity[0]
        d = st.means2D[0].astype(np.float64) - 8.0
        assert co[3] * np.exp(-0.5 * (co[0] * d[0] ** 2 + co[2] * d[1] ** 2) - co[1] * d[0] * d[1]) > 0.99
        assert {0, 1} <= set((f64["n"] % 2).tolist())
    assert R.reference("sh3", "fixed")["st"].clamped.any()
    ref = R.reference("frustum_cov", "fixed")
    inp, st = ref["inp"], ref["st"]
    b64 = R.replay_backward(ref, "fixed", ref["ofwd"][4])
    moved = np.zeros(len(st.radii), bool)
    moved[::8] = True
    assert (moved & (b64["A_dconic"].sum(1) > 0)).sum() >= 20
    for name in ("odd37", "aligned96", "tail100"):
        lens = R.reference(name, "fixed")["st"].ranges.reshape(-1, 2).astype(np.int64)
        assert (lens[:, 1] - lens[:, 0]).max() > 512


def _oracle_results(name, compat, cam=0):
    ref = R.reference(name, compat, cam)
    o = ref["ofwd"]
    images = dict(color=o[1], feature=o[2], depth=o[3], alpha=o[4])
    ob = dict(zip(R.GRAD_NAMES, H.oracle_backward(ref["inp"], o, ref["grads"], compat)))
    return ref, images, ob


@pytest.mark.parametrize("compat", ["reference", "fixed"])
@pytest.mark.parametrize("name", R.ALL_SCENES)
def test_oracle_passes_elementwise(name, compat):
    """The fp32 C oracle against the replay, every pixel and every Gaussian:
    same last contributor everywhere, direct tensors within 1.5 x K_ORACLE
    (the recorded worst case of these very runs), downstream tensors within
    the HIP kernels' own bar of 10 x K_DOWN."""
    inps, _ = R.robust_scene(name)
    worst = {}
    for cam in range(len(inps)):
        ref, images, ob = _oracle_results(name, compat, cam)
        st, f64, inp = ref["st"], ref["fwd64"], ref["inp"]
        W, Hh = inp["image_width"], inp["image_height"]
        np.testing.assert_array_equal(R.last_ids(st.n_contrib, st.ranges, st.point_list, W, Hh), f64["last_id"])
        np.testing.assert_array_equal(st.n_contrib, f64["last_pos"])
        R.check_forward(f"{name}/{compat}/cam{cam}", images, f64, lambda t: 1.5 * R.K_ORACLE[t], worst)
        b64 = R.replay_backward(ref, compat, images["alpha"])
        R.check_direct_grads(f"{name}/{compat}/cam{cam}", ob, b64, lambda t: 1.5 * R.K_ORACLE[t],
                             inp["sh"] is not None, worst)
        val, scale = R.downstream(ref, compat, b64)
        R.check_downstream(f"{name}/{compat}/cam{cam}", ob, val, scale, 10 * R.K_DOWN, worst)
    print(f"oracle32 vs replay, {name}/{compat}: worst |diff| / (u A):", {k: round(v, 1) for k, v in worst.items()})


# ------------------------------------------------------------- sensitivity

GPU_BAR = lambda t: 10 * R.K_ORACLE[t]  # noqa: E731


def _refuses(check, *a):
    with pytest.raises(AssertionError):
        check(*a)


def test_sensitivity_the_gap_the_aggregates_leave():
    """Corruptions of the fp32 oracle's own outputs (which pass both kinds of
    check untouched): each is refused by the per-element check at the HIP
    kernels' bar and accepted by the aggregate criteria of test_gpu_parity
    (99.9 % of pixels within 1e-5, colour PSNR >= 80 dB, rel-L2 <= 1e-4)."""
    name, compat = "odd37", "fixed"
    ref, images, ob = _oracle_results(name, compat)
    f64, inp = ref["fwd64"], ref["inp"]
    b64 = R.replay_backward(ref, compat, images["alpha"])
    use_sh = inp["sh"] is not None
    R.check_forward("clean", images, f64, GPU_BAR)
    R.check_direct_grads("clean", ob, b64, GPU_BAR, use_sh)
    assert R.aggregate_forward_ok(images, images) and R.aggregate_backward_ok(ob, ob)

    # 40 K u A on one channel of one edge pixel (the last column of a partial strip)
    bad = {k: v.copy() for k, v in images.items()}
    y, x = inp["image_height"] - 1, inp["image_width"] - 1
    assert f64["A_color"][1, y, x] > 0
    bad["color"][1, y, x] += np.float32(40 * R.K_ORACLE["color"] * R.U * f64["A_color"][1, y, x])
    _refuses(R.check_forward, "edge pixel", bad, f64, GPU_BAR)
    assert R.aggregate_forward_ok(bad, images)

    # one feature channel zeroed at one pixel
    bad = {k: v.copy() for k, v in images.items()}
    y, x = np.unravel_index(np.argmax(np.abs(images["feature"][5])), images["feature"][5].shape)
    bad["feature"][5, y, x] = 0.0
    _refuses(R.check_forward, "feature channel", bad, f64, GPU_BAR)
    assert R.aggregate_forward_ok(bad, images)

    # one low-magnitude Gaussian's dopacity off by 1 %
    bad = {k: v.copy() for k, v in ob.items()}
    v, A = np.abs(ob["dopacity"].reshape(-1)).astype(np.float64), b64["A_dopacity"]
    small = (v > 0) & (v < np.median(v[v > 0])) & (0.01 * v > 2 * GPU_BAR("dopacity") * R.U * A)
    g = int(np.flatnonzero(small)[np.argmin(v[small])])
    bad["dopacity"][g] *= np.float32(1.01)
    _refuses(R.check_direct_grads, "dopacity", bad, b64, GPU_BAR, use_sh)
    assert R.aggregate_backward_ok(bad, ob)

    # the dmeans2D of two Gaussians below the tensor's median norm, swapped
    bad = {k: v.copy() for k, v in ob.items()}
    nrm = np.linalg.norm(ob["dmeans2D"].astype(np.float64), axis=1)
    low = np.flatnonzero((nrm > 0) & (nrm < np.median(nrm[nrm > 0])))
    low = low[np.argsort(nrm[low])]    # the smallest pair that differs by more than twice the bar
    d = np.abs(ob["dmeans2D"][low[1:], :2].astype(np.float64) - ob["dmeans2D"][low[:-1], :2])
    room = 2 * GPU_BAR("dmeans2D") * R.U * np.maximum(b64["A_dmean2D"][low[1:]], b64["A_dmean2D"][low[:-1]])
    k = int(np.flatnonzero((d > room).any(1))[0])
    i, j = int(low[k]), int(low[k + 1])
    bad["dmeans2D"][[i, j]] = bad["dmeans2D"][[j, i]]
    _refuses(R.check_direct_grads, "dmeans2D swap", bad, b64, GPU_BAR, use_sh)
    assert R.aggregate_backward_ok(bad, ob)
