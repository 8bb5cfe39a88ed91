"""Per-pixel and per-Gaussian parity of the HIP blend kernels (render_fwd /
render_bwd, and preprocess_bwd behind them) with the fp64 replay of the blend,
on decision-robust scenes (tests/_robust.py): no pixel and no Gaussian is left
out.

Forward, every pixel: the exported records equal the oracle's bit for bit;
the last contributor (as a Gaussian id) is the replay's; colour, depth, alpha
and every feature channel lie within 10 K_ORACLE u A of the replay, A the
pixel's own absolute sum; the replay over the GPU's pruned lists gives what it
gives over the oracle's full lists, so pruning and strip culling dropped
nothing that blends.

Backward, every Gaussian: dmeans2D, dopacity, dcolors, dsemantic within
10 K_ORACLE u A_g of the replay (exactly 0 where A_g is 0); dmeans3D, dscales,
drotations, dcov3D, dsh within 10 K_DOWN u s_g of or_preprocess_bwd applied to
the replay's upstream sums (s_g = |J| A_g), which reaches the frustum-clamped
(Q3) and SH-clamped Gaussians one by one.

The aggregate tests (test_gpu_parity, test_gpu_envelope) keep their guarantee
on full-size scenes, where a decision may flip on a rare pixel; these add the
guarantee that on scenes without such pixels nothing at all is off.

Measured on the MI355X (worst |gpu - ref64| / (u A) over all scenes and both
compat modes): see DESIGN.md section 5.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

from dynamic3dgaussians_amd import _C
from tests import _harness as H
from tests import _robust as R

pytestmark = pytest.mark.gpu

SINGLE = tuple(n for n in R.ALL_SCENES if n != "rig2")


def _bar(t):
    return 10 * R.K_ORACLE[t]


def _images(g):
    return dict(color=g[1].cpu().numpy(), feature=g[2].cpu().numpy(), depth=g[3].cpu().numpy(),
                alpha=g[4].cpu().numpy())


@pytest.mark.parametrize("compat", ["reference", "fixed"])
@pytest.mark.parametrize("name", SINGLE)
def test_every_pixel_and_every_gaussian(name, compat):
    ref = R.reference(name, compat)
    inp, st, f64 = ref["inp"], ref["st"], ref["fwd64"]
    P, W, Hh = inp["means3D"].shape[0], inp["image_width"], inp["image_height"]
    label = f"{name}/{compat}"
    worst = {}

    g = H.gpu_forward(inp, compat)
    st_g = H.export_state(P, W, Hh, g)
    # the records the blend reads: the oracle's, bit for bit
    vis = st.radii > 0
    assert g[0] == ref["ofwd"][0]
    np.testing.assert_array_equal(g[5].cpu().numpy(), st.radii)
    np.testing.assert_array_equal(st_g["tiles"], st.tiles_touched)
    np.testing.assert_array_equal(st_g["means2D"][vis], st.means2D[vis])
    np.testing.assert_array_equal(st_g["depths"][vis], st.depths[vis])
    np.testing.assert_array_equal(st_g["conic_opacity"][vis], st.conic_opacity[vis])
    if inp["sh"] is not None:
        np.testing.assert_array_equal(st_g["rgb"][vis], st.rgb[vis])
    # every pixel's last contributor
    gid = R.last_ids(st_g["n_contrib"], st_g["ranges"], st_g["point_list"], W, Hh)
    diff = np.flatnonzero(gid != f64["last_id"])
    assert diff.size == 0, (f"{label}: last contributor differs at {diff.size} pixels, first (y, x) = "
                            f"{divmod(int(diff[0]), W)}: gpu {gid[diff[0]]}, replay {f64['last_id'][diff[0]]}")
    # every pixel's values
    images = _images(g)
    R.check_forward(label, images, f64, _bar, worst)
    # the replay over the GPU's pruned lists: the same terms in the same order
    pruned = R.replay_forward(inp, st_g, st, compat)
    for k in ("last_id", "n") + tuple(R.FWD_TENSORS) + tuple("A_" + t for t in R.FWD_TENSORS):
        np.testing.assert_array_equal(pruned[k], f64[k], err_msg=f"{label}: pruned lists change {k}")

    grads = ref["grads"]
    gb = dict(zip(R.GRAD_NAMES, H.gpu_backward(inp, g, grads, compat)))
    b64 = R.replay_backward(ref, compat, images["alpha"])
    R.check_direct_grads(label, gb, b64, _bar, inp["sh"] is not None, worst)
    val, scale = R.downstream(ref, compat, b64)
    R.check_downstream(label, gb, val, scale, 10 * R.K_DOWN, worst)
    print(f"gpu vs replay, {label}: decision closeness {f64['closeness'].min():.2f}, worst |diff| / (u A):",
          {k: round(v, 1) for k, v in worst.items()})


@pytest.mark.parametrize("compat", ["reference", "fixed"])
def test_batch_of_two_cameras_with_a_tile_window(compat):
    """The 37x29 scene from two rig cameras in one batch call, the second
    restricted to the tile window [1,3) x [1,2) -- the bottom-right corner,
    whose tiles are partial in x and y.  Camera c's images are held to the
    single-camera bounds (zeros outside the window); the gradients, summed
    over the cameras, to the sum of the cameras' replays and absolute sums
    with the window's upstream gradients only."""
    inps, _ = R.robust_scene("rig2")
    refs = [R.reference("rig2", compat, c) for c in range(2)]
    inp0 = inps[0]
    W, Hh, C = inp0["image_width"], inp0["image_height"], 2
    windows = [None, (1, 1, 3, 2)]
    inside = [np.ones((Hh, W), bool), np.zeros((Hh, W), bool)]
    inside[1][16:, 16:] = True
    d = lambda k: H._to(inp0[k], H.DEV)  # noqa: E731
    stack = lambda k: torch.stack([i[k] for i in inps]).to(H.DEV)  # noqa: E731
    lst = lambda k: [float(i[k]) for i in inps]  # noqa: E731
    views, projs, cpos = stack("viewmatrix"), stack("projmatrix"), stack("campos")
    out = _C.rasterize_gaussians_batch(
        d("bg"), d("means3D"), d("colors"), d("semantic_feature"), d("opacity"), d("scales"), d("rotations"), 1.0,
        d("cov3D_precomp"), views, projs, lst("c_x"), lst("c_y"), lst("tan_fovx"), lst("tan_fovy"), Hh, W, d("sh"),
        inp0["degree"], cpos, False, False, compat=compat, windows=windows)
    torch.cuda.synchronize()
    NR, color, fmap, depth, alpha, radii, geom, binning, img, NI = out
    worst = {}
    per_cam = []
    for c in range(C):
        f64 = refs[c]["fwd64"]
        images = dict(color=color[c].cpu().numpy(), feature=fmap[c].cpu().numpy(), depth=depth[c].cpu().numpy(),
                      alpha=alpha[c].cpu().numpy())
        np.testing.assert_array_equal(radii[c].cpu().numpy(), refs[c]["st"].radii)
        for t in R.FWD_TENSORS:
            assert not images[t][:, ~inside[c]].any(), (c, t)   # outside the window: zeros
        masked = {k: (v * inside[c] if k in R.FWD_TENSORS or k[2:] in R.FWD_TENSORS else v) for k, v in f64.items()}
        R.check_forward(f"rig2/{compat}/cam{c}", images, masked, _bar, worst)
        per_cam.append(images)
    ups = [refs[c]["grads"] for c in range(C)]
    up = [torch.stack([ups[c][i] for c in range(C)]).to(H.DEV) for i in range(4)]
    swap = compat == "reference"
    cam4 = list(zip(*[H.bwd_cam4(i, swap) for i in inps]))
    gb = _C.rasterize_gaussians_batch_backward(
        d("bg"), d("means3D"), radii, d("colors"), d("semantic_feature"), d("scales"), d("rotations"), 1.0,
        d("cov3D_precomp"), views, projs, *[list(map(float, x)) for x in cam4], *up, d("sh"), inp0["degree"], cpos,
        geom, NI, binning, img, alpha, False, compat=compat, windows=windows)
    torch.cuda.synchronize()
    gb = dict(zip(R.GRAD_NAMES, [t.cpu().numpy() for t in gb]))
    tot, val, scale = None, None, None
    for c in range(C):
        m = torch.from_numpy(inside[c])
        win_up = tuple(t * m for t in ups[c])    # upstream gradients outside the window are ignored
        b64 = R.replay_backward(refs[c], compat, per_cam[c]["alpha"], win_up)
        v, s = R.downstream(refs[c], compat, b64)
        if tot is None:
            tot, val, scale = b64, {k: x.astype(np.float64) for k, x in v.items()}, s
        else:
            tot = {k: tot[k] + b64[k] for k in tot}
            val = {k: val[k] + v[k] for k in val}
            scale = {k: scale[k] + s[k] for k in scale}
    R.check_direct_grads(f"rig2/{compat}", gb, tot, _bar, False, worst)
    R.check_downstream(f"rig2/{compat}", gb, val, scale, 10 * R.K_DOWN, worst)
    print(f"gpu vs replay, rig2 batch/{compat}: worst |diff| / (u A):", {k: round(v, 1) for k, v in worst.items()})
