"""Decision-robust scenes and the per-element comparison against the fp64
replay of the blend (oracle/gs_oracle.c, "fp64 replay of the blend").

A scene is decision-robust when no (pixel, Gaussian) pair the blend visits
has a decision (power > 0, alpha >= 1/255, the T < 1e-4 stop) closer to its
threshold than fp32 evaluation can resolve -- the replay's "undecided" flags
under oracle.MARGIN_FACTOR.  Every implementation whose exponent error stays
below that margin then takes exactly the replay's decisions, so nothing has
to be left out of a comparison: every pixel and every Gaussian is held to a
bound that scales with its own absolute sum,

    |x - ref64| <= K * u * A,        u = 2^-24,

where A is the replay's absolute sum of that element (every leaf product
replaced by its magnitude) and K the tensor's constant: K_ORACLE is the fp32
C oracle's own worst |oracle32 - ref64| / (u A) over every scene of SCENES in
both compat modes (measured by tests/test_blend_replay.py, which pins the
oracle at 1.5 x K_ORACLE); the HIP kernels get 10 x K_ORACLE, the project's
bar for "within the reference algorithm's own fp32 noise"
(tests/test_gpu_envelope.py).  An element whose A is 0 must be exactly 0.

Gradients behind preprocess_bwd (dmeans3D, dscales, drotations, dcov3D, dsh)
are compared with or_preprocess_bwd applied to the replay's upstream sums
(rounded to fp32), on the scale s = |J| A: the sum over the upstream
components (dmean2D x y, dconic a b c, dcolor r g b, ddepth) of
|or_preprocess_bwd(that component = its absolute sum, the rest 0)| -- the
kernel is linear in its upstream.  K_DOWN is the C oracle's worst distance
from torch autograd through the dense fp64 splat in units of u s (fixed mode,
the scene of tests/test_autograd_oracle.py); the bar is again 10 x.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from dynamic3dgaussians_amd.camera import setup_camera
from oracle import oracle as O
from tests import _harness as H

U = O.U32
MAX_ROUNDS = 8
assert O.MARGIN_FACTOR <= 64

# Measured by tests/test_blend_replay.py::test_oracle_passes_elementwise (worst
# over SCENES x both compat modes, rounded up to two digits) and
# ::test_k_down_against_autograd.
K_ORACLE = dict(color=21.0, depth=18.0, alpha=3.4, feature=30.0,
                dmeans2D=6.2, dopacity=6.6, dcolors=27.0, dsemantic=51.0)
K_DOWN = 154.0   # dscales; dsh 145, dmeans3D 41, drotations 33
DOWN_NAMES = ("dmeans3D", "dcov3D", "dsh", "dscales", "drotations")
GRAD_NAMES = ["dmeans2D", "dcolors", "dsemantic", "dopacity", "dmeans3D", "dcov3D", "dsh", "dscales",
              "drotations"]


# ------------------------------------------------------------------ scenes

def _feature_ranges(inps):
    """Feature channels spanning 1e-6 .. 1e6 across the channels."""
    f = inps[0]["semantic_feature"]
    scale = torch.logspace(-6, 6, f.shape[1], dtype=torch.float64).float()
    f = (f * scale[None]).contiguous()
    for inp in inps:
        inp["semantic_feature"] = f


def _past_frustum(inps):
    """Every 8th Gaussian moved to 1.05 x the frustum clamp in x (alternating
    sides) and every 16th in y as well, and enlarged 20-fold so that it still
    reaches the image: the clamped branch of the EWA Jacobian (Q3 in reference mode)."""
    inp = inps[0]
    v = inp["viewmatrix"].double().reshape(4, 4)       # column-major: p_view = [p, 1] @ v
    m = inp["means3D"].double()
    pv = torch.cat([m, torch.ones(len(m), 1, dtype=torch.float64)], 1) @ v
    W, Hh = inp["image_width"], inp["image_height"]
    fx, fy = W / (2 * inp["tan_fovx"]), Hh / (2 * inp["tan_fovy"])
    lxp, lxn = (W - inp["c_x"]) / fx + 0.3 * inp["tan_fovx"], inp["c_x"] / fx + 0.3 * inp["tan_fovx"]
    lyp, lyn = (Hh - inp["c_y"]) / fy + 0.3 * inp["tan_fovy"], inp["c_y"] / fy + 0.3 * inp["tan_fovy"]
    idx = torch.arange(0, len(m), 8)
    side = (idx // 8) % 2 == 0
    pv[idx, 0] = torch.where(side, torch.tensor(1.05 * lxp), torch.tensor(-1.05 * lxn)) * pv[idx, 2]
    idy = idx[::2]
    sidy = (idy // 16) % 4 < 2
    pv[idy, 1] = torch.where(sidy, torch.tensor(1.05 * lyp), torch.tensor(-1.05 * lyn)) * pv[idy, 2]
    back = (pv @ torch.linalg.inv(v))[:, :3].float().contiguous()
    inp["means3D"] = back
    # use_cov: Sigma scales with the square of the size
    cov = inp["cov3D_precomp"].clone()
    cov[idx] *= 400.0
    inp["cov3D_precomp"] = cov.contiguous()


def _stack(n):
    """One 16x16 tile, n Gaussians on one screen point (8.03, 8.03) at growing
    depth: one list of exactly n records.  The first is nearly opaque (the
    centre pixel hits the 0.99 clamp), the rest are faint enough that pixels
    saturate (T < 1e-4) at list positions that depend on their distance from
    the centre -- odd and even survivor counts, stops inside and at the end of
    a 64-record chunk."""
    g = torch.Generator().manual_seed(n)
    cam = setup_camera(16, 16, np.array([[16, 0, 8], [0, 16, 8], [0, 0, 1.0]]), np.eye(4))
    z = 2.0 + 0.01 * torch.arange(n, dtype=torch.float64)
    xy = 0.033125 * z                                   # NDC 0.06625 -> pixel 8.03
    op = torch.rand(n, 1, generator=g) * 0.25 + 0.03
    op[0] = 0.995
    op[1::7] = 0.6
    return [dict(bg=torch.tensor([0.3, 0.6, 0.1]), means3D=torch.stack([xy, xy, z], 1).float().contiguous(),
                 colors=torch.rand(n, 3, generator=g), semantic_feature=torch.randn(n, 8, generator=g),
                 opacity=op, scales=(torch.rand(n, 3, generator=g) * 0.4 + 0.2).contiguous(),
                 rotations=torch.nn.functional.normalize(torch.randn(n, 4, generator=g), dim=1),
                 scale_modifier=1.0, cov3D_precomp=None, viewmatrix=torch.from_numpy(cam.viewmatrix.copy()),
                 projmatrix=torch.from_numpy(cam.projmatrix.copy()), c_x=cam.c_x, c_y=cam.c_y,
                 tan_fovx=cam.tanfovx, tan_fovy=cam.tanfovy, image_height=16, image_width=16, sh=None,
                 degree=0, campos=torch.from_numpy(cam.campos.copy()))]


ODD37 = dict(W=37, H=29, P=1500, scale_mult=6.0, F=8, bg=(0.2, 0.5, 0.9))

# name -> (H.scene keywords, mutation of the inputs or None, camera indices of the rig)
SCENES = {
    "odd37": (ODD37, None, (0,)),
    "aligned96": (dict(W=96, H=64, P=4000, F=32), None, (0,)),
    "tail100": (dict(W=100, H=75, P=3000, scale_mult=5.0, F=36), None, (0,)),
    "wide80": (dict(W=80, H=48, P=2000, F=64), None, (0,)),
    "f3": (dict(W=70, H=44, P=1500, F=3, bg=(0.3, 0.1, 0.7)), None, (0,)),
    "sh3": (dict(W=70, H=44, P=1500, F=0, use_sh=True, sh_degree=3), None, (0,)),
    "ranges32": (dict(W=64, H=48, P=2000, F=32), _feature_ranges, (0,)),
    "ranges36": (dict(W=60, H=44, P=2000, F=36), _feature_ranges, (0,)),
    "frustum_cov": (dict(W=72, H=56, P=2000, F=8, use_cov=True, scale_mult=2.0), _past_frustum, (0,)),
    "rig2": (ODD37, None, (0, 9)),
}
STACKS = (63, 64, 65, 127, 128, 129)
ALL_SCENES = tuple(SCENES) + tuple(f"stack{n}" for n in STACKS)
CAMERA_KEYS = ("viewmatrix", "projmatrix", "c_x", "c_y", "tan_fovx", "tan_fovy", "campos")


def _build(name):
    if name.startswith("stack"):
        return _stack(int(name[5:]))
    kw, mutate, cams = SCENES[name]
    inps = [H.scene(**kw, cam_index=c) for c in cams]
    for inp in inps[1:]:    # one set of Gaussians, several cameras
        for k, v in inps[0].items():
            if k not in CAMERA_KEYS:
                inp[k] = v
    if mutate is not None:
        mutate(inps)
    return inps


def blend_colors(inp, st):
    return inp["colors"] if inp["colors"] is not None else st.rgb


def replay_forward(inp, rec, st, compat):
    """The fp64 forward replay over the lists of `rec` (st: the oracle state,
    whose SH colours the blend reads when the scene has no precomputed ones)."""
    return O.render_forward64(rec, inp["image_width"], inp["image_height"], blend_colors(inp, st),
                              inp["semantic_feature"], inp["bg"], compat)


def robust_inputs(inps):
    """Perturb the shared Gaussians of `inps` (one dict per camera) until no
    pixel of any camera has an undecided pair: the opacity of a Gaussian
    owning a pair near the alpha or the stop threshold is scaled by
    1 - 2^-9 (round + 1), the mean of one owning a |power| ~ 0 pair is moved
    by 1e-3 of the scene extent.  Returns the number of rounds taken."""
    extent = float(inps[0]["means3D"].abs().max())
    for rnd in range(MAX_ROUNDS + 1):
        gflag = 0
        flagged = 0
        for inp in inps:
            st = H.oracle_forward(inp, "fixed")[6]
            r = replay_forward(inp, st, st, "fixed")
            gflag = gflag | r["gflag"]
            flagged += int(np.count_nonzero(r["flag"]))
        if flagged == 0:
            return rnd
        assert rnd < MAX_ROUNDS, f"{flagged} pixels still undecided after {MAX_ROUNDS} rounds"
        op = inps[0]["opacity"].clone()
        op[torch.from_numpy((gflag & 5) != 0)] *= 1.0 - 2.0 ** -9 * (rnd + 1)
        m = inps[0]["means3D"].clone()
        m[torch.from_numpy((gflag & 2) != 0)] += 1e-3 * extent * torch.tensor([1.0, 0.5, 0.25])
        for inp in inps:
            inp["opacity"], inp["means3D"] = op.contiguous(), m.contiguous()
    raise AssertionError("unreachable")


@functools.lru_cache(maxsize=None)
def robust_scene(name):
    """-> (inputs per camera, rounds).  Cached: treat as read-only."""
    inps = _build(name)
    return inps, robust_inputs(inps)


@functools.lru_cache(maxsize=None)
def reference(name, compat, cam=0):
    """The robust scene's inputs, the C oracle's forward and the forward
    replay (cached, read-only): dict(inp, ofwd, st, fwd64, rounds, grads)."""
    inps, rounds = robust_scene(name)
    inp = inps[cam]
    ofwd = H.oracle_forward(inp, compat)
    st = ofwd[6]
    fwd64 = replay_forward(inp, st, st, compat)
    assert not fwd64["flag"].any()
    F = 0 if inp["semantic_feature"] is None else inp["semantic_feature"].shape[1]
    grads = H.upstream_grads(inp["image_height"], inp["image_width"], F, seed=1 + cam)
    return dict(inp=inp, ofwd=ofwd, st=st, fwd64=fwd64, rounds=rounds, grads=grads, F=F)


def replay_backward(ref, compat, alpha, grads=None):
    """fp64 replay of the blend backward for the backward's own alpha input."""
    inp, st = ref["inp"], ref["st"]
    return O.render_backward64(st, inp["image_width"], inp["image_height"], blend_colors(inp, st),
                               inp["semantic_feature"], inp["bg"], alpha, grads or ref["grads"], compat)


def downstream(ref, compat, up):
    """or_preprocess_bwd on the replay's upstream sums `up` (rounded to
    fp32) -> (reference values, scales s = |J| A), dicts over DOWN_NAMES."""
    inp, st = ref["inp"], ref["st"]

    def run(d2, dco, dcol, dd):
        return O.preprocess_backward(
            inp["means3D"], st.radii, inp["sh"], inp["degree"], inp["scales"], inp["rotations"],
            inp["scale_modifier"], inp["cov3D_precomp"], inp["viewmatrix"], inp["projmatrix"],
            *H.bwd_cam4(inp, compat == "reference"), inp["campos"], inp["image_width"], inp["image_height"],
            st, d2, dco, dcol, dd, compat)
    val = run(up["dmean2D"], up["dconic"], up["dcolors"], up["ddepth"])
    P = len(st.radii)
    scale = {k: np.zeros(v.shape, np.float64) for k, v in val.items()}
    parts = [("dmean2D", 2), ("dconic", 3), ("dcolors", 3), ("ddepth", 1)]
    for pi, (name, n) in enumerate(parts):
        if name == "dcolors" and inp["sh"] is None:
            continue   # colours reach preprocess_bwd only through the SH evaluation
        for j in range(n):
            args = [np.zeros((P, m)) for _, m in parts]
            args[pi][:, j] = up["A_" + name].reshape(P, n)[:, j]
            for k, v in run(*args).items():
                scale[k] += np.abs(v.astype(np.float64))
    return val, scale


# ------------------------------------------------------------ the assertion

def normalised_error(got, ref, A):
    """max |got - ref| / (u A) over the elements with A > 0 (0 if none)."""
    got, ref, A = (np.asarray(x, np.float64) for x in (got, ref, A))
    nz = A > 0
    return float((np.abs(got - ref)[nz] / (U * A[nz])).max()) if nz.any() else 0.0


def assert_elementwise(label, got, ref, A, K):
    """Every element: |got - ref| <= K u A, exactly 0 where A is 0.  Returns
    the worst normalised error; a failure names the worst element's index."""
    got, ref, A = (np.asarray(x, np.float64) for x in (got, ref, A))
    assert got.shape == ref.shape == A.shape, (label, got.shape, ref.shape, A.shape)
    if got.size == 0:
        return 0.0
    assert np.isfinite(got).all(), f"{label}: non-finite values"
    err = np.abs(got - ref)
    zero = A == 0
    if zero.any():
        i = np.unravel_index(np.argmax(np.where(zero, np.abs(got), 0)), got.shape)
        assert got[i] == 0 or not zero[i], f"{label}: element {i} has absolute sum 0 but value {got[i]!r}"
    ratio = np.where(zero, 0.0, err / (U * np.where(zero, 1.0, A)))
    i = np.unravel_index(np.argmax(ratio), ratio.shape)
    assert ratio[i] <= K, (f"{label}: element {i}: got {got[i]!r}, fp64 replay {ref[i]!r}, absolute sum {A[i]!r}: "
                           f"{ratio[i]:.1f} u A > {K:.1f} u A ({int((ratio > K).sum())} elements over)")
    return float(ratio[i])


FWD_TENSORS = ("color", "feature", "depth", "alpha")


def check_forward(label, images, fwd64, K_of, worst=None):
    """images: dict color / feature / depth / alpha -> [C,H,W] arrays."""
    for t in FWD_TENSORS:
        w = assert_elementwise(f"{label} {t} [channel, y, x]", images[t], fwd64[t], fwd64["A_" + t], K_of(t))
        if worst is not None:
            worst[t] = max(worst.get(t, 0.0), w)


def check_direct_grads(label, grads, bwd64, K_of, use_sh, worst=None):
    """grads: dict over GRAD_NAMES -> arrays (dmeans2D [P,3], dopacity [P,1])."""
    pairs = [("dmeans2D", grads["dmeans2D"][:, :2], "dmean2D"), ("dopacity", grads["dopacity"].reshape(-1), "dopacity"),
             ("dsemantic", grads["dsemantic"], "dsemantic")]
    if not use_sh:
        pairs.append(("dcolors", grads["dcolors"], "dcolors"))
    for t, got, key in pairs:
        w = assert_elementwise(f"{label} {t} [Gaussian, component]", got, bwd64[key], bwd64["A_" + key], K_of(t))
        if worst is not None:
            worst[t] = max(worst.get(t, 0.0), w)


def check_downstream(label, grads, val, scale, K, worst=None):
    for t in DOWN_NAMES:
        got = np.asarray(grads[t])
        if got.size == 0 and val[t].size == 0:
            continue
        w = assert_elementwise(f"{label} {t} [Gaussian, component]", got.reshape(val[t].shape), val[t], scale[t], K)
        if worst is not None:
            worst[t] = max(worst.get(t, 0.0), w)


def last_ids(n_contrib, ranges, point_list, W, Hh):
    return H._last_ids(np.asarray(n_contrib, np.int64), np.asarray(ranges, np.int64).reshape(-1, 2),
                       np.asarray(point_list, np.int64), W, Hh)


# ------------------------------------------- the existing aggregate criteria

def aggregate_forward_ok(images, ref):
    """tests/test_gpu_parity.py::_cmp_forward's criteria."""
    ok = H.psnr(images["color"], ref["color"]) >= 80.0
    ok &= np.mean(np.abs(images["color"] - ref["color"]) <= 1e-5) >= 0.999
    ok &= np.mean(np.abs(images["depth"] - ref["depth"]) <= 1e-5 * max(1.0, np.abs(ref["depth"]).max())) >= 0.999
    if ref["feature"].size:
        ok &= np.mean(np.abs(images["feature"] - ref["feature"]) <= 1e-5) >= 0.999
    ok &= np.mean(np.abs(images["alpha"] - ref["alpha"]) <= 1e-5) >= 0.999
    return bool(ok)


def aggregate_backward_ok(grads, ref):
    """tests/test_gpu_parity.py::test_backward_parity's criterion."""
    for k in GRAD_NAMES:
        a, b = np.asarray(grads[k]), np.asarray(ref[k])
        if b.size == 0 or not np.any(b):
            if np.any(a) and np.abs(a).max() >= 1e-6:
                return False
            continue
        if H.rel_l2(a, b) > 1e-4:
            return False
    return True
