"""Densification on the GPU (csrc/gs_densify.hip) against densify_torch on the CPU, given
the same inputs and the same noise z.

What is compared, for every output (parameters, both moments and the step count of each, the
three statistics):
  * structure (length, row order) exactly;
  * copied values bit for bit: every tensor but means3D / log_scales, and in those two every
    row that is a copy (a kept original or a clone);
  * transformed values (the split rows of means3D and log_scales, and the accumulated
    gradient norms of an accumulate-only iteration) within ENVELOPE = 10 x the
    error of the fp32 CPU restatement itself against an fp64 evaluation of the same formulas,
    with a floor of 4 ulp of the value: the project's envelope convention
    (tests/test_gpu_envelope.py).  No output row is excluded.
Every randomly built case asserts, on its CPU values, the fixture's margin condition: nothing
within 1e-3 relative of a threshold it is compared with, so one ulp of exp cannot change the
structure.

Shapes are the small ones at which the kernels can go wrong: the scan workgroup covers
B = gs_densify_scan_block() Gaussians, so P runs over 1, 2, 63, 64, 65, B - 1, B, B + 1,
3B + 17, and one P past the first boundary of the block-sum scan (B * gs_densify_scan_tile()).
"""
from __future__ import annotations

import functools
import importlib

import numpy as np
import pytest
import torch

from dynamic3dgaussians_amd import _lib, densify, densify_torch
from dynamic3dgaussians_amd.optim import FusedAdam
from tests import _densify_cases as C

D = importlib.import_module("dynamic3dgaussians_amd.densify")
pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ENVELOPE, FLOOR_ULP = 10.0, 4.0
# what the device computes: the split rows, and the accumulated gradient norms of an iteration
# that only accumulates; everything else is copied or zero
COMPUTED = C.TRANSFORMED + ("means2D_gradient_accum",)


@functools.lru_cache(maxsize=None)
def _gold():
    return np.load(C.GOLD)


def _ulp(x: torch.Tensor) -> torch.Tensor:
    """The fp32 spacing at |x| (x fp64)."""
    x32 = x.abs().float()
    return (torch.nextafter(x32, torch.full_like(x32, float("inf"))) - x32).double()


def _oracle(parts, i, z, accumulate, dtype=torch.float32, **kw):
    params, variables, opt = C.build(**parts, dtype=dtype, **kw)
    noise = None if z is None else z.to(dtype)
    params, variables = densify_torch(params, variables, opt, i, accumulate=accumulate, noise=noise)
    return C.snapshot(params, variables, opt), (params, variables, opt)


def _device(parts, i, z, accumulate, optim_cls=torch.optim.Adam, **kw):
    params, variables, opt = C.build(**parts, device=DEV, optim_cls=optim_cls, **kw)
    noise = None if z is None else z.to(DEV)
    params, variables = densify(params, variables, opt, i, accumulate=accumulate, noise=noise)
    return C.snapshot(params, variables, opt), (params, variables, opt)


def _compare(got, want32, want64, inputs, label=""):
    assert set(got) == set(want32), (label, set(got) ^ set(want32))
    report = {}
    for k, w in want32.items():
        g = got[k]
        assert tuple(g.shape) == tuple(w.shape), (label, k, tuple(g.shape), tuple(w.shape))
        assert g.dtype == w.dtype, (label, k)
        if k not in COMPUTED or g.numel() == 0:
            assert torch.equal(g, w), (label, k)
            continue
        rows_in, rows = inputs[k].reshape(inputs[k].shape[0], -1), w.reshape(w.shape[0], -1)
        is_copy = torch.zeros(w.shape[0], dtype=torch.bool)
        for lo in range(0, w.shape[0], 2048):  # a row that exists in the input is a copy
            is_copy[lo:lo + 2048] = (rows[lo:lo + 2048, None, :] == rows_in[None]).all(-1).any(-1)
        assert torch.equal(g[is_copy], w[is_copy]), (label, k, "copied rows")
        w64 = want64[k]
        env = float((w.double() - w64).abs().max())
        err = (g.double() - w64).abs()
        tol = torch.maximum(torch.full_like(err, ENVELOPE * env), FLOOR_ULP * _ulp(w64))
        report[k] = (float(err.max()), env)
        print(f"{label} {k}: max error {float(err.max()):.3e}, restatement's own {env:.3e}, "
              f"split rows {int((~is_copy).sum())}")
        assert bool((err <= tol).all()), (label, k, float(err.max()), env)
    return report


def _check(parts, i, z, accumulate=False, label="", **kw):
    want32, _ = _oracle(parts, i, z, accumulate, **kw)
    want64, _ = _oracle(parts, i, z, accumulate, dtype=torch.float64, **kw)
    got, live = _device(parts, i, z, accumulate, **kw)
    _compare(got, want32, want64, {**parts["tensors"], **parts["stats"]}, label)
    return got, want32, live


def _noise_for(parts, i, seed=0):
    """z for the case, sized by the oracle's own classification."""
    sch = D.schedule(i)
    t, s, r = parts["tensors"], parts["stats"], parts["scene_radius"]
    flags = D.classify_torch(s["means2D_gradient_accum"], s["denom"], t["log_scales"], t["logit_opacities"],
                             grad_thresh=C.GRAD_THRESH, clone_max_scale=0.01 * r,
                             prune_min_opacity=sch["remove_threshold"],
                             prune_max_scale=0.1 * r if sch["big_points"] else 0.0)
    n = int(((flags & _lib.GS_DENSIFY_SPLIT) != 0).sum())
    return torch.randn(2 * n, 3, generator=torch.Generator().manual_seed(seed)), flags


@pytest.mark.parametrize("name", C.CASES)
def test_fixture_cases_on_the_device(name):
    parts, i, z = C.fixture_parts(_gold(), name)
    got, want32, _ = _check(parts, i, z if z.numel() else None, accumulate=True, label=name)
    # the oracle is the fixture (pinned on the CPU by tests/test_densify.py); the length once more
    assert got["means3D"].shape[0] == _gold()[f"{name}.out.means3D"].shape[0]


def _scan_sizes():
    L = _lib.load()
    B, T = L.gs_densify_scan_block(), L.gs_densify_scan_tile()
    return [1, 2, 63, 64, 65, B - 1, B, B + 1, 3 * B + 17, B * T + 17]


@pytest.mark.parametrize("n", range(10))
def test_scan_boundaries(n):
    """Flags, the four exclusive ranks and the four totals of the plan against a cumulative sum,
    and (below the block-sum boundary) the whole pass against the oracle."""
    P = _scan_sizes()[n]
    density = [(0.5, 0.5), (0.9, 0.1), (0.1, 0.8), (0.5, 0.3)][n % 4]  # seeded flags of mixed density
    parts = C.random_parts(P, 40 + n, hot=density[0], split=density[1])
    C.parts_margins(parts, 3000)
    z, flags = _noise_for(parts, 3000, seed=n)
    t, s, r = parts["tensors"], parts["stats"], parts["scene_radius"]
    ws, counts = D.plan(s["means2D_gradient_accum"].to(DEV), s["denom"].to(DEV), t["log_scales"].to(DEV),
                        t["logit_opacities"].to(DEV), grad_thresh=C.GRAD_THRESH, clone_max_scale=0.01 * r,
                        prune_min_opacity=0.005, prune_max_scale=0.1 * r)
    assert torch.equal(D.plan_flags(ws, P).cpu(), flags)
    bit = lambda b: (flags & b) != 0  # noqa: E731
    split, prune = bit(_lib.GS_DENSIFY_SPLIT), bit(_lib.GS_DENSIFY_PRUNE)
    sets = torch.stack([~split & ~prune, bit(_lib.GS_DENSIFY_CLONE) & ~prune, split,
                        split & ~bit(_lib.GS_DENSIFY_PRUNE_SPLIT)], dim=1).to(torch.int32)
    incl = sets.cumsum(0, dtype=torch.int32)
    assert torch.equal(D.plan_ranks(ws, P).cpu(), incl - sets)
    assert counts == incl[-1].tolist()
    if P <= 8192:
        _check(parts, 3000, z, label=f"P={P}")


@pytest.mark.parametrize("outcome", ["nothing", "all_cloned", "all_split", "all_pruned"])
def test_degenerate_outcomes(outcome):
    P = 1500
    kw = {"nothing": dict(hot=0, faint=0, big=0), "all_cloned": dict(hot=1, split=0, big=0, faint=0),
          "all_split": dict(hot=1, split=1, big=0, faint=0), "all_pruned": dict(faint=1)}[outcome]
    i = 600
    parts = C.random_parts(P, 70, **kw)
    C.parts_margins(parts, i)
    z, _ = _noise_for(parts, i)
    got, want32, (params, variables, opt) = _check(parts, i, z if z.numel() else None, label=outcome)
    n = got["means3D"].shape[0]
    assert n == {"nothing": P, "all_cloned": 2 * P, "all_split": 2 * P, "all_pruned": 0}[outcome]
    for k in C.KEYS:
        assert isinstance(params[k], torch.nn.Parameter) and params[k].grad is None and params[k].shape[0] == n
        assert [g for g in opt.param_groups if g["name"] == k][0]["params"][0] is params[k]
    for k in C.STATS:
        assert variables[k].shape == (n,) and not variables[k].any()
    if outcome == "nothing":  # every output equals its input bit for bit
        for k in C.KEYS:
            assert torch.equal(got[k], parts["tensors"][k]), k
            assert torch.equal(got[k + ".exp_avg"], parts["moments"][k][0]), k
            assert torch.equal(got[k + ".exp_avg_sq"], parts["moments"][k][1]), k
    if outcome == "all_cloned":
        assert torch.equal(got["means3D"][P:], parts["tensors"]["means3D"]) and not got["means3D.exp_avg"][P:].any()
    if outcome == "all_split":
        assert not got["rgb_colors.exp_avg_sq"].any()
        assert torch.equal(got["rgb_colors"], parts["tensors"]["rgb_colors"].repeat(2, 1))


def test_statistics_edge_cases():
    """denom = 0 with accum = 0 (NaN -> not densified), denom = 0 with accum > 0 (Inf -> densified),
    and accum / denom == grad_thresh exactly (densified: >=)."""
    P = 200
    parts = C.random_parts(P, 90, hot=0.3, faint=0, big=0)
    acc, den = parts["stats"]["means2D_gradient_accum"], parts["stats"]["denom"]
    den[:6] = 0.0
    acc[:3] = 0.0
    acc[3:6] = 1e-3
    thresh = torch.tensor(C.GRAD_THRESH, dtype=torch.float32)
    den[10], acc[10] = 4.0, thresh * 4.0
    assert float(acc[10] / den[10]) == float(thresh)
    C.parts_margins(parts, 500, exact_rows=1)
    z, flags = _noise_for(parts, 500)
    hot = (flags & (_lib.GS_DENSIFY_CLONE | _lib.GS_DENSIFY_SPLIT)) != 0
    assert not hot[:3].any() and hot[3:6].all() and hot[10]
    ws, _ = D.plan(acc.to(DEV), den.to(DEV), parts["tensors"]["log_scales"].to(DEV),
                   parts["tensors"]["logit_opacities"].to(DEV), grad_thresh=C.GRAD_THRESH,
                   clone_max_scale=0.01 * parts["scene_radius"], prune_min_opacity=0.005)
    assert torch.equal(D.plan_flags(ws, P).cpu(), flags)
    _check(parts, 500, z, label="stats edges")


def test_widths_alignment_and_missing_moments():
    """Widths 1, 3, 4, 32 and 35; a width-32 tensor and a width-4 tensor handed in one float into
    a larger buffer (4-byte, not 16-byte aligned); a group whose state does not exist yet; a
    tensor with no group at all."""
    P = 1100  # more than one scan workgroup and more than one chunk of every tensor
    extra = {"semantic_feature": 32, "f35": 35, "f32_odd": 32, "f4": 4, "f4_odd": 4, "f1": 1, "lazy32": 32,
             "const3": 3}
    have = [k for k in list(C.KEYS) + list(extra) if k not in ("lazy32", "const3")]
    parts = C.random_parts(P, 110, extra=extra, moments_for=have)
    C.parts_margins(parts, 500)
    z, _ = _noise_for(parts, 500)
    kw = dict(no_group=("const3",), misalign=("f32_odd", "f4_odd"))
    got, want32, (params, variables, opt) = _check(parts, 500, z, label="widths", **kw)
    n = got["means3D"].shape[0]
    assert n != P
    for k, w in extra.items():
        assert got[k].shape == (n, w)
    assert "lazy32.exp_avg" not in got and "const3.exp_avg" not in got
    assert isinstance(params["lazy32"], torch.nn.Parameter) and not isinstance(params["const3"], torch.nn.Parameter)
    assert len(opt.state.get(params["lazy32"], {})) == 0


def _weights(shape, dev):
    return torch.sin(torch.arange(int(np.prod(shape)), dtype=torch.float32) * 0.37).view(shape).to(dev)


@pytest.mark.parametrize("optim_cls", [torch.optim.Adam, FusedAdam], ids=["Adam", "FusedAdam"])
def test_optimizers_and_the_step_after(optim_cls):
    """densify under torch.optim.Adam and under FusedAdam, then one backward + step on the new
    parameters against the same step (torch.optim.Adam on the CPU) on the oracle's output.
    Tolerance: rtol 1e-6 / atol 1e-7, that of the CPU fixture test for the transformed values;
    the step adds at most lr = 1e-3 times a few ulps to it."""
    P = 700
    parts = C.random_parts(P, 130, extra={"semantic_feature": 32})
    C.parts_margins(parts, 500)
    z, _ = _noise_for(parts, 500)
    want32, (op, ov, oopt) = _oracle(parts, 500, z, False)
    want64, _ = _oracle(parts, 500, z, False, dtype=torch.float64)
    got, (gp, gv, gopt) = _device(parts, 500, z, False, optim_cls=optim_cls)
    _compare(got, want32, want64, {**parts["tensors"], **parts["stats"]}, optim_cls.__name__)
    for params, opt, dev in ((op, oopt, "cpu"), (gp, gopt, DEV)):
        loss = sum((p * _weights(p.shape, dev)).sum() for p in params.values())
        loss.backward()
        opt.step()
    after_cpu, after_dev = C.snapshot(op, ov, oopt), C.snapshot(gp, gv, gopt)
    assert set(after_cpu) == set(after_dev)
    for k, w in after_cpu.items():
        torch.testing.assert_close(after_dev[k], w, rtol=1e-6, atol=1e-7, msg=lambda m: f"{k}: {m}")  # noqa: B023
        if k.endswith(".step"):
            assert float(after_dev[k]) == parts["steps"][k[:-5]] + 1
    assert not torch.equal(after_dev["means3D"], got["means3D"])  # the step moved the new parameters


def test_determinism():
    P = 2500
    parts = C.random_parts(P, 150, extra={"semantic_feature": 32})
    C.parts_margins(parts, 3000)
    z, _ = _noise_for(parts, 3000)
    a, _ = _device(parts, 3000, z, False)
    b, _ = _device(parts, 3000, z, False)
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert bool((a["logit_opacities"] == a["logit_opacities"][0]).all())  # i = 3000: the reset, folded in


def test_generated_noise_and_accumulation():
    """Without `noise` the wrapper draws it on the device from `generator`: two runs from one
    seed agree, and the HIP accumulation equals the oracle's."""
    parts, i, _z = C.fixture_parts(_gold(), "i550")
    got, want32, _ = _check(parts, i, None, accumulate=True, label="accumulate")
    assert not torch.equal(got["denom"], parts["stats"]["denom"])
    parts = C.random_parts(900, 170)
    C.parts_margins(parts, 500)
    outs = []
    for _ in range(2):
        params, variables, opt = C.build(**parts, device=DEV)
        params, variables = densify(params, variables, opt, 500, accumulate=False,
                                    generator=torch.Generator(device=DEV).manual_seed(5))
        outs.append(C.snapshot(params, variables, opt))
    assert all(torch.equal(outs[0][k], outs[1][k]) for k in outs[0])


def test_driver_step_with_the_hip_callback():
    """One TimestepDriver step at t = 0, i = 500 on a small scene with densify as the callback
    equals the same step with densify_torch as the callback.  The new Parameters carry no .grad,
    so the step after the callback leaves them as densification wrote them."""
    from dynamic3dgaussians_amd.camera import camera_rig
    from dynamic3dgaussians_amd.rasterizer import GaussianRasterizationSettings
    from dynamic3dgaussians_amd.timesteps import TimestepDriver, batch_renderer

    n_cams, W, H, P = 3, 96, 64, 1500
    settings = [GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=c.tanfovx, tanfovy=c.tanfovy, c_x=c.c_x, c_y=c.c_y,
        bg=torch.zeros(3, device=DEV), viewmatrix=torch.from_numpy(c.viewmatrix.copy()).to(DEV),
        projmatrix=torch.from_numpy(c.projmatrix.copy()).to(DEV), sh_degree=0,
        campos=torch.from_numpy(c.campos.copy()).to(DEV), compat="reference")
        for c in camera_rig(n_cams, W, H, seed=3)]
    parts = C.random_parts(P, 190)
    parts["tensors"]["means3D"] *= 0.5
    parts["tensors"].pop("seg_colors")
    parts["moments"].pop("seg_colors")
    parts["stats"]["denom"] += 20.0  # one step's increments cannot carry a mean across the threshold
    parts["stats"]["means2D_gradient_accum"] *= parts["stats"]["denom"] / (parts["stats"]["denom"] - 20.0)
    targets = torch.rand(n_cams, 3, H, W, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    seen_margins = []

    def callback(fn):
        def run(params, variables, optimizer, i):
            C.assert_margins(params["log_scales"].cpu(), params["logit_opacities"].cpu(),
                             variables["means2D_gradient_accum"].cpu(), variables["denom"].cpu(),
                             float(variables["scene_radius"]), i)
            seen_margins.append(i)
            return fn(params, variables, optimizer, i, accumulate=False,
                      generator=torch.Generator(device=DEV).manual_seed(11))
        return run

    outs = []
    for fn in (densify, densify_torch):
        params, variables, opt = C.build(**parts, device=DEV)
        drv = TimestepDriver(params, variables, opt, n_cams, batch_renderer(settings), densify=callback(fn))
        loss = drv.step(targets, t=0, i=500)
        assert np.isfinite(loss)
        outs.append(C.snapshot(drv.params, drv.variables, opt))
        assert drv.params["means3D"].shape[0] != P
    assert seen_margins == [500, 500]
    hip, ref = outs
    assert set(hip) == set(ref)
    for k, w in ref.items():
        assert hip[k].shape == w.shape, k  # the structure, exactly
        if k in C.TRANSFORMED:
            torch.testing.assert_close(hip[k], w, rtol=1e-6, atol=1e-7)
        else:
            assert torch.equal(hip[k], w), k
