#!/usr/bin/env python3
"""Generate tests/golden/densify.npz from the REFERENCE's own Python code (run
where the reference checkout exists; the fixture -- data only -- is committed,
the reference never travels).

The reference's densify(params, variables, optimizer, i) (external.py:244-292)
is loaded as make_golden.py loads such modules: an empty placeholder for
Open3D while it imports, and its hard-coded device="cuda" redirected to the
CPU.  In that module's view torch.normal(mean, std) is mean + std * z with z
from a seeded generator, recorded: that is what ATen's tensor-tensor normal
computes, and it lets a later run start from the same noise.  Everything runs
in fp32 on the CPU under torch.optim.Adam, whose moments and step counts come
from three real steps on random gradients.

Cases (all seeded), the six reference keys plus cam_m / cam_c:
  i500   P 300  mixed clone, split and prune
  i3000  P 200  the big-point prune and the opacity reset
  i5000  P 200  the 0.25 opacity threshold
  i550   P 100  accumulate only
  i600   P 100  nothing qualifies: every gradient below the threshold, every
                opacity above it

Recorded per case: the inputs (parameters, both moments and step count of
each, the statistics, seen, means2D.grad, scene_radius), z, and every output.

Margin condition, asserted here: no compared quantity (accum / denom after the
accumulation, the largest scale and that of a split copy, the opacity) sits
within 1e-3 relative of the threshold it is compared with, so the fixture does
not depend on one ulp of exp.  The exception is one deliberate row per
case but i600 with accum / denom == grad_thresh exactly (IEEE division),
which `>=` includes.

Usage: python tests/golden/make_golden_densify.py --reference <reference checkout>
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests.golden.make_golden import _TorchOnCPUAll, _load_with_placeholders  # noqa: E402

CASES = {"i500": (500, 300, 21), "i3000": (3000, 200, 22), "i5000": (5000, 200, 23), "i550": (550, 100, 24),
         "i600": (600, 100, 25)}
KEYS = ("means3D", "rgb_colors", "seg_colors", "unnorm_rotations", "logit_opacities", "log_scales")
CAM_KEYS = ("cam_m", "cam_c")
STATS = ("means2D_gradient_accum", "denom", "max_2D_radius")
GRAD_THRESH = 0.0002
SCENE_RADIUS = 2.0
MARGIN = 1e-3


class _TorchRecordedNormal(_TorchOnCPUAll):
    """torch as external.py sees it: on the CPU, with normal(mean, std) = mean + std * z."""

    def __init__(self, name, gen):
        super().__init__(name)
        self._gen = gen
        self.recorded = []

    def normal(self, mean, std):
        z = torch.randn(std.shape, generator=self._gen, dtype=std.dtype)
        self.recorded.append(z)
        return mean + std * z


def _pick(gen, n, ranges, weights):
    """n values, each log-uniform in one of `ranges` chosen with `weights`."""
    which = torch.multinomial(torch.tensor(weights, dtype=torch.float32), n, replacement=True, generator=gen)
    lo = torch.tensor([r[0] for r in ranges])[which]
    hi = torch.tensor([r[1] for r in ranges])[which]
    return torch.exp(torch.log(lo) + torch.rand(n, generator=gen) * (torch.log(hi) - torch.log(lo)))


def case_inputs(name):
    i, P, seed = CASES[name]
    gen = torch.Generator().manual_seed(seed)
    quiet = name == "i600"
    # largest scale: clone range, split range, big (its copies survive), huge (its copies do not)
    smax = _pick(gen, P, [(0.004, 0.019), (0.022, 0.18), (0.22, 0.30), (0.36, 0.6)], [4, 4, 1, 1])
    scales = smax[:, None] * (0.3 + 0.7 * torch.rand(P, 3, generator=gen))
    scales[torch.arange(P), torch.randint(0, 3, (P,), generator=gen)] = smax
    opac = _pick(gen, P, [(0.0005, 0.004), (0.007, 0.2), (0.3, 0.95)], [0, 0, 1] if quiet else [1, 2, 5])
    params = {
        "means3D": torch.randn(P, 3, generator=gen),
        "rgb_colors": torch.rand(P, 3, generator=gen),
        "seg_colors": torch.rand(P, 3, generator=gen),
        "unnorm_rotations": torch.randn(P, 4, generator=gen) * torch.exp(0.3 * torch.randn(P, 1, generator=gen)),
        "logit_opacities": torch.log(opac / (1 - opac))[:, None],
        "log_scales": torch.log(scales),
        "cam_m": 0.05 * torch.randn(5, 3, generator=gen),
        "cam_c": 0.05 * torch.randn(5, 3, generator=gen),
    }
    params = {k: torch.nn.Parameter(v.float().contiguous()) for k, v in params.items()}
    # statistics before this iteration's accumulation
    denom = torch.randint(0, 12, (P,), generator=gen).float()
    g = _pick(gen, P, [(2e-5, 1.6e-4), (2.5e-4, 2e-3)], [1, 0] if quiet else [1, 1])
    accum = (g * denom).float()
    seen = torch.rand(P, generator=gen) < 0.7
    m2d_grad = torch.zeros(P, 3)
    m2d_grad[:, :2] = (g[:, None] * (0.5 + torch.rand(P, 2, generator=gen)) * 0.7).float()
    if quiet:  # the accumulation must leave every mean below the threshold too
        m2d_grad *= 0.5
    never = denom == 0  # NaN -> not densified; a few with a gradient but no count: Inf -> densified
    accum[never] = 0.0
    seen[never] = False
    if not quiet:
        inf_rows = torch.nonzero(never).reshape(-1)[:2]
        accum[inf_rows] = 1e-3
        exact = int(torch.nonzero(~never).reshape(-1)[7])
        denom[exact], seen[exact] = 4.0, False
        accum[exact] = torch.tensor(GRAD_THRESH, dtype=torch.float32) * 4.0
        assert float(accum[exact] / denom[exact]) == float(torch.tensor(GRAD_THRESH, dtype=torch.float32))
    variables = {"means2D_gradient_accum": accum, "denom": denom,
                 "max_2D_radius": torch.rand(P, generator=gen) * 40.0, "scene_radius": SCENE_RADIUS,
                 "seen": seen, "means2D_grad": m2d_grad}
    return i, gen, params, variables


def real_steps(params, gen):
    """torch.optim.Adam as train.py:119-135 builds it; three steps on random gradients."""
    groups = [{"params": [v], "name": k, "lr": 1e-4} for k, v in params.items()]
    opt = torch.optim.Adam(groups, lr=0.0, eps=1e-15)
    for _ in range(3):
        for v in params.values():
            v.grad = torch.randn(v.shape, generator=gen) * 0.01
        opt.step()
    opt.zero_grad(set_to_none=True)
    return opt


def check_margins(name, params, accum, denom, i):
    """The margin condition on the values densify() compares (after the accumulation)."""
    def clear(x, thresh, what, allow_equal=0):
        rel = ((x - thresh).abs() / thresh)
        near = (rel < MARGIN) & torch.isfinite(x)
        equal = int((x == thresh).sum())
        assert int(near.sum()) - equal == 0 and equal == allow_equal, (name, what, int(near.sum()), equal)

    g = accum / denom
    g[g.isnan()] = 0.0
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))  # noqa: E731
    clear(g, f32(GRAD_THRESH), "grad", allow_equal=0 if name == "i600" else 1)
    s = torch.exp(params["log_scales"].detach()).max(dim=1).values
    clear(s, 0.01 * SCENE_RADIUS, "clone/split scale")
    clear(s, 0.1 * SCENE_RADIUS, "big scale")
    clear(s / 1.6, 0.1 * SCENE_RADIUS, "big scale of a split copy")
    o = torch.sigmoid(params["logit_opacities"].detach()).reshape(-1)
    clear(o, 0.25 if i == 5000 else 0.005, "opacity")
    clear(o, 0.005, "opacity 0.005")


def snapshot(prefix, params, opt, variables, out):
    for k, v in params.items():
        out[f"{prefix}.{k}"] = v.detach().numpy().copy()
    for grp in opt.param_groups:
        st = opt.state.get(grp["params"][0], None)
        k = grp["name"]
        if st is not None and "exp_avg" in st:
            out[f"{prefix}.{k}.exp_avg"] = st["exp_avg"].numpy().copy()
            out[f"{prefix}.{k}.exp_avg_sq"] = st["exp_avg_sq"].numpy().copy()
            out[f"{prefix}.{k}.step"] = np.float32(float(st["step"]))
    for k in STATS:
        out[f"{prefix}.{k}"] = variables[k].numpy().copy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference (external.py)")
    a = ap.parse_args()
    ex = _load_with_placeholders("ref_external_densify", os.path.join(a.reference, "external.py"))
    out = {}
    for name in CASES:
        i, gen, params, variables = case_inputs(name)
        opt = real_steps(params, gen)
        snapshot(f"{name}.in", params, opt, variables, out)
        out[f"{name}.in.seen"] = variables["seen"].numpy().copy()
        out[f"{name}.in.means2D_grad"] = variables["means2D_grad"].numpy().copy()
        out[f"{name}.in.scene_radius"] = np.float64(SCENE_RADIUS)
        out[f"{name}.i"] = np.int64(i)
        # the values the tests compare, after accumulate_mean2d_gradient
        seen = variables["seen"]
        acc = variables["means2D_gradient_accum"].clone()
        den = variables["denom"].clone()
        acc[seen] += torch.norm(variables["means2D_grad"][seen, :2], dim=-1)
        den[seen] += 1
        check_margins(name, params, acc, den, i)

        shim = _TorchRecordedNormal("torch", torch.Generator().manual_seed(1000 + i))
        ex.torch = shim
        means2D = torch.zeros_like(params["means3D"].detach(), requires_grad=True)
        means2D.grad = variables.pop("means2D_grad")
        variables["means2D"] = means2D
        P0 = params["means3D"].shape[0]
        params, variables = ex.densify(params, variables, opt, i)
        assert len(shim.recorded) <= 1
        z = shim.recorded[0] if shim.recorded else torch.zeros(0, 3)
        out[f"{name}.z"] = z.numpy().copy()
        snapshot(f"{name}.out", params, opt, variables, out)
        assert all(v.dtype == torch.float32 for v in params.values())
        print(f"{name}: i {i}  P {P0} -> {params['means3D'].shape[0]}  split sources {z.shape[0] // 2}")
    path = os.path.join(HERE, "densify.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("wrote", path, size, "bytes")
    assert size < 512 * 1024


if __name__ == "__main__":
    main()
