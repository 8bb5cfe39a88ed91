"""Shared builders of the densification tests (tests/test_densify.py on the CPU,
tests/test_gpu_densify.py on the device): the fixture's cases as live
(params, variables, optimizer) triples, seeded random cases that keep the
fixture's 1e-3 margin from every threshold, and the snapshot both sides are
compared through."""
from __future__ import annotations

import os

import numpy as np
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "densify.npz")
CASES = ("i500", "i3000", "i5000", "i550", "i600")
KEYS = ("means3D", "rgb_colors", "seg_colors", "unnorm_rotations", "logit_opacities", "log_scales")
CAM_KEYS = ("cam_m", "cam_c")
STATS = ("means2D_gradient_accum", "denom", "max_2D_radius")
GRAD_THRESH = 0.0002
MARGIN = 1e-3
TRANSFORMED = ("means3D", "log_scales")  # what a split computes; everything else is copied


def build(tensors: dict, moments: dict, steps: dict, stats: dict, scene_radius: float, *, device="cpu",
          dtype=torch.float32, optim_cls=torch.optim.Adam, seen=None, means2D_grad=None, no_group=(), misalign=(),
          lr=1e-3):
    """(params, variables, optimizer) from plain tensors: one named group per key (except
    `no_group`), state = {'step', 'exp_avg', 'exp_avg_sq'} where `moments` has the key."""
    params, groups = {}, []
    for k, v in tensors.items():
        v = v.to(device=device, dtype=dtype).contiguous().clone()
        if k in misalign:  # one float into a larger buffer: 4-byte aligned, not 16
            buf = torch.empty(v.numel() + 1, device=device, dtype=dtype)
            buf[1:].copy_(v.reshape(-1))
            v = buf[1:].view(v.shape)
            assert v.is_contiguous() and (torch.device(device).type == "cpu" or v.data_ptr() % 16 == 4)
        if k in no_group:
            params[k] = v
        else:
            params[k] = torch.nn.Parameter(v)
            groups.append({"params": [params[k]], "name": k, "lr": lr})
    opt = optim_cls(groups, lr=0.0, eps=1e-15)
    for k, (m, v) in moments.items():
        opt.state[params[k]] = {"step": torch.tensor(float(steps[k]), dtype=torch.float32),
                                "exp_avg": m.to(device=device, dtype=dtype).contiguous().clone(),
                                "exp_avg_sq": v.to(device=device, dtype=dtype).contiguous().clone()}
    variables = {k: stats[k].to(device).contiguous().clone() for k in STATS}
    variables["scene_radius"] = scene_radius
    if seen is not None:
        variables["seen"] = seen.to(device)
        means2D = torch.zeros(seen.numel(), 3, device=device, dtype=dtype, requires_grad=True)
        means2D.grad = means2D_grad.to(device=device, dtype=dtype).contiguous().clone()
        variables["means2D"] = means2D
    return params, variables, opt


def fixture_parts(gold, name):
    t = lambda k: torch.from_numpy(gold[k])  # noqa: E731
    pre = f"{name}.in"
    tensors = {k: t(f"{pre}.{k}") for k in KEYS + CAM_KEYS}
    moments = {k: (t(f"{pre}.{k}.exp_avg"), t(f"{pre}.{k}.exp_avg_sq")) for k in KEYS + CAM_KEYS}
    steps = {k: float(gold[f"{pre}.{k}.step"]) for k in KEYS + CAM_KEYS}
    stats = {k: t(f"{pre}.{k}") for k in STATS}
    return dict(tensors=tensors, moments=moments, steps=steps, stats=stats,
                scene_radius=float(gold[f"{pre}.scene_radius"]), seen=t(f"{pre}.seen"),
                means2D_grad=t(f"{pre}.means2D_grad")), int(gold[f"{name}.i"]), t(f"{name}.z")


def snapshot(params, variables, optimizer) -> dict:
    """Every output as CPU tensors: parameters, '<key>.exp_avg' / '.exp_avg_sq' / '.step' of
    every group with state, and the statistics."""
    out = {k: v.detach().cpu().clone() for k, v in params.items()}
    for g in optimizer.param_groups:
        st = optimizer.state.get(g["params"][0], None)
        if st and "exp_avg" in st:
            out[g["name"] + ".exp_avg"] = st["exp_avg"].detach().cpu().clone()
            out[g["name"] + ".exp_avg_sq"] = st["exp_avg_sq"].detach().cpu().clone()
            out[g["name"] + ".step"] = torch.as_tensor(float(st["step"]))
    for k in STATS:
        out[k] = variables[k].detach().cpu().clone()
    return out


def assert_margins(log_scales, logit_opacities, accum, denom, scene_radius, i, exact_rows=0):
    """The fixture's margin condition, on CPU values: nothing within 1e-3 relative of a
    threshold it is compared with, except `exact_rows` rows with accum / denom == grad_thresh."""
    def clear(x, thresh, what, allow_equal=0):
        near = ((x - thresh).abs() / thresh < MARGIN) & torch.isfinite(x)
        equal = int((x == thresh).sum())
        assert int(near.sum()) - equal == 0 and equal == allow_equal, (what, int(near.sum()), equal)

    g = accum / denom
    g = torch.where(g.isnan(), torch.zeros_like(g), g)
    clear(g, float(torch.tensor(GRAD_THRESH, dtype=torch.float32)), "gradient", exact_rows)
    s = torch.exp(log_scales.detach().float()).max(dim=1).values
    clear(s, 0.01 * scene_radius, "clone / split scale")
    clear(s, 0.1 * scene_radius, "big scale")
    clear(s / 1.6, 0.1 * scene_radius, "big scale of a split copy")
    o = torch.sigmoid(logit_opacities.detach().float()).reshape(-1)
    clear(o, 0.25 if i == 5000 else 0.005, "opacity")


def _pick(gen, n, ranges, weights):
    which = torch.multinomial(torch.tensor(weights, dtype=torch.float32), n, replacement=True, generator=gen)
    lo = torch.tensor([r[0] for r in ranges])[which]
    hi = torch.tensor([r[1] for r in ranges])[which]
    return torch.exp(torch.log(lo) + torch.rand(n, generator=gen) * (torch.log(hi) - torch.log(lo)))


def random_parts(P, seed, *, hot=0.5, split=0.5, faint=0.15, big=0.1, extra=None, moments_for=None,
                 scene_radius=2.0):
    """A seeded case of P Gaussians: a fraction `hot` over the gradient threshold, `split` of
    them too large to clone, `faint` below every opacity threshold, `big` above the big-point
    scale (half of those so large that their split copies go too).  `extra` = {key: width} adds
    plain per-Gaussian tensors.  Values are drawn from ranges that stay 2 % clear of every
    threshold."""
    gen = torch.Generator().manual_seed(seed)
    small = max(0.0, 1.0 - split - big)
    smax = _pick(gen, P, [(0.004, 0.019), (0.022, 0.18), (0.22, 0.30), (0.36, 0.6)],
                 [small + 1e-9, split + 1e-9, big / 2 + 1e-9, big / 2 + 1e-9])
    scales = smax[:, None] * (0.3 + 0.7 * torch.rand(P, 3, generator=gen))
    scales[torch.arange(P), torch.randint(0, 3, (P,), generator=gen)] = smax
    opac = _pick(gen, P, [(0.0005, 0.004), (0.3, 0.95)], [faint + 1e-9, 1.0 - faint + 1e-9])
    tensors = {"means3D": torch.randn(P, 3, generator=gen),
               "rgb_colors": torch.rand(P, 3, generator=gen),
               "seg_colors": torch.rand(P, 3, generator=gen),
               "unnorm_rotations": torch.randn(P, 4, generator=gen) * torch.exp(0.3 * torch.randn(P, 1, generator=gen)),
               "logit_opacities": torch.log(opac / (1 - opac))[:, None],
               "log_scales": torch.log(scales)}
    for k, w in (extra or {}).items():
        tensors[k] = torch.randn(P, w, generator=gen)
    tensors = {k: v.float().contiguous() for k, v in tensors.items()}
    denom = torch.randint(1, 12, (P,), generator=gen).float()
    g = _pick(gen, P, [(2e-5, 1.6e-4), (2.5e-4, 2e-3)], [1.0 - hot + 1e-9, hot + 1e-9])
    stats = {"means2D_gradient_accum": (g * denom).float(), "denom": denom,
             "max_2D_radius": torch.rand(P, generator=gen) * 40.0}
    names = list(tensors) if moments_for is None else list(moments_for)
    moments = {k: (0.01 * torch.randn(tensors[k].shape, generator=gen),
                   1e-4 * torch.rand(tensors[k].shape, generator=gen)) for k in names}
    steps = {k: 3.0 + n for n, k in enumerate(names)}
    return dict(tensors=tensors, moments=moments, steps=steps, stats=stats, scene_radius=scene_radius)


def parts_margins(parts, i, exact_rows=0):
    assert_margins(parts["tensors"]["log_scales"], parts["tensors"]["logit_opacities"],
                   parts["stats"]["means2D_gradient_accum"], parts["stats"]["denom"], parts["scene_radius"], i,
                   exact_rows)


def to_numpy(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
