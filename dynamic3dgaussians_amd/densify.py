"""The reference's densification (external.py:244-292) on the HIP kernels of
csrc/gs_densify.hip (C ABI include/gs_densify.h): clone, split and prune every
per-Gaussian tensor and the Adam moments that belong to it with one plan (a
classification and a prefix scan), one readback of four counts and ONE gather
launch, instead of three rounds of boolean-mask indexing and torch.cat.

    params, variables = densify(params, variables, optimizer, i)

has the reference's signature and schedule, so it is the `densify` a training
loop calls after backward() and before optimizer.step().  For the
`TimestepDriver`, which accumulates the statistics itself, pass

    TimestepDriver(..., densify=functools.partial(densify, accumulate=False))

Output rows are the reference's, row for row:

    [ kept originals | kept clones | kept split copy 0 | kept split copy 1 ]

each block in source-index order.  Originals keep parameter and moments bit for
bit, clones and split copies start with zero moments, and copy j of the split
source with rank r among ALL split sources (counted before pruning) uses noise
row j * n_split_sources + r, the order of the reference's `repeat(n, 1)`.

One deliberate departure: `semantic_feature` is treated like every other
optimizer parameter.  The reference's remove_points leaves it out of its key
list, which drops it from the optimizer at the first densification.

`densify_torch` states the same pass in PyTorch operations for any device and
dtype: the parity oracle (pinned to the reference by
tests/golden/densify.npz), the benchmark's baseline and the CPU path of tests
that have no GPU.  The HIP path has no CPU fallback: host tensors raise.
"""
from __future__ import annotations

import ctypes
import functools
from typing import Optional

import torch

from . import _args, _lib
from ._lib import GsplatError

N_SPLIT = _lib.GS_DENSIFY_N_SPLIT
SKIP_KEYS = ("cam_m", "cam_c")  # per camera, not per Gaussian
STATS = ("means2D_gradient_accum", "denom", "max_2D_radius")
ROLE_OF = {"means3D": "means", "log_scales": "log_scales", "unnorm_rotations": "rotations",
           "logit_opacities": "logit_opacities"}
LAST_DENSIFY, FIRST_PASS, PASS_EVERY, BIG_FROM, RESET_EVERY = 5000, 500, 100, 3000, 3000


def schedule(i: int) -> dict:
    """What the reference does at iteration i (external.py:245-288): `active` (i <= 5000),
    `structure` (the clone / split / prune pass), its `remove_threshold` and whether the
    `big_points` prune applies, and `reset` (the opacity reset)."""
    active = i <= LAST_DENSIFY
    return {"active": active,
            "structure": active and i >= FIRST_PASS and i % PASS_EVERY == 0,
            "remove_threshold": 0.25 if i == LAST_DENSIFY else 0.005,
            "big_points": i >= BIG_FROM,
            "reset": active and i > 0 and i % RESET_EVERY == 0}


def _need(t, name: str, rows: Optional[int] = None) -> torch.Tensor:
    return _args.need(t, name, rows=rows, op="densification needs", twin="densify_torch runs")


def _device(t: torch.Tensor) -> torch.device:
    """The tensor's HIP device; the last check before a pointer reaches a kernel."""
    if t.device.type != "cuda":
        raise GsplatError(f"tensor on {t.device} cannot reach a HIP kernel")
    return t.device


def _keys(params: dict):
    return [k for k in params if k not in SKIP_KEYS]


def _group(optimizer, name: str):
    for g in optimizer.param_groups:
        if g.get("name") == name:
            return g
    return None


def _reset_value(like: torch.Tensor) -> torch.Tensor:
    """inverse_sigmoid(0.01) as the reference evaluates it in the tensor's dtype
    (external.py:208-209, 289)."""
    x = torch.full((1,), 0.01, dtype=like.dtype)
    return torch.log(x / (1 - x))


def _install(params, optimizer, key, value, exp_avg, exp_avg_sq):
    """Put `value` in place of params[key]: a new Parameter in the optimizer group named after
    the key, with the group's state moved to it ('step' kept, the moments replaced), as
    external.py:158-205 does; a plain tensor where there is no such group."""
    group = _group(optimizer, key) if optimizer is not None else None
    if group is None:
        params[key] = value
        return
    old = group["params"][0]
    state = optimizer.state.get(old, None)
    new = torch.nn.Parameter(value.requires_grad_(True))
    if state is not None:
        del optimizer.state[old]
        if exp_avg is not None:
            state["exp_avg"], state["exp_avg_sq"] = exp_avg, exp_avg_sq
        optimizer.state[new] = state
    group["params"][0] = new
    params[key] = new


def _moments(optimizer, key):
    """(group or None, exp_avg or None, exp_avg_sq or None) of params[key]."""
    group = _group(optimizer, key) if optimizer is not None else None
    if group is None:
        return None, None, None
    state = optimizer.state.get(group["params"][0], None)
    if not state or "exp_avg" not in state:
        return group, None, None
    return group, state["exp_avg"], state["exp_avg_sq"]


def _accumulate_hip(variables: dict):
    """accumulate_mean2d_gradient (external.py:136-140) on the statistics kernel of gs_optim.hip."""
    seen = variables["seen"]
    g = variables["means2D"].grad
    if g is None:
        raise GsplatError("variables['means2D'].grad is None (call after backward)")
    P = seen.numel()
    acc, den = _need(variables["means2D_gradient_accum"], "variables['means2D_gradient_accum']", P), \
        _need(variables["denom"], "variables['denom']", P)
    g = _need(g.contiguous(), "means2D.grad", P)
    if tuple(g.shape) != (P, 3):
        raise GsplatError(f"means2D.grad must be [P, 3] (got {tuple(g.shape)})")
    if P == 0:
        return
    _device(acc)
    radii = seen.to(torch.int32).contiguous()  # seen = radius > 0
    st = _lib.GsDensifyStats(P=P, radii=radii.data_ptr(), means2D_grad=g.data_ptr(), max_radius=None,
                             grad_accum=acc.data_ptr(), denom=den.data_ptr())
    args = _lib.GsAdamArgs(n_tensors=0, beta1=0.9, beta2=0.999, eps=1e-8)
    _lib.check(_lib.load().gs_adam_step(ctypes.byref(args), ctypes.byref(st), _lib.stream(seen.device)),
               "densify accumulate")


def plan(grad_accum, denom, log_scales, logit_opacities, *, grad_thresh, clone_max_scale, prune_min_opacity,
         prune_max_scale=0.0):
    """gs_densify_plan and the readback of its four totals.  Returns (workspace, counts):
    counts = [kept originals, kept clones, all split sources, kept split sources].  The flag
    bytes and ranks stay in the workspace (`plan_flags`, `plan_ranks`)."""
    L = _lib.load()
    P = grad_accum.numel()
    for name, t in (("grad_accum", grad_accum), ("denom", denom), ("log_scales", log_scales),
                    ("logit_opacities", logit_opacities)):
        _need(t, name)
    if denom.numel() != P or logit_opacities.numel() != P or log_scales.numel() != 3 * P:
        raise GsplatError("grad_accum, denom, logit_opacities [P] and log_scales [P, 3] disagree about P")
    dev = _device(grad_accum)
    ws = torch.empty(L.gs_densify_workspace_bytes(P), dtype=torch.uint8, device=dev)
    args = _lib.GsDensifyPlanArgs(P=P, grad_accum=grad_accum.data_ptr(), denom=denom.data_ptr(),
                                  log_scales=log_scales.data_ptr(), logit_opacities=logit_opacities.data_ptr(),
                                  grad_thresh=grad_thresh, clone_max_scale=clone_max_scale,
                                  prune_min_opacity=prune_min_opacity, prune_max_scale=prune_max_scale,
                                  n_split=N_SPLIT, workspace=ws.data_ptr(), workspace_bytes=ws.numel())
    _lib.check(L.gs_densify_plan(ctypes.byref(args), _lib.stream(dev)), "densify plan")
    if P == 0:
        return ws, [0, 0, 0, 0]
    off = L.gs_densify_counts_offset(P)
    counts = ws[off:off + 32].view(torch.int64).tolist()  # the pass's only host synchronisation
    return ws, counts


def plan_flags(ws: torch.Tensor, P: int) -> torch.Tensor:
    off = _lib.load().gs_densify_flags_offset(P)
    return ws[off:off + P]


def plan_ranks(ws: torch.Tensor, P: int) -> torch.Tensor:
    off = _lib.load().gs_densify_ranks_offset(P)
    return ws[off:off + 16 * P].view(torch.int32).view(P, 4)


def _hip_pass(params, variables, optimizer, sch, noise, generator, grad_thresh):
    L = _lib.load()
    keys = _keys(params)
    if len(keys) > _lib.GS_DENSIFY_MAX_TENSORS:
        raise GsplatError(f"at most {_lib.GS_DENSIFY_MAX_TENSORS} per-Gaussian tensors (got {len(keys)})")
    for k in ROLE_OF:
        if k not in params:
            raise GsplatError(f"params['{k}'] is required")
    P = params["means3D"].shape[0]
    for k in keys:
        _need(params[k], f"params['{k}']", P)
    acc = _need(variables["means2D_gradient_accum"], "variables['means2D_gradient_accum']", P)
    den = _need(variables["denom"], "variables['denom']", P)
    dev = _device(params["means3D"])
    radius = float(variables["scene_radius"])
    ws, counts = plan(acc, den,
                      params["log_scales"].detach(), params["logit_opacities"].detach(),
                      grad_thresh=grad_thresh, clone_max_scale=0.01 * radius,
                      prune_min_opacity=sch["remove_threshold"],
                      prune_max_scale=0.1 * radius if sch["big_points"] else 0.0)
    n_all = counts[2]
    P_new = counts[0] + counts[1] + N_SPLIT * counts[3]
    if noise is None:
        noise = torch.randn(N_SPLIT * n_all, 3, device=dev, dtype=torch.float32, generator=generator)
    _need(noise, "noise")
    if tuple(noise.shape) != (N_SPLIT * n_all, 3):
        raise GsplatError(f"noise must have shape {(N_SPLIT * n_all, 3)} (got {tuple(noise.shape)})")
    args = _lib.GsDensifyApplyArgs(P=P, workspace=ws.data_ptr(), workspace_bytes=ws.numel(), n_split=N_SPLIT,
                                   n_tensors=len(keys), noise=noise.data_ptr() if noise.numel() else None,
                                   reset_opacity=1 if sch["reset"] else 0,
                                   opacity_reset=float(_reset_value(params["logit_opacities"])))
    for j in range(4):
        args.counts[j] = counts[j]
    new_stats = [torch.empty(P_new, dtype=torch.float32, device=dev) for _ in STATS]
    for j, t in enumerate(new_stats):
        args.stats[j] = t.data_ptr() if P_new else None
    outs = []
    for n, k in enumerate(keys):
        src = params[k].detach()
        _, m, v = _moments(optimizer, k)
        if m is not None:
            _need(m, f"exp_avg of '{k}'", P)
            _need(v, f"exp_avg_sq of '{k}'", P)
            if m.numel() != src.numel() or v.numel() != src.numel():
                raise GsplatError(f"the moments of '{k}' do not have its shape")
        dst = torch.empty((P_new,) + tuple(src.shape[1:]), dtype=torch.float32, device=dev)
        dm, dv = (torch.empty_like(dst), torch.empty_like(dst)) if m is not None else (None, None)
        width = src.numel() // P if P else max(1, int(torch.Size(src.shape[1:]).numel()))
        p = functools.partial(_args.ptr, empty_is_null=True)
        tk = args.t[n]
        tk.src, tk.src_exp_avg, tk.src_exp_avg_sq = p(src), p(m), p(v)
        tk.dst, tk.dst_exp_avg, tk.dst_exp_avg_sq = p(dst), p(dm), p(dv)
        tk.width, tk.role = width, _lib.GS_DENSIFY_ROLES[ROLE_OF.get(k, "plain")]
        outs.append((k, src, m, v, dst, dm, dv))
    _lib.check(L.gs_densify_apply(ctypes.byref(args), _lib.stream(dev)), "densify apply")
    for k, _src, _m, _v, dst, dm, dv in outs:
        _install(params, optimizer, k, dst, dm, dv)
    for name, t in zip(STATS, new_stats):
        variables[name] = t
    del ws, noise
    return params, variables


def _reset_only(params, optimizer):
    """The opacity reset on an iteration without a structure pass (update_params_and_optimizer,
    external.py:143-155): plain fills."""
    lo = params["logit_opacities"]
    value = torch.full_like(lo.detach(), float(_reset_value(lo)))
    _, m, _v = _moments(optimizer, "logit_opacities")
    zeros = (torch.zeros_like(value), torch.zeros_like(value)) if m is not None else (None, None)
    _install(params, optimizer, "logit_opacities", value, *zeros)
    return params


def densify(params: dict, variables: dict, optimizer, i: int, *, accumulate: bool = True,
            noise: Optional[torch.Tensor] = None, generator: Optional[torch.Generator] = None,
            grad_thresh: float = 0.0002):
    """The reference's densify(params, variables, optimizer, i) (external.py:244-292) on HIP.

    Nothing for i > 5000.  With `accumulate`, accumulate_mean2d_gradient first (from
    variables['seen'] and variables['means2D'].grad).  The clone / split / prune pass runs when
    i >= 500 and i % 100 == 0, prunes below 0.005 opacity (0.25 at i == 5000) and, from
    i >= 3000, above 0.1 scene_radius; the opacity reset (i == 3000) is folded into the same
    launch.  Every entry of `params` except cam_m / cam_c is compacted: entries with an
    optimizer group named after them come back as new Parameters (no .grad, so the following
    optimizer.step() skips them, as in the reference) with the group's state moved and both
    moments rebuilt; the others as plain tensors.  variables['means2D_gradient_accum' | 'denom'
    | 'max_2D_radius'] come back zeroed at the new length.  `noise` [2 * split sources, 3]
    defaults to torch.randn on the device with `generator`.  Works with torch.optim.Adam and
    optim.FusedAdam.  Contiguous float32 device tensors only."""
    sch = schedule(i)
    if not sch["active"]:
        return params, variables
    if accumulate:
        _accumulate_hip(variables)
    if sch["structure"]:
        return _hip_pass(params, variables, optimizer, sch, noise, generator, grad_thresh)
    if sch["reset"]:
        _need(params["logit_opacities"], "params['logit_opacities']")
        params = _reset_only(params, optimizer)
    return params, variables


# ---- the same pass in PyTorch operations ----

def _rotation_matrices(q: torch.Tensor) -> torch.Tensor:
    """build_rotation's element formulas (external.py:61-78) for unnormalised (r, x, y, z)."""
    norm = torch.sqrt(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3])
    r, x, y, z = (q / norm[:, None]).unbind(1)
    rows = [1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
            2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
            2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)]
    return torch.stack(rows, dim=1).view(-1, 3, 3)


def classify_torch(grad_accum, denom, log_scales, logit_opacities, *, grad_thresh, clone_max_scale,
                   prune_min_opacity, prune_max_scale=0.0):
    """The flag byte of every Gaussian (include/gs_densify.h), in PyTorch operations."""
    g = grad_accum / denom
    g = torch.where(g.isnan(), torch.zeros_like(g), g)
    s = torch.exp(log_scales).max(dim=1).values
    hot = g >= grad_thresh
    clone = hot & (s <= clone_max_scale)
    split = hot & (s > clone_max_scale)
    faint = torch.sigmoid(logit_opacities.reshape(-1)) < prune_min_opacity
    prune, prune_split = faint, faint
    if prune_max_scale > 0:
        prune = faint | (s > prune_max_scale)
        s_copy = torch.exp(torch.log(torch.exp(log_scales) / (0.8 * N_SPLIT))).max(dim=1).values
        prune_split = faint | (s_copy > prune_max_scale)
    return (clone.to(torch.uint8) * _lib.GS_DENSIFY_CLONE + split.to(torch.uint8) * _lib.GS_DENSIFY_SPLIT
            + prune.to(torch.uint8) * _lib.GS_DENSIFY_PRUNE
            + prune_split.to(torch.uint8) * _lib.GS_DENSIFY_PRUNE_SPLIT)


def _torch_pass(params, variables, optimizer, sch, noise, generator, grad_thresh):
    keys = _keys(params)
    P = params["means3D"].shape[0]
    dev, dtype = params["means3D"].device, params["means3D"].dtype
    radius = float(variables["scene_radius"])
    flags = classify_torch(variables["means2D_gradient_accum"], variables["denom"],
                           params["log_scales"].detach(), params["logit_opacities"].detach(),
                           grad_thresh=grad_thresh, clone_max_scale=0.01 * radius,
                           prune_min_opacity=sch["remove_threshold"],
                           prune_max_scale=0.1 * radius if sch["big_points"] else 0.0)
    bit = lambda b: (flags & b) != 0  # noqa: E731
    clone, split, prune, prune_split = (bit(_lib.GS_DENSIFY_CLONE), bit(_lib.GS_DENSIFY_SPLIT),
                                        bit(_lib.GS_DENSIFY_PRUNE), bit(_lib.GS_DENSIFY_PRUNE_SPLIT))
    originals = torch.nonzero(~split & ~prune).reshape(-1)
    clones = torch.nonzero(clone & ~prune).reshape(-1)
    sources = torch.nonzero(split).reshape(-1)          # every split source, before pruning
    kept = torch.nonzero(~prune_split[sources]).reshape(-1)  # ranks among them of the kept ones
    n_all, n_kept = sources.numel(), kept.numel()
    if noise is None:
        noise = torch.randn(N_SPLIT * n_all, 3, device=dev, dtype=dtype, generator=generator)
    if tuple(noise.shape) != (N_SPLIT * n_all, 3):
        raise GsplatError(f"noise must have shape {(N_SPLIT * n_all, 3)} (got {tuple(noise.shape)})")
    split_rows = sources[kept]
    gather = torch.cat([originals, clones] + [split_rows] * N_SPLIT)
    P_new = gather.numel()
    first_copy = originals.numel() + clones.numel()
    noise_rows = torch.cat([j * n_all + kept for j in range(N_SPLIT)])

    ls = params["log_scales"].detach()[split_rows].repeat(N_SPLIT, 1)
    rot = _rotation_matrices(params["unnorm_rotations"].detach()[split_rows]).repeat(N_SPLIT, 1, 1)
    samples = torch.exp(ls) * noise[noise_rows]
    offsets = torch.bmm(rot, samples.unsqueeze(-1)).squeeze(-1)
    for k in keys:
        src = params[k].detach()
        if src.shape[0] != P:
            raise GsplatError(f"params['{k}'] must have {P} rows (got shape {tuple(src.shape)})")
        dst = src[gather].clone()
        if k == "means3D":
            dst[first_copy:] += offsets
        elif k == "log_scales":
            dst[first_copy:] = torch.log(torch.exp(ls) / (0.8 * N_SPLIT))
        elif k == "logit_opacities" and sch["reset"]:
            dst[:] = _reset_value(dst).to(dev)
        _, m, v = _moments(optimizer, k)
        dm = dv = None
        if m is not None:
            dm, dv = torch.zeros_like(dst), torch.zeros_like(dst)
            if not (k == "logit_opacities" and sch["reset"]):
                dm[:originals.numel()] = m[originals]
                dv[:originals.numel()] = v[originals]
        _install(params, optimizer, k, dst, dm, dv)
    for name in STATS:
        variables[name] = torch.zeros(P_new, device=dev, dtype=variables[name].dtype)
    return params, variables


def densify_torch(params: dict, variables: dict, optimizer, i: int, *, accumulate: bool = True,
                  noise: Optional[torch.Tensor] = None, generator: Optional[torch.Generator] = None,
                  grad_thresh: float = 0.0002):
    """densify in PyTorch operations, any device and dtype: the same arguments, schedule, row
    order, noise indexing and optimizer-state surgery."""
    sch = schedule(i)
    if not sch["active"]:
        return params, variables
    if accumulate:
        seen = variables["seen"]
        g = variables["means2D"].grad
        if g is None:
            raise GsplatError("variables['means2D'].grad is None (call after backward)")
        variables["means2D_gradient_accum"][seen] += torch.norm(g[seen, :2], dim=-1)
        variables["denom"][seen] += 1
    if sch["structure"]:
        return _torch_pass(params, variables, optimizer, sch, noise, generator, grad_thresh)
    if sch["reset"]:
        params = _reset_only(params, optimizer)
    return params, variables
