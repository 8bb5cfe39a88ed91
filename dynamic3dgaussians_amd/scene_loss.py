"""The scene regularisers of the reference's per-step loss (floor, bg,
soft_col_cons) and its foreground / background split on the HIP kernels of
csrc/gs_scene_loss.hip (C ABI include/gs_scene_loss.h): no boolean indexing, so
no host round trip, and deterministic gradients.

Drop-in for the rest of the reference's `if not is_initial_timestep:` block
(train.py:253-282; dyn_train.py:278-311; cvpr_dyn.py:304-330) around the
neighbour block neighbor.neighbor_losses already covers:

    fg_pts = rendervar['means3D'][is_fg];  fg_rot = rendervar['rotations'][is_fg]
    losses['floor'] = torch.clamp(fg_pts[:, 1], min=0).mean()
    bg_pts = rendervar['means3D'][~is_fg]; bg_rot = rendervar['rotations'][~is_fg]
    losses['bg'] = l1_loss_v2(bg_pts, variables["init_bg_pts"]) + l1_loss_v2(bg_rot, variables["init_bg_rot"])
    losses['soft_col_cons'] = l1_loss_v2(params['rgb_colors'], variables["prev_col"])

becomes

    split = foreground_split(is_fg, variables)                  # once per sequence, cached
    fg_pts, fg_rot = gather_foreground(rendervar['means3D'], rendervar['rotations'], split)
    losses['rigid'], losses['rot'], losses['iso'] = neighbor_losses(fg_pts, fg_rot, variables)
    losses['floor'], losses['bg'], losses['soft_col_cons'] = regularizer_losses(
        rendervar['means3D'], rendervar['rotations'], params['rgb_colors'], variables, split)

or, as one `extra_loss` for timesteps.TimestepDriver, reference_extra_loss().

Each of the four `x[is_fg]` / `x[~is_fg]` gathers of the reference runs a
nonzero whose element count the host waits for, and its backward is an
index_put_(accumulate=True).  The split here is an int32 table built once
(`slot`: rank r >= 0 among the foreground rows, -1 - r among the background
rows, in row order, so slot r addresses row r of init_bg_pts, init_bg_rot,
neighbor_indices and prev_offset as the reference made them); the kernels read
it per row.  `regularizer_losses_torch` states the three terms in PyTorch
operations in the reference's order, for any device and dtype: the parity
oracle, the benchmark's baseline and the CPU path of tests that have no GPU.
The HIP path has no CPU fallback: host tensors raise.
"""
from __future__ import annotations

import functools
from typing import Callable, Dict, Optional

import torch

from . import _args, _lib
from ._lib import GsplatError
from .neighbor import neighbor_losses

_SPLIT_KEY = "_scene_loss_fg_split"
_MASK_KEY = "_scene_loss_fg_mask"
WEIGHTS = {"rigid": 0.4, "rot": 0.4, "iso": 0.2, "floor": 0.2, "bg": 2.0, "soft_col_cons": 0.01}  # dyn_train.py:313


class ForegroundSplit:
    """`slot` int32 [P] (>= 0: rank among the foreground rows; < 0: -1 - rank among the background
    rows), the Python ints n_fg / n_bg, and the mask it was built from."""
    __slots__ = ("slot", "n_fg", "n_bg", "is_fg")

    def __init__(self, slot: torch.Tensor, n_fg: int, n_bg: int, is_fg: torch.Tensor):
        self.slot, self.n_fg, self.n_bg, self.is_fg = slot, n_fg, n_bg, is_fg

    @property
    def P(self) -> int:
        return self.n_fg + self.n_bg


def foreground_split(is_fg: torch.Tensor, variables: Optional[dict] = None) -> ForegroundSplit:
    """The split of a bool [P] mask (`seg_colors[:, 0] > 0.5`, `label == 1`; any device).  Built
    with torch (a cumsum) and one read-back of the foreground count: once per sequence, where the
    reference builds its neighbour graph, not on the per-step path.  With `variables` the result
    is cached there, keyed like neighbor's reverse CSR by the mask object itself and its version
    counter: a new mask object (even at a recycled address) or an in-place edit builds it again."""
    if not isinstance(is_fg, torch.Tensor) or is_fg.dtype != torch.bool or is_fg.dim() != 1:
        raise GsplatError("is_fg must be a bool [P] tensor")
    if variables is not None:
        cached = variables.get(_SPLIT_KEY)
        if cached is not None and cached[0] is is_fg and cached[1] == is_fg._version:
            return cached[2]
    P = is_fg.shape[0]
    if P >= 2 ** 31:
        raise GsplatError(f"is_fg has {P} rows; the split holds ranks as int32")
    version = is_fg._version
    fg_seen = torch.cumsum(is_fg.to(torch.int32), 0, dtype=torch.int32)  # foreground rows up to and including i
    row = torch.arange(P, dtype=torch.int32, device=is_fg.device)
    slot = torch.where(is_fg, fg_seen - 1, -1 - (row - fg_seen)).contiguous()
    n_fg = int(fg_seen[-1]) if P else 0  # the one read-back
    split = ForegroundSplit(slot, n_fg, P - n_fg, is_fg)
    if variables is not None:
        variables[_SPLIT_KEY] = (is_fg, version, split)
    return split


def _need(t, name: str, shape, dtype=torch.float32) -> torch.Tensor:
    return _args.need(t, name, shape, dtype=dtype, shape_first=True, op="scene losses need",
                      twin="regularizer_losses_torch runs")


def _need_split(split, P: int) -> ForegroundSplit:
    if not isinstance(split, ForegroundSplit):
        raise GsplatError("split must come from foreground_split")
    if split.P != P:
        raise GsplatError(f"the split is over {split.P} rows, the tables have {P}")
    _need(split.slot, "split.slot", (P,), torch.int32)
    return split


_ptr = functools.partial(_args.ptr, empty_is_null=True)


class _GatherForeground(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means3D, rotations, split: ForegroundSplit):
        L = _lib.load()
        dev = means3D.device
        means, rot = means3D.detach(), rotations.detach()
        fg_pts = torch.empty(split.n_fg, 3, dtype=torch.float32, device=dev)
        fg_rot = torch.empty(split.n_fg, 4, dtype=torch.float32, device=dev)
        _lib.check(L.gs_fg_gather_forward(split.P, split.n_fg, split.slot.data_ptr(), means.data_ptr(),
                                          rot.data_ptr(), _ptr(fg_pts), _ptr(fg_rot), _lib.stream(dev)),
                   "fg gather forward")
        ctx.split = split
        ctx.set_materialize_grads(False)  # an unused output arrives as None, not as a filled table
        return fg_pts, fg_rot

    @staticmethod
    def backward(ctx, g_pts, g_rot):
        split = ctx.split
        L = _lib.load()
        dev = split.slot.device
        g_pts = g_pts.to(torch.float32).contiguous() if g_pts is not None else None
        g_rot = g_rot.to(torch.float32).contiguous() if g_rot is not None else None
        d_means = torch.empty(split.P, 3, dtype=torch.float32, device=dev) if ctx.needs_input_grad[0] else None
        d_rot = torch.empty(split.P, 4, dtype=torch.float32, device=dev) if ctx.needs_input_grad[1] else None
        if d_means is not None or d_rot is not None:
            _lib.check(L.gs_fg_gather_backward(split.P, split.n_fg, split.slot.data_ptr(), _ptr(g_pts), _ptr(g_rot),
                                               _ptr(d_means), _ptr(d_rot), _lib.stream(dev)), "fg gather backward")
        return d_means, d_rot, None


def gather_foreground(means3D: torch.Tensor, rotations: torch.Tensor, split: ForegroundSplit):
    """(fg_pts [n_fg, 3], fg_rot [n_fg, 4]) = (means3D[is_fg], rotations[is_fg]), bit for bit, and
    so is the backward: one launch each way, every element of the full [P, 3] and [P, 4] gradients
    written exactly once (a foreground row its compact row, a background row zero), no atomics,
    no fill, no nonzero.  The output feeds neighbor_losses as it stands.  Contiguous float32
    device tensors only."""
    P = means3D.shape[0] if isinstance(means3D, torch.Tensor) and means3D.dim() == 2 else -1
    _need(means3D, "means3D", (P, 3))
    _need(rotations, "rotations", (P, 4))
    _need_split(split, P)
    return _GatherForeground.apply(means3D, rotations, split)


def _struct(split, means, rot, col, bg_pts, bg_rot, prev_col, raw, losses, ws):
    return _lib.GsSceneLoss(P=split.P, n_fg=split.n_fg, n_bg=split.n_bg, slot=split.slot.data_ptr(),
                            means=means.data_ptr(), rotations=rot.data_ptr(), colors=col.data_ptr(),
                            init_bg_pts=_ptr(bg_pts), init_bg_rot=_ptr(bg_rot), prev_col=prev_col.data_ptr(),
                            raw_rotations=int(raw), _pad=0, losses=_ptr(losses), workspace=_ptr(ws),
                            workspace_bytes=ws.numel() if ws is not None else 0)


class _RegularizerLosses(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means3D, rotations, rgb_colors, bg_pts, bg_rot, prev_col, split, raw):
        L = _lib.load()
        dev = means3D.device
        means, rot, col = means3D.detach(), rotations.detach(), rgb_colors.detach()
        losses = torch.empty(3, dtype=torch.float32, device=dev)
        ws = torch.empty(L.gs_scene_loss_workspace_bytes(split.P), dtype=torch.uint8, device=dev)
        args = _struct(split, means, rot, col, bg_pts, bg_rot, prev_col, raw, losses, ws)
        _lib.check(L.gs_scene_loss_forward(args, _lib.stream(dev)), "scene loss forward")
        ctx.save_for_backward(means, rot, col, bg_pts, bg_rot, prev_col)  # the backward needs no workspace
        ctx.split, ctx.raw = split, raw
        ctx.set_materialize_grads(False)
        return losses[0], losses[1], losses[2]

    @staticmethod
    def backward(ctx, g_floor, g_bg, g_col):
        means, rot, col, bg_pts, bg_rot, prev_col = ctx.saved_tensors
        split = ctx.split
        L = _lib.load()
        dev = means.device
        z = torch.zeros((), dtype=torch.float32, device=dev)
        up = torch.stack([g if g is not None else z for g in (g_floor, g_bg, g_col)]).float().contiguous()  # on the device
        d_means, d_rot, d_col = torch.empty_like(means), torch.empty_like(rot), torch.empty_like(col)
        args = _struct(split, means, rot, col, bg_pts, bg_rot, prev_col, ctx.raw, None, None)
        _lib.check(L.gs_scene_loss_backward(args, up.data_ptr(), d_means.data_ptr(), d_rot.data_ptr(),
                                            d_col.data_ptr(), _lib.stream(dev)), "scene loss backward")
        return d_means, d_rot, d_col, None, None, None, None, None


def regularizer_losses(means3D: torch.Tensor, rotations: torch.Tensor, rgb_colors: torch.Tensor, variables: dict,
                       split: ForegroundSplit, *, raw_rotations: bool = False):
    """(floor, bg, soft_col_cons) of train.py:275-282 as three device scalars, differentiable in the
    full tables means3D [P, 3], rotations [P, 4] and rgb_colors [P, 3]:

        floor         = mean over fg of max(y, 0)
        bg            = mean over bg of sum |p - init_bg_pts[r]| + mean over bg of sum |q - init_bg_rot[r]|
        soft_col_cons = mean over all P of sum |c - prev_col|

    with torch's mean (an empty set gives NaN).  `variables` is the reference's dict
    (init_bg_pts [n_bg, 3], init_bg_rot [n_bg, 4], prev_col [P, 3]); `split` comes from
    foreground_split.  raw_rotations=True: `rotations` is unnorm_rotations and the kernels apply
    F.normalize (eps 1e-12) themselves, forward and backward -- the companion of
    GaussianRasterizerBatch(raw_params=True), which leaves no torch normalize in the step to
    share.  Two forward launches, one backward launch, nothing read back, no atomics: the
    gradients follow torch's autograd at the kinks (abs: sign, 0 at 0; clamp: passes at y == 0) and
    two runs give the same bits.  Contiguous float32 device tensors only."""
    P = means3D.shape[0] if isinstance(means3D, torch.Tensor) and means3D.dim() == 2 else -1
    _need(means3D, "means3D", (P, 3))
    _need(rotations, "rotations", (P, 4))
    _need(rgb_colors, "rgb_colors", (P, 3))
    _need_split(split, P)
    bg_pts = _need(variables["init_bg_pts"], "init_bg_pts", (split.n_bg, 3))
    bg_rot = _need(variables["init_bg_rot"], "init_bg_rot", (split.n_bg, 4))
    prev_col = _need(variables["prev_col"], "prev_col", (P, 3))
    for t, name in ((bg_pts, "init_bg_pts"), (bg_rot, "init_bg_rot"), (prev_col, "prev_col")):
        if t.requires_grad:
            raise GsplatError(f"{name} gets no gradient from the scene losses ({name}.requires_grad is set)")
    return _RegularizerLosses.apply(means3D, rotations, rgb_colors, bg_pts, bg_rot, prev_col, split,
                                    bool(raw_rotations))


def _l1_loss_v2(x, y):  # helpers.py:114-115
    return torch.abs(x - y).sum(-1).mean()


def regularizer_losses_torch(means3D: torch.Tensor, rotations: torch.Tensor, rgb_colors: torch.Tensor,
                             variables: dict, split, *, raw_rotations: bool = False):
    """regularizer_losses in PyTorch operations, any device and dtype, in the reference's order:
    boolean indexing by the mask, clamp, l1_loss_v2; autograd for the backward.  `split` is a
    ForegroundSplit or the bool mask itself."""
    is_fg = split.is_fg if isinstance(split, ForegroundSplit) else split
    if raw_rotations:
        rotations = torch.nn.functional.normalize(rotations)
    fg_pts = means3D[is_fg]
    floor = torch.clamp(fg_pts[:, 1], min=0).mean()
    bg_pts, bg_rot = means3D[~is_fg], rotations[~is_fg]
    bg = _l1_loss_v2(bg_pts, variables["init_bg_pts"]) + _l1_loss_v2(bg_rot, variables["init_bg_rot"])
    soft_col_cons = _l1_loss_v2(rgb_colors, variables["prev_col"])
    return floor, bg, soft_col_cons


def _cached_mask(params: dict, variables: dict) -> torch.Tensor:
    """timesteps._fg_mask as ONE mask object per seg_colors tensor (object and version), so the
    split cached beside it is found again every step."""
    seg = params.get("seg_colors")
    P, dev = params["means3D"].shape[0], params["means3D"].device
    key = (seg, seg._version) if seg is not None else (None, (P, dev))
    cached = variables.get(_MASK_KEY)
    if cached is not None and cached[0] is key[0] and cached[1] == key[1]:
        return cached[2]
    from .timesteps import _fg_mask
    mask = _fg_mask(params)
    variables[_MASK_KEY] = (key[0], key[1], mask)
    return mask


def reference_extra_loss(weights: Optional[Dict[str, float]] = None) -> Callable:
    """The reference's `if not is_initial_timestep:` block (train.py:253-282) as an
    `extra_loss(params, variables, rendervar, t)` for timesteps.TimestepDriver:

        sum_k weights[k] * losses[k]   over rigid, rot, iso, floor, bg, soft_col_cons

    from the cached foreground split (seg_colors[:, 0] > 0.5; every row without seg colours),
    gather_foreground, neighbor_losses and regularizer_losses on rendervar's means3D and
    rotations and params' rgb_colors.  None at t == 0 or before the neighbour graph exists
    (initialize_post_first_timestep).  Default weights: dyn_train.py:313 (0.4 / 0.4 / 0.2 / 0.2 /
    2.0 / 0.01); a weights dict replaces them key by key.  After the first call has built and
    cached the split, a call and its backward make no host round trip and the gradients are
    deterministic.  The callable reads and writes no `semantic_feature`: it is safe beside the
    sharded step's overlapped feature exchange, which owns that table while the loss runs."""
    w = dict(WEIGHTS)
    if weights:
        unknown = set(weights) - set(WEIGHTS)
        if unknown:
            raise ValueError(f"unknown loss names {sorted(unknown)}; the block has {sorted(WEIGHTS)}")
        w.update({k: float(v) for k, v in weights.items()})

    def extra_loss(params, variables, rendervar, t):
        if t == 0 or "neighbor_indices" not in variables:
            return None
        split = foreground_split(_cached_mask(params, variables), variables)
        means, rot = rendervar["means3D"], rendervar["rotations"]
        fg_pts, fg_rot = gather_foreground(means, rot, split)
        rigid, rot_l, iso = neighbor_losses(fg_pts, fg_rot, variables)
        floor, bg, col = regularizer_losses(means, rot, params["rgb_colors"], variables, split)
        return (w["rigid"] * rigid + w["rot"] * rot_l + w["iso"] * iso + w["floor"] * floor + w["bg"] * bg
                + w["soft_col_cons"] * col)

    return extra_loss
