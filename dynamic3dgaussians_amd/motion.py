"""The reference's motion-basis scene on the HIP kernels of csrc/gs_motion.hip
(C ABI include/gs_motion.h): every Gaussian's canonical mean moved by its own
blend of K shared SE(3) trajectories, one launch forward and three backward.

Drop-in for the block of the reference's temporal-window step
(dyn_train.py:410-431; MotionBases external.py:27-58 / motion_utils.py:24-55;
cont_6d_to_rmat motion_utils.py:10-22):

    coefs     = softmax(motion_coefs, -1)
    transfms  = bases.compute_transforms(ts, coefs)                        # (G, B, 3, 4)
    positions = einsum("pnij,pj->pni", transfms, pad(means, (0, 1), value=1.0))

becomes

    from dynamic3dgaussians_amd import MotionBases
    positions = bases.compute_means(ts, means, motion_coefs, softmax=True)   # (G, B, 3)

and `positions[:, b]` feeds the rasterizer's means3D.  `motion_positions` /
`motion_transforms` are the autograd functions underneath;
`motion_positions_torch` states the same block in PyTorch operations for any
device and dtype: the parity oracle, the benchmark's baseline, and the path
that CPU or non-fp32 inputs take.

Frame indices `ts` are a list, a range or an integer tensor.  They travel to
the kernels by value, so a device tensor is read back once (a
synchronisation): pass host indices in a training loop.  Negative indices
count from the end as in Python, indices outside [-T, T) raise IndexError, and
more than 32 frames are split into calls of at most 32, so callers see no
limit on B.  More than 64 bases raise ValueError.

The backward is deterministic (no atomics).  At a degenerate
blend -- a zero 3-vector, or parallel halves of the 6-vector -- the forward is
what the clamp of F.normalize makes it; the HIP backward there is unspecified.
"""
from __future__ import annotations

from typing import Sequence

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib

MAX_BASES = _lib.GS_MOTION_MAX_K
MAX_FRAMES_PER_CALL = _lib.GS_MOTION_MAX_B


def cont_6d_to_rmat(cont_6d: torch.Tensor) -> torch.Tensor:
    """(*, 6) -> (*, 3, 3): Gram-Schmidt of the two halves, the third axis their cross product;
    the three axes are the matrix's COLUMNS (motion_utils.py:10-22)."""
    x1 = cont_6d[..., 0:3]
    y1 = cont_6d[..., 3:6]
    x = F.normalize(x1, dim=-1)
    y = F.normalize(y1 - (y1 * x).sum(dim=-1, keepdim=True) * x, dim=-1)
    z = torch.linalg.cross(x, y, dim=-1)
    return torch.stack([x, y, z], dim=-1)


def normalise_ts(ts, num_frames: int) -> list:
    """ts (list, range or integer tensor) as a list of ints in [0, num_frames).  A device tensor
    is read back here, once."""
    if isinstance(ts, torch.Tensor):
        if ts.is_floating_point() or ts.is_complex() or ts.dtype == torch.bool:
            raise TypeError(f"ts must hold integers (got {ts.dtype})")
        ts = ts.reshape(-1).tolist()
    out = []
    for t in ts:
        t = int(t)
        if not -num_frames <= t < num_frames:
            raise IndexError(f"frame index {t} is out of range for {num_frames} frames")
        out.append(t + num_frames if t < 0 else t)
    return out


def motion_positions_torch(means, coefs, rots, transls, ts, softmax: bool = False,
                           return_transforms: bool = False):
    """The reference's block op for op, any dtype and device: positions (G, B, 3), and the
    transforms (G, B, 3, 4) with them when return_transforms is set.  means may be None when only
    the transforms are wanted (positions is then None)."""
    ts = normalise_ts(ts, rots.shape[1])
    if softmax:
        coefs = F.softmax(coefs, dim=-1)
    tr = transls[:, ts]  # (K, B, 3)
    ro = rots[:, ts]  # (K, B, 6)
    tr = torch.einsum("pk,kni->pni", coefs, tr)
    ro = torch.einsum("pk,kni->pni", coefs, ro)  # (G, B, 6)
    rotmats = cont_6d_to_rmat(ro)  # (G, B, 3, 3)
    transfms = torch.cat([rotmats, tr[..., None]], dim=-1)
    positions = None
    if means is not None:
        positions = torch.einsum("pnij,pj->pni", transfms, F.pad(means, (0, 1), value=1.0))
    return (positions, transfms) if return_transforms else positions


def _desc(means, coefs, rots, transls, ts, softmax):
    G, K = coefs.shape
    d = _lib.GsMotionDesc(G=G, K=K, T=rots.shape[1], B=len(ts), coef_mode=1 if softmax else 0,
                          rots=rots.data_ptr(), transls=transls.data_ptr(),
                          coefs=coefs.data_ptr() if G else None,
                          means=means.data_ptr() if means is not None and G else None)
    for b, t in enumerate(ts):
        d.ts[b] = t
    return d


class _MotionWarp(torch.autograd.Function):
    """One call of at most 32 frames: positions (G, B, 3) when means is given, the transforms
    (G, B, 3, 4) otherwise."""

    @staticmethod
    def forward(ctx, means, coefs, rots, transls, ts, softmax):
        L = _lib.load()
        dev = coefs.device
        means = means.detach().contiguous() if means is not None else None
        coefs, rots, transls = coefs.detach().contiguous(), rots.detach().contiguous(), transls.detach().contiguous()
        G, B = coefs.shape[0], len(ts)
        out = torch.empty((G, B, 3) if means is not None else (G, B, 3, 4), dtype=torch.float32, device=dev)
        if G:  # an empty output has no address to hand over, and there is nothing to launch
            desc = _desc(means, coefs, rots, transls, ts, softmax)
            _lib.check(L.gs_motion_forward(desc, out.data_ptr() if means is not None else None,
                                           out.data_ptr() if means is None else None, None, _lib.stream(dev)),
                       "motion forward")
        ctx.save_for_backward(means, coefs, rots, transls)
        ctx.ts, ctx.softmax = ts, softmax
        return out

    @staticmethod
    def backward(ctx, g_out):
        means, coefs, rots, transls = ctx.saved_tensors
        L = _lib.load()
        dev = coefs.device
        G, K = coefs.shape
        g_out = g_out.to(torch.float32).contiguous()
        want_means = means is not None and ctx.needs_input_grad[0]
        d_means = torch.empty_like(means) if want_means else None
        d_coefs = torch.empty_like(coefs)
        d_rots, d_transls = torch.empty_like(rots), torch.empty_like(transls)
        ws = torch.empty(L.gs_motion_workspace_bytes(G, K, len(ctx.ts), 1), dtype=torch.uint8, device=dev)
        desc = _desc(means, coefs, rots, transls, ctx.ts, ctx.softmax)
        _lib.check(L.gs_motion_backward(desc, g_out.data_ptr() if means is not None else None,
                                        g_out.data_ptr() if means is None else None,
                                        d_means.data_ptr() if want_means else None, d_coefs.data_ptr(),
                                        d_rots.data_ptr(), d_transls.data_ptr(), ws.data_ptr(), _lib.stream(dev)),
                   "motion backward")
        return d_means, d_coefs, d_rots, d_transls, None, None


def _on_hip_path(*tensors) -> bool:
    return all(t.is_cuda and t.dtype == torch.float32 for t in tensors)


def _check_shapes(means, coefs, rots, transls):
    if coefs.dim() != 2:
        raise ValueError(f"coefs must be (G, K) (got {tuple(coefs.shape)})")
    G, K = coefs.shape
    if rots.dim() != 3 or rots.shape[0] != K or rots.shape[2] != 6:
        raise ValueError(f"rots must be ({K}, T, 6) (got {tuple(rots.shape)})")
    if tuple(transls.shape) != (K, rots.shape[1], 3):
        raise ValueError(f"transls must be ({K}, {rots.shape[1]}, 3) (got {tuple(transls.shape)})")
    if means is not None and tuple(means.shape) != (G, 3):
        raise ValueError(f"means must be ({G}, 3) (got {tuple(means.shape)})")
    if K < 1:
        raise ValueError("at least one basis is required")


def _warp(means, coefs, rots, transls, ts, softmax):
    _check_shapes(means, coefs, rots, transls)
    tensors = (coefs, rots, transls) + ((means,) if means is not None else ())
    if not _on_hip_path(*tensors):
        out = motion_positions_torch(means, coefs, rots, transls, ts, softmax=softmax, return_transforms=True)
        return out[0] if means is not None else out[1]
    if coefs.shape[1] > MAX_BASES:
        raise ValueError(f"the HIP motion warp takes at most {MAX_BASES} bases (got {coefs.shape[1]})")
    ts = normalise_ts(ts, rots.shape[1])
    chunks = [tuple(ts[i:i + MAX_FRAMES_PER_CALL]) for i in range(0, len(ts), MAX_FRAMES_PER_CALL)]
    if not chunks:
        return coefs.new_empty((coefs.shape[0], 0, 3) if means is not None else (coefs.shape[0], 0, 3, 4))
    outs = [_MotionWarp.apply(means, coefs, rots, transls, c, bool(softmax)) for c in chunks]
    return outs[0] if len(outs) == 1 else torch.cat(outs, dim=1)


def motion_positions(means: torch.Tensor, coefs: torch.Tensor, rots: torch.Tensor, transls: torch.Tensor, ts,
                     softmax: bool = False) -> torch.Tensor:
    """positions (G, B, 3) of means (G, 3) at the frames ts under coefs (G, K) (logits with
    softmax=True) and the bases rots (K, T, 6), transls (K, T, 3).  Differentiable in all four.
    fp32 device tensors run the HIP kernels; anything else takes motion_positions_torch."""
    if means is None:
        raise ValueError("motion_positions needs means; motion_transforms does not")
    return _warp(means, coefs, rots, transls, ts, softmax)


def motion_transforms(coefs: torch.Tensor, rots: torch.Tensor, transls: torch.Tensor, ts,
                      softmax: bool = False) -> torch.Tensor:
    """The transforms (G, B, 3, 4) = [R | t] alone (MotionBases.compute_transforms), differentiable
    in coefs and both bases."""
    return _warp(None, coefs, rots, transls, ts, softmax)


class MotionBases(nn.Module):
    """The reference's MotionBases (external.py:27-58): K trajectories of T frames as a 6-vector
    rotation and a translation each, under the same parameter names (`params.rots`,
    `params.transls`).  The parameters stay on the device of the tensors given; move the module
    with .to() as any other.  compute_transforms honours its ts (motion_utils.py:47 overwrites
    them with range(9), a leftover of an experiment); compute_means is the whole block fused."""

    def __init__(self, rots: torch.Tensor, transls: torch.Tensor):
        super().__init__()
        if rots.dim() != 3 or rots.shape[-1] != 6 or tuple(transls.shape) != (*rots.shape[:2], 3):
            raise ValueError(f"rots must be (K, T, 6) and transls (K, T, 3) "
                             f"(got {tuple(rots.shape)}, {tuple(transls.shape)})")
        self.num_frames = rots.shape[1]
        self.num_bases = rots.shape[0]
        self.params = nn.ParameterDict({
            "rots": nn.Parameter(rots.detach().float().contiguous().clone()),
            "transls": nn.Parameter(transls.detach().float().contiguous().clone()),
        })

    @staticmethod
    def init_from_state_dict(state_dict, prefix: str = "params."):
        keys = ["rots", "transls"]
        missing = [f"{prefix}{k}" for k in keys if f"{prefix}{k}" not in state_dict]
        if missing:
            raise KeyError(f"state_dict lacks {missing}")
        return MotionBases(**{k: state_dict[f"{prefix}{k}"] for k in keys})

    def compute_transforms(self, ts, coefs: torch.Tensor, softmax: bool = False) -> torch.Tensor:
        """(G, B, 3, 4) for the frames ts and the coefficients (G, K)."""
        return motion_transforms(coefs, self.params["rots"], self.params["transls"], ts, softmax=softmax)

    def compute_means(self, ts, means: torch.Tensor, coefs: torch.Tensor, softmax: bool = False) -> torch.Tensor:
        """(G, B, 3): the means at the frames ts; softmax=True takes coefs as logits."""
        return motion_positions(means, coefs, self.params["rots"], self.params["transls"], ts, softmax=softmax)


__all__: Sequence[str] = ("MotionBases", "cont_6d_to_rmat", "motion_positions", "motion_positions_torch",
                          "motion_transforms", "normalise_ts")
