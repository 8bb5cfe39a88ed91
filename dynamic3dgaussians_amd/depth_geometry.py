"""Geometry on depth maps on the HIP kernels of csrc/gs_depth_geometry.hip (C ABI
include/gs_depth_geometry.h): the point z-buffer and the abs-rel score behind the
reference's mMDE, dense and sparse unprojection, the optical flow a depth map
induces between two cameras, and one bilinear border sampler with the flow warping
and chaining built on it.  Forward only; every camera of a batch in one launch.

What the reference computes in PyTorch and where:

    unproject_image(...)  z-buffer part     metrics.py:131-195  -> point_depth_maps(points, w2c, K, (H, W))
    unproject_image(...)  score part        metrics.py:197-205  -> depth_abs_rel(est, gt, exclude)
    mMDE().update(...) / .compute()         metrics.py:254-292  -> metrics.MeanDepthError
    pixel_to_camera_coordinates(depth, K)   ideaII.py:102-110 \\
    camera_to_world_coordinates(pts, c2w)   ideaII.py:112-121  > -> unproject_depth(depth, K, w2c)
    depth2point_world(depth, K, w2c)        dyn_utils.py:442-480 /
    compute_optical_flow(d1, K1, E1, d2, K2, E2)  ideaII.py:135-157  -> depth_flow(d1, K1, c2w1, K2, w2c2)
    warp_flow(flow, displacement)           ideaII.py:159-198   -> warp_flow
    accumulate_flows(flows)                 ideaII.py:200-206   -> accumulate_flows
    resize_optical_flow(flow, size)         ideaII.py:219-257   -> resize_flow
    2-D tracks lifted through depth maps    dyn_som.py:268-286  -> lift_tracks

One formula, xyz = c2w (depth * K^-1 (x, y, 1), 1) with x the column and y the row of the
pixel, covers the three dense unprojections.  ideaII's pair is that formula for a pinhole K
without skew.  dyn_utils.depth2point_world builds x / (W - 1) * (W - 1) -- the pixel index
again, up to its fp32 round trip -- multiplies by the depth and by K^-1, and applies
inverse(extrinsic): the same formula with a general K.  K and w2c are inverted here in fp64
on the tensors' device and cast to fp32 for the kernel.

A naming quirk of ideaII.compute_optical_flow: both of its matrices are called `extrinsics`,
but the first (camera_to_world_coordinates) is used as camera-to-world and the second
(world_to_camera_2d) as world-to-camera.  The arguments here are named for what they are:
depth_flow(depth1, K1, c2w1, K2, w2c2).  Its depth2 argument is never read and has no
counterpart.

Every function has a `_torch` twin in PyTorch operations for any device and dtype: the fp64
parity oracle, the CPU path and the benchmark's baseline.  The HIP functions have no CPU
fallback: host tensors, other dtypes than float32, wrong shapes and non-contiguous tensors
raise GsplatError.  Nothing is read back; the z-buffer, the score and evaluate_cameras'
"mde" are tested to make no host synchronisation (the matrix inverses of unproject_depth,
depth_flow and lift_tracks are torch.linalg.inv_ex, which reads no error code back).

Parity unpinned: lift_tracks.  dyn_som.py is a fragment that defines neither normalize_coords
nor its imports, so it cannot be run; the coordinates are taken as pixel units under
align_corners=True, which its call states, and the oracle is torch's grid_sample.
"""
from __future__ import annotations

import functools
from typing import Optional, Sequence, Tuple

import torch

from . import _args, _lib
from ._lib import GsplatError

FLOW_MIN_Z = 1e-7  # ideaII.py:132: points_2d[:, 2:].clamp(min=1e-7)


# ---- argument checks

_need = functools.partial(_args.need, op="depth geometry needs", twin="the _torch twins run")


def _mats(m, name: str, n: int) -> Tuple[torch.Tensor, bool]:
    """[n, n] or [B, n, n] -> ([B, n, n], single)."""
    if not isinstance(m, torch.Tensor) or m.dim() not in (2, 3) or tuple(m.shape[-2:]) != (n, n):
        raise GsplatError(f"{name} must be a [B, {n}, {n}] or [{n}, {n}] tensor")
    if not m.is_floating_point():
        raise GsplatError(f"{name} must be a floating-point tensor (got {m.dtype})")
    if m.dim() == 3 and m.shape[0] < 1:
        raise GsplatError(f"{name} must not be empty")
    return (m[None], True) if m.dim() == 2 else (m, False)


def _same_batch(B: int, m: torch.Tensor, name: str) -> None:
    if m.shape[0] != B:
        raise GsplatError(f"{name} must have {B} matrices (got {m.shape[0]})")


def _maps(d, name: str) -> Tuple[torch.Tensor, bool]:
    """[H, W] or [B, H, W] -> ([B, H, W], single)."""
    if not isinstance(d, torch.Tensor) or d.dim() not in (2, 3):
        raise GsplatError(f"{name} must be a [B, H, W] or [H, W] tensor")
    if d.numel() == 0:
        raise GsplatError(f"{name} must not be empty (got {tuple(d.shape)})")
    return (d[None], True) if d.dim() == 2 else (d, False)


def _hw(hw) -> Tuple[int, int]:
    try:
        H, W = (int(s) for s in hw)
    except (TypeError, ValueError):
        raise GsplatError(f"hw must be (H, W) (got {hw!r})") from None
    if H < 1 or W < 1:
        raise GsplatError(f"hw must be positive (got {(H, W)})")
    return H, W


def _f32(m: torch.Tensor) -> torch.Tensor:
    return m.detach().to(torch.float32).contiguous()


def _inv(m: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """The inverse taken in fp64 on m's device (no error check, so no readback), cast to dtype."""
    return torch.linalg.inv_ex(m.detach().double()).inverse.to(dtype)


def _pixel_grid(H: int, W: int, like: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """x (column) and y (row) of every pixel, [H, W] each, in like's dtype."""
    y, x = torch.meshgrid(torch.arange(H, device=like.device, dtype=like.dtype),
                          torch.arange(W, device=like.device, dtype=like.dtype), indexing="ij")
    return x, y


# ---- the point z-buffer

def _check_cloud(points, w2c, K, need: bool):
    w2c, single = _mats(w2c, "w2c", 4)
    K, _ = _mats(K, "K", 3)
    B = w2c.shape[0]
    _same_batch(B, K, "K")
    if not isinstance(points, torch.Tensor) or points.dim() not in (2, 3) or points.shape[-1] != 3:
        raise GsplatError("points must be a [P, 3] or [B, P, 3] tensor")
    if points.dim() == 3 and points.shape[0] != B:
        raise GsplatError(f"points must hold one cloud per camera ({B}) or one for all (got {tuple(points.shape)})")
    if need:
        _need(points, "points")
        for t, n in ((w2c, "w2c"), (K, "K")):
            if not t.is_cuda:
                raise GsplatError(f"the HIP depth geometry needs device tensors ({n} is on the CPU)")
    return w2c, K, single


def point_depth_maps(points: torch.Tensor, w2c: torch.Tensor, K: torch.Tensor, hw) -> torch.Tensor:
    """The depth of the nearest point per pixel, [B, H, W] (or [H, W] for one [4, 4] camera),
    +inf where no point lands: unproject_image's z-buffer (metrics.py:137-195) for every camera
    at once.  points [P, 3] is one cloud for all cameras, [B, P, 3] one per camera (one timestep
    each); w2c [B, 4, 4], K [B, 3, 3].  A point counts where its camera depth is > 0 and its
    pixel, round-half-to-even of the projection, is inside the image.  Integer min atomics on
    the depth's bits: two calls give the same bits.  Contiguous float32 device points."""
    w2c, K, single = _check_cloud(points, w2c, K, need=True)
    H, W = _hw(hw)
    B, P = w2c.shape[0], points.shape[-2]
    L = _lib.load()
    dev = points.device
    pts, w2c, K = points.detach(), _f32(w2c), _f32(K)
    depth = torch.empty(B, H, W, dtype=torch.float32, device=dev)
    args = _lib.GsPointDepth(P=P, B=B, H=H, W=W, points=pts.data_ptr() if P else None,
                             points_batch_stride=P * 3 if points.dim() == 3 else 0, w2c=w2c.data_ptr(),
                             K=K.data_ptr(), depth=depth.data_ptr())
    _lib.check(L.gs_point_depth(args, _lib.stream(dev)), "point depth")
    return depth[0] if single else depth


def point_depth_maps_torch(points: torch.Tensor, w2c: torch.Tensor, K: torch.Tensor, hw) -> torch.Tensor:
    """point_depth_maps in PyTorch operations, any device and dtype (the points' dtype): the
    reference's arithmetic (metrics.py:140-168) with its per-pixel Python loop restated as one
    scatter_reduce(amin).  The bounds are tested on the rounded floats, so NaN and inf never
    become an index.  No boolean indexing: nothing is read back."""
    w2c, K, single = _check_cloud(points, w2c, K, need=False)
    H, W = _hw(hw)
    B, P = w2c.shape[0], points.shape[-2]
    dt = points.dtype
    pts = points if points.dim() == 3 else points[None].expand(B, P, 3)
    hom = torch.cat([pts, torch.ones(B, P, 1, dtype=dt, device=pts.device)], dim=-1)
    cam = torch.matmul(hom, w2c.to(dt).transpose(1, 2))[..., :3]  # pc_hom @ w2c.T
    z = cam[..., 2]
    q = torch.matmul(K.to(dt), cam.transpose(1, 2))  # K @ coords, [B, 3, P]
    u, v = torch.round(q[:, 0] / q[:, 2]), torch.round(q[:, 1] / q[:, 2])
    ok = (z > 0) & (u >= 0) & (u < W) & (v >= 0) & (v < H)
    idx = torch.where(ok, v * W + u, torch.zeros_like(u)).long()
    inf = torch.full((), float("inf"), dtype=dt, device=pts.device)
    depth = torch.full((B, H * W), float("inf"), dtype=dt, device=pts.device)
    depth = depth.scatter_reduce(1, idx, torch.where(ok, z, inf), "amin", include_self=True).reshape(B, H, W)
    return depth[0] if single else depth


# ---- the abs-rel score

def _check_depth_pair(est, gt, exclude, need: bool):
    est3, single = _maps(est, "est")
    if need:
        _need(est, "est")
        _need(gt, "gt", est.shape)
    elif not isinstance(gt, torch.Tensor) or gt.shape != est.shape:
        raise GsplatError(f"gt must have shape {tuple(est.shape)}")
    B, H, W = est3.shape
    if exclude is not None:
        if not isinstance(exclude, torch.Tensor) or (need and not exclude.is_cuda):
            raise GsplatError("exclude must be a device tensor")
        if tuple(exclude.shape) not in ((H, W), (B, H, W)):
            raise GsplatError(f"exclude must have shape {(H, W)} or {(B, H, W)} (got {tuple(exclude.shape)})")
    return est3, gt.reshape(est3.shape), single


def depth_abs_rel_sums(est: torch.Tensor, gt: torch.Tensor, exclude: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[B, 2] fp64 on the device: per image the sum of |gt - est| / gt over the valid pixels and
    their count (depth_abs_rel divides)."""
    est3, gt3, _ = _check_depth_pair(est, gt, exclude, need=True)
    B, H, W = est3.shape
    L = _lib.load()
    dev = est.device
    est3, gt3 = est3.detach(), gt3.detach()
    if exclude is not None:
        exclude = exclude.detach().to(torch.float32).contiguous()
    out = torch.empty(B, 2, dtype=torch.float64, device=dev)
    ws = torch.empty(L.gs_depth_abs_rel_workspace_bytes(B, H, W), dtype=torch.uint8, device=dev)
    args = _lib.GsDepthAbsRel(B=B, H=H, W=W, est=est3.data_ptr(), gt=gt3.data_ptr(),
                              exclude=exclude.data_ptr() if exclude is not None else None,
                              exclude_batch_stride=H * W if exclude is not None and exclude.dim() == 3 else 0,
                              out=out.data_ptr(), workspace=ws.data_ptr(), workspace_bytes=ws.numel())
    _lib.check(L.gs_depth_abs_rel(args, _lib.stream(dev)), "depth abs-rel")
    return out


def depth_abs_rel(est: torch.Tensor, gt: torch.Tensor, exclude: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The absolute relative depth error of unproject_image (metrics.py:197-205) per image of
    [B, H, W] (0-dim for one [H, W] pair), fp64 on the device: the mean of |gt - est| / gt over
    the pixels where est is finite, gt > 0 and exclude != 1 (exclude [H, W] or [B, H, W],
    optional; the reference's (1 - mask).bool()).  NaN for an image without a valid pixel, as
    torch.mean of an empty tensor.  Contiguous float32 device tensors (exclude of another dtype
    is converted).  Two calls give the same bits."""
    s = depth_abs_rel_sums(est, gt, exclude)
    r = s[:, 0] / s[:, 1]
    return r[0] if est.dim() == 2 else r


def depth_abs_rel_torch(est: torch.Tensor, gt: torch.Tensor, exclude: Optional[torch.Tensor] = None) -> torch.Tensor:
    """depth_abs_rel in PyTorch operations, any device and dtype (est's dtype throughout)."""
    est3, gt3, single = _check_depth_pair(est, gt, exclude, need=False)
    ok = torch.isfinite(est3) & (gt3 > 0)
    if exclude is not None:
        ok = ok & (exclude.to(est3.dtype) != 1)  # [H, W] broadcasts over the batch
    term = torch.where(ok, torch.abs(gt3 - est3) / gt3, torch.zeros_like(est3))
    r = term.sum(dim=(1, 2)) / ok.sum(dim=(1, 2)).to(est3.dtype)
    return r[0] if single else r


# ---- depth -> world points

def _check_depth_cams(depth, mats, need: bool):
    """depth [B, H, W] / [H, W] and (matrix, name, n) triples of its cameras."""
    d3, single = _maps(depth, "depth")
    if need:
        _need(depth, "depth")
    out = []
    for m, name, n in mats:
        m, _ = _mats(m, name, n)
        _same_batch(d3.shape[0], m, name)
        if need and not m.is_cuda:
            raise GsplatError(f"the HIP depth geometry needs device tensors ({name} is on the CPU)")
        out.append(m)
    return d3, out, single


def _unproject(depth3: torch.Tensor, xy: Optional[torch.Tensor], Kinv: torch.Tensor, c2w: torch.Tensor):
    B, H, W = depth3.shape
    L = _lib.load()
    dev = depth3.device
    xyz = torch.empty(B, H, W, 3, dtype=torch.float32, device=dev)
    args = _lib.GsDepthUnproject(B=B, H=H, W=W, depth=depth3.data_ptr(), xy=xy.data_ptr() if xy is not None else None,
                                 Kinv=Kinv.data_ptr(), c2w=c2w.data_ptr(), xyz=xyz.data_ptr())
    _lib.check(L.gs_depth_unproject(args, _lib.stream(dev)), "depth unproject")
    return xyz


def unproject_depth(depth: torch.Tensor, K: torch.Tensor, w2c: torch.Tensor) -> torch.Tensor:
    """World points [B, H, W, 3] ([H, W, 3] for one map) of depth maps [B, H, W] seen by cameras
    K [B, 3, 3], w2c [B, 4, 4]: xyz = c2w (depth * K^-1 (x, y, 1), 1), x the column, y the row
    (the module docstring maps the reference's three versions onto it).  K and w2c are
    inverted in fp64 on the device.  Contiguous float32 device depth."""
    d3, (K, w2c), single = _check_depth_cams(depth, ((K, "K", 3), (w2c, "w2c", 4)), need=True)
    xyz = _unproject(d3.detach(), None, _inv(K, torch.float32).contiguous(), _inv(w2c, torch.float32).contiguous())
    return xyz[0] if single else xyz


def _unproject_torch(depth3, x, y, K, w2c):
    """c2w (depth * K^-1 (x, y, 1), 1) with x, y broadcastable to depth3 [B, ...]; -> [B, ..., 3]."""
    dt = depth3.dtype
    Kinv, c2w = _inv(K, dt), _inv(w2c, dt)
    pix = torch.stack([x.expand_as(depth3), y.expand_as(depth3), torch.ones_like(depth3)], dim=-1)
    lead = (slice(None),) + (None,) * (depth3.dim() - 1)
    cam = depth3[..., None] * (Kinv[lead] * pix[..., None, :]).sum(-1)
    return (c2w[:, :3, :3][lead] * cam[..., None, :]).sum(-1) + c2w[:, :3, 3][lead]


def unproject_depth_torch(depth: torch.Tensor, K: torch.Tensor, w2c: torch.Tensor) -> torch.Tensor:
    """unproject_depth in PyTorch operations, any device and dtype (depth's dtype; the inverses
    are taken in fp64 and cast to it)."""
    d3, (K, w2c), single = _check_depth_cams(depth, ((K, "K", 3), (w2c, "w2c", 4)), need=False)
    x, y = _pixel_grid(d3.shape[1], d3.shape[2], d3)
    xyz = _unproject_torch(d3, x[None], y[None], K, w2c)
    return xyz[0] if single else xyz


# ---- depth-induced optical flow

def depth_flow(depth1: torch.Tensor, K1: torch.Tensor, c2w1: torch.Tensor, K2: torch.Tensor, w2c2: torch.Tensor,
               return_valid: bool = False):
    """The optical flow [B, 2, H, W] ([2, H, W] for one map) that depth1 [B, H, W] induces
    from camera 1 (K1, c2w1: camera-to-world) to camera 2 (K2, w2c2: world-to-camera):
    compute_optical_flow (ideaII.py:135-157).  q = K2 T (depth1 * K1^-1 (x, y, 1), 1) with
    T = w2c2 c2w1 composed in fp64, uv = q.xy / max(q.z, 1e-7) (the reference's clamp, kept),
    flow = uv - (x, y); channel 0 is along x.  With return_valid also the uint8 map
    depth1 > 0 and q.z > 1e-7.  Contiguous float32 device depth."""
    d3, (K1, c2w1, K2, w2c2), single = _check_depth_cams(
        depth1, ((K1, "K1", 3), (c2w1, "c2w1", 4), (K2, "K2", 3), (w2c2, "w2c2", 4)), need=True)
    B, H, W = d3.shape
    L = _lib.load()
    dev = d3.device
    Kinv1 = _inv(K1, torch.float32).contiguous()
    T = torch.matmul(w2c2.detach().double(), c2w1.detach().double()).to(torch.float32).contiguous()
    K2 = _f32(K2)
    flow = torch.empty(B, 2, H, W, dtype=torch.float32, device=dev)
    valid = torch.empty(B, H, W, dtype=torch.uint8, device=dev) if return_valid else None
    args = _lib.GsDepthFlow(B=B, H=H, W=W, depth1=d3.detach().data_ptr(), Kinv1=Kinv1.data_ptr(), T=T.data_ptr(),
                            K2=K2.data_ptr(), flow=flow.data_ptr(), valid=valid.data_ptr() if return_valid else None)
    _lib.check(L.gs_depth_flow(args, _lib.stream(dev)), "depth flow")
    if single:
        flow, valid = flow[0], valid[0] if return_valid else None
    return (flow, valid) if return_valid else flow


def depth_flow_torch(depth1: torch.Tensor, K1: torch.Tensor, c2w1: torch.Tensor, K2: torch.Tensor,
                     w2c2: torch.Tensor, return_valid: bool = False):
    """depth_flow in PyTorch operations, any device and dtype (depth1's dtype; K1^-1 and T are
    taken in fp64 and cast to it)."""
    d3, (K1, c2w1, K2, w2c2), single = _check_depth_cams(
        depth1, ((K1, "K1", 3), (c2w1, "c2w1", 4), (K2, "K2", 3), (w2c2, "w2c2", 4)), need=False)
    dt = d3.dtype
    x, y = _pixel_grid(d3.shape[1], d3.shape[2], d3)
    Kinv1 = _inv(K1, dt)[:, None, None]
    T = torch.matmul(w2c2.detach().double(), c2w1.detach().double()).to(dt)[:, None, None]
    K2 = K2.to(dt)[:, None, None]
    pix = torch.stack([x, y, torch.ones_like(x)], dim=-1)[None].expand(d3.shape[0], -1, -1, -1)
    cam1 = d3[..., None] * (Kinv1 * pix[..., None, :]).sum(-1)
    cam2 = (T[..., :3, :3] * cam1[..., None, :]).sum(-1) + T[..., :3, 3]
    q = (K2 * cam2[..., None, :]).sum(-1)
    uv = q[..., :2] / q[..., 2:].clamp(min=FLOW_MIN_Z)
    flow = (uv - pix[..., :2]).permute(0, 3, 1, 2)
    valid = ((d3 > 0) & (q[..., 2] > FLOW_MIN_Z)).to(torch.uint8)
    if single:
        flow, valid = flow[0], valid[0]
    return (flow, valid) if return_valid else flow


# ---- the bilinear border sampler

def _check_src(src, name: str, need: bool):
    if not isinstance(src, torch.Tensor) or src.dim() not in (3, 4):
        raise GsplatError(f"{name} must be a [B, Ch, H, W] or [Ch, H, W] tensor")
    if need:
        _need(src, name)
    if src.numel() == 0:
        raise GsplatError(f"{name} must not be empty (got {tuple(src.shape)})")
    return (src[None], True) if src.dim() == 3 else (src, False)


def _check_xy(src4, xy, need: bool):
    B = src4.shape[0]
    if not isinstance(xy, torch.Tensor) or xy.dim() not in (2, 3) or xy.shape[-1] != 2:
        raise GsplatError("xy must be a [B, N, 2] or [N, 2] tensor")
    if need:
        _need(xy, "xy")
    xy3 = xy[None] if xy.dim() == 2 else xy
    if xy3.shape[0] != B or xy3.shape[1] < 1:
        raise GsplatError(f"xy must hold N >= 1 positions for each of the {B} sources (got {tuple(xy.shape)})")
    return xy3


def _sample(src4, coords, mode, N, h=0, w=0, add=False):
    B, Ch, H, W = src4.shape
    L = _lib.load()
    dev = src4.device
    out = torch.empty(B, Ch, N, dtype=torch.float32, device=dev)
    args = _lib.GsSampleBilinear(B=B, Ch=Ch, H=H, W=W, mode=mode, add_displacement=1 if add else 0, N=N, h=h, w=w,
                                 src=src4.detach().data_ptr(), coords=coords.detach().data_ptr(), out=out.data_ptr())
    _lib.check(L.gs_sample_bilinear(args, _lib.stream(dev)), "sample bilinear")
    return out


def sample_bilinear(src: torch.Tensor, xy: torch.Tensor) -> torch.Tensor:
    """src [B, Ch, H, W] sampled at pixel coordinates xy [B, N, 2] (x, y) -> [B, Ch, N]
    ([Ch, N] for a [Ch, H, W] source with xy [N, 2]): F.grid_sample(mode='bilinear',
    padding_mode='border', align_corners=True) at those pixels.  A NaN coordinate gives NaN.
    Contiguous float32 device tensors."""
    src4, single = _check_src(src, "src", need=True)
    xy3 = _check_xy(src4, xy, need=True)
    out = _sample(src4, xy3, _lib.GS_SAMPLE_POINTS, xy3.shape[1])
    return out[0] if single else out


def sample_bilinear_torch(src: torch.Tensor, xy: torch.Tensor) -> torch.Tensor:
    """sample_bilinear in PyTorch operations, any device and dtype (src's dtype): clamp x to
    [0, W - 1] and y to [0, H - 1], x0 = min(floor(x), W - 2) (0 when W == 1), likewise y0, and
    the four taps gathered by index and blended with (1 - tx)(1 - ty), tx (1 - ty), (1 - tx) ty,
    tx ty.  In fp64 it equals torch's fp64 grid_sample to rounding."""
    src4, single = _check_src(src, "src", need=False)
    xy3 = _check_xy(src4, xy, need=False).to(src4.dtype)
    B, Ch, H, W = src4.shape
    x, y = xy3[..., 0], xy3[..., 1]
    bad = torch.isnan(x) | torch.isnan(y)
    x = torch.where(bad, torch.zeros_like(x), x).clamp(0, W - 1)
    y = torch.where(bad, torch.zeros_like(y), y).clamp(0, H - 1)
    x0 = torch.floor(x).clamp(max=max(W - 2, 0))
    y0 = torch.floor(y).clamp(max=max(H - 2, 0))
    tx, ty = (x - x0)[:, None], (y - y0)[:, None]
    x0, y0 = x0.long(), y0.long()
    x1, y1 = x0 + (1 if W > 1 else 0), y0 + (1 if H > 1 else 0)
    flat = src4.reshape(B, Ch, H * W)

    def tap(yy, xx):
        return torch.gather(flat, 2, (yy * W + xx)[:, None].expand(B, Ch, -1))

    out = (tap(y0, x0) * ((1 - tx) * (1 - ty)) + tap(y0, x1) * (tx * (1 - ty)) + tap(y1, x0) * ((1 - tx) * ty)
           + tap(y1, x1) * (tx * ty))
    out = torch.where(bad[:, None], torch.full((), float("nan"), dtype=out.dtype, device=out.device), out)
    return out[0] if single else out


def _check_flow_pair(flow, displacement, need: bool):
    f4, single = _check_src(flow, "flow", need)
    d4, d_single = _check_src(displacement, "displacement", need)
    if f4.shape[0] != d4.shape[0] or d4.shape[1] != 2 or single != d_single:
        raise GsplatError(f"displacement must be [B, 2, h, w] for flow [B, Ch, H, W], or [2, h, w] for [Ch, H, W] "
                          f"(got {tuple(displacement.shape)} for {tuple(flow.shape)})")
    return f4, d4, single


def warp_flow(flow: torch.Tensor, displacement: torch.Tensor) -> torch.Tensor:
    """flow [B, Ch, H, W] sampled at the pixel grid of displacement [B, 2, h, w] moved by it
    (channel 0 along x): warp_flow (ideaII.py:159-198), bilinear with border clamping;
    -> [B, Ch, h, w] ([Ch, h, w] for unbatched arguments).  Contiguous float32 device tensors."""
    f4, d4, single = _check_flow_pair(flow, displacement, need=True)
    h, w = d4.shape[-2:]
    out = _sample(f4, d4, _lib.GS_SAMPLE_DISPLACEMENT, h * w, h, w).reshape(f4.shape[0], f4.shape[1], h, w)
    return out[0] if single else out


def _displaced_xy(d4: torch.Tensor) -> torch.Tensor:
    x, y = _pixel_grid(d4.shape[-2], d4.shape[-1], d4)
    return torch.stack([x + d4[:, 0], y + d4[:, 1]], dim=-1).reshape(d4.shape[0], -1, 2)


def warp_flow_torch(flow: torch.Tensor, displacement: torch.Tensor) -> torch.Tensor:
    """warp_flow in PyTorch operations, any device and dtype (flow's dtype)."""
    f4, d4, single = _check_flow_pair(flow, displacement, need=False)
    h, w = d4.shape[-2:]
    out = sample_bilinear_torch(f4, _displaced_xy(d4.to(f4.dtype))).reshape(f4.shape[0], f4.shape[1], h, w)
    return out[0] if single else out


def _check_flows(flows, need: bool):
    flows = list(flows)
    if not flows:
        raise GsplatError("accumulate_flows: no flow")
    for i, f in enumerate(flows):
        if not isinstance(f, torch.Tensor) or f.dim() not in (3, 4) or f.shape[-3] != 2 or f.shape != flows[0].shape:
            raise GsplatError(f"flows[{i}] must be a [2, H, W] or [B, 2, H, W] tensor of the first flow's shape")
        if need:
            _need(f, f"flows[{i}]")
    return flows


def accumulate_flows(flows: Sequence[torch.Tensor]) -> torch.Tensor:
    """The chain of accumulate_flows (ideaII.py:200-206): acc = flows[0], then
    acc = acc + warp_flow(flows[i], acc) for every further flow, each step one launch.  flows
    are [2, H, W] or [B, 2, H, W], all of one shape.  Contiguous float32 device tensors."""
    flows = _check_flows(flows, need=True)
    acc = flows[0].detach().clone()
    a4 = acc[None] if acc.dim() == 3 else acc
    B, _, H, W = a4.shape
    for f in flows[1:]:
        f4 = f[None] if f.dim() == 3 else f
        a4 = _sample(f4, a4, _lib.GS_SAMPLE_DISPLACEMENT, H * W, H, W, add=True).reshape(B, 2, H, W)
    return a4[0] if flows[0].dim() == 3 else a4


def accumulate_flows_torch(flows: Sequence[torch.Tensor]) -> torch.Tensor:
    """accumulate_flows in PyTorch operations, any device and dtype."""
    flows = _check_flows(flows, need=False)
    acc = flows[0].clone()
    for f in flows[1:]:
        acc = acc + warp_flow_torch(f, acc)
    return acc


def resize_flow(flow: torch.Tensor, size) -> torch.Tensor:
    """resize_optical_flow (ideaII.py:219-257) for channels-first flows [2, H, W] or
    [B, 2, H, W]: resample.bilinear_resize(flow, size, align_corners=False), then channel 0
    times w / W and channel 1 times h / H.  Contiguous float32 device tensors."""
    from .resample import bilinear_resize
    if not isinstance(flow, torch.Tensor) or flow.dim() not in (3, 4) or flow.shape[-3] != 2:
        raise GsplatError("flow must be a [2, H, W] or [B, 2, H, W] tensor")
    out = bilinear_resize(flow.detach(), size, align_corners=False)
    h, w = out.shape[-2:]
    H, W = flow.shape[-2:]
    out[..., 0, :, :] *= w / W  # Python scalars: kernel arguments, no copy to the device
    out[..., 1, :, :] *= h / H
    return out


def resize_flow_torch(flow: torch.Tensor, size) -> torch.Tensor:
    """resize_flow in PyTorch operations, any device and dtype; the axis rule is evaluated in
    fp64 for fp64 flows (F.interpolate's weights for them), in fp32 otherwise."""
    from .resample import bilinear_resize_torch
    if not isinstance(flow, torch.Tensor) or flow.dim() not in (3, 4) or flow.shape[-3] != 2:
        raise GsplatError("flow must be a [2, H, W] or [B, 2, H, W] tensor")
    axis = torch.float64 if flow.dtype == torch.float64 else torch.float32
    out = bilinear_resize_torch(flow, size, align_corners=False, axis_dtype=axis).clone()
    h, w = out.shape[-2:]
    H, W = flow.shape[-2:]
    out[..., 0, :, :] *= w / W
    out[..., 1, :, :] *= h / H
    return out


# ---- 2-D tracks lifted to 3-D

def _check_tracks(tracks_xy, depths, K, w2c, need: bool):
    if not isinstance(depths, torch.Tensor) or depths.dim() != 3 or depths.numel() == 0:
        raise GsplatError("depths must be a non-empty [T, H, W] tensor")
    T = depths.shape[0]
    if not isinstance(tracks_xy, torch.Tensor) or tracks_xy.dim() != 3 or tracks_xy.shape[0] != T \
            or tracks_xy.shape[1] < 1 or tracks_xy.shape[2] != 2:
        raise GsplatError(f"tracks_xy must be [T, N, 2] with T = {T}, N >= 1")
    if need:
        _need(depths, "depths")
        _need(tracks_xy, "tracks_xy")
    K, _ = _mats(K, "K", 3)
    w2c, _ = _mats(w2c, "w2c", 4)
    _same_batch(T, K, "K")
    _same_batch(T, w2c, "w2c")
    return K, w2c


def lift_tracks(tracks_xy: torch.Tensor, depths: torch.Tensor, K: torch.Tensor, w2c: torch.Tensor) -> torch.Tensor:
    """2-D tracks tracks_xy [T, N, 2] (pixel x, y in each of T frames) lifted to world points
    [N, T, 3] through the frames' depth maps depths [T, H, W] and cameras K [T, 3, 3],
    w2c [T, 4, 4] (dyn_som.py:268-286): the depth is sampled bilinearly with border clamping
    (one sample_bilinear launch) and the point is c2w (depth * K^-1 (x, y, 1), 1) at the track's
    own sub-pixel coordinates (one unprojection launch).  Parity unpinned (module docstring).
    Contiguous float32 device tensors."""
    K, w2c = _check_tracks(tracks_xy, depths, K, w2c, need=True)
    T, N = tracks_xy.shape[:2]
    xy = tracks_xy.detach()
    d = _sample(depths.detach()[:, None], xy, _lib.GS_SAMPLE_POINTS, N)  # [T, 1, N]
    xyz = _unproject(d, xy, _inv(K, torch.float32).contiguous(), _inv(w2c, torch.float32).contiguous())
    return xyz.reshape(T, N, 3).transpose(0, 1).contiguous()


def lift_tracks_torch(tracks_xy: torch.Tensor, depths: torch.Tensor, K: torch.Tensor,
                      w2c: torch.Tensor) -> torch.Tensor:
    """lift_tracks in PyTorch operations, any device and dtype (the depths' dtype)."""
    K, w2c = _check_tracks(tracks_xy, depths, K, w2c, need=False)
    xy = tracks_xy.to(depths.dtype)
    d = sample_bilinear_torch(depths[:, None], xy)[:, 0]  # [T, N]
    return _unproject_torch(d, xy[..., 0], xy[..., 1], K, w2c).transpose(0, 1).contiguous()


# ---- the cameras of rasterization settings

def cameras_of_settings(settings_list) -> Tuple[torch.Tensor, torch.Tensor, Tuple[int, int]]:
    """(w2c [C, 4, 4], K [C, 3, 3], (H, W)) of a list of GaussianRasterizationSettings of one
    image size: w2c is the transposed viewmatrix, K the pinhole of tanfovx / tanfovy and the
    principal point (camera.setup_camera read backwards).  On the viewmatrices' device, with
    no blocking copy: K is staged in pinned memory."""
    from .rasterizer import _principal_point
    sets = list(settings_list)
    if not sets:
        raise GsplatError("cameras_of_settings: no camera")
    H, W = int(sets[0].image_height), int(sets[0].image_width)
    rows = []
    for s in sets:
        if (int(s.image_height), int(s.image_width)) != (H, W):
            raise GsplatError("cameras_of_settings: the cameras must share one image size")
        cx, cy = _principal_point(s)
        rows.append([W / (2.0 * s.tanfovx), 0.0, cx, 0.0, H / (2.0 * s.tanfovy), cy, 0.0, 0.0, 1.0])
    w2c = torch.stack([s.viewmatrix.detach().reshape(4, 4).t() for s in sets]).to(torch.float32).contiguous()
    K = torch.tensor(rows, dtype=torch.float32)
    if w2c.is_cuda:
        K = K.pin_memory().to(w2c.device, non_blocking=True)
    return w2c, K.reshape(len(sets), 3, 3), (H, W)
