"""Point tracking on a reconstructed sequence: where does a pixel of camera c
at time t0 go in every other frame and camera?  (C ABI include/gs_track.h,
kernels csrc/gs_track.hip.)

The reference carries the evaluation side of tracking -- PCK
(metrics.py:489-520; here metrics.PCK) over 2-D tracks it loads or derives
(dyn_som.py:171-230 load_target_tracks / get_tracks_3d) -- and no kernel that
says which Gaussians a pixel is made of.  Here the tracks come from the
rasterizer itself:

    contributor_maps   per pixel the K Gaussians of largest blend weight w = alpha T among
                       those the forward blended there, with their weights (HIP, needs the device)
    select_gaussians   the Gaussian under each query pixel
    project_tracks     the chosen Gaussians' means through every camera at every timestep,
                       exactly as the forward projects them (HIP; a torch fallback on the CPU)
    track_points       the three together: 2-D tracks, depths and visibility of query pixels

Pixel convention: the forward's (means2D): pixel centres at integer
coordinates, x right, y down; a coordinate's pixel is floor(v + 0.5).
The maps are piecewise constant in every input: nothing here is differentiable
and everything runs under torch.no_grad().
"""
from __future__ import annotations

from typing import Callable, NamedTuple, Optional, Sequence, Tuple, Union

import torch

from . import _C, _lib
from ._lib import GsplatError

MAX_K = _lib.GS_TRACK_MAX_K


def _cameras(settings_list):
    """The stacked cameras of a batch: a list of GaussianRasterizationSettings, or (reused over
    calls: built once, its background comparison reads device values) a GaussianRasterizerBatch
    or this function's own result."""
    from .rasterizer import GaussianRasterizerBatch, _BatchCameras
    if isinstance(settings_list, _BatchCameras):
        return settings_list
    if isinstance(settings_list, GaussianRasterizerBatch):
        return settings_list._cams
    return _BatchCameras(list(settings_list))


def _pixel(v: torch.Tensor) -> torch.Tensor:
    return torch.floor(v + 0.5).long()


def contributor_maps(settings_list, rendervar: dict, K: int = 1, *, compat: Optional[str] = None, windows=None,
                     plan_state=None):
    """Render the cameras `settings_list` from `rendervar` (timesteps.params2rendervar; the
    keyword inputs of GaussianRasterizerBatch) forward only and return
    (top_id int32 [C,K,H,W], top_w [C,K,H,W], color [C,3,H,W], depth [C,1,H,W], alpha [C,1,H,W]).

    top_id[c, k, y, x] is the Gaussian with the k-th largest blend weight w = alpha T among the
    entries the forward blended at that pixel of camera c (between equal weights the nearer
    one), top_w its weight; -1 / 0 where fewer than k + 1 entries blended and outside a
    camera's tile window.  K in 1..4.  colour, depth and alpha are the batch forward's, bit for
    bit.  `compat`: the settings' numerics unless given (the maps do not depend on it);
    `windows`: per-camera tile windows, the settings' `tile_window`s unless given;
    `plan_state`: a _C.BinningPlan for the sync-free forward (the same maps).  Semantic features
    are not rendered.  Device tensors only."""
    from .rasterizer import _compat_of, _empty_like_none
    K = int(K)
    if not 1 <= K <= MAX_K:
        raise ValueError(f"K must be in 1..{MAX_K}, got {K}")
    cams = _cameras(settings_list)
    rs0 = cams.rs0
    means3D = rendervar["means3D"]
    if not isinstance(means3D, torch.Tensor) or not means3D.is_cuda:
        raise GsplatError("contributor_maps needs device tensors (there is no CPU rasterizer)")
    compat = _compat_of(rs0) if compat is None else compat
    windows = cams.windows if windows is None else windows
    cx, cy = [p[0] for p in cams.pp], [p[1] for p in cams.pp]
    with torch.no_grad():
        get = lambda k: _empty_like_none(rendervar.get(k))  # noqa: E731
        shs, colors = rendervar.get("shs"), rendervar.get("colors_precomp")
        if (shs is None) == (colors is None):
            raise ValueError("provide exactly one of shs / colors_precomp")
        out = _C.rasterize_gaussians_batch(
            rs0.bg, means3D.detach(), get("colors_precomp"), None, rendervar["opacities"], get("scales"),
            get("rotations"), rs0.scale_modifier, get("cov3D_precomp"), cams.views, cams.projs, cx, cy, cams.tx,
            cams.ty, rs0.image_height, rs0.image_width, get("shs"), rs0.sh_degree, cams.cpos, rs0.prefiltered, False,
            compat=compat, windows=windows, plan_state=plan_state)
        _, color, _, depth, alpha, _, geom, binning, img, num_instances = out
        top_id, top_w = _C.rasterize_gaussians_batch_contributors(
            geom, binning, img, num_instances, cx, cy, cams.tx, cams.ty, rs0.bg, cams.views, cams.projs, cams.cpos,
            rs0.image_height, rs0.image_width, means3D.size(0), K, compat=compat, windows=windows)
    return top_id, top_w, color, depth, alpha


def select_gaussians(top_id: torch.Tensor, xy: torch.Tensor, cam: Union[int, torch.Tensor], rank: int = 0
                     ) -> torch.Tensor:
    """The Gaussian under each query: top_id[cam, rank] ([C,K,H,W], contributor_maps) at the
    pixel floor(xy + 0.5) of every query xy [N, 2] (x, y); `cam` one camera index or [N] of
    them.  int64 [N]; -1 outside the image and where nothing was blended.  Plain torch, any
    device."""
    if top_id.dim() != 4:
        raise ValueError(f"top_id must be [C, K, H, W], got {tuple(top_id.shape)}")
    C, K, H, W = top_id.shape
    if not 0 <= int(rank) < K:
        raise ValueError(f"rank {rank} outside 0..{K - 1}")
    xy = torch.as_tensor(xy, device=top_id.device)
    if xy.dim() != 2 or xy.size(1) != 2:
        raise ValueError(f"xy must be [N, 2], got {tuple(xy.shape)}")
    N = xy.size(0)
    if isinstance(cam, int) and not 0 <= cam < C:
        raise ValueError(f"cam {cam} outside 0..{C - 1}")
    cam = torch.as_tensor(cam, device=top_id.device, dtype=torch.long)
    cam = cam.expand(N) if cam.dim() == 0 else cam.reshape(N)
    px, py = _pixel(xy[:, 0].float()), _pixel(xy[:, 1].float())
    ok = (px >= 0) & (px < W) & (py >= 0) & (py < H) & (cam >= 0) & (cam < C)  # a camera index out of range: -1
    ids = top_id[cam.clamp(0, C - 1), int(rank), py.clamp(0, max(H - 1, 0)), px.clamp(0, max(W - 1, 0))].long()
    return torch.where(ok, ids, torch.full_like(ids, -1))


def project_tracks_torch(means3D_T: torch.Tensor, ids: torch.Tensor, views: torch.Tensor, projs: torch.Tensor,
                         W: int, H: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """gs_track_project in PyTorch operations, in the kernel's operation order (elementwise
    fp32 products and sums, the pixel conversion in fp64): views / projs [C,16] as the settings
    hold them (element 4 i + j: input i, output j)."""
    m = means3D_T.float()
    T, P = m.shape[0], m.shape[1]
    ids = ids.long()
    N, C = ids.numel(), views.shape[0]
    valid = (ids >= 0) & (ids < P)
    p = m[:, ids.clamp(0, max(P - 1, 0))] if P else m.new_zeros(T, N, 3)  # [T,N,3]
    x, y, z = (p[:, None, :, i] for i in range(3))  # [T,1,N]
    v, pr = views.float().reshape(C, 16), projs.float().reshape(C, 16)

    def row(mat, j):  # output j of p through mat: m[j] x + m[4+j] y + m[8+j] z + m[12+j]
        e = lambda i: mat[None, :, i, None]  # noqa: E731  [1,C,1]
        return e(j) * x + e(4 + j) * y + e(8 + j) * z + e(12 + j)

    depth = row(v, 2)
    pw = 1.0 / (row(pr, 3) + 0.0000001)
    ndc_x, ndc_y = row(pr, 0) * pw, row(pr, 1) * pw
    u = (((ndc_x.double() + 1.0) * float(W) - 1.0) * 0.5).float()
    w_ = (((ndc_y.double() + 1.0) * float(H) - 1.0) * 0.5).float()
    ru, rv = torch.floor(u + 0.5), torch.floor(w_ + 0.5)
    inside = (depth > 0) & (ru >= 0) & (ru < W) & (rv >= 0) & (rv < H) & valid[None, None]
    keep = (ids >= 0)[None, None] & (P > 0)
    zero = torch.zeros((), dtype=torch.float32, device=m.device)
    uv = torch.stack([torch.where(keep, u, zero), torch.where(keep, w_, zero)], dim=-1)
    return uv, torch.where(keep, depth, zero), inside


def project_tracks(means3D_T: torch.Tensor, ids: torch.Tensor, settings_list
                   ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The means means3D_T[t, ids[n]] ([T,P,3]; ids [N], -1 = none) through every camera of
    `settings_list` at every timestep, as the forward's preprocess projects them:
    (uv [T,C,N,2], depth [T,C,N], inside bool [T,C,N]).  uv and depth equal the forward's
    means2D and depths bit for bit; inside = in front of the camera (z > 0) and the pixel
    floor(uv + 0.5) in the image.  ids < 0 give zeros and inside = False; an id >= P is a
    caller's error (ValueError where the ids are host tensors; on the device it is clamped and
    flagged inside = False).  Device tensors run the HIP kernel, CPU tensors the torch
    statement of it (project_tracks_torch)."""
    if means3D_T.dim() != 3 or means3D_T.size(2) != 3:
        raise ValueError(f"means3D_T must be [T, P, 3], got {tuple(means3D_T.shape)}")
    cams = _cameras(settings_list)
    rs0 = cams.rs0
    ids = torch.as_tensor(ids, device=means3D_T.device).reshape(-1)
    with torch.no_grad():
        if not means3D_T.is_cuda:
            if ids.numel() and int(ids.max()) >= means3D_T.size(1):
                raise ValueError(f"ids must be < P = {means3D_T.size(1)}")
            return project_tracks_torch(means3D_T, ids, cams.views.cpu(), cams.projs.cpu(), rs0.image_width,
                                        rs0.image_height)
        return _C.track_project(means3D_T.detach(), ids, rs0.bg, cams.views, cams.projs, [p[0] for p in cams.pp],
                                [p[1] for p in cams.pp], cams.tx, cams.ty, cams.cpos, rs0.image_height,
                                rs0.image_width)


def visible_in_maps(top_id: torch.Tensor, ids: torch.Tensor, uv: torch.Tensor, inside: torch.Tensor
                    ) -> torch.Tensor:
    """One timestep's visibility: visible[c, n] = inside[c, n] and ids[n] is among the K ids of
    top_id ([C,K,H,W]) at the pixel floor(uv[c, n] + 0.5).  uv [C,N,2], inside [C,N].  Plain
    torch, any device."""
    C, K, H, W = top_id.shape
    px = _pixel(uv[..., 0]).clamp(0, max(W - 1, 0))
    py = _pixel(uv[..., 1]).clamp(0, max(H - 1, 0))
    cam = torch.arange(C, device=top_id.device)[:, None].expand_as(px)
    at_pixel = top_id[cam, :, py, px].long()  # [C,N,K]
    ids = ids.long()
    hit = (at_pixel == ids[None, :, None]).any(dim=-1)
    return inside.bool() & hit & (ids >= 0)[None]


class Tracks(NamedTuple):
    """track_points' result for N queries, C cameras, T timesteps."""
    ids: torch.Tensor      # [N] int64: the Gaussian under each query, -1 = none
    uv: torch.Tensor       # [T,C,N,2] pixel coordinates (zeros for id -1)
    depth: torch.Tensor    # [T,C,N] view-space z
    inside: torch.Tensor   # [T,C,N] bool: in front of the camera and in the image
    visible: torch.Tensor  # [T,C,N] bool: inside, and among the pixel's K largest contributors


def _rendervars(params_seq, num_timesteps, device) -> Tuple[Callable[[int], dict], int]:
    """t -> rendervar and T of track_points' `params_seq`."""
    from .timesteps import params2rendervar

    def as_rv(d):
        d = {k: torch.as_tensor(v, device=device) for k, v in d.items()}
        return d if "opacities" in d else params2rendervar(d)

    if callable(params_seq):
        if num_timesteps is None:
            raise ValueError("a callable params_seq needs num_timesteps")
        return params_seq, int(num_timesteps)
    if isinstance(params_seq, dict):  # params_io.load_params: per-timestep keys stacked [T, ...], the others once
        T = int(params_seq["means3D"].shape[0])
        if len(params_seq["means3D"].shape) != 3:
            raise ValueError("a params dict holds means3D stacked over timesteps, [T, P, 3]")
        once = {"means3D": 2, "rgb_colors": 2, "unnorm_rotations": 2}  # dimensions of a key saved once
        return (lambda t: as_rv({k: (v[t] if len(v.shape) == once.get(k, -2) + 1 else v)
                                 for k, v in params_seq.items()})), T
    seq = list(params_seq)
    return (lambda t: as_rv(seq[t])), len(seq)


def track_points(params_seq, settings_list, queries_xy: torch.Tensor, query_cam: Union[int, torch.Tensor],
                 query_t: int = 0, K: int = 1, *, num_timesteps: Optional[int] = None) -> Tracks:
    """2-D tracks of query pixels: the Gaussian of largest blend weight under each query
    (queries_xy [N,2] in camera `query_cam` at timestep `query_t`) is followed through every
    camera of `settings_list` at every timestep.

    `params_seq`: the sequence's parameters -- a list of per-timestep dicts (Dynamic3DGaussians
    params, or rendervars: timesteps.params2rendervar is applied to the former), the dict
    params_io.load_params reads back (per-timestep keys stacked [T, ...]), or a callable
    t -> rendervar with `num_timesteps`.  Every timestep holds the same Gaussians.

    visible[t, c, n] = inside[t, c, n] and the query's Gaussian is among the K largest
    contributors of the pixel it lands on in camera c at timestep t: one contributor_maps call
    per timestep, the gather in plain torch.  Nothing is read back."""
    cams = _cameras(settings_list)
    device = cams.views.device
    rv_of, T = _rendervars(params_seq, num_timesteps, device)
    if not 0 <= int(query_t) < T:
        raise ValueError(f"query_t {query_t} outside 0..{T - 1}")
    with torch.no_grad():
        maps, means = [], []
        for t in range(T):
            rv = rv_of(t)
            maps.append(contributor_maps(cams, rv, K)[0])
            means.append(rv["means3D"].detach().float())
        ids = select_gaussians(maps[int(query_t)], torch.as_tensor(queries_xy, device=device), query_cam, 0)
        uv, depth, inside = project_tracks(torch.stack(means), ids.int(), cams)
        visible = torch.stack([visible_in_maps(maps[t], ids, uv[t], inside[t]) for t in range(T)])
    return Tracks(ids, uv, depth, inside, visible)
