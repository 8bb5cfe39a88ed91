"""Positional mirror of the reference's pybind module `diff_gaussian_rasterization._C`.

Reference: DGR/ext.cpp:15-19 and DGR/rasterize_points.cu:35-246 (DGR =
submodules_fsgs/diff-gaussian-rasterization-confidence).  The three functions
keep the reference's exact positional signatures and return tuples, so the
reference's own autograd wrapper could call them unchanged.  Their arguments
are marshalled by the C++ binding (csrc/gs_torch_binding.cpp, a torch
extension next to the library): it allocates outputs with torch (caching
allocator) and hands raw device pointers to the HIP C ABI (libgsplat_hip.so).
This module keeps what is cheaper or clearer in Python in front of it: the
answers for an empty scene, the `out`-name checks and the sync-free plan's
bookkeeping.  There is no CPU fallback and no second binding: non-device
inputs, a missing library or a missing extension raise.

Superset behaviour (documented in DESIGN.md "Boundary"):
  * semantic_feature may be None/empty (F = 0), [P, F] or [P, 1, F]; any F is
    accepted and zero-padded to the next compiled width (0, 4, 8, 16, 32, 36, 64).
  * keyword-only `compat` selects "reference" (as-shipped numerics, default)
    or "fixed" numerics; see DESIGN.md "Quirks".
"""
from __future__ import annotations

import importlib.util
import math
import os

import torch

from . import _lib
from ._lib import check

_default_compat = "reference"

_native = None  # the C++ binding (csrc/gs_torch_binding.cpp), once loaded


def _native_mod():
    """The C++ binding, loaded by the library's own rule (_lib.load): rebuilt
    first when it is older than its source, a public header or the library."""
    global _native
    if _native is not None:
        return _native
    _lib.load()
    build = _lib._build
    path = build.NATIVE
    try:
        if build.native_is_stale():
            build.build_native()
    except Exception as ex:  # no toolchain, or a compile error
        raise _lib.GsplatError(f"{os.path.basename(path)} is missing or older than its sources and could not be "
                               f"rebuilt ({ex}); build it with `python -m dynamic3dgaussians_amd.build`") from None
    spec = importlib.util.spec_from_file_location(build.NATIVE_NAME, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    if mod.abi_version() != _lib.ABI_VERSION:
        raise _lib.GsplatError(f"{os.path.basename(path)} was built for ABI {mod.abi_version()}, the library is "
                               f"{_lib.ABI_VERSION}; rebuild with `python -m dynamic3dgaussians_amd.build`")
    _native = mod
    return _native


def native_loaded() -> bool:
    """Whether the C++ binding is loaded (loads it; tests / diagnostics)."""
    return _native_mod() is not None


def _opt(t):
    return t if isinstance(t, torch.Tensor) else None


def set_default_compat(mode: str) -> None:
    """Process-wide default numerics mode ("reference" or "fixed")."""
    global _default_compat
    if mode not in _lib.GS_COMPAT:
        raise ValueError(f"compat must be one of {list(_lib.GS_COMPAT)}, got {mode!r}")
    _default_compat = mode


def get_default_compat() -> str:
    return _default_compat


def _present(t) -> bool:
    return t is not None and isinstance(t, torch.Tensor) and t.numel() > 0


def _dev(t: torch.Tensor, device, name: str) -> torch.Tensor:
    if t.device != device:
        raise _lib.GsplatError(f"{name} is on {t.device}, expected {device} (HIP device tensors only)")
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def _feature_width(F: int) -> int:
    for k in _lib.SUPPORTED_F:
        if k >= F:
            return k
    raise _lib.GsplatError(f"semantic feature width {F} exceeds the largest compiled width "
                           f"{_lib.SUPPORTED_F[-1]}")


def _compat_code(compat) -> int:
    mode = _default_compat if compat is None else compat
    if mode not in _lib.GS_COMPAT:
        raise ValueError(f"compat must be one of {list(_lib.GS_COMPAT)}, got {mode!r}")
    return _lib.GS_COMPAT[mode]


def _num_points(means3D, windowed=False) -> int:
    """P of a call, after the two checks every call answers before anything
    else is looked at.  `windowed`: a temporal window's (P, B, 3) means."""
    if windowed:
        if means3D.ndimension() != 3 or means3D.size(2) != 3:
            raise RuntimeError("means3D must have dimensions (num_points, frames, 3) with cam_frames")
    elif means3D.ndimension() != 2 or means3D.size(1) != 3:
        raise RuntimeError("means3D must have dimensions (num_points, 3)")  # rasterize_points.cu:60-62
    if means3D.device.type != "cuda":
        raise _lib.GsplatError("the HIP rasterizer needs device tensors (means3D is on the CPU)")
    return means3D.size(0)


# A single camera is a batch of one: the two functions below wrap their
# camera as one-element lists, call the batch code further down (the one place
# the arguments are handled) and strip the leading camera dimension (views).

def rasterize_gaussians(background, means3D, colors, semantic_feature, opacity, scales, rotations,
                        scale_modifier, cov3D_precomp, viewmatrix, projmatrix, c_x, c_y, tan_fovx,
                        tan_fovy, image_height, image_width, sh, degree, campos, prefiltered, debug,
                        *, compat=None):
    """RasterizeGaussiansCUDA (DGR/rasterize_points.cu:35-126).

    Returns (num_rendered, color[3,H,W], feature_map[F,H,W], depth[1,H,W],
    alpha[1,H,W], radii[P] int32, geomBuffer, binningBuffer, imgBuffer).
    """
    # num_rendered is the reference's count (returned, like the reference);
    # the binned tile lists hold num_instances <= num_rendered entries
    NR, color, fmap, depth, alpha, radii, geom, binning, img, NI = rasterize_gaussians_batch(
        background, means3D, colors, semantic_feature, opacity, scales, rotations, scale_modifier,
        cov3D_precomp, viewmatrix, projmatrix, [c_x], [c_y], [tan_fovx], [tan_fovy], image_height,
        image_width, sh, degree, campos, prefiltered, debug, compat=compat)
    if not NI[0]:
        binning = binning[:0]  # no instances: the empty buffer this function has always returned
    return (NR[0], color[0], fmap[0], depth[0], alpha[0], radii[0], geom, binning, img)


def spatial_order(means3D: torch.Tensor) -> torch.Tensor:
    """gs_spatial_order: the ids 0..P-1 in 3-D Morton order of the means
    (int32 [P] on the means' device) -- a walk order for the binning passes
    (gs_gaussians.walk_order) that keeps each binning workgroup's slice of
    the Gaussians compact on the screen."""
    if not (means3D.is_cuda and means3D.dtype == torch.float32 and means3D.dim() == 2 and means3D.size(1) == 3):
        raise RuntimeError("spatial_order: means3D must be an fp32 [P, 3] device tensor")
    L_ = _lib.load()
    m = means3D.detach().contiguous()
    P = m.size(0)
    order = torch.empty(P, dtype=torch.int32, device=m.device)
    scratch = torch.empty(max(1, L_.gs_spatial_order_scratch_bytes(P)), dtype=torch.uint8, device=m.device)
    check(L_.gs_spatial_order(P, m.data_ptr(), order.data_ptr(), scratch.data_ptr(), _lib.stream(m.device)),
          "spatial order")
    return order


def _buffer_shapes(P, F, M):
    """The backward's nine gradients, in the order of its return tuple."""
    return dict(dmeans2D=(P, 3), dcolors=(P, 3), dsem=(P, F), dopacity=(P, 1), dmeans3D=(P, 3),
                dcov3D=(P, 6), dsh=(P, M, 3), dscales=(P, 3), drot=(P, 4))


_BUFFER_ORDER = tuple(_buffer_shapes(0, 0, 0))
_BUFFER_NAMES = frozenset(_BUFFER_ORDER)
_NO_DEST = torch.empty(0)  # the native backward's `out` entry: allocate this gradient


def backward_buffers(P, F, M, device, flat=False):
    """Uninitialised gradient outputs of rasterize_gaussians_backward (F = the
    compiled feature width, M = SH coefficients per Gaussian).  With
    `flat=True` they are contiguous views into one buffer (each starting on a
    256-byte boundary) and (views, buffer, offsets) is returned, so that sums
    of whole gradient sets take one elementwise launch."""
    shapes = _buffer_shapes(P, F, M)
    if not flat:
        return {k: torch.empty(*shape, dtype=torch.float32, device=device) for k, shape in shapes.items()}
    offs, o = {}, 0
    for k, shape in shapes.items():
        n = math.prod(shape)
        offs[k] = (o, n, shape)
        o += (n + 63) // 64 * 64
    buf = torch.empty(max(o, 1), dtype=torch.float32, device=device)
    return carve_buffers(buf, offs), buf, offs


def carve_buffers(buf, offs) -> dict:
    """The per-gradient views of a flat backward buffer (see backward_buffers)."""
    return {k: buf[o:o + n].view(*shape) for k, (o, n, shape) in offs.items()}


def rasterize_gaussians_backward(background, means3D, radii, colors, semantic_feature, scales,
                                 rotations, scale_modifier, cov3D_precomp, viewmatrix, projmatrix,
                                 c_x, c_y, tan_fovx, tan_fovy, dL_dout_color, dL_dout_feature,
                                 dL_dout_depth, dL_dout_alpha, sh, degree, campos, geomBuffer, R,
                                 binningBuffer, imageBuffer, alphas, debug, *, compat=None,
                                 grad_mask=None, out=None, accumulate=False, densify=None):
    """RasterizeGaussiansBackwardCUDA (DGR/rasterize_points.cu:128-225).

    Camera scalars are consumed in this positional order, exactly as the
    reference binding consumes them.  Returns (dL_dmeans2D[P,3],
    dL_dcolors[P,3], dL_dsemantic[P,F], dL_dopacity[P,1], dL_dmeans3D[P,3],
    dL_dcov3D[P,6], dL_dsh[P,M,3], dL_dscales[P,3], dL_drotations[P,4]).

    `grad_mask` (keyword-only, no reference analogue in the binding): an
    optional per-Gaussian [P] mask fused into the kernel, equal to the
    reference wrapper's `grad * label` (__init__.py:159-173) on every returned
    gradient except dL_dmeans2D and dL_dsemantic.

    `out` / `accumulate` (keyword-only, no reference analogue): caller-owned
    gradient buffers (a dict with the keys of `backward_buffers`) written in
    place, and with `accumulate=True` ADDED to (GS_FLAG_ACCUMULATE) -- the
    multi-camera gradient sink (rasterizer.GradientSink).  Accumulating calls
    into the same buffers must be ordered on one stream.

    `densify` (keyword-only, no reference analogue): optional (accum, denom,
    max_radius) fp32 [P] tensors that receive this view's densification
    statistics (external.py:136-140, train.py:288-290; gsplat_hip.h
    gs_gaussians.densify_accum), written or, with `accumulate`, added.
    """
    return _backward(background, means3D, radii.unsqueeze(0), colors, semantic_feature, scales, rotations,
                     scale_modifier, cov3D_precomp, viewmatrix, projmatrix, [c_x], [c_y], [tan_fovx], [tan_fovy],
                     dL_dout_color, dL_dout_feature, dL_dout_depth, dL_dout_alpha, sh, degree, campos, geomBuffer,
                     [R], binningBuffer, imageBuffer, alphas, debug, compat=compat, grad_mask=grad_mask,
                     densify=densify, out=out, exact_out=True, accumulate=accumulate)


def binned_instances(imageBuffer, image_height, image_width) -> int:
    """Length of the tile lists a forward binned (num_instances <= the
    returned num_rendered): read from the image buffer's tile ranges.  An
    introspection helper (byte models, tests); synchronises the stream."""
    L_ = _lib.load()
    W, H = int(image_width), int(image_height)
    tiles = ((W + 15) // 16) * ((H + 15) // 16)
    rg = torch.empty(max(tiles, 1), 2, dtype=torch.int32, device=imageBuffer.device)
    check(L_.gs_debug_export(0, W, H, None, None, imageBuffer.data_ptr(), 0, None, None, None, None, None,
                             None, rg.data_ptr(), None, _lib.stream(imageBuffer.device)), "binned_instances")
    r = rg[:tiles].cpu().numpy().view("uint32")
    return int(r[:, 1].max()) if tiles else 0


def mark_visible(means3D, viewmatrix, projmatrix):
    """markVisible (DGR/rasterize_points.cu:227-246): bool[P], view-space z > 0."""
    L_ = _lib.load()
    dev = means3D.device
    if dev.type != "cuda":
        raise _lib.GsplatError("mark_visible needs device tensors")
    P = means3D.size(0)
    present = torch.zeros(P, dtype=torch.bool, device=dev)
    if P:
        m = _dev(means3D, dev, "means3D")
        v = _dev(viewmatrix, dev, "viewmatrix").reshape(-1)
        pr = _dev(projmatrix, dev, "projmatrix").reshape(-1)
        check(L_.gs_mark_visible(P, m.data_ptr(), v.data_ptr(), pr.data_ptr(), present.data_ptr(),
                                 _lib.stream(dev)), "mark_visible")
    return present


# ---------------------------------------------------------------------------
# Camera batches (include/gsplat_hip.h gs_*_batch; no reference analogue): the
# C cameras of one multi-camera step rendered with one launch per stage.
# rasterize_gaussians_batch and _backward are the forward and backward bodies
# of every call, the single-camera functions above included (C = 1, where the
# batch entry points run exactly what the single-camera ones run).

def _event_handle(ev) -> int:
    """The hipEvent_t of a recorded torch.cuda.Event (0 = none)."""
    return 0 if ev is None else int(ev.cuda_event)


def _frames_arg(cam_frames):
    """A temporal window's per-camera frames as the native binding takes
    them: C ints, or an empty list for none."""
    return [] if cam_frames is None else [int(f) for f in cam_frames]


def _windows_arg(windows):
    """Tile windows as the native binding takes them: C x [x0, y0, x1, y1]
    (all 0 = the whole image), or an empty list for none."""
    if windows is None:
        return []
    return [[0, 0, 0, 0] if w is None else [int(v) for v in w] for w in windows]


class BinningPlan:
    """State of the sync-free batch forward (gs_forward_batch, ABI 11) over
    the calls of one camera set: per camera the binning buffer's capacity
    (the last call's exact list instances x (1 + margin) + slack) and the
    previous plan's sort extents (gs_batch_hint).  The first call has no
    capacity: it runs with capacity 0, which never fits, and takes the retry
    with the exact lengths -- one forward in the two-phase path's cost.
    `calls`, `retries` (attempts that did not fit after the first call) and
    `num_instances` (exact, last call) are for the caller to inspect;
    `force_capacity` (tests) replaces the computed capacities once."""

    def __init__(self, margin: float = 0.125, slack: int = 4096):
        self.margin, self.slack = float(margin), int(slack)
        self.capacity = None
        self.hint = [0, 0, 0, 0, 0, 0]  # gs_batch_hint {valid, p1, q1, p2, max_len, total}
        self.num_instances = None
        self.calls = 0
        self.retries = 0
        self.force_capacity = None

    def next_capacity(self, C):
        if self.force_capacity is not None:
            cap, self.force_capacity = [int(x) for x in self.force_capacity], None
            return cap
        if self.capacity is None or len(self.capacity) != C:
            return [0] * C
        return list(self.capacity)

    def update(self, num_instances, hint, fitted, first):
        self.calls += 1
        if not fitted and not first:
            self.retries += 1
        self.num_instances = [int(x) for x in num_instances]
        self.capacity = [int(n * (1.0 + self.margin)) + self.slack for n in self.num_instances]
        self.hint = [int(x) for x in hint]


def batch_backward_scratch(means3D, semantic_feature, C: int):
    """An uninitialised scratch tensor of the batch backward's size
    (gs_batch_backward_scratch_bytes at the compiled feature width), for a
    caller that has the forward zero it (rasterize_gaussians_batch zero_fill)
    and hands it to the backward."""
    L_ = _lib.load()
    P = means3D.size(0)
    Fu = semantic_feature.numel() // max(P, 1) if _present(semantic_feature) else 0
    n = L_.gs_batch_backward_scratch_bytes(P, _feature_width(Fu), int(C))
    return torch.empty(max(16, n), dtype=torch.uint8, device=means3D.device)


def rasterize_gaussians_batch(background, means3D, colors, semantic_feature, opacity, scales, rotations,
                              scale_modifier, cov3D_precomp, viewmatrices, projmatrices, c_x, c_y, tan_fovx,
                              tan_fovy, image_height, image_width, sh, degree, campos, prefiltered, debug,
                              *, compat=None, activate=False, windows=None, feature_ready=None, plan_state=None,
                              walk_order=None, zero_fill=None, cam_frames=None):
    """The forward of C cameras at once (gs_forward_plan_batch +
    gs_forward_render_batch): the arguments of rasterize_gaussians with
    per-camera matrices stacked ([C,4,4] or [C,16], campos [C,3]) and the
    camera scalars as length-C sequences.  Returns (num_rendered[C],
    color[C,3,H,W], feature_map[C,F,H,W], depth[C,1,H,W], alpha[C,1,H,W],
    radii[C,P] int32, geomBuffer, binningBuffer, imgBuffer, num_instances[C]);
    camera c's outputs equal rasterize_gaussians' for that camera.
    `activate`: opacity / scales / rotations are the raw parameters
    (logit, log, unnormalised; GS_FLAG_ACTIVATE).  `windows`: per camera a
    tile window (x0, y0, x1, y1) or None (gs_camera tile_*).  `feature_ready`:
    a torch.cuda.Event (recorded) the blend waits for before reading the
    features (gs_gaussians.feature_ready), or None.  `plan_state`: a
    BinningPlan -- the sync-free forward (gs_forward_batch): no host round
    trip between the plan and the render stages, the binning buffer sized
    from the previous call and re-rendered with the exact lengths when it
    does not fit (bit-identical outputs either way).  The returned
    num_instances is then the per-camera length the binning buffer is laid
    out with (what the backward takes); the exact counts are in
    plan_state.num_instances.  `walk_order`: an int32 device tensor of the P
    ids in the order the binning passes walk them (spatial_order), or None
    (gs_gaussians.walk_order; outputs do not depend on it).  `zero_fill`: a
    device tensor the blend zeroes (its whole bytes, rounded down to 16) --
    the backward's scratch, handed to rasterize_gaussians_batch_backward
    with scratch_zeroed=True (gs_gaussians.zero_fill, ABI 13).  `cam_frames`:
    a temporal window (include/gs_window.h) -- C non-decreasing frame indices;
    means3D is then (P, B, 3) Gaussian-major and camera c renders
    means3D[:, cam_frames[c]]; everything else is shared by the frames."""
    sync_free = plan_state is not None and not debug
    cm = _compat_code(compat)
    P, C = _num_points(means3D, cam_frames is not None), len(c_x)
    if P == 0:  # answered before any camera argument is looked at
        H, W = int(image_height), int(image_width)
        f32 = dict(dtype=torch.float32, device=means3D.device)
        u8 = dict(dtype=torch.uint8, device=means3D.device)
        return ([0] * C, torch.zeros(C, 3, H, W, **f32), torch.zeros(C, 0, H, W, **f32),
                torch.zeros(C, 1, H, W, **f32), torch.zeros(C, 1, H, W, **f32),
                torch.zeros(C, 0, dtype=torch.int32, device=means3D.device), torch.empty(0, **u8),
                torch.empty(0, **u8), torch.empty(0, **u8), [0] * C)
    if feature_ready is not None and _present(semantic_feature):
        sf = semantic_feature
        Fu = sf.numel() // P
        if not (sf.is_cuda and sf.dtype == torch.float32 and sf.is_contiguous() and _feature_width(Fu) == Fu):
            # the binding copies / pads the features on the calling stream
            # before any kernel runs: that copy has to wait too
            torch.cuda.current_stream(means3D.device).wait_event(feature_ready)
            feature_ready = None
    cap = plan_state.next_capacity(C) if sync_free else []
    try:
        out = _native_mod().forward_batch(
            background, means3D, _opt(colors), _opt(semantic_feature), _opt(opacity), _opt(scales), _opt(rotations),
            float(scale_modifier), _opt(cov3D_precomp), viewmatrices, projmatrices, [float(x) for x in c_x],
            [float(x) for x in c_y], [float(x) for x in tan_fovx], [float(x) for x in tan_fovy], int(image_height),
            int(image_width), _opt(sh), int(degree), campos, bool(prefiltered), bool(debug), cm, bool(activate),
            _windows_arg(windows), _event_handle(feature_ready), cap, plan_state.hint if sync_free else [],
            _opt(walk_order), _opt(zero_fill), _frames_arg(cam_frames), _lib.stream(means3D.device))
    except RuntimeError as ex:
        raise _lib.GsplatError(str(ex)) from None
    NR, color, fmap, depth, alpha, radii, geom, binning, img, NI, layout, hint, fitted = out
    if sync_free:
        plan_state.update(NI, hint, fitted, first=not any(cap))
        return (NR, color, fmap, depth, alpha, radii, geom, binning, img, layout)
    return (NR, color, fmap, depth, alpha, radii, geom, binning, img, NI)


def rasterize_gaussians_batch_backward(background, means3D, radii, colors, semantic_feature, scales,
                                       rotations, scale_modifier, cov3D_precomp, viewmatrices, projmatrices,
                                       c_x, c_y, tan_fovx, tan_fovy, dL_dout_color, dL_dout_feature,
                                       dL_dout_depth, dL_dout_alpha, sh, degree, campos, geomBuffer,
                                       num_instances, binningBuffer, imageBuffer, alphas, debug, *,
                                       compat=None, grad_mask=None, densify=None, opacity=None,
                                       activate=False, windows=None, out=None, scratch=None,
                                       scratch_zeroed=False, cam_frames=None):
    """The backward of a camera batch (gs_backward_batch): the arguments of
    rasterize_gaussians_backward with stacked per-camera matrices, scalars
    and upstream gradients ([C, ...]), in the binding's positional camera
    semantics.  Returns the rasterize_gaussians_backward tuple with every
    per-Gaussian gradient SUMMED over the cameras.  `densify` as in
    rasterize_gaussians_backward (per-camera statistics, summed).
    `activate` (with the raw `opacity`): the gradients of the raw opacity /
    scale / rotation parameters (GS_FLAG_ACTIVATE).  `out`: optional
    {name: tensor} destinations of backward_buffers' names (e.g. the views of
    a gradient bucket, distributed.ShardedAdam.grad_views): those gradients
    are WRITTEN there (every element, not accumulated) instead of into fresh
    tensors; each must be a contiguous fp32 device tensor of the gradient's
    element count (dsem at the compiled feature width).  `scratch`: the
    backward's scratch (gs_batch_backward_scratch_bytes) kept from the
    forward, `scratch_zeroed`: the forward's blend zeroed it
    (rasterize_gaussians_batch zero_fill; GS_FLAG_SCRATCH_ZEROED).
    `cam_frames`: the forward's temporal window; means3D is (P, B, 3) and so is
    dL_dmeans3D (and its `out` destination): frame b holds the sum over the
    cameras of frame b, zeros for a frame without cameras."""
    return _backward(background, means3D, radii, colors, semantic_feature, scales, rotations, scale_modifier,
                     cov3D_precomp, viewmatrices, projmatrices, c_x, c_y, tan_fovx, tan_fovy, dL_dout_color,
                     dL_dout_feature, dL_dout_depth, dL_dout_alpha, sh, degree, campos, geomBuffer, num_instances,
                     binningBuffer, imageBuffer, alphas, debug, compat=compat, grad_mask=grad_mask, densify=densify,
                     opacity=opacity, activate=activate, windows=windows, out=out, scratch=scratch,
                     scratch_zeroed=scratch_zeroed, cam_frames=cam_frames)


camera_grad_calls = 0  # camera-gradient launches so far (tests: none without a camera tensor that requires grad)


def rasterize_gaussians_batch_camera_grad(background, means3D, radii, cov3D_precomp, viewmatrices, projmatrices,
                                          c_x, c_y, tan_fovx, tan_fovy, image_height, image_width, sh, degree,
                                          campos, geomBuffer, scratch, *, compat=None, windows=None,
                                          cam_frames=None):
    """The gradients of a camera batch's matrices and positions
    (gs_camera_grad_batch, include/gs_camera_grad.h), to be called after
    rasterize_gaussians_batch_backward on the same stream with the same
    inputs and the `scratch` that call was given (its accumulation records
    are read).  Returns (dL_dviewmatrices [C,16], dL_dprojmatrices [C,16],
    dL_dcampos [C,3]): the exact derivative of the compat="fixed" forward;
    compat="reference" is refused.  The tan(fov/2) and principal-point
    scalars are not differentiated.  With tile `windows` the gradient is that
    of the windows' pixels."""
    global camera_grad_calls
    cm = _compat_code(compat)
    if cm != _lib.GS_COMPAT["fixed"]:
        raise ValueError('camera gradients need compat="fixed": the reference-mode backward is not the derivative '
                         'of its forward')
    C = len(c_x)
    if _num_points(means3D, cam_frames is not None) == 0:  # answered like the forward and the backward
        f32 = dict(dtype=torch.float32, device=means3D.device)
        return torch.zeros(C, 16, **f32), torch.zeros(C, 16, **f32), torch.zeros(C, 3, **f32)
    camera_grad_calls += 1
    try:
        return tuple(_native_mod().camera_grad_batch(
            background, means3D, radii, _opt(cov3D_precomp) if _present(cov3D_precomp) else None, viewmatrices,
            projmatrices, [float(x) for x in c_x], [float(x) for x in c_y], [float(x) for x in tan_fovx],
            [float(x) for x in tan_fovy], int(image_height), int(image_width), _opt(sh) if _present(sh) else None,
            int(degree), campos, geomBuffer, scratch, cm, _windows_arg(windows), _frames_arg(cam_frames),
            _lib.stream(means3D.device)))
    except RuntimeError as ex:
        raise _lib.GsplatError(str(ex)) from None


def rasterize_gaussians_batch_contributors(geomBuffer, binningBuffer, imgBuffer, num_instances, c_x, c_y, tan_fovx,
                                           tan_fovy, background, viewmatrices, projmatrices, campos, image_height,
                                           image_width, P, K, *, compat=None, windows=None):
    """The K largest blend weights of every pixel and the Gaussians they
    belong to (gs_contributors_batch, include/gs_track.h), to be called after
    rasterize_gaussians_batch on the same stream with its state buffers, its
    returned num_instances, its cameras and its tile `windows`.  Returns
    (top_id int32 [C,K,H,W], top_w fp32 [C,K,H,W]): rank k holds the Gaussian
    with the k-th largest w = alpha T among the entries the forward blended at
    the pixel (the nearer one first between equal weights), -1 / 0 past the
    number of blended entries and outside a camera's tile window.  K in 1..4.
    P = 0 (the forward's empty buffers) gives -1 / 0 everywhere."""
    cm = _compat_code(compat)
    try:
        return tuple(_native_mod().contributors_batch(
            geomBuffer, _opt(binningBuffer), imgBuffer, [int(x) for x in num_instances], background, viewmatrices,
            projmatrices, [float(x) for x in c_x], [float(x) for x in c_y], [float(x) for x in tan_fovx],
            [float(x) for x in tan_fovy], int(image_height), int(image_width), campos, int(P), int(K), cm,
            _windows_arg(windows), _lib.stream(viewmatrices.device)))
    except RuntimeError as ex:
        raise _lib.GsplatError(str(ex)) from None


def track_project(means3D, ids, background, viewmatrices, projmatrices, c_x, c_y, tan_fovx, tan_fovy, campos,
                  image_height, image_width):
    """gs_track_project (include/gs_track.h): the means means3D[t, ids[n]]
    ([T,P,3] fp32, ids [N] integer, device tensors) through each of the C
    cameras as the forward's preprocess projects them.  Returns (uv [T,C,N,2],
    depth [T,C,N], inside bool [T,C,N]); uv and depth equal the forward's
    means2D and depths bit for bit, inside = in front of the camera and the
    rounded pixel in the image; ids < 0 give zeros and inside = False."""
    if means3D.device.type != "cuda":
        raise _lib.GsplatError("the HIP track projection needs device tensors (means3D is on the CPU)")
    try:
        return tuple(_native_mod().track_project(
            means3D, ids, background, viewmatrices, projmatrices, [float(x) for x in c_x], [float(x) for x in c_y],
            [float(x) for x in tan_fovx], [float(x) for x in tan_fovy], int(image_height), int(image_width), campos,
            _lib.stream(means3D.device)))
    except RuntimeError as ex:
        raise _lib.GsplatError(str(ex)) from None


def _backward(background, means3D, radii, colors, semantic_feature, scales, rotations, scale_modifier,
              cov3D_precomp, viewmatrices, projmatrices, c_x, c_y, tan_fovx, tan_fovy, dL_dout_color,
              dL_dout_feature, dL_dout_depth, dL_dout_alpha, sh, degree, campos, geomBuffer, num_instances,
              binningBuffer, imageBuffer, alphas, debug, *, compat, grad_mask, densify, opacity=None,
              activate=False, windows=None, out=None, exact_out=False, accumulate=False, scratch=None,
              scratch_zeroed=False, cam_frames=None):
    """The one backward body, for C = len(c_x) cameras (gs_backward_batch; at
    C = 1 what the single-camera entry point runs).  `exact_out`: `out` holds every gradient
    name in its exact shape (else any subset, by element count);
    `accumulate`: the gradients are ADDED to `out` (GS_FLAG_ACCUMULATE)."""
    cm = _compat_code(compat)
    if activate and not _present(opacity):
        raise RuntimeError("activate=True needs the raw opacities")
    if accumulate and out is None:
        raise ValueError("accumulate=True needs the caller's gradient buffers (out=...)")
    if out is not None:
        odd = _BUFFER_NAMES - out.keys() if exact_out else out.keys() - _BUFFER_NAMES
        if odd:
            raise RuntimeError(f"out: {'missing' if exact_out else 'unknown'} gradient names {sorted(odd)}")
    if _num_points(means3D, cam_frames is not None) == 0:  # answered before any camera argument is looked at
        shapes = _buffer_shapes(0, 0, 0)
        if cam_frames is not None:
            shapes["dmeans3D"] = (0, means3D.size(1), 3)
        return tuple(torch.zeros(*shape, dtype=torch.float32, device=means3D.device) for shape in shapes.values())
    try:
        return tuple(_native_mod().backward_batch(
            background, means3D, radii, _opt(colors), _opt(semantic_feature), _opt(scales), _opt(rotations),
            float(scale_modifier), _opt(cov3D_precomp), viewmatrices, projmatrices, [float(x) for x in c_x],
            [float(x) for x in c_y], [float(x) for x in tan_fovx], [float(x) for x in tan_fovy],
            _opt(dL_dout_color), _opt(dL_dout_feature), _opt(dL_dout_depth), _opt(dL_dout_alpha), _opt(sh),
            int(degree), campos, geomBuffer, [int(x) for x in num_instances], _opt(binningBuffer), imageBuffer,
            alphas, bool(debug), cm, _opt(grad_mask), None if densify is None else list(densify),
            _opt(opacity), bool(activate), _windows_arg(windows),
            [out.get(k, _NO_DEST) for k in _BUFFER_ORDER] if out else [], bool(exact_out), bool(accumulate),
            _opt(scratch), bool(scratch_zeroed), _frames_arg(cam_frames), _lib.stream(means3D.device)))
    except RuntimeError as ex:
        raise _lib.GsplatError(str(ex)) from None
