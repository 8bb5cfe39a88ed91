"""The refusals the operator front ends share (dynamic3dgaussians_amd/_args.py): every public
entry point of the nine modules, driven through each of them on the CPU, must raise the type and
the full text recorded in EXPECTED before the modules shared one implementation."""
import importlib

import pytest
import torch

from dynamic3dgaussians_amd import (_lib, depth_geometry, depth_loss, feature_decoder, image_loss, metrics,
                                    resample, robust_loss, scene_loss)

densify = importlib.import_module("dynamic3dgaussians_amd.densify")  # the package exports the function under this name


class _DeviceClaim(torch.Tensor):
    """A host tensor that reports is_cuda, so the wrappers' dtype / layout / shape rules (all
    checked before any device work) can be exercised where there is no GPU."""

    @staticmethod
    def __new__(cls, t):
        return torch.Tensor._make_subclass(cls, t, t.requires_grad)

    @property
    def is_cuda(self):
        return True


D = _DeviceClaim


def _im():
    return torch.rand(2, 3, 9, 7)


def _im_t():  # an image that is not contiguous
    return torch.rand(2, 3, 7, 9).transpose(2, 3)


def _tab(cols=3):
    return torch.rand(8, cols)


def _tab_t(cols=3):  # a table that is not contiguous
    return torch.rand(cols, 8).t()


def _planes():
    return torch.rand(2, 9, 7)


def _planes_t():
    return torch.rand(2, 7, 9).transpose(1, 2)


def _eye(n):
    return torch.eye(n)[None].repeat(2, 1, 1)


def _scene(**replace):
    """(params, variables) of 8 Gaussians for densify, every tensor claiming the device."""
    params = {"means3D": _tab(), "rgb_colors": _tab(), "unnorm_rotations": _tab(4), "logit_opacities": _tab(1),
              "log_scales": _tab()}
    variables = {"means2D_gradient_accum": torch.rand(8), "denom": torch.rand(8), "max_2D_radius": torch.rand(8)}
    for k, v in replace.items():
        (variables if k in variables else params)[k] = v
    params = {k: v if k in replace else D(v) for k, v in params.items()}
    variables = {k: v if k in replace else D(v) for k, v in variables.items()}
    variables["scene_radius"] = 1.0
    return params, variables


def _densify(**replace):
    params, variables = _scene(**replace)
    return densify.densify(params, variables, None, 500, accumulate=False)


def _accumulate(**replace):
    params, variables = _scene(**replace)
    variables["seen"] = torch.ones(8, dtype=torch.bool)
    variables["means2D"] = torch.zeros(8, 3, requires_grad=True)
    variables["means2D"].grad = torch.rand(8, 3)
    return densify.densify(params, variables, None, 1, accumulate=True)


def _plan(**replace):
    a = {"grad_accum": D(torch.rand(8)), "denom": D(torch.rand(8)), "log_scales": D(_tab()),
         "logit_opacities": D(_tab(1))}
    a.update(replace)
    return densify.plan(a["grad_accum"], a["denom"], a["log_scales"], a["logit_opacities"], grad_thresh=2e-4,
                        clone_max_scale=0.02, prune_min_opacity=0.005)


_IS_FG = torch.tensor([True, False] * 4)


def _split(slot_dtype=torch.int32, claim=True):
    s = scene_loss.foreground_split(_IS_FG)
    slot = s.slot.to(slot_dtype)
    return scene_loss.ForegroundSplit(D(slot) if claim else slot, s.n_fg, s.n_bg, _IS_FG)


def _regularizers(means=None, split=None, **replace):
    v = {"init_bg_pts": D(torch.rand(4, 3)), "init_bg_rot": D(torch.rand(4, 4)), "prev_col": D(_tab())}
    v.update(replace)
    return scene_loss.regularizer_losses(D(_tab()) if means is None else means, D(_tab(4)), D(_tab()), v,
                                         split or _split())


def _decode(x=None, w=None, b=None):
    return feature_decoder.decode_features(D(_im()) if x is None else x, D(torch.rand(4, 3)) if w is None else w,
                                           D(torch.rand(4)) if b is None else b)


def _decoded_l1(x=None, target=None, twin=False, **kw):
    f = feature_decoder.decoded_l1_loss_torch if twin else feature_decoder.decoded_l1_loss
    return f(D(_im()) if x is None else x, D(torch.rand(4, 3)), D(torch.rand(4)),
             D(torch.rand(2, 4, 9, 7)) if target is None else target, **kw)


def _tracks(tracks=None, depths=None):
    return depth_geometry.lift_tracks(D(torch.rand(2, 5, 2)) if tracks is None else tracks,
                                      D(_planes()) if depths is None else depths, D(_eye(3)), D(_eye(4)))


PL, DC, MT = image_loss.photometric_loss, depth_loss.depth_correlation_loss, robust_loss.masked_trimmed_mse_loss
IM, G = metrics.image_metrics, depth_geometry

CASES = {
    # ---- image_loss
    "photometric_loss/cpu": lambda: PL(_im(), _im()),
    "photometric_loss/not_a_tensor": lambda: PL(D(_im()), [1.0]),
    "photometric_loss/dtype": lambda: PL(D(_im().double()), D(_im().double())),
    "photometric_loss/half": lambda: PL(D(_im().half()), D(_im().half())),
    "photometric_loss/contiguous": lambda: PL(D(_im_t()), D(_im())),
    "photometric_loss/shape": lambda: PL(D(_im()), D(torch.rand(2, 3, 9, 8))),
    "photometric_loss/gain_shape": lambda: PL(D(_im()), D(_im()), gain=D(torch.rand(2, 4)), offset=D(torch.rand(2, 4))),
    "photometric_loss/gain_cpu": lambda: PL(D(_im()), D(_im()), gain=torch.rand(2, 3)),
    "photometric_loss/mask_shape": lambda: PL(D(_im()), D(_im()), mask=D(torch.ones(7, 9))),
    "photometric_loss/mask_batch_shape": lambda: PL(D(_im()), D(_im()), mask=D(torch.ones(3, 9, 7))),
    "photometric_loss/mask_host": lambda: PL(D(_im()), D(_im()), mask=torch.ones(9, 7)),
    "photometric_loss/mask_not_a_tensor": lambda: PL(D(_im()), D(_im()), mask=[[1.0]]),
    "photometric_loss/reduction": lambda: PL(D(_im()), D(_im()), reduction="mean"),
    "photometric_image_loss/cpu": lambda: image_loss.photometric_image_loss(_im(), _im()),
    "photometric_image_loss/dtype": lambda: image_loss.photometric_image_loss(D(_im()), D(_im().double())),
    "photometric_image_loss/mask_host": lambda: image_loss.photometric_image_loss(D(_im()), D(_im()), mask=torch.ones(9, 7)),
    "photometric_loss_torch/reduction": lambda: image_loss.photometric_loss_torch(_im(), _im(), reduction="mean"),
    # ---- depth_loss
    "depth_correlation_loss/cpu": lambda: DC(torch.rand(2, 1, 9, 7), torch.rand(2, 1, 9, 7)),
    "depth_correlation_loss/target_cpu": lambda: DC(D(torch.rand(2, 1, 9, 7)), torch.rand(2, 1, 9, 7)),
    "depth_correlation_loss/dtype": lambda: DC(D(_planes().half()), D(_planes().half())),
    "depth_correlation_loss/contiguous": lambda: DC(D(_planes_t()), D(_planes())),
    "depth_correlation_loss/shape": lambda: DC(D(torch.rand(2, 1, 9, 7)), D(_planes())),
    "depth_correlation_loss/mask_shape": lambda: DC(D(_planes()), D(_planes()), mask=D(torch.ones(7, 9))),
    "depth_correlation_loss/mask_host": lambda: DC(D(_planes()), D(_planes()), mask=torch.ones(9, 7)),
    "depth_correlation_loss/reduction": lambda: DC(D(_planes()), D(_planes()), reduction="mean"),
    "depth_correlation_loss_torch/reduction": lambda: depth_loss.depth_correlation_loss_torch(_planes(), _planes(),
                                                                                             reduction=None),
    # ---- robust_loss
    "plane_quantile/cpu": lambda: robust_loss.plane_quantile(torch.rand(2, 63), 0.5),
    "plane_quantile/dtype": lambda: robust_loss.plane_quantile(D(torch.rand(2, 63).double()), 0.5),
    "plane_quantile/contiguous": lambda: robust_loss.plane_quantile(D(torch.rand(63, 2).t()), 0.5),
    "masked_trimmed_mse_loss/cpu": lambda: MT(_im(), _im()),
    "masked_trimmed_mse_loss/dtype": lambda: MT(D(_im()), D(_im().half())),
    "masked_trimmed_mse_loss/contiguous": lambda: MT(D(_im()), D(_im_t())),
    "masked_trimmed_mse_loss/shape": lambda: MT(D(_im()), D(torch.rand(2, 3, 9, 8))),
    "masked_trimmed_mse_loss/mask_shape": lambda: MT(D(_im()), D(_im()), mask=D(torch.ones(2, 7, 9))),
    "masked_trimmed_mse_loss/mask_host": lambda: MT(D(_im()), D(_im()), mask=torch.ones(2, 9, 7, dtype=torch.uint8)),
    "masked_trimmed_mse_loss/reduction": lambda: MT(D(_im()), D(_im()), reduction="mean"),
    "masked_trimmed_mse_loss_torch/reduction": lambda: robust_loss.masked_trimmed_mse_loss_torch(_im(), _im(),
                                                                                                 reduction="mean"),
    "trimmed_mse_loss/cpu": lambda: robust_loss.trimmed_mse_loss(_tab(), _tab()),
    "trimmed_mse_loss/dtype": lambda: robust_loss.trimmed_mse_loss(D(_tab().double()), D(_tab())),
    "trimmed_mse_loss/contiguous": lambda: robust_loss.trimmed_mse_loss(D(_tab_t()), D(_tab())),
    "trimmed_mse_loss/shape": lambda: robust_loss.trimmed_mse_loss(D(_tab()), D(_tab(4))),
    # ---- metrics
    "image_metrics/cpu": lambda: IM(_im(), _im()),
    "image_metrics/dtype": lambda: IM(D(_im().double()), D(_im().double())),
    "image_metrics/contiguous": lambda: IM(D(_im_t()), D(_im())),
    "image_metrics/shape": lambda: IM(D(_im()), D(torch.rand(2, 3, 9, 8))),
    "image_metrics/mask_shape": lambda: IM(D(_im()), D(_im()), D(torch.ones(7, 9)), ssim=False),
    "image_metrics/mask_host": lambda: IM(D(_im()), D(_im()), torch.ones(9, 7), ssim=False),
    "image_metrics_torch/mask_shape": lambda: metrics.image_metrics_torch(_im(), _im(), torch.ones(7, 9), ssim=False),
    "image_metrics_torch/mask_not_a_tensor": lambda: metrics.image_metrics_torch(_im(), _im(), [[1.0]], ssim=False),
    "mask_iou/cpu": lambda: metrics.mask_iou(_planes(), _planes()),
    "mask_iou/dtype": lambda: metrics.mask_iou(D(_planes() > 0.5), D(_planes() > 0.5)),
    "mask_iou/contiguous": lambda: metrics.mask_iou(D(_planes_t()), D(_planes())),
    "mask_iou/shape": lambda: metrics.mask_iou(D(_planes()), D(torch.rand(2, 9, 8))),
    # ---- depth_geometry
    "point_depth_maps/cpu": lambda: G.point_depth_maps(_tab(), D(_eye(4)), D(_eye(3)), (9, 7)),
    "point_depth_maps/dtype": lambda: G.point_depth_maps(D(_tab().double()), D(_eye(4)), D(_eye(3)), (9, 7)),
    "point_depth_maps/contiguous": lambda: G.point_depth_maps(D(_tab_t()), D(_eye(4)), D(_eye(3)), (9, 7)),
    "point_depth_maps/camera_cpu": lambda: G.point_depth_maps(D(_tab()), _eye(4), D(_eye(3)), (9, 7)),
    "depth_abs_rel/cpu": lambda: G.depth_abs_rel(_planes(), _planes()),
    "depth_abs_rel/dtype": lambda: G.depth_abs_rel(D(_planes()), D(_planes().double())),
    "depth_abs_rel/contiguous": lambda: G.depth_abs_rel(D(_planes_t()), D(_planes())),
    "depth_abs_rel/shape": lambda: G.depth_abs_rel(D(_planes()), D(torch.rand(2, 9, 8))),
    "depth_abs_rel_sums/cpu": lambda: G.depth_abs_rel_sums(_planes(), _planes()),
    "unproject_depth/cpu": lambda: G.unproject_depth(_planes(), D(_eye(3)), D(_eye(4))),
    "unproject_depth/dtype": lambda: G.unproject_depth(D(_planes().half()), D(_eye(3)), D(_eye(4))),
    "unproject_depth/contiguous": lambda: G.unproject_depth(D(_planes_t()), D(_eye(3)), D(_eye(4))),
    "depth_flow/cpu": lambda: G.depth_flow(_planes(), D(_eye(3)), D(_eye(4)), D(_eye(3)), D(_eye(4))),
    "depth_flow/dtype": lambda: G.depth_flow(D(_planes().double()), D(_eye(3)), D(_eye(4)), D(_eye(3)), D(_eye(4))),
    "sample_bilinear/cpu": lambda: G.sample_bilinear(_im(), D(torch.rand(2, 5, 2))),
    "sample_bilinear/dtype": lambda: G.sample_bilinear(D(_im().double()), D(torch.rand(2, 5, 2))),
    "sample_bilinear/contiguous": lambda: G.sample_bilinear(D(_im_t()), D(torch.rand(2, 5, 2))),
    "sample_bilinear/xy_cpu": lambda: G.sample_bilinear(D(_im()), torch.rand(2, 5, 2)),
    "sample_bilinear/xy_dtype": lambda: G.sample_bilinear(D(_im()), D(torch.rand(2, 5, 2).double())),
    "warp_flow/cpu": lambda: G.warp_flow(_im(), D(torch.rand(2, 2, 9, 7))),
    "warp_flow/displacement_dtype": lambda: G.warp_flow(D(_im()), D(torch.rand(2, 2, 9, 7).half())),
    "accumulate_flows/cpu": lambda: G.accumulate_flows([D(_planes()), _planes()]),
    "accumulate_flows/dtype": lambda: G.accumulate_flows([D(_planes().double())]),
    "accumulate_flows/contiguous": lambda: G.accumulate_flows([D(_planes_t())]),
    "resize_flow/cpu": lambda: G.resize_flow(_planes(), (4, 5)),
    "lift_tracks/cpu": lambda: _tracks(depths=_planes()),
    "lift_tracks/tracks_cpu": lambda: _tracks(tracks=torch.rand(2, 5, 2)),
    "lift_tracks/dtype": lambda: _tracks(depths=D(_planes().double())),
    "lift_tracks/tracks_contiguous": lambda: _tracks(tracks=D(torch.rand(2, 2, 5).transpose(1, 2))),
    # ---- densify
    "densify/cpu": lambda: _densify(means3D=_tab()),
    "densify/not_a_tensor": lambda: _densify(rgb_colors=[1.0]),
    "densify/dtype": lambda: _densify(rgb_colors=D(_tab().double())),
    "densify/contiguous": lambda: _densify(means3D=D(_tab_t())),
    "densify/rows": lambda: _densify(rgb_colors=D(torch.rand(7, 3))),
    "densify/stat_dtype": lambda: _densify(denom=D(torch.rand(8).half())),
    "densify/stat_rows": lambda: _densify(means2D_gradient_accum=D(torch.rand(7))),
    "densify/accumulate_cpu": lambda: _accumulate(denom=torch.rand(8)),
    "densify/accumulate_rows": lambda: _accumulate(means2D_gradient_accum=D(torch.rand(9))),
    "densify/accumulate_grad_cpu": lambda: _accumulate(),
    "plan/cpu": lambda: _plan(grad_accum=torch.rand(8)),
    "plan/dtype": lambda: _plan(log_scales=D(_tab().double())),
    "plan/contiguous": lambda: _plan(log_scales=D(_tab_t())),
    # ---- scene_loss
    "gather_foreground/cpu": lambda: scene_loss.gather_foreground(_tab(), _tab(4), _split()),
    "gather_foreground/dtype": lambda: scene_loss.gather_foreground(D(_tab()), D(_tab(4).double()), _split()),
    "gather_foreground/shape": lambda: scene_loss.gather_foreground(D(_tab()), D(_tab(3)), _split()),
    "gather_foreground/contiguous": lambda: scene_loss.gather_foreground(D(_tab_t()), D(_tab(4)), _split()),
    "gather_foreground/shape_before_contiguity": lambda: scene_loss.gather_foreground(D(_tab()), D(_tab_t(3)), _split()),
    "gather_foreground/slot_dtype": lambda: scene_loss.gather_foreground(D(_tab()), D(_tab(4)), _split(torch.int64)),
    "gather_foreground/slot_cpu": lambda: scene_loss.gather_foreground(D(_tab()), D(_tab(4)), _split(claim=False)),
    "regularizer_losses/cpu": lambda: _regularizers(means=_tab()),
    "regularizer_losses/not_a_tensor": lambda: _regularizers(means=[1.0]),
    "regularizer_losses/dtype": lambda: _regularizers(means=D(_tab().half())),
    "regularizer_losses/table_cpu": lambda: _regularizers(prev_col=_tab()),
    "regularizer_losses/table_shape": lambda: _regularizers(init_bg_pts=D(torch.rand(3, 3))),
    "regularizer_losses/table_contiguous": lambda: _regularizers(init_bg_rot=D(torch.rand(4, 4).t())),
    # ---- resample
    "bilinear_resize/cpu": lambda: resample.bilinear_resize(_im(), (4, 5)),
    "bilinear_resize/dtype": lambda: resample.bilinear_resize(D(_im().half()), (4, 5)),
    "bilinear_resize/contiguous": lambda: resample.bilinear_resize(D(_im_t()), (4, 5)),
    # ---- feature_decoder
    "decode_features/cpu": lambda: _decode(x=_im()),
    "decode_features/weight_cpu": lambda: _decode(w=torch.rand(4, 3)),
    "decode_features/dtype": lambda: _decode(x=D(_im().double())),
    "decode_features/weight_contiguous": lambda: _decode(w=D(torch.rand(3, 4).t())),
    "decode_features/bias_dtype": lambda: _decode(b=D(torch.rand(4).half())),
    "decoded_l1_loss/cpu": lambda: _decoded_l1(x=_im()),
    "decoded_l1_loss/target_dtype": lambda: _decoded_l1(target=D(torch.rand(2, 4, 9, 7).double())),
    "decoded_l1_loss/target_contiguous": lambda: _decoded_l1(target=D(torch.rand(2, 4, 7, 9).transpose(2, 3))),
    "decoded_l1_loss/mask_shape": lambda: _decoded_l1(mask=D(torch.ones(7, 9))),
    "decoded_l1_loss/mask_host": lambda: _decoded_l1(mask=torch.ones(9, 7)),
    "decoded_l1_loss/mask_dtype": lambda: _decoded_l1(mask=D(torch.ones(9, 7, dtype=torch.uint8))),
    "decoded_l1_loss/reduction": lambda: _decoded_l1(reduction="mean"),
    "decoded_l1_loss_torch/reduction": lambda: _decoded_l1(twin=True, reduction="mean"),
}

E, V = _lib.GsplatError, ValueError
_GEOM = "the HIP depth geometry needs device tensors ({} is on the CPU); the _torch twins run anywhere"
_DECODER = ("the HIP feature decoder needs device tensors ({} is on the CPU); "
            "decode_features_torch / decoded_l1_loss_torch run anywhere")
_DENSIFY = "the HIP densification needs device tensors ({} is on the CPU); densify_torch runs anywhere"
_DEPTH = ("the HIP depth-correlation loss needs device tensors ({} is on the CPU); "
          "depth_correlation_loss_torch runs anywhere")
_SCENE = "the HIP scene losses need device tensors ({} is on the CPU); regularizer_losses_torch runs anywhere"
_METRICS = "the HIP metrics need device tensors ({} is on the CPU); image_metrics_torch / mask_iou_torch run anywhere"
_ROBUST = "the HIP robust losses need device tensors ({} is on the CPU); the _torch twins run anywhere"
_PHOTO = "the HIP photometric loss needs device tensors ({} is on the CPU); photometric_loss_torch runs anywhere"
_RESAMPLE = "the HIP resample needs device tensors (x is on the CPU); bilinear_resize_torch runs anywhere"
_REDUCTION = "reduction must be 'sum' or 'none' (got 'mean')"
_MASK = "mask must have shape (9, 7) or (2, 9, 7) (got {})"
# recorded from the commit before _args.py existed, with this file's CASES
EXPECTED = {
    "accumulate_flows/contiguous": (E, "flows[0] must be contiguous"),
    "accumulate_flows/cpu": (E, _GEOM.format("flows[1]")),
    "accumulate_flows/dtype": (E, "flows[0] must be float32 (got torch.float64)"),
    "bilinear_resize/contiguous": (E, "x must be contiguous"),
    "bilinear_resize/cpu": (E, _RESAMPLE),
    "bilinear_resize/dtype": (E, "x must be float32 (got torch.float16)"),
    "decode_features/bias_dtype": (E, "bias must be float32 (got torch.float16)"),
    "decode_features/cpu": (E, _DECODER.format("x")),
    "decode_features/dtype": (E, "x must be float32 (got torch.float64)"),
    "decode_features/weight_contiguous": (E, "weight must be contiguous"),
    "decode_features/weight_cpu": (E, _DECODER.format("weight")),
    "decoded_l1_loss/cpu": (E, _DECODER.format("x")),
    "decoded_l1_loss/mask_dtype": (E, "mask must be float32 (got torch.uint8)"),
    "decoded_l1_loss/mask_host": (E, _DECODER.format("mask")),
    "decoded_l1_loss/mask_shape": (E, "mask must be [h, w] or [B, h, w] (got (7, 9))"),
    "decoded_l1_loss/reduction": (E, _REDUCTION),
    "decoded_l1_loss/target_contiguous": (E, "target must be contiguous"),
    "decoded_l1_loss/target_dtype": (E, "target must be float32 (got torch.float64)"),
    "decoded_l1_loss_torch/reduction": (E, _REDUCTION),
    "densify/accumulate_cpu": (E, _DENSIFY.format("variables['denom']")),
    "densify/accumulate_grad_cpu": (E, _DENSIFY.format("means2D.grad")),
    "densify/accumulate_rows": (E, "variables['means2D_gradient_accum'] must have 8 rows (got shape (9,))"),
    "densify/contiguous": (E, "params['means3D'] must be contiguous"),
    "densify/cpu": (E, _DENSIFY.format("params['means3D']")),
    "densify/dtype": (E, "params['rgb_colors'] must be float32 (got torch.float64)"),
    "densify/not_a_tensor": (E, "params['rgb_colors'] must be a tensor"),
    "densify/rows": (E, "params['rgb_colors'] must have 8 rows (got shape (7, 3))"),
    "densify/stat_dtype": (E, "variables['denom'] must be float32 (got torch.float16)"),
    "densify/stat_rows": (E, "variables['means2D_gradient_accum'] must have 8 rows (got shape (7,))"),
    "depth_abs_rel/contiguous": (E, "est must be contiguous"),
    "depth_abs_rel/cpu": (E, _GEOM.format("est")),
    "depth_abs_rel/dtype": (E, "gt must be float32 (got torch.float64)"),
    "depth_abs_rel/shape": (E, "gt must have shape (2, 9, 7) (got (2, 9, 8))"),
    "depth_abs_rel_sums/cpu": (E, _GEOM.format("est")),
    "depth_correlation_loss/contiguous": (E, "depth must be contiguous"),
    "depth_correlation_loss/cpu": (E, _DEPTH.format("depth")),
    "depth_correlation_loss/dtype": (E, "depth must be float32 (got torch.float16)"),
    "depth_correlation_loss/mask_host": (E, "mask must be a device tensor"),
    "depth_correlation_loss/mask_shape": (E, _MASK.format("(7, 9)")),
    "depth_correlation_loss/reduction": (V, _REDUCTION),
    "depth_correlation_loss/shape": (E, "target must have shape (2, 1, 9, 7) (got (2, 9, 7))"),
    "depth_correlation_loss/target_cpu": (E, _DEPTH.format("target")),
    "depth_correlation_loss_torch/reduction": (V, "reduction must be 'sum' or 'none' (got None)"),
    "depth_flow/cpu": (E, _GEOM.format("depth")),
    "depth_flow/dtype": (E, "depth must be float32 (got torch.float64)"),
    "gather_foreground/contiguous": (E, "means3D must be contiguous"),
    "gather_foreground/cpu": (E, _SCENE.format("means3D")),
    "gather_foreground/dtype": (E, "rotations must be torch.float32 (got torch.float64)"),
    "gather_foreground/shape": (E, "rotations must have shape (8, 4) (got (8, 3))"),
    "gather_foreground/shape_before_contiguity": (E, "rotations must have shape (8, 4) (got (8, 3))"),
    "gather_foreground/slot_cpu": (E, _SCENE.format("split.slot")),
    "gather_foreground/slot_dtype": (E, "split.slot must be torch.int32 (got torch.int64)"),
    "image_metrics/contiguous": (E, "pred must be contiguous"),
    "image_metrics/cpu": (E, _METRICS.format("pred")),
    "image_metrics/dtype": (E, "pred must be float32 (got torch.float64)"),
    "image_metrics/mask_host": (E, "mask must be a device tensor"),
    "image_metrics/mask_shape": (E, _MASK.format("(7, 9)")),
    "image_metrics/shape": (E, "target must have shape (2, 3, 9, 7) (got (2, 3, 9, 8))"),
    "image_metrics_torch/mask_not_a_tensor": (E, "mask must be a device tensor"),
    "image_metrics_torch/mask_shape": (E, _MASK.format("(7, 9)")),
    "lift_tracks/cpu": (E, _GEOM.format("depths")),
    "lift_tracks/dtype": (E, "depths must be float32 (got torch.float64)"),
    "lift_tracks/tracks_contiguous": (E, "tracks_xy must be contiguous"),
    "lift_tracks/tracks_cpu": (E, _GEOM.format("tracks_xy")),
    "mask_iou/contiguous": (E, "pred_mask must be contiguous"),
    "mask_iou/cpu": (E, _METRICS.format("pred_mask")),
    "mask_iou/dtype": (E, "pred_mask must be float32 (got torch.bool)"),
    "mask_iou/shape": (E, "target_mask must have shape (2, 9, 7) (got (2, 9, 8))"),
    "masked_trimmed_mse_loss/contiguous": (E, "gt must be contiguous"),
    "masked_trimmed_mse_loss/cpu": (E, _ROBUST.format("pred")),
    "masked_trimmed_mse_loss/dtype": (E, "gt must be float32 (got torch.float16)"),
    "masked_trimmed_mse_loss/mask_host": (E, "mask must be a device tensor"),
    "masked_trimmed_mse_loss/mask_shape": (E, _MASK.format("(2, 7, 9)")),
    "masked_trimmed_mse_loss/reduction": (V, _REDUCTION),
    "masked_trimmed_mse_loss/shape": (E, "gt must have shape (2, 3, 9, 7) (got (2, 3, 9, 8))"),
    "masked_trimmed_mse_loss_torch/reduction": (V, _REDUCTION),
    "photometric_image_loss/cpu": (E, _PHOTO.format("image")),
    "photometric_image_loss/dtype": (E, "target must be float32 (got torch.float64)"),
    "photometric_image_loss/mask_host": (E, "mask must be a device tensor"),
    "photometric_loss/contiguous": (E, "image must be contiguous"),
    "photometric_loss/cpu": (E, _PHOTO.format("image")),
    "photometric_loss/dtype": (E, "image must be float32 (got torch.float64)"),
    "photometric_loss/gain_cpu": (E, _PHOTO.format("gain")),
    "photometric_loss/gain_shape": (E, "gain must have shape (2, 3) (got (2, 4))"),
    "photometric_loss/half": (E, "image must be float32 (got torch.float16)"),
    "photometric_loss/mask_batch_shape": (E, _MASK.format("(3, 9, 7)")),
    "photometric_loss/mask_host": (E, "mask must be a device tensor"),
    "photometric_loss/mask_not_a_tensor": (E, "mask must be a device tensor"),
    "photometric_loss/mask_shape": (E, _MASK.format("(7, 9)")),
    "photometric_loss/not_a_tensor": (E, "target must be a tensor"),
    "photometric_loss/reduction": (V, _REDUCTION),
    "photometric_loss/shape": (E, "target must have shape (2, 3, 9, 7) (got (2, 3, 9, 8))"),
    "photometric_loss_torch/reduction": (V, _REDUCTION),
    "plan/contiguous": (E, "log_scales must be contiguous"),
    "plan/cpu": (E, _DENSIFY.format("grad_accum")),
    "plan/dtype": (E, "log_scales must be float32 (got torch.float64)"),
    "plane_quantile/contiguous": (E, "x must be contiguous"),
    "plane_quantile/cpu": (E, _ROBUST.format("x")),
    "plane_quantile/dtype": (E, "x must be float32 (got torch.float64)"),
    "point_depth_maps/camera_cpu": (E, "the HIP depth geometry needs device tensors (w2c is on the CPU)"),
    "point_depth_maps/contiguous": (E, "points must be contiguous"),
    "point_depth_maps/cpu": (E, _GEOM.format("points")),
    "point_depth_maps/dtype": (E, "points must be float32 (got torch.float64)"),
    "regularizer_losses/cpu": (E, _SCENE.format("means3D")),
    "regularizer_losses/dtype": (E, "means3D must be torch.float32 (got torch.float16)"),
    "regularizer_losses/not_a_tensor": (E, "means3D must be a tensor"),
    "regularizer_losses/table_contiguous": (E, "init_bg_rot must be contiguous"),
    "regularizer_losses/table_cpu": (E, _SCENE.format("prev_col")),
    "regularizer_losses/table_shape": (E, "init_bg_pts must have shape (4, 3) (got (3, 3))"),
    "resize_flow/cpu": (E, _RESAMPLE),
    "sample_bilinear/contiguous": (E, "src must be contiguous"),
    "sample_bilinear/cpu": (E, _GEOM.format("src")),
    "sample_bilinear/dtype": (E, "src must be float32 (got torch.float64)"),
    "sample_bilinear/xy_cpu": (E, _GEOM.format("xy")),
    "sample_bilinear/xy_dtype": (E, "xy must be float32 (got torch.float64)"),
    "trimmed_mse_loss/contiguous": (E, "pred must be contiguous"),
    "trimmed_mse_loss/cpu": (E, _ROBUST.format("pred")),
    "trimmed_mse_loss/dtype": (E, "pred must be float32 (got torch.float64)"),
    "trimmed_mse_loss/shape": (E, "gt must have shape (8, 3) (got (8, 4))"),
    "unproject_depth/contiguous": (E, "depth must be contiguous"),
    "unproject_depth/cpu": (E, _GEOM.format("depth")),
    "unproject_depth/dtype": (E, "depth must be float32 (got torch.float16)"),
    "warp_flow/cpu": (E, _GEOM.format("flow")),
    "warp_flow/displacement_dtype": (E, "displacement must be float32 (got torch.float16)"),
}


def refusal(case):
    """(exception type, full text) of what CASES[case] raises."""
    try:
        CASES[case]()
    except Exception as e:  # noqa: BLE001 -- the type is what is compared
        return type(e), str(e)
    return None, "nothing was raised"


def test_every_case_has_its_recorded_refusal():
    assert sorted(CASES) == sorted(EXPECTED)


@pytest.mark.parametrize("case", sorted(CASES))
def test_refusal_is_unchanged(case):
    assert refusal(case) == EXPECTED[case]
