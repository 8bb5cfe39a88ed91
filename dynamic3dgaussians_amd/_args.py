"""The argument checks the operator front ends share: what a HIP kernel cannot take raises
here, in one wording.  Private; each operator module binds `need` to its own sentence."""
from __future__ import annotations

import torch

from ._lib import GsplatError


def need(t, name: str, shape=None, *, op: str, twin: str, dtype=torch.float32, rows=None,
         shape_first: bool = False) -> torch.Tensor:
    """t if a kernel can take it: a contiguous device tensor of `dtype` and, where given, of
    `shape` or with `rows` rows.  `op` ("photometric loss needs") and `twin`
    ("photometric_loss_torch runs") fill the sentence about host tensors; a wrong dtype reads
    "{name} must be float32 (got torch.float64)".  shape_first is scene_loss's form: the shape is
    checked before contiguity and the dtype is spelt as torch prints it ("must be torch.float32")."""
    if not isinstance(t, torch.Tensor):
        raise GsplatError(f"{name} must be a tensor")
    if not t.is_cuda:
        raise GsplatError(f"the HIP {op} device tensors ({name} is on the CPU); {twin} anywhere")
    if t.dtype != dtype:
        raise GsplatError(f"{name} must be {dtype if shape_first else str(dtype).split('.')[-1]} (got {t.dtype})")
    bad_shape = None
    if shape is not None and tuple(t.shape) != tuple(shape):
        bad_shape = GsplatError(f"{name} must have shape {tuple(shape)} (got {tuple(t.shape)})")
    if bad_shape and shape_first:
        raise bad_shape
    if not t.is_contiguous():
        raise GsplatError(f"{name} must be contiguous")
    if bad_shape:
        raise bad_shape
    if rows is not None and (t.dim() < 1 or t.shape[0] != rows):
        raise GsplatError(f"{name} must have {rows} rows (got shape {tuple(t.shape)})")
    return t


def check_mask(mask, B: int, H: int, W: int, need_device: bool = True) -> None:
    """A mask is a tensor [H, W] (one for all) or [B, H, W] (one per camera)."""
    if not isinstance(mask, torch.Tensor) or (need_device and not mask.is_cuda):
        raise GsplatError("mask must be a device tensor")
    if tuple(mask.shape) not in ((H, W), (B, H, W)):
        raise GsplatError(f"mask must have shape {(H, W)} or {(B, H, W)} (got {tuple(mask.shape)})")


def mask_u8(mask, B: int, H: int, W: int):
    """The mask as the kernels' bytes: uint8 passes through, anything else becomes != 0."""
    if mask is None:
        return None
    check_mask(mask, B, H, W)
    if mask.dtype != torch.uint8:
        mask = (mask != 0).to(torch.uint8)
    return mask.detach().contiguous()


def mask_f32(mask, B: int, H: int, W: int):
    """The mask as the kernels' float weights."""
    if mask is None:
        return None
    check_mask(mask, B, H, W)
    return mask.detach().to(torch.float32).contiguous()


def check_reduction(reduction: str, error=ValueError) -> None:
    if reduction not in ("sum", "none"):
        raise error(f"reduction must be 'sum' or 'none' (got {reduction!r})")


def reduce_losses(losses: torch.Tensor, reduction: str, single: bool) -> torch.Tensor:
    """The sum over the cameras, or the vector [B] (a scalar for a single image)."""
    return losses.sum() if reduction == "sum" else (losses[0] if single else losses)


def ptr(t, empty_is_null: bool = False):
    """The tensor's address for a C struct: NULL for None and, where asked, for an empty tensor."""
    if t is None or (empty_is_null and not t.numel()):
        return None
    return t.data_ptr()
