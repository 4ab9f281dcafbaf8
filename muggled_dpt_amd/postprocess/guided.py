"""The enlargement of a map to its photo's size with the photo as the guide (guided_upsample_images: the fast guided filter; not in the
reference, every demo of which resizes its map bilinearly; DPTModel.inference_guided makes the whole call). Kernels: csrc/post_guided.inc."""

from __future__ import annotations

import numpy as np
import torch

from .. import native
from ._common import (GUIDED_RECORD, _launch, _photo_list, _prediction_list, _upload_records, _views, packed_offsets, prediction_count, ptr, record_table,
                      scratch_bytes, upload)


def _guided_checked(predictions, images_bgr, radius, eps, what: str) -> tuple[int, float]:
    """everything guided_upsample_images can refuse from shapes and values alone, before any tensor has to be on the device"""
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 0 <= int(radius) <= native.GUIDED_MAX_RADIUS:
        raise ValueError(f"{what}: radius must be an int in 0 .. {native.GUIDED_MAX_RADIUS} (cells of the map), got {radius!r}")
    eps = float(eps)
    if not 0.0 < eps < float("inf"):
        raise ValueError(f"{what}: eps must be finite and > 0, got {eps}")
    shapes = None
    if isinstance(predictions, torch.Tensor) and predictions.dim() == 3:
        shapes = [tuple(predictions.shape[1:])] * predictions.shape[0]
    elif isinstance(predictions, (list, tuple)):
        shapes = [tuple(p.shape[-2:]) if isinstance(p, torch.Tensor) and p.dim() in (2, 3) else None for p in predictions]
    if shapes is None or not isinstance(images_bgr, (list, tuple)):
        return int(radius), eps  # (_prediction_list / _photo_list name what is wrong)
    if len(images_bgr) != len(shapes):
        raise ValueError(f"{what}: {len(shapes)} predictions but {len(images_bgr)} images")
    for k, (f, hw) in enumerate(zip(images_bgr, shapes)):
        if not isinstance(f, (np.ndarray, torch.Tensor)):
            continue
        if f.dtype != (torch.uint8 if isinstance(f, torch.Tensor) else np.uint8) or f.ndim != 3 or f.shape[2] != 3:
            raise ValueError(f"{what}: image {k} is not a uint8 HxWx3 BGR photo (shape {tuple(f.shape)}, dtype {f.dtype}): the guide is the BGR photo itself")
        if hw is not None and (f.shape[0] < hw[0] or f.shape[1] < hw[1]):
            raise ValueError(f"{what}: photo {k} of {f.shape[0]}x{f.shape[1]} is smaller than its {hw[0]}x{hw[1]} map: guided upsampling only enlarges "
                             "(to shrink a map use scale_prediction / scale_prediction_images)")
    return int(radius), eps


def guided_upsample_images(predictions, images_bgr, radius: int = 8, eps: float = 1e-4, return_coefficients: bool = False):
    """Depth maps and the photos they came from -> one fp32 [1,H_i,W_i] map per photo, in order, at each photo's own size, with the photo as the guide of the enlargement
    (not in the reference, whose demos resize bilinearly; He & Sun's fast guided filter): where scale_prediction_images turns a depth edge into a ramp several photo
    pixels wide, the result follows the photo's own edges. The photo averaged over the cell of each map pixel (pixel (Y, X) belongs to cell (Y h // H, X w // W)) is the
    guide g at map resolution; per cell, over the window of the cells within `radius` in both axes (clipped to the map, mean = sum / its own count): Sigma = mean(g g^T) -
    mean(g) mean(g)^T + eps I, a = Sigma^-1 (mean(g p) - mean(g) mean(p)), b = mean(p) - a . mean(g); (a, b) are window-averaged once more, resampled bilinearly at every
    photo pixel's centre, and q = a_B B / 255 + a_G G / 255 + a_R R / 255 + b. eps is the variance (of a 0 .. 1 guide) below which the photo's texture is ignored; radius
    0 gives the bilinear resize, a flat photo the window mean of the map. predictions: a [B,h,w] tensor or a list of [1,h,w] / [h,w] CUDA maps of one dtype whose sizes
    may differ (DPTModel.inference_images returns one). images_bgr: one uint8 HxWx3 BGR photo per map, none smaller than its map: host arrays (staged through pinned
    memory) or CUDA tensors read in place - a sliced view photo[y1:y2, x1:x2] is read through its row pitch, no copy. fp64 arithmetic rounded to fp32 once;
    bit-deterministic; every pair independent of the others; six launches for the whole call, nothing read back, no synchronisation. The outputs are views into one
    allocation. return_coefficients: -> (maps, [fp64 [h_i,w_i,4] mean coefficients (a_B, a_G, a_R, b) per pair])."""
    what = "guided_upsample_images"
    radius, eps = _guided_checked(predictions, images_bgr, radius, eps, what)
    n = prediction_count(predictions)
    checked, on_device = _photo_list(images_bgr, n, what) if n >= 0 else (None, False)
    maps = _prediction_list(predictions, what)
    dev = maps[0].device
    keep = None
    if on_device:
        if checked[0].device != dev:
            raise RuntimeError(f"{what}: the predictions are on {dev} but the images are on {checked[0].device}")
        # a view whose pixels are packed and whose rows are at least a row apart is read in place through its pitch; anything else as its packed copy
        in_place = [f.stride(2) == 1 and f.stride(1) == 3 and f.stride(0) >= 3 * f.shape[1] for f in images_bgr]
        keep = [f.detach() if ok else c for f, c, ok in zip(images_bgr, checked, in_place)]
        img_ptrs, pitches = [f.data_ptr() for f in keep], [int(f.stride(0)) for f in keep]
    else:
        keep, img_ptrs = upload(checked, dev, 16)
        pitches = [3 * f.shape[1] for f in checked]
    hws = [(int(f.shape[0]), int(f.shape[1])) for f in checked]
    if any(h * w >= 2 ** 31 for h, w in hws):
        raise ValueError(f"{what}: a photo of 2^31 pixels or more is not supported")
    records = record_table(GUIDED_RECORD, maps, photo=img_ptrs, pitch=pitches, H=[h for h, _ in hws], W=[w for _, w in hws])
    # (a pair's scratch region is what the call asks for its record alone; the regions lie end to end)
    records["scratch_off"], at = packed_offsets([scratch_bytes("mdpt_post_guided_scratch_bytes", records[k:k + 1].ctypes.data, 1) for k in range(len(maps))])
    offs, total = packed_offsets([h * w for h, w in hws])
    out = torch.empty(total, device=dev, dtype=torch.float32)
    records["out"] = [out.data_ptr() + 4 * o for o in offs]
    scratch = torch.empty(at // 8, device=dev, dtype=torch.float64)
    coeffs = torch.empty(4 * int(sum(m.numel() for m in maps)), device=dev, dtype=torch.float64) if return_coefficients else None
    table = _upload_records(records, dev)
    _launch(dev, "mdpt_post_guided_upsample", records.ctypes.data, table.data_ptr(), len(maps), native.dtype_code(maps[0].dtype), radius, eps,
            scratch.data_ptr(), at, ptr(coeffs))
    del table, keep, scratch  # (the caching allocator reuses them in stream order only)
    result = _views(out, hws)
    if not return_coefficients:
        return result
    return result, [c[0] for c in _views(coeffs, [tuple(m.shape) for m in maps], (4,))]
