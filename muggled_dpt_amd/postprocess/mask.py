"""The depth masking demo's display and cutouts (depth_mask_display / depth_mask_images: the reference's experiments/depth_masking.py, background
removal by depth). Both start from still.py's plane-removed chain. Kernels: csrc/post_mask.inc."""

from __future__ import annotations

import numpy as np
import torch
from torch import Tensor

from .. import native
from ._common import _batch_maps, _launch, _need_cuda, _photo_list, _prediction_list, _views, packed_offsets, prediction_count, upload
from .still import _plane_removed, _sample_table, _threshold, plane_sample_points


def depth_mask_display(prediction: Tensor, images_bgr: Tensor, target_wh: tuple[int, int] | None, plane_removal: float = 0.0, threshold=(0.0, 1.0),
                       invert: bool = False, samples_per_side: int = 16, sample_xy=None) -> tuple[Tensor, Tensor]:
    """[B,h,w] depth prediction and uint8 [B,ih,iw,3] BGR photos (or [ih,iw,3] for B = 1) on the device -> (mask uint8 [B,H,W], composite uint8 [B,H,W,3]) at the display
    size target_wh = (W, H) (None: the map's size), the display loop of the reference's depth masking demo (experiments/depth_masking.py:189-199, 314-332) for every
    image: n = normalize_01(d - plane_removal * plane) in fp64, d = normalize_01( remove_inf(scale_prediction(x))) as depth_to_display prepares it (its plane fit,
    sample_xy as there, at the display size); mask = 255 where threshold[0] <= n <= threshold[1], else 0 (NaN: 0); invert: 255 - mask. The composite is the photo resized
    to (W, H) where the mask is 255 and the reference's CheckerPattern() (169 / 214, 32-px tiles, centred) where it is 0. The photo resize restates
    cv2.resize(INTER_LINEAR) on uint8 by its scalar fixed-point formula (weights round(2048 w), (v + 2^21) >> 22); cv2's SIMD and IPP paths round differently, so a
    composite byte may differ from a given cv2 build's by 1. Mask and checker bytes do not depend on that. Four launches; nothing is read back."""
    _threshold(threshold)
    b = prediction_count(prediction) if isinstance(prediction, torch.Tensor) and prediction.dim() == 3 else 1
    what = "depth_mask_display"
    _need_cuda([images_bgr], what, "images_bgr must be a uint8 CUDA tensor")
    photos = images_bgr.detach()[None] if images_bgr.dim() == 3 else images_bgr.detach()
    if photos.dtype != torch.uint8 or photos.dim() != 4 or photos.shape[3] != 3 or photos.shape[1] == 0 or photos.shape[2] == 0:
        raise TypeError(f"{what}: images_bgr must be uint8 [B,H,W,3] or [H,W,3] BGR, got {photos.dtype} {tuple(images_bgr.shape)}")
    if photos.shape[0] != b:
        raise ValueError(f"{what}: {b} predictions but {photos.shape[0]} images")
    photos = photos.contiguous()
    x = _batch_maps(prediction, what)
    if photos.device != x.device:
        raise RuntimeError(f"depth_mask_display: the prediction is on {x.device} but the images are on {photos.device}")
    s = _plane_removed(x, target_wh, plane_removal, threshold, samples_per_side, sample_xy, False, what)
    dev = x.device
    mask = torch.empty((b, s.oh, s.ow), device=dev, dtype=torch.uint8)
    comp = torch.empty((b, s.oh, s.ow, 3), device=dev, dtype=torch.uint8)
    _launch(dev, "mdpt_post_mask_display", *s.args(), int(bool(invert)), photos.data_ptr(), photos.shape[1], photos.shape[2], mask.data_ptr(), comp.data_ptr())
    return mask, comp


def _size_group_batch(maps: list[Tensor]) -> Tensor:
    """contiguous [h,w] maps of one size -> [B,h,w]: a view when they lie back to back in ONE storage (rows of a [B,h,w] tensor, a chunk of inference_images), else a
    stacked copy. Separate allocations may sit back to back in memory, but a view across them would reach past the first one's storage."""
    first = maps[0]
    h, w = first.shape
    base = first.untyped_storage().data_ptr()
    step = h * w * first.element_size()
    if all(m.untyped_storage().data_ptr() == base and m.data_ptr() == first.data_ptr() + j * step for j, m in enumerate(maps)):
        return first.as_strided((len(maps), h, w), (h * w, w, 1))
    return torch.stack(maps)


def depth_mask_images(predictions, images_bgr, plane_removal: float = 0.0, threshold=(0.0, 1.0), invert: bool = False, samples_per_side: int = 16,
                      sample_xy=None) -> list[tuple[Tensor, Tensor]]:
    """Depth maps and the photos they came from -> one (cutout uint8 [ih,iw,4] BGRA, mask uint8 [ih,iw]) per photo, in order, at each photo's own size: the save path of
    the reference's depth masking demo (experiments/depth_masking.py:341-361). For every map: p = normalize_01(remove_inf(x)) at model resolution (as depth_for_saving
    prepares it), n = normalize_01(p - plane_removal * plane) in fp64 with its own plane fit, s = cv2.resize(n, (iw, ih)) (INTER_LINEAR on CV_64F, restated: fp32 weights,
    fp64 sums), mask = 255 where threshold[0] <= s <= threshold[1] (NaN: 0), 255 - mask with invert, cutout = (BGR AND mask, alpha = mask). predictions: a [B,h,w] tensor
    or a list of [1,h,w] / [h,w] maps whose sizes may differ (DPTModel.inference_images returns one). images_bgr: a list of uint8 HxWx3 BGR host arrays (staged through
    pinned memory) or CUDA tensors (read in place). sample_xy: None (plane_sample_points per map, in list order) or one [N,2] int point set per map. Maps of one size
    share one prep / fit / min-max chain; the cutouts are one launch per 32 photos; nothing is read back or synchronised. Element k equals the call on map k and photo k
    alone, bit for bit. The cutouts are views into one allocation, the masks into another."""
    tmin, tmax = _threshold(threshold)
    what = "depth_mask_images"
    n = prediction_count(predictions)
    photos, on_device = _photo_list(images_bgr, n, what) if n >= 0 else (None, False)
    maps = _prediction_list(predictions, what)
    dev = maps[0].device
    if on_device and photos[0].device != dev:
        raise RuntimeError(f"{what}: the predictions are on {dev} but the images are on {photos[0].device}")
    sets = [None] * len(maps)  # (per-map [N,2] point sets; None: drawn below, per map in list order)
    if sample_xy is not None:
        sets = list(sample_xy.unbind(0)) if isinstance(sample_xy, torch.Tensor) else list(sample_xy if isinstance(sample_xy, (list, tuple)) else np.asarray(sample_xy))
        if len(sets) != len(maps):
            raise ValueError(f"{what}: {len(maps)} predictions but {len(sets)} sample point sets")
    # groups of equal map size (first-appearance order); the sample points of each, checked and drawn before anything is launched
    groups: dict[tuple[int, int], list[int]] = {}
    for k, m in enumerate(maps):
        groups.setdefault(tuple(m.shape), []).append(k)
    drawn = [plane_sample_points(m.shape, samples_per_side) if s is None else s for m, s in zip(maps, sets)]
    tables = {}
    for (h, w), idx in groups.items():
        pts = [drawn[k] for k in idx]
        if len({tuple(p.shape) for p in pts}) != 1:
            raise ValueError(f"{what}: the sample point sets of the {h}x{w} maps differ in shape: {[tuple(p.shape) for p in pts]}")
        stacked = torch.stack([torch.as_tensor(p) for p in pts]) if any(isinstance(p, torch.Tensor) for p in pts) else np.stack([np.asarray(p) for p in pts])
        if isinstance(stacked, torch.Tensor) and stacked.device.type == "cuda" and any(not isinstance(p, torch.Tensor) or p.device.type != "cuda" for p in pts):
            raise TypeError(f"{what}: sample_xy mixes host and device point sets")
        tables[(h, w)] = _sample_table(stacked, len(idx), h, w, samples_per_side, 0.75, dev, what)[0]
    # the map side: one chain per size group
    order, stats = [], []
    for (h, w), idx in groups.items():
        x = _size_group_batch([maps[k] for k in idx])
        s = _plane_removed(x, None, plane_removal, threshold, samples_per_side, tables[(h, w)], False, what)
        for j, k in enumerate(idx):
            order.append(k)
            stats.append((s.x.data_ptr() + j * h * w * s.x.element_size(), s.parts[j].data_ptr(), s.coef[j].data_ptr(), s.vparts[j].data_ptr(), s))
    # outputs: photo k at a 16-pixel aligned offset of one allocation
    hws = [tuple(int(v) for v in f.shape[0:2]) for f in photos]
    offs, at = packed_offsets([ih * iw for ih, iw in hws], 16)
    bgra = torch.empty(at * 4, device=dev, dtype=torch.uint8)
    mask = torch.empty(at, device=dev, dtype=torch.uint8)
    staged, img_ptrs = (None, [f.data_ptr() for f in photos]) if on_device else upload(photos, dev, 16)
    arr = lambda v, t: np.ascontiguousarray(np.asarray(v, dtype=t))  # noqa: E731
    map_ptrs, parts, coef, vparts = (arr(column, np.uint64) for column in list(zip(*stats))[:4])
    map_hw = arr([maps[k].shape for k in order], np.int32).reshape(-1)
    img_arr = arr([img_ptrs[k] for k in order], np.uint64)
    img_hw = arr([hws[k] for k in order], np.int32).reshape(-1)
    off_arr = arr([offs[k] for k in order], np.int64)
    _launch(dev, "mdpt_post_mask_cutout_images", map_ptrs.ctypes.data, map_hw.ctypes.data, native.dtype_code(maps[0].dtype), parts.ctypes.data,
            coef.ctypes.data, vparts.ctypes.data, float(plane_removal), img_arr.ctypes.data, img_hw.ctypes.data, off_arr.ctypes.data, len(order), tmin, tmax,
            int(bool(invert)), bgra.data_ptr(), mask.data_ptr())
    del staged  # (the caching allocator reuses it in stream order only)
    return [(b[0], m[0]) for b, m in zip(_views(bgra, hws, (4,), 16), _views(mask, hws, (), 16))]
