"""Synthetic depth of field (not in the reference): a photo refocused by its depth map, "portrait mode". A focal plane is put where the caller says -
a value, or a point of the photo - every photo pixel gets a blur radius from its signed defocus, and the blur, which varies per pixel, is
occlusion-aware: a sharp foreground is not smeared by the blurred background behind it, a blurred foreground spreads over what is behind it.
refocus_images makes the whole call, defocus_planes the preparation alone; DPTModel.inference_refocus starts from the photos.
Kernels: csrc/post_refocus.inc (mdpt_post_refocus); the arithmetic is written out in include/mdpt.h.

Known limits: what a blurred foreground edge uncovers is not inpainted (the gather can only average what the photo shows); the disc is hard-edged, with
no bokeh shapes and no highlight boost; the average is taken on the gamma-encoded bytes, not in linear light. Output quality on real photographs is
unverified - no checkpoint can be loaded where this was written; the tests hold the arithmetic and synthetic scenes only."""

from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import native
from .postprocess._common import (REFOCUS_RECORD, _launch, _photo_list, _photo_pointers, _prediction_list, _upload_records, _views, packed_offsets,
                                  prediction_count, ptr, record_table, scratch_bytes)

__all__ = ["REFOCUS_SPACES", "REFOCUS_APERTURE", "refocus_images", "defocus_planes"]

REFOCUS_SPACES = {"inverse": native.REFOCUS_INVERSE, "depth": native.REFOCUS_DEPTH}
REFOCUS_APERTURE = 32.0  # photo pixels of blur radius per unit of defocus: half the map's range away from the focal plane reaches the default max_radius
# (REFOCUS_RECORD, mdpt_refocus_pair of include/mdpt.h, stands with the other record tables in postprocess/_common.py; csrc/mdpt_post_photo.cpp
# static_asserts the layout)


def _refocus_checked(predictions, images_bgr, focus, focus_xy, aperture, max_radius, focus_range, space, what: str):
    """everything the refocus calls can refuse from shapes and values alone, before any tensor has to be on the device -> the checked scalars"""
    if space not in REFOCUS_SPACES:
        raise ValueError(f"{what}: space must be one of {sorted(REFOCUS_SPACES)}, got {space!r}")
    if isinstance(max_radius, bool) or not isinstance(max_radius, (int, np.integer)) or not 0 <= int(max_radius) <= native.REFOCUS_MAX_RADIUS:
        raise ValueError(f"{what}: max_radius must be an int in 0 .. {native.REFOCUS_MAX_RADIUS} (photo pixels), got {max_radius!r}")
    aperture, focus_range = float(aperture), float(focus_range)
    if not 0.0 <= aperture < float("inf"):
        raise ValueError(f"{what}: aperture must be finite and >= 0 (photo pixels per unit of defocus), got {aperture}")
    if not 0.0 <= focus_range < float("inf"):
        raise ValueError(f"{what}: focus_range must be finite and >= 0, got {focus_range}")
    if focus_xy is not None:
        if len(focus_xy) != 2 or not all(0.0 <= float(v) <= 1.0 for v in focus_xy):
            raise ValueError(f"{what}: focus_xy must be (x, y) in [0, 1]^2, got {focus_xy!r}")
        focus_xy = (float(focus_xy[0]), float(focus_xy[1]))
        focus = 0.5  # (replaced on the device by the value under focus_xy)
    else:
        focus = float(focus)
        if space == "inverse" and not 0.0 <= focus <= 1.0:
            raise ValueError(f"{what}: focus must be in [0, 1] of the map's range in inverse space, got {focus}")
        if space == "depth" and not 0.0 < focus < float("inf"):
            raise ValueError(f"{what}: focus must be a finite depth > 0 in depth space, got {focus}")
    n = prediction_count(predictions)
    if n >= 0 and isinstance(images_bgr, (list, tuple)):
        if len(images_bgr) != n:
            raise ValueError(f"{what}: {n} predictions but {len(images_bgr)} images")
        for k, f in enumerate(images_bgr):
            if isinstance(f, (np.ndarray, torch.Tensor)) and (f.dtype != (torch.uint8 if isinstance(f, torch.Tensor) else np.uint8) or f.ndim != 3 or f.shape[2] != 3):
                raise ValueError(f"{what}: image {k} is not a uint8 HxWx3 BGR photo (shape {tuple(f.shape)}, dtype {f.dtype})")
    return focus, focus_xy, aperture, int(max_radius), focus_range


def _run(predictions, images_bgr, checked, space, what: str, gather: bool, planes: bool):
    focus, focus_xy, aperture, max_radius, focus_range = checked
    n = prediction_count(predictions)
    photos, on_device = _photo_list(images_bgr, n, what) if n >= 0 else (None, False)
    maps = _prediction_list(predictions, what)
    dev = maps[0].device
    keep, img_ptrs, pitches = _photo_pointers(images_bgr, photos, on_device, dev, what)
    hws = [(int(f.shape[0]), int(f.shape[1])) for f in photos]
    if any(h * w >= 2 ** 31 for h, w in hws):
        raise ValueError(f"{what}: a photo of 2^31 pixels or more is not supported")
    records = record_table(REFOCUS_RECORD, maps, photo=img_ptrs, pitch=pitches, H=[h for h, _ in hws], W=[w for _, w in hws])
    tile = native.REFOCUS_TILE
    records["tile_off"], _ = packed_offsets([((h + tile - 1) // tile) * ((w + tile - 1) // tile) for h, w in hws])
    # (a pair's scratch region is what the call asks for its record alone; the regions lie end to end)
    records["scratch_off"], at = packed_offsets([scratch_bytes("mdpt_post_refocus_scratch_bytes", records[k:k + 1].ctypes.data, 1, max_radius)
                                                 for k in range(len(maps))])
    offs, total = packed_offsets([h * w for h, w in hws])
    out = rq = e32 = None
    if gather:
        out = torch.empty(3 * total, device=dev, dtype=torch.uint8)
        records["out"] = [out.data_ptr() + 3 * o for o in offs]
    if planes:
        rq, e32 = torch.empty(total, device=dev, dtype=torch.uint8), torch.empty(total, device=dev, dtype=torch.float32)
    scratch = torch.empty(at // 8, device=dev, dtype=torch.float64)
    table = _upload_records(records, dev)
    xy = None if focus_xy is None else (ctypes.c_double * 2)(*focus_xy)
    _launch(dev, "mdpt_post_refocus", records.ctypes.data, table.data_ptr(), len(maps), native.dtype_code(maps[0].dtype), REFOCUS_SPACES[space], focus, xy,
            aperture, focus_range, max_radius, scratch.data_ptr(), at, ptr(rq), ptr(e32))
    del table, keep, scratch  # (the caching allocator reuses them in stream order only)
    images = [v[0] for v in _views(out, hws, (3,))] if gather else None
    both = [(r[0], e[0]) for r, e in zip(_views(rq, hws), _views(e32, hws))] if planes else None
    return images, both


def refocus_images(predictions, images_bgr, focus: float = 0.5, focus_xy=None, aperture: float = REFOCUS_APERTURE, max_radius: int = 16,
                   focus_range: float = 0.0, space: str = "inverse", return_radius: bool = False):
    """Depth maps and the photos they came from -> one refocused uint8 [H_i,W_i,3] BGR photo per pair, in order, on the device (views into one allocation): everything
    at the focal plane stays sharp, the rest is blurred by a disc whose radius grows with its distance from that plane, and the blur respects the depth order.
    space="inverse" (relative models; the map is affine in 1 / depth): e = (s - lo) / (hi - lo) - focus with s the map at the photo pixel's centre (bilinear), lo / hi
    the min / max of the map's finite values and focus in [0, 1] (1 = the nearest the map holds); space="depth" (metric maps): e = 1 / s - 1 / focus, focus a depth > 0
    in map units, a finite s <= 0 infinitely far. A thin lens's circle of confusion is linear in |1 / z - 1 / z_f|: both are that shape. focus_xy = (x, y) in [0, 1]^2
    focuses by pointing: the focus is the value under photo pixel (min(H - 1, floor(y H)), min(W - 1, floor(x W))), read on the device. Radius:
    r = min(max_radius, aperture max(0, |e| - focus_range / 2)) photo pixels, in quarter pixels; aperture = pixels per unit of e, focus_range = the width in e of the
    band that stays sharp, max_radius an int in 0 .. 32. Blur: for output pixel p, every pixel q within reach spreads its colour over its own lattice disc with weight 1 /
    (points of the disc); q reaches p with its own disc if it is nearer than p (e(q) > e(p)), else only with the smaller of the two discs (what is behind never bleeds
    over something sharper in front of it); the result is the weighted mean, rounded once. A pixel without a finite depth, a flat map and a pointed pixel without a
    usable depth mean "in focus": that photo comes back byte for byte. The defaults (focus 0.5, aperture 32, max_radius 16, focus_range 0) are user-facing choices,
    not measured optima. predictions / images_bgr as guided_upsample_images takes them - a [B,h,w] tensor or a list of [1,h,w] / [h,w] CUDA maps of one dtype whose
    sizes may differ; one uint8 HxWx3 BGR photo per map, of any size relative to it: host arrays (staged through pinned memory) or CUDA tensors read in place, a sliced
    view through its row pitch. fp64 arithmetic, bit-deterministic, every pair independent of the others, four launches for the whole call, nothing read back, no
    synchronisation. return_radius: -> (photos, [(rq uint8 [H_i,W_i] = floor(4 r), e32 fp32 [H_i,W_i]) per pair]). Limits: see this module's docstring."""
    what = "refocus_images"
    checked = _refocus_checked(predictions, images_bgr, focus, focus_xy, aperture, max_radius, focus_range, space, what)
    images, planes = _run(predictions, images_bgr, checked, space, what, True, bool(return_radius))
    return (images, planes) if return_radius else images


def defocus_planes(predictions, images_bgr, focus: float = 0.5, focus_xy=None, aperture: float = REFOCUS_APERTURE, max_radius: int = 16,
                   focus_range: float = 0.0, space: str = "inverse"):
    """The preparation of refocus_images alone, for inspection: -> [(rq uint8 [H_i,W_i], e32 fp32 [H_i,W_i]) per pair], the blur radius in quarter photo pixels and the
    signed defocus (positive: nearer than the focal plane) of every photo pixel. Arguments as refocus_images; three launches, no gather."""
    what = "defocus_planes"
    checked = _refocus_checked(predictions, images_bgr, focus, focus_xy, aperture, max_radius, focus_range, space, what)
    return _run(predictions, images_bgr, checked, space, what, False, True)[1]
