"""Depth segmentation (not in the reference): which pixels belong to the same surface as this one? Connected-component labelling of a depth map over the
criterion the mesh export cuts faces by and the normals stop differences at - a depth discontinuity between neighbouring nodes. segment_depth gives the label
maps and a table of the regions (area, box, depth range, mean depth), region_cutouts "the region under this point" as a mask and a BGRA cutout at the photo's
size, label_colors a picture of the labels; DPTModel.inference_segments starts from the photos. A picked region's mask can serve as a cutout, as the object of
refocus_images' focus_xy or as the alpha of pack_depth_u24_frames. Kernels: csrc/post_segment.inc (mdpt_segment_*); the definition is written out in
include/mdpt.h and restated in numpy in tests/segment_restate.py.

Known limits: a surface seen at a grazing angle has large steps between neighbouring pixels and breaks into slivers; a gentle ramp such as the ground connects
whatever stands on it to the background (the reference README's turtle, which threshold masking cannot separate from the ground, is reduced to this but not
removed; plane removal before the segmentation is not done here); regions below min_area are dropped, not merged into a neighbour. Output quality on real
photographs is unverified - no checkpoint can be loaded where this was written; the tests hold the definition and synthetic scenes only."""

from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np
import torch
from torch import Tensor

from . import native
from .postprocess._common import (SEGMENT_PHOTO_RECORD, SEGMENT_RECORD, _launch, _photo_list, _photo_pointers, _prediction_list, _upload_records, packed_offsets,
                                  record_table, scratch_bytes, upload)

__all__ = ["SEGMENT_SPACES", "SEGMENT_STEP", "DepthSegments", "segment_depth", "region_cutouts", "label_colors"]

SEGMENT_SPACES = {"inverse": native.ALIGN_INVERSE, "depth": native.ALIGN_DEPTH}
SEGMENT_STEP = 0.02  # a link spans at most 2 % of the map's range (inverse space) or of the nearer depth (depth space): a user-facing choice, not a measured optimum


@dataclass
class DepthSegments:
    """What segment_depth returns, all on the device. labels: one int32 [h_i,w_i] map per image (views into one allocation), a node's region or -1. counts: int32 [B],
    the regions K_i of every image. The region tables are slabs: image i owns rows region_offsets[i] .. + capacities[i] (R_i = min(h w, h w // min_area), an exact
    bound) of which the first K_i are filled: area int32, bbox int32 [.,4] = x0, y0, x1, y1 inclusive, first int32 (the lowest linear index y w + x of the region),
    vmin / vmax fp32, sum_q int64. lo / hi: fp64 [B], the min / max of every image's valid nodes. Nothing here has been read back; region_views() does, once."""
    labels: list
    counts: Tensor
    area: Tensor
    bbox: Tensor
    first: Tensor
    vmin: Tensor
    vmax: Tensor
    sum_q: Tensor
    lo: Tensor
    hi: Tensor
    region_offsets: list
    capacities: list
    min_area: int
    _records: np.ndarray = field(repr=False, default=None)
    _keep: tuple = field(repr=False, default=())

    def region_views(self) -> list[dict]:
        """One dict per image of the K_i filled rows of every column (views) and mean fp64 [K_i] = lo + (hi - lo) sum_q / (area 2^24), derived on the device.
        Reads counts back once (the one synchronisation of this module), as mesh_views does."""
        counts = self.counts.tolist()
        views = []
        for i, (k, o) in enumerate(zip(counts, self.region_offsets)):
            rows = {name: getattr(self, name)[o:o + k] for name in ("area", "bbox", "first", "vmin", "vmax", "sum_q")}
            rows["mean"] = self.lo[i] + (self.hi[i] - self.lo[i]) * rows["sum_q"].to(torch.float64) / (rows["area"].to(torch.float64) * float(2 ** 24))
            rows["count"] = k
            views.append(rows)
        return views


def _segment_checked(space, step, connectivity, min_area, what: str):
    """what the scalars alone can refuse -> (step, connectivity, min_area)"""
    if space not in SEGMENT_SPACES:
        raise ValueError(f"{what}: space must be one of {sorted(SEGMENT_SPACES)}, got {space!r}")
    step = float(step)
    if not 0.0 <= step < float("inf"):
        raise ValueError(f"{what}: step must be finite and >= 0, got {step}")
    if isinstance(connectivity, bool) or connectivity not in (4, 8):
        raise ValueError(f"{what}: connectivity must be 4 or 8, got {connectivity!r}")
    if isinstance(min_area, bool) or not isinstance(min_area, (int, np.integer)) or int(min_area) < 1 or int(min_area) >= 2 ** 31:
        raise ValueError(f"{what}: min_area must be an int >= 1 (1 keeps every component), got {min_area!r}")
    return step, int(connectivity), int(min_area)


def segment_depth(predictions, *, space: str = "inverse", step: float = SEGMENT_STEP, connectivity: int = 4, min_area: int = 16) -> DepthSegments:
    """Depth maps -> their depth-connected surfaces (DepthSegments), at each map's own resolution, on the device. A node is valid iff its value v (as fp32) is finite
    and, in space="depth", v > 0; lo / hi are the min / max of an image's valid nodes. Two valid neighbours are linked iff, in fp64 on the exact fp32 values,
    |v_p - v_q| <= step (hi - lo) (space="inverse": relative models) or <= step min(v_p, v_q) (space="depth": metric maps); connectivity 4, or 8 with the diagonals
    under the same test. A component is a connected set of valid nodes; those of fewer than min_area nodes are dropped (their nodes get -1, as invalid nodes do; 1
    keeps all) and the rest are numbered 0 .. K - 1 in the order of their lowest linear index. The default step (0.02) is a user-facing choice,
    not a measured optimum. predictions as refocus_images takes them - a [B,h,w] tensor or a list of [1,h,w] / [h,w] CUDA maps of one dtype (fp32 / bf16 / fp16) whose sizes
    may differ; every map is independent of the others and equals its own call bit for bit. Ten launches whatever B is: a union-find per 32 x 32 tile in LDS, a
    lock-free merge across tile edges with integer atomics, an order-preserving compaction; every output is an integer or an fp32 value that was moved, not
    computed: bit-deterministic. Nothing is read back, no synchronisation. Limits: see this module's docstring."""
    what = "segment_depth"
    step, connectivity, min_area = _segment_checked(space, step, connectivity, min_area, what)
    maps = _prediction_list(predictions, what)
    if len(maps) > 65535:
        raise ValueError(f"{what}: {len(maps)} maps, a call takes 1 .. 65535")
    dev = maps[0].device
    hws = [(int(m.shape[0]), int(m.shape[1])) for m in maps]
    if any(h * w >= 2 ** 31 for h, w in hws):
        raise ValueError(f"{what}: a map of 2^31 nodes or more is not supported")
    caps = [min(h * w, h * w // min_area) for h, w in hws]
    region_offs, rows = packed_offsets(caps)
    pixel_offs, total = packed_offsets([h * w for h, w in hws])
    tile = native.SEGMENT_TILE
    tile_offs, _ = packed_offsets([((h + tile - 1) // tile) * ((w + tile - 1) // tile) for h, w in hws])
    labels = torch.empty(total, device=dev, dtype=torch.int32)
    records = record_table(SEGMENT_RECORD, maps, labels=[labels.data_ptr() + 4 * o for o in pixel_offs], region_off=region_offs, tile_off=tile_offs,
                           pixel_off=pixel_offs)
    records["scratch_off"], at = packed_offsets([scratch_bytes("mdpt_segment_scratch_bytes", records[k:k + 1].ctypes.data, 1) for k in range(len(maps))])
    rows = max(rows, 1)
    counts = torch.empty(len(maps), device=dev, dtype=torch.int32)
    area, first = torch.empty(rows, device=dev, dtype=torch.int32), torch.empty(rows, device=dev, dtype=torch.int32)
    bbox, vrange = torch.empty((rows, 4), device=dev, dtype=torch.int32), torch.empty((rows, 2), device=dev, dtype=torch.float32)
    sum_q, lohi = torch.empty(rows, device=dev, dtype=torch.int64), torch.empty((len(maps), 2), device=dev, dtype=torch.float64)
    scratch = torch.empty(at // 8, device=dev, dtype=torch.float64)
    table = _upload_records(records, dev)
    _launch(dev, "mdpt_segment_depth", records.ctypes.data, table.data_ptr(), len(maps), native.dtype_code(maps[0].dtype), SEGMENT_SPACES[space], step, connectivity,
            min_area, scratch.data_ptr(), at, counts.data_ptr(), area.data_ptr(), bbox.data_ptr(), first.data_ptr(), vrange.data_ptr(), sum_q.data_ptr(),
            lohi.data_ptr())
    del table, scratch  # (the caching allocator reuses them in stream order only)
    views = [labels[o:o + h * w].view(h, w) for o, (h, w) in zip(pixel_offs, hws)]
    return DepthSegments(views, counts, area, bbox, first, vrange[:, 0], vrange[:, 1], sum_q, lohi[:, 0], lohi[:, 1], region_offs, caps, min_area, records, (labels,))


def _picks(seg: DepthSegments, points, labels, what: str) -> tuple[np.ndarray, bool]:
    """points / labels per image -> (int32 [N,2] = {image, node or region}, by_label); every value checked on the host"""
    n = len(seg.labels)
    if points is not None and labels is not None:
        raise ValueError(f"{what}: give points or labels, not both")
    given = points if points is not None else labels
    if given is None:
        return np.zeros((0, 2), np.int32), False
    if not isinstance(given, (list, tuple)) or len(given) != n:
        raise ValueError(f"{what}: {'points' if points is not None else 'labels'} must be a list with one list per image ({n}), got {given!r}")
    out = []
    for i, items in enumerate(given):
        h, w = (int(v) for v in seg.labels[i].shape)
        for item in items:
            if points is not None:
                if len(item) != 2 or not all(0.0 <= float(v) <= 1.0 for v in item):
                    raise ValueError(f"{what}: a point must be (x, y) in [0, 1]^2, got {item!r} (image {i})")
                x, y = min(w - 1, math.floor(float(item[0]) * w)), min(h - 1, math.floor(float(item[1]) * h))
                out.append((i, y * w + x))
            else:
                if isinstance(item, bool) or not isinstance(item, (int, np.integer)) or not 0 <= int(item) < seg.capacities[i]:
                    raise ValueError(f"{what}: a label must be a region index in 0 .. {seg.capacities[i] - 1} (image {i}), got {item!r}")
                out.append((i, int(item)))
    return np.asarray(out, np.int32).reshape(-1, 2), labels is not None


def region_cutouts(seg: DepthSegments, images_bgr, points=None, labels=None, invert: bool = False) -> list[tuple[Tensor, Tensor]]:
    """A segmentation and the photos it came from -> one (cutout uint8 [H,W,4] BGRA, mask uint8 [H,W]) per photo, in order, at each photo's own size (the layout of
    depth_mask_images). points: per image a list of normalised (x, y) in [0, 1]; each becomes node (min(w - 1, floor(x w)), min(h - 1, floor(y h))) on the host, and
    the region under it is looked up on the device and selected (a point on a -1 node selects nothing; nothing is read back). labels: per image a list of region
    indices instead. Photo pixel (Y, X) belongs to node ((Y h) // H, (X w) // W), integers throughout; mask = 255 where that node's region is selected, flipped by
    invert; cutout = (BGR AND mask, alpha = mask). images_bgr as depth_mask_images takes them: uint8 HxWx3 host arrays (staged through pinned memory) or CUDA
    tensors read in place, a sliced view through its row pitch. All photos in one launch, one more for the picks. The cutouts are views into one allocation, the
    masks into another."""
    what = "region_cutouts"
    if not isinstance(seg, DepthSegments):
        raise TypeError(f"{what} expects the DepthSegments of segment_depth, got {type(seg)}")
    picks, by_label = _picks(seg, points, labels, what)
    n = len(seg.labels)
    photos, on_device = _photo_list(images_bgr, n, what)
    dev = seg.labels[0].device
    keep, img_ptrs, pitches = _photo_pointers(images_bgr, photos, on_device, dev, what)
    hws = [(int(f.shape[0]), int(f.shape[1])) for f in photos]
    if any(h * w >= 2 ** 31 for h, w in hws):
        raise ValueError(f"{what}: a photo of 2^31 pixels or more is not supported")
    offs, at = packed_offsets([h * w for h, w in hws], 16)
    bgra, mask = torch.empty(at * 4, device=dev, dtype=torch.uint8), torch.empty(at, device=dev, dtype=torch.uint8)
    selected = torch.zeros(max(1, seg.region_offsets[-1] + seg.capacities[-1]), device=dev, dtype=torch.uint8)
    records = record_table(SEGMENT_PHOTO_RECORD, seg.labels, lead=("labels", "h", "w"), photo=img_ptrs, pitch=pitches, H=[h for h, _ in hws], W=[w for _, w in hws],
                           bgra=[bgra.data_ptr() + 4 * o for o in offs], mask=[mask.data_ptr() + o for o in offs], region_off=seg.region_offsets,
                           regions=seg.capacities)
    table = _upload_records(records, dev)
    staged = upload([picks], dev, 4) if len(picks) else None
    _launch(dev, "mdpt_segment_cutout", records.ctypes.data, table.data_ptr(), n, staged[1][0] if staged else None, len(picks), int(by_label), selected.data_ptr(),
            selected.numel(), int(bool(invert)))
    del table, keep, staged, selected  # (the caching allocator reuses them in stream order only)
    return [(bgra[4 * o:4 * (o + h * w)].view(h, w, 4), mask[o:o + h * w].view(h, w)) for o, (h, w) in zip(offs, hws)]


def label_colors(seg: DepthSegments) -> list[Tensor]:
    """The labels as pictures, for looking at a result: one uint8 [h_i,w_i,3] BGR map per image (views into one allocation), a fixed integer hash of the label
    (the same region index always gets the same colour, no channel below 32), -1 black. One launch."""
    what = "label_colors"
    if not isinstance(seg, DepthSegments):
        raise TypeError(f"{what} expects the DepthSegments of segment_depth, got {type(seg)}")
    dev = seg.labels[0].device
    hws = [(int(m.shape[0]), int(m.shape[1])) for m in seg.labels]
    offs, total = packed_offsets([h * w for h, w in hws])
    colors = torch.empty(3 * total, device=dev, dtype=torch.uint8)
    table = _upload_records(seg._records, dev)
    _launch(dev, "mdpt_segment_colors", seg._records.ctypes.data, table.data_ptr(), len(hws), colors.data_ptr())
    del table
    return [colors[3 * o:3 * (o + h * w)].view(h, w, 3) for o, (h, w) in zip(offs, hws)]
