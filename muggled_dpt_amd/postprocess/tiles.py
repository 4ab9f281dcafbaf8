"""The stitching of tile maps into one map at a photo's resolution (stitch_tiles; not in the reference, which only describes the fit; layouts in
tiling.py, DPTModel.inference_tiled makes the whole call). Kernels: csrc/post_tiles.inc."""

from __future__ import annotations

import numpy as np
import torch

from .. import native
from ._common import TILE_RECORD, _launch, _prediction_list, _upload_records, ptr, record_table, scratch_bytes

TILE_ALIGN = ("affine", "none")


def stitch_tiles(tile_maps, boxes, image_hw, guide=None, align: str = "affine", feather=None, return_fit: bool = False):
    """The depth maps of overlapping tiles of one photo -> one fp32 [1,H,W] map at the photo's resolution (not in the reference: its .readme_assets/results_explainer.md
    says why tiles cannot simply be pasted - every forward has its own scale and shift, "Results are scene-specific!" - and names the cure under "Fitting to (more) known
    data", a least-squares fit of the two terms, without code for it). tile_maps: [1,h,w] / [h,w] CUDA maps of one dtype and any sizes, as DPTModel.inference_regions
    returns them; boxes: each map's (x1, y1, x2, y2) pixel box in the photo, half-open; image_hw = (H, W). align="affine" fits every tile to `guide` - a [1,gh,gw] /
    [gh,gw] CUDA map of the WHOLE photo, e.g. its inference at model size - over the tile's own box with one scale and one shift (least squares over one sample per
    tile-map pixel, the guide sampled bilinearly at the pixel's centre; samples that are not finite are skipped; a tile the fit cannot use - flat, negatively correlated,
    fewer than two samples - takes the guide's mean over its box, a tile without any sample is left out); align="none" blends the maps as they are. The tiles are resized
    to their boxes by cv2.resize's INTER_LINEAR rule and blended with weights that ramp over `feather` pixels from every tile edge that is not the photo's own border
    (default: the smallest overlap between neighbouring boxes, 0 for one tile). A pixel no tile covers is NaN. fp64 arithmetic rounded once; bit-deterministic; three
    launches (fit, solve, blend), nothing read back, no synchronisation. return_fit: -> (map, fit fp64 [T,2] {scale, shift}, sums fp64 [T,6] {n, Sx, Sy, Sxx, Sxy, Syy}),
    both None with align="none"."""
    what = "stitch_tiles"
    if align not in TILE_ALIGN:
        raise ValueError(f"{what}: align must be 'affine' or 'none', got {align!r}")
    if align == "affine" and guide is None:
        raise ValueError(f"{what}: align='affine' fits the tiles to a guide map of the whole photo: pass guide=, or align='none'")
    if not hasattr(image_hw, "__len__") or len(image_hw) != 2:
        raise TypeError(f"{what}: image_hw must be (H, W), got {image_hw!r}")
    ih, iw = int(image_hw[0]), int(image_hw[1])
    if ih <= 0 or iw <= 0 or ih >= 2 ** 31 or iw >= 2 ** 31:
        raise ValueError(f"{what}: bad photo size {ih}x{iw}")
    if not isinstance(boxes, (list, tuple, np.ndarray)) or len(boxes) == 0:
        raise ValueError(f"{what} expects a non-empty list of (x1, y1, x2, y2) boxes, got {boxes!r}")
    for k, b in enumerate(boxes):
        if not hasattr(b, "__len__") or len(b) != 4 or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in b):
            raise TypeError(f"{what}: box {k} must be four ints (x1, y1, x2, y2), got {b!r}")
        x1, y1, x2, y2 = (int(v) for v in b)
        if not (0 <= x1 < x2 <= iw and 0 <= y1 < y2 <= ih):
            raise ValueError(f"{what}: box {k} ({x1}, {y1})-({x2}, {y2}) is empty or outside the {ih}x{iw} photo")
    boxes = [tuple(int(v) for v in b) for b in boxes]
    if not isinstance(tile_maps, (list, tuple)):
        raise TypeError(f"{what} expects a list of [1,h,w] / [h,w] tile maps, got {type(tile_maps)}")
    if len(tile_maps) != len(boxes):
        raise ValueError(f"{what}: {len(tile_maps)} tile maps but {len(boxes)} boxes")
    if feather is None:
        from ..tiling import smallest_overlap
        feather = smallest_overlap(boxes)
    feather = float(feather)
    if not (0.0 <= feather < float("inf")):
        raise ValueError(f"{what}: feather must be finite and >= 0, got {feather}")
    maps = _prediction_list(list(tile_maps), what)
    dev = maps[0].device
    g = None
    if align == "affine":
        g = _prediction_list([guide], what + " (guide)")[0]
        if g.device != dev:
            raise RuntimeError(f"{what}: the tiles are on {dev} but the guide is on {g.device}")
    n_tiles = len(maps)
    records = record_table(TILE_RECORD, maps, **{name: [b[k] for b in boxes] for k, name in enumerate(("x1", "y1", "x2", "y2"))})
    table = _upload_records(records, dev)
    dt = native.dtype_code(maps[0].dtype)
    fit = sums = None
    if g is not None:
        need = scratch_bytes("mdpt_post_tile_scratch_bytes", records.ctypes.data, n_tiles)
        scratch = torch.empty(max(need // 8, 1), device=dev, dtype=torch.float64)
        fit = torch.empty((n_tiles, 2), device=dev, dtype=torch.float64)
        sums = torch.empty((n_tiles, 6), device=dev, dtype=torch.float64)
        _launch(dev, "mdpt_post_tile_fit", records.ctypes.data, table.data_ptr(), n_tiles, dt, g.data_ptr(), native.dtype_code(g.dtype), g.shape[0], g.shape[1],
                ih, iw, fit.data_ptr(), sums.data_ptr(), scratch.data_ptr(), need)
    out = torch.empty((1, ih, iw), device=dev, dtype=torch.float32)
    _launch(dev, "mdpt_post_tile_blend", records.ctypes.data, table.data_ptr(), n_tiles, dt, ih, iw, ptr(fit), ptr(sums), feather, out.data_ptr())
    del table  # (the caching allocator reuses it in stream order only)
    return (out, fit, sums) if return_fit else out
