"""Tile layouts for tiled high-resolution inference (DPTModel.inference_tiled, postprocess.stitch_tiles): pure Python, no torch, no device.

A box is (x1, y1, x2, y2) in pixels, half-open, as DPTModel.inference_regions takes it after the image index. Boxes come row by row, left to
right. Per axis of length L the rule is the same: the tile side is clamped to L; n = 1 if the tile covers the axis, else
n = ceil((L - ov) / (tile - ov)) tiles, the fewest whose neighbours overlap by at least ov; tile i starts at round(i (L - tile) / (n - 1)), so
the first tile starts at 0, the last ends at L and the spare overlap is spread evenly (round is Python's: halves go to the even integer)."""

from __future__ import annotations

import math


def _pair(v, what: str) -> tuple:
    if isinstance(v, (tuple, list)):
        if len(v) != 2:
            raise ValueError(f"{what} must be one value or a (y, x) pair, got {v!r}")
        return v[0], v[1]
    return v, v


def _int(v, what: str) -> int:
    if isinstance(v, bool) or int(v) != v:
        raise TypeError(f"{what} must be an integer, got {v!r}")
    return int(v)


def axis_starts(length: int, tile: int, min_overlap: int) -> tuple[int, list[int]]:
    """One axis -> (the clamped tile side, the start of every tile)"""
    length, tile, ov = _int(length, "the image side"), _int(tile, "the tile side"), _int(min_overlap, "min_overlap")
    if length <= 0 or tile <= 0:
        raise ValueError(f"image and tile sides must be positive, got {length} and {tile}")
    tile = min(tile, length)
    if tile == length:
        return tile, [0]
    if not 0 <= ov < tile:
        raise ValueError(f"min_overlap must be in [0, tile side), got {ov} for tiles of {tile}")
    n = -(-(length - ov) // (tile - ov))
    return tile, [round(i * (length - tile) / (n - 1)) for i in range(n)]


def tile_boxes(image_hw, tile_hw, min_overlap=0) -> list[tuple[int, int, int, int]]:
    """Boxes of tile_hw = (h, w) (or one side for both) that cover an image of image_hw = (h, w), neighbours overlapping by at least
    min_overlap pixels (one value, or (y, x)). A tile at least as large as the image gives the one box of the whole image."""
    (h, w), (th, tw), (oy, ox) = _pair(image_hw, "image_hw"), _pair(tile_hw, "tile_hw"), _pair(min_overlap, "min_overlap")
    th, ys = axis_starts(h, th, oy)
    tw, xs = axis_starts(w, tw, ox)
    return [(x, y, x + tw, y + th) for y in ys for x in xs]


def grid_tile_side(length: int, n: int, overlap_frac: float) -> int:
    """The side of n equal tiles that cover `length` when neighbours share overlap_frac of a side: ceil(L / (n - (n - 1) f)), at most L"""
    length, n = _int(length, "the image side"), _int(n, "the tile count")
    f = float(overlap_frac)
    if not 0.0 <= f < 1.0:
        raise ValueError(f"overlap_frac must be in [0, 1), got {overlap_frac}")
    if not 1 <= n <= length:
        raise ValueError(f"an axis of {length} pixels takes 1..{length} tiles, got {n}")
    return min(length, math.ceil(length / (n - (n - 1) * f)))


def tile_grid_boxes(image_hw, grid, overlap_frac: float = 0.25) -> list[tuple[int, int, int, int]]:
    """An ny x nx grid (grid = (ny, nx)) of equal tiles over an image of image_hw = (h, w): per axis the side is grid_tile_side - n tiles whose
    neighbours share about overlap_frac of a side - and the starts are spread as in tile_boxes. A 1 x 1 grid is the whole image."""
    (h, w), (ny, nx) = _pair(image_hw, "image_hw"), _pair(grid, "grid")
    h, w, ny, nx = _int(h, "image_hw"), _int(w, "image_hw"), _int(ny, "grid"), _int(nx, "grid")
    if h <= 0 or w <= 0:
        raise ValueError(f"image sides must be positive, got {h}x{w}")
    th, tw = grid_tile_side(h, ny, overlap_frac), grid_tile_side(w, nx, overlap_frac)

    def starts(length, tile, n):
        return [0] if n == 1 else [round(i * (length - tile) / (n - 1)) for i in range(n)]

    return [(x, y, x + tw, y + th) for y in starts(h, th, ny) for x in starts(w, tw, nx)]


def smallest_overlap(boxes) -> int:
    """The smallest overlap, in pixels, between NEIGHBOURING boxes: for every box and axis, the boxes that intersect it and start later on that
    axis are looked at, and the one that starts soonest is its neighbour there (several that start together count alike); the overlap is the
    intersection's extent along the axis. Tiles two apart that still intersect (overlaps above half a side) are no neighbours. 0 when no two
    boxes overlap (one tile, abutting tiles). stitch_tiles' default feather width."""
    boxes = [tuple(int(v) for v in b) for b in boxes]
    best = None
    for a in boxes:
        for lo, hi in ((0, 2), (1, 3)):
            nearest, overlap = None, None
            for b in boxes:
                if b[lo] <= a[lo] or min(a[2], b[2]) <= max(a[0], b[0]) or min(a[3], b[3]) <= max(a[1], b[1]):
                    continue
                ext = min(a[hi], b[hi]) - b[lo]
                if nearest is None or b[lo] < nearest:
                    nearest, overlap = b[lo], ext
                elif b[lo] == nearest:
                    overlap = min(overlap, ext)
            if overlap is not None:
                best = overlap if best is None else min(best, overlap)
    return 0 if best is None else best
