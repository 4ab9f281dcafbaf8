"""Synthetic depth maps for the segmentation tests (tests/test_segment_cpu.py checks with the restatement alone that they have the properties the GPU
tests rely on). Every scene is an fp32 [h,w] numpy array; TILE is the side of the device's union-find tiles."""
import numpy as np

TILE = 32
SIZES = [(1, 1), (1, 37), (33, 1), (33, 65), (70, 45)]  # a single tile, ragged tiles on both axes


def plate_before_wall(h=40, w=50, box=(8, 10, 29, 33)):
    """a plate (value 1) over rows y0 .. y1, columns x0 .. x1 (inclusive) before a wall (value 0)"""
    y0, x0, y1, x1 = box
    v = np.zeros((h, w), np.float32)
    v[y0:y1 + 1, x0:x1 + 1] = 1.0
    return v


def checkerboard(h, w):
    return ((np.add.outer(np.arange(h), np.arange(w)) & 1) * 10.0).astype(np.float32)


def diagonal(n):
    """a one-pixel diagonal line (1) on a NaN ground"""
    v = np.full((n, n), np.nan, np.float32)
    v[np.arange(n), np.arange(n)] = 1.0
    return v


def serpentine(h=97, w=130):
    """one path (1) that snakes through every tile: every even row, joined to the next at alternating ends; the walls between (0) are far from it"""
    v = np.zeros((h, w), np.float32)
    v[0::2] = 1.0
    for k, y in enumerate(range(1, h, 2)):
        v[y, w - 1 if k % 2 == 0 else 0] = 1.0
    return v


def comb(h=70, w=99):
    """teeth (every even column, 1) that join only in the last row; the gaps (0) are one component each"""
    v = np.zeros((h, w), np.float32)
    v[:, 0::2] = 1.0
    v[h - 1] = 1.0
    return v


def piecewise(seed: int, h: int, w: int, noise: float, positive: bool = False):
    """random rectangles of levels k / 8 on a ground, a few single specks, plus uniform noise of amplitude `noise`; positive: shifted to 1 .. 2 (a metric map)"""
    rng = np.random.default_rng(seed)
    v = np.full((h, w), 0.5, np.float32)
    for _ in range(12):
        y0, x0 = int(rng.integers(0, h)), int(rng.integers(0, w))
        y1, x1 = min(h, y0 + int(rng.integers(2, max(3, h // 2)))), min(w, x0 + int(rng.integers(2, max(3, w // 2))))
        v[y0:y1, x0:x1] = float(rng.integers(0, 9)) / 8.0
    for _ in range(10):  # specks: components far below any min_area
        v[int(rng.integers(0, h)), int(rng.integers(0, w))] = float(rng.integers(0, 9)) / 8.0
    v[0, 0], v[h - 1, w - 1] = 0.0, 1.0  # (the range is 0 .. 1 whatever was drawn, up to the noise)
    v = v + (rng.random((h, w), dtype=np.float32) - 0.5) * np.float32(2.0 * noise)
    v[int(rng.integers(0, h)), int(rng.integers(0, w))] = np.nan
    v[int(rng.integers(0, h)), int(rng.integers(0, w))] = np.inf
    return (v + 1.0).astype(np.float32) if positive else v.astype(np.float32)


# (seed, h, w, noise): noise 0.004 stays below the default step's 0.02 of the range, 0.05 goes above it and shatters the levels
RANDOM_SCENES = [(3, 70, 90, 0.004), (4, 45, 100, 0.05)]


def region_properties(res, valid):
    """of a restated result and the map's valid nodes: valid nodes of dropped components, a region over more than one tile, regions on the four image edges"""
    lab, bbox = res["labels"], res["bbox"]
    multi = any((b[2] // TILE > b[0] // TILE) or (b[3] // TILE > b[1] // TILE) for b in bbox)
    edges = bool((lab[0] >= 0).any() and (lab[-1] >= 0).any() and (lab[:, 0] >= 0).any() and (lab[:, -1] >= 0).any())
    return dict(dropped=bool(((lab < 0) & valid).any()), multi_tile=multi, edges=edges)
