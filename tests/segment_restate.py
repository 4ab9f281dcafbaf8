"""The definition of the depth segmentation (include/mdpt.h, muggled_dpt_amd/segment.py) restated in numpy, from the definition and not from the kernels:
links from shifted comparisons in fp64, components by iterating label = min(label, linked neighbours' labels) to a fixed point (with pointer jumping, which
changes no fixed point), numbering by sorted roots, statistics by np.bincount / np.minimum.at, the integer node rule for the cutouts."""
import math

import numpy as np


def valid_nodes(v32: np.ndarray, space: str) -> np.ndarray:
    ok = np.isfinite(v32)
    return ok & (v32 > 0) if space == "depth" else ok


def value_range(v32: np.ndarray, space: str) -> tuple[float, float]:
    """lo, hi over the valid nodes as fp64 (a zero takes the sign +; no valid node: 0, 0)"""
    ok = valid_nodes(v32, space)
    if not ok.any():
        return 0.0, 0.0
    return float(np.float64(v32[ok].min()) + 0.0), float(np.float64(v32[ok].max()) + 0.0)


def link_planes(v32: np.ndarray, space: str, step: float, connectivity: int) -> dict:
    """{(dy, dx): bool [h,w]}: node (y, x) is linked to node (y + dy, x + dx); every pair belongs to its upper (for dy == 0: left) node"""
    assert v32.dtype == np.float32 and v32.ndim == 2 and space in ("inverse", "depth") and connectivity in (4, 8)
    h, w = v32.shape
    ok, v = valid_nodes(v32, space), v32.astype(np.float64)
    lo, hi = value_range(v32, space)
    planes = {}
    for dy, dx in [(0, 1), (1, 0)] + ([(1, 1), (1, -1)] if connectivity == 8 else []):
        ys, xs = slice(0, h - dy), slice(max(0, -dx), w - max(0, dx))
        yq, xq = slice(dy, h), slice(max(0, dx), w - max(0, -dx))
        a, b = v[ys, xs], v[yq, xq]
        with np.errstate(invalid="ignore", over="ignore"):
            bound = np.float64(step) * (np.float64(hi) - np.float64(lo)) if space == "inverse" else np.float64(step) * np.minimum(a, b)
            linked = np.abs(a - b) <= bound
        plane = np.zeros((h, w), bool)
        plane[ys, xs] = linked & ok[ys, xs] & ok[yq, xq]
        planes[(dy, dx)] = plane
    return planes


def component_roots(v32: np.ndarray, space: str, step: float, connectivity: int) -> np.ndarray:
    """int64 [h,w]: the lowest linear index of every valid node's component, -1 for a node that is not valid"""
    h, w = v32.shape
    ok = valid_nodes(v32, space)
    big = h * w
    lab = np.where(ok, np.arange(h * w, dtype=np.int64).reshape(h, w), big)
    planes = link_planes(v32, space, step, connectivity)
    while True:
        before = lab.copy()
        for (dy, dx), plane in planes.items():
            ys, xs = slice(0, h - dy), slice(max(0, -dx), w - max(0, dx))
            yq, xq = slice(dy, h), slice(max(0, dx), w - max(0, -dx))
            m = plane[ys, xs]
            low = np.minimum(lab[ys, xs], lab[yq, xq])
            lab[ys, xs] = np.where(m, low, lab[ys, xs])
            lab[yq, xq] = np.where(m, np.minimum(low, lab[yq, xq]), lab[yq, xq])  # (the slices overlap: a node may just have got a lower label)
        flat = np.append(lab.reshape(-1), big)  # (pointer jumping: a label is a node of the same component whose own label is no greater)
        lab = flat[flat[:-1]].reshape(h, w)
        if np.array_equal(lab, before):
            break
    return np.where(ok, lab, -1)


def segment(v32: np.ndarray, space: str = "inverse", step: float = 0.02, connectivity: int = 4, min_area: int = 16) -> dict:
    """-> labels int32 [h,w], count, area, bbox [K,4] = x0, y0, x1, y1, first, vmin, vmax (fp32), sum_q (int64), lo, hi, mean (fp64)"""
    v32 = np.ascontiguousarray(v32, dtype=np.float32)
    h, w = v32.shape
    roots = component_roots(v32, space, step, connectivity)
    lo, hi = value_range(v32, space)
    sizes = np.bincount(roots[roots >= 0], minlength=h * w)
    kept = np.flatnonzero(sizes >= min_area)  # (sorted: the order of the roots; a root's size is counted at the root alone)
    kept = kept[sizes[kept] > 0]
    new_id = np.full(h * w + 1, -1, np.int64)
    new_id[kept] = np.arange(len(kept))
    labels = new_id[roots]  # (roots == -1 reads the last entry: -1)
    K = len(kept)
    on = labels >= 0
    ids = labels[on]
    ys, xs = np.nonzero(on)
    vals = v32[on]
    area = np.bincount(ids, minlength=K).astype(np.int32)
    bbox = np.empty((K, 4), np.int32)
    for col, (src, fn, init) in enumerate([(xs, np.minimum, 2 ** 31 - 1), (ys, np.minimum, 2 ** 31 - 1), (xs, np.maximum, -1), (ys, np.maximum, -1)]):
        acc = np.full(K, init, np.int64)
        fn.at(acc, ids, src)
        bbox[:, col] = acc
    vmin, vmax = np.full(K, np.inf, np.float32), np.full(K, -np.inf, np.float32)
    np.minimum.at(vmin, ids, vals)
    np.maximum.at(vmax, ids, vals)
    if hi > lo:
        q = np.floor((vals.astype(np.float64) - lo) / (hi - lo) * 16777216.0 + 0.5).astype(np.int64)
    else:
        q = np.zeros(len(vals), np.int64)
    sum_q = np.zeros(K, np.int64)
    np.add.at(sum_q, ids, q)
    mean = np.float64(lo) + (np.float64(hi) - np.float64(lo)) * sum_q.astype(np.float64) / (area.astype(np.float64) * float(2 ** 24))
    return dict(labels=labels.astype(np.int32), count=K, area=area, bbox=bbox, first=kept.astype(np.int32), vmin=vmin, vmax=vmax, sum_q=sum_q, lo=lo, hi=hi,
                mean=mean)


def point_nodes(points, h: int, w: int) -> list[tuple[int, int]]:
    """normalised (x, y) -> node (y, x) = (min(h - 1, floor(y h)), min(w - 1, floor(x w)))"""
    return [(min(h - 1, math.floor(float(y) * h)), min(w - 1, math.floor(float(x) * w))) for x, y in points]


def picked(labels: np.ndarray, points) -> set:
    """the regions under the points (a point on a -1 node selects nothing)"""
    h, w = labels.shape
    return {int(labels[y, x]) for y, x in point_nodes(points, h, w) if labels[y, x] >= 0}


def cutout(labels: np.ndarray, photo: np.ndarray, selected, invert: bool = False) -> tuple[np.ndarray, np.ndarray]:
    """-> (BGRA uint8 [H,W,4], mask uint8 [H,W]): photo pixel (Y, X) belongs to node ((Y h) // H, (X w) // W)"""
    h, w = labels.shape
    H, W = photo.shape[:2]
    ny, nx = (np.arange(H, dtype=np.int64) * h) // H, (np.arange(W, dtype=np.int64) * w) // W
    lab = labels[ny[:, None], nx[None, :]]
    on = np.isin(lab, np.asarray(sorted(selected), dtype=np.int64)) & (lab >= 0)
    if invert:
        on = ~on
    mask = np.where(on, 255, 0).astype(np.uint8)
    bgra = np.concatenate([photo & mask[:, :, None], mask[:, :, None]], axis=2)
    return bgra, mask


def colors(labels: np.ndarray) -> np.ndarray:
    """uint8 [h,w,3] BGR: the fixed integer hash of muggled_dpt_amd/csrc/post_segment.inc's header (-1: black)"""
    m = np.uint64(0xffffffff)
    x = ((labels.astype(np.int64) + 1).astype(np.uint64) * np.uint64(2654435761)) & m
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(2246822519)) & m
    x ^= x >> np.uint64(13)
    x |= np.uint64(0x202020)
    x = np.where(labels >= 0, x, np.uint64(0))
    return np.stack([(x & np.uint64(255)), (x >> np.uint64(8)) & np.uint64(255), (x >> np.uint64(16)) & np.uint64(255)], axis=2).astype(np.uint8)
