"""fp64 numpy restatement of tiled high-resolution inference (postprocess.stitch_tiles: mdpt_post_tile_fit / mdpt_post_tile_blend) for
tests/test_tiling_cpu.py, tests/test_gpu_tiles.py and tests/test_gpu_inference_tiled.py, written from the definitions of the feature and not from
the kernels. Nothing comes from the reference, which describes the fit (.readme_assets/results_explainer.md, "Fitting to (more) known data") and
has no code for it.

A tile t has a map m_t (h x w) and a half-open pixel box (x1, y1, x2, y2) in an H x W photo, bw = x2 - x1, bh = y2 - y1; the guide g (gh x gw)
covers the whole photo. Every step is float64, one IEEE operation at a time in the order written; the sums of the fit are math.fsum's (exact,
rounded once)."""
from __future__ import annotations

import math

import numpy as np

from tests.mask_restate import linear_taps


def guide_samples(guide: np.ndarray, box, hw, image_hw) -> np.ndarray:
    """y of every sample (j, i) of an h x w tile map: the guide sampled bilinearly (fp64 weights, rows first) at u = X gw / W - 0.5,
    v = Y gh / H - 0.5 clamped to the guide, (X, Y) = (x1 + (i + 0.5) bw / w, y1 + (j + 0.5) bh / h) -> float64 [h, w]"""
    g = np.asarray(guide, dtype=np.float64)
    gh, gw = g.shape
    (x1, y1, x2, y2), (h, w), (H, W) = box, hw, image_hw
    X = float(x1) + (np.arange(w, dtype=np.float64) + 0.5) * float(x2 - x1) / float(w)
    Y = float(y1) + (np.arange(h, dtype=np.float64) + 0.5) * float(y2 - y1) / float(h)
    u = np.clip(X * float(gw) / float(W) - 0.5, 0.0, float(gw - 1))
    v = np.clip(Y * float(gh) / float(H) - 0.5, 0.0, float(gh - 1))
    xa, ya = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
    xb, yb = np.minimum(xa + 1, gw - 1), np.minimum(ya + 1, gh - 1)
    ax, ay = (u - xa)[None, :], (v - ya)[:, None]
    with np.errstate(invalid="ignore"):
        top = g[ya][:, xa] * (1.0 - ax) + g[ya][:, xb] * ax
        bot = g[yb][:, xa] * (1.0 - ax) + g[yb][:, xb] * ax
        return top * (1.0 - ay) + bot * ay


def fit_terms(tile_map: np.ndarray, guide: np.ndarray, box, image_hw):
    """-> the six lists of terms {1, x, y, xx, xy, yy} over the samples whose x and y are finite, in sample order (float64 arrays)"""
    x = np.asarray(tile_map, dtype=np.float64)
    y = guide_samples(guide, box, x.shape, image_hw)
    keep = np.isfinite(x) & np.isfinite(y)
    x, y = x[keep], y[keep]
    return [np.ones_like(x), x, y, x * x, x * y, y * y]


def solve(sums):
    """{n, Sx, Sy, Sxx, Sxy, Syy} -> (s, t): var = n Sxx - Sx^2, s = (n Sxy - Sx Sy) / var, t = (Sy - s Sx) / n; a degenerate tile (n < 2,
    var <= 0, s not finite or <= 0) gets s = 0 and the guide's mean t = Sy / n; n == 0: t = 0 (the tile is empty)"""
    n, sx, sy, sxx, sxy, _ = (float(v) for v in sums)
    if n == 0:
        return 0.0, 0.0
    var = n * sxx - sx * sx
    with np.errstate(all="ignore"):
        s = float(np.float64(n * sxy - sx * sy) / np.float64(var))
    if n < 2 or not var > 0 or not math.isfinite(s) or s <= 0:
        return 0.0, sy / n
    return s, (sy - s * sx) / n


def fit(tile_maps, boxes, guide, image_hw):
    """-> (fit float64 [T, 2], sums float64 [T, 6], abs_terms float64 [T, 6]): the fsum of every term list, the fit solved from those sums, and the
    fsum of the terms' absolute values (the scale of the bound on any other summation order)"""
    T = len(tile_maps)
    out_fit, sums, abs_terms = np.zeros((T, 2)), np.zeros((T, 6)), np.zeros((T, 6))
    for t, (m, b) in enumerate(zip(tile_maps, boxes)):
        terms = fit_terms(m, guide, b, image_hw)
        sums[t] = [math.fsum(v) for v in terms]
        abs_terms[t] = [math.fsum(np.abs(v)) for v in terms]
        out_fit[t] = solve(sums[t])
    return out_fit, sums, abs_terms


def resize_tile(x: np.ndarray, wh) -> np.ndarray:
    """cv2.resize(x, wh) (INTER_LINEAR) on a float64 map as mask_restate.resize_f64 states it - fp32 weights 1 - a and a, fp64 sums, rows first, one
    tap where a == 0 - with one change: a lerp of two EQUAL taps is that tap. cv2's two fp32 weights need not sum to 1 (in the first source
    interval a carries bits below 2^-24), and a flat region must keep exactly the value the tiles hold there."""
    w_out, h_out = int(wh[0]), int(wh[1])
    xs0, xs1, xa = linear_taps(w_out, x.shape[1])
    ys0, ys1, ya = linear_taps(h_out, x.shape[0])

    def lerp(v0, v1, a):
        with np.errstate(invalid="ignore", over="ignore"):
            mixed = v0 * (np.float32(1) - a).astype(np.float64) + v1 * a.astype(np.float64)
        return np.where((a == 0) | (v0 == v1), v0, mixed)

    rows = lerp(x[:, xs0], x[:, xs1], xa[None, :])
    return lerp(rows[ys0], rows[ys1], ya[:, None])


def axis_weights(lo: int, hi: int, n: int, feather: float) -> np.ndarray:
    """min(1, (d + 1) / (r + 1)) for every coordinate of [lo, hi), d the distance to the nearer of the edges lo and hi - 1; an edge on the photo's
    border (lo == 0, hi == n) does not count, neither counting gives 1"""
    c = np.arange(lo, hi, dtype=np.float64)
    d = np.full(c.shape, np.inf)
    if lo > 0:
        d = np.minimum(d, c - lo)
    if hi < n:
        d = np.minimum(d, (hi - 1) - c)
    return np.minimum(1.0, (d + 1.0) / (float(feather) + 1.0))


def blend(tile_maps, boxes, image_hw, fit_st=None, empty=None, feather: float = 0.0) -> np.ndarray:
    """-> float64 [H, W]: per pixel sum_t w_t z_t / sum_t w_t over the tiles whose box holds it, in tile order, skipping the tiles flagged in
    `empty`; z_t = s_t val_t + t_t (fit_st None: s = 1, t = 0), val_t = cv2.resize(m_t, (bw, bh)) (resize_tile),
    w_t = wx wy (axis_weights). NaN where no tile covers the pixel. Round with .astype(np.float32) for the device's result."""
    H, W = image_hw
    num, den = np.zeros((H, W)), np.zeros((H, W))
    for t, (m, (x1, y1, x2, y2)) in enumerate(zip(tile_maps, boxes)):
        if empty is not None and empty[t]:
            continue
        s, sh = (1.0, 0.0) if fit_st is None else (float(fit_st[t][0]), float(fit_st[t][1]))
        val = resize_tile(np.asarray(m, dtype=np.float64), (x2 - x1, y2 - y1))
        w = axis_weights(y1, y2, H, feather)[:, None] * axis_weights(x1, x2, W, feather)[None, :]
        with np.errstate(invalid="ignore", over="ignore"):
            z = s * val + sh
            num[y1:y2, x1:x2] += w * z
        den[y1:y2, x1:x2] += w
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(den > 0, num / den, np.nan)


def stitch(tile_maps, boxes, image_hw, guide=None, feather: float = 0.0):
    """the whole of stitch_tiles -> (float32 [H, W], fit, sums): align="affine" with a guide, align="none" without"""
    if guide is None:
        return blend(tile_maps, boxes, image_hw, None, None, feather).astype(np.float32), None, None
    fit_st, sums, _ = fit(tile_maps, boxes, guide, image_hw)
    return blend(tile_maps, boxes, image_hw, fit_st, sums[:, 0] == 0, feather).astype(np.float32), fit_st, sums


def ulps(a: np.ndarray, b: np.ndarray) -> int:
    """the largest distance of two float32 arrays in fp32 ulps; NaNs must sit at the same pixels"""
    assert a.dtype == np.float32 and b.dtype == np.float32 and a.shape == b.shape
    assert np.array_equal(np.isnan(a), np.isnan(b)), "NaN at different pixels"
    keep = ~np.isnan(a)

    def ordered(v):
        k = v.view(np.int32).astype(np.int64)
        return np.where(k < 0, -(k & 0x7fffffff), k)

    return int(np.abs(ordered(a[keep]) - ordered(b[keep])).max()) if keep.any() else 0
