"""fp64 numpy restatement of the synthetic depth of field (muggled_dpt_amd.refocus / mdpt_post_refocus), written from the definition in
include/mdpt.h: vectorised over the pixels, a Python loop over the taps in the stated order, N(k) by brute-force lattice counting, the resampler
that tests/guided_restate.py restates. Nothing of the kernel's scheme (tiles, halo, the per-tile window, the -inf texels) is in here.

  1. s(Y, X) = the map at the centre of photo pixel (Y, X) (bilinear, fp64 weights, rows first); a map of the photo's size is taken as it is
  2. e: inverse space (s - lo) / (hi - lo) - focus with lo, hi the min / max of the finite map values (+0 for a zero of either sign); depth space
     (1 / s for s > 0, 0 for a finite s <= 0) - 1 / focus; focus_xy: the focus is the value at photo pixel (min(H-1, floor(y H)), min(W-1, floor(x W)));
     e = 0 where s is not finite, and everywhere for a flat map, a map without a finite value, or a pointed s that is not finite (depth: not > 0)
  3. r = min(max_radius, aperture max(0, |e| - focus_range / 2)), rq = floor(4 r), k = (rq rq) >> 4, e32 = fp32(e)
  4. per output pixel p, taps q = p + (dy, dx) inside the photo, dy outer, dx inner, ascending: k_eff = k(q) if e32(q) > e32(p) else min(k(q), k(p));
     where dx^2 + dy^2 <= k_eff: sums += w (B, G, R, 1), w = 1.0 / N(k_eff); out = floor(sum_c / sum_w + 0.5)"""
import functools

import numpy as np

from tests import guided_restate as gr

MAX_RADIUS = 32


@functools.lru_cache(maxsize=None)
def lattice_counts(kmax: int = MAX_RADIUS * MAX_RADIUS) -> np.ndarray:
    """N(k), k = 0 .. kmax: the lattice points (dx, dy) with dx^2 + dy^2 <= k, counted one k at a time"""
    side = int(np.floor(np.sqrt(kmax))) + 1
    d = np.arange(-side, side + 1, dtype=np.int64)
    d2 = d[:, None] ** 2 + d[None, :] ** 2
    counts = np.array([int((d2 <= k).sum()) for k in range(kmax + 1)], dtype=np.int64)
    counts.setflags(write=False)
    return counts


def map_at_pixels(p: np.ndarray, H: int, W: int) -> np.ndarray:
    """the map [h,w] (its values taken as they are) at the centres of the H x W photo pixels -> fp64 [H,W]"""
    p = np.asarray(p)
    if p.shape == (H, W):
        return p.astype(np.float64)
    return gr.bilinear_resize(p, H, W)


def defocus_planes(p, H: int, W: int, focus=0.5, focus_xy=None, aperture=32.0, max_radius=16, focus_range=0.0, space="inverse"):
    """-> (rq uint8 [H,W], e32 fp32 [H,W])"""
    p = np.asarray(p)
    with np.errstate(all="ignore"):
        s = map_at_pixels(p, H, W)
        live = True
        at = None
        if focus_xy is not None:
            at = (min(H - 1, int(np.floor(float(focus_xy[1]) * H))), min(W - 1, int(np.floor(float(focus_xy[0]) * W))))
        if space == "inverse":
            finite = p[np.isfinite(p)]
            lo = np.float64(finite.min()) + 0.0 if finite.size else np.float64(0.0)
            hi = np.float64(finite.max()) + 0.0 if finite.size else np.float64(0.0)
            live = bool(finite.size) and hi > lo
            v = (s - lo) / (hi - lo) if live else np.zeros_like(s)
            f = np.float64(focus)
            if at is not None:
                live = live and bool(np.isfinite(s[at]))
                f = v[at]
        elif space == "depth":
            v = np.where(s > 0.0, 1.0 / s, 0.0)
            if at is not None:
                live = bool(np.isfinite(s[at])) and bool(s[at] > 0.0)
                f = 1.0 / s[at]
            else:
                f = 1.0 / np.float64(focus)
        else:
            raise ValueError(space)
        e = np.where(np.isfinite(s), v - f, 0.0) if live else np.zeros_like(s)
        r = np.minimum(np.float64(max_radius), np.float64(aperture) * np.maximum(0.0, np.abs(e) - np.float64(focus_range) / 2.0))
        rq = np.floor(4.0 * r).astype(np.int64)
        assert rq.min() >= 0 and rq.max() <= 4 * max_radius
        return rq.astype(np.uint8), e.astype(np.float32)


def gather(photo: np.ndarray, rq: np.ndarray, e32: np.ndarray) -> np.ndarray:
    """uint8 BGR [H,W,3], rq, e32 -> the refocused uint8 [H,W,3]"""
    H, W = rq.shape
    counts = lattice_counts()
    k = (rq.astype(np.int64) * rq.astype(np.int64)) >> 4
    reach = int(np.floor(np.sqrt(int(k.max()))))
    colour = photo.astype(np.float64)
    sums = np.zeros((H, W, 3), dtype=np.float64)
    sum_w = np.zeros((H, W), dtype=np.float64)
    for dy in range(-reach, reach + 1):
        py = slice(max(0, -dy), min(H, H - dy))  # the output rows whose tap row lies inside the photo
        qy = slice(py.start + dy, py.stop + dy)
        for dx in range(-reach, reach + 1):
            d2 = dx * dx + dy * dy
            if d2 > int(k.max()):
                continue
            px = slice(max(0, -dx), min(W, W - dx))
            qx = slice(px.start + dx, px.stop + dx)
            if py.start >= py.stop or px.start >= px.stop:
                continue
            kq, kp = k[qy, qx], k[py, px]
            k_eff = np.where(e32[qy, qx] > e32[py, px], kq, np.minimum(kq, kp))
            cover = d2 <= k_eff
            if not cover.any():
                continue
            w = 1.0 / counts[k_eff[cover]].astype(np.float64)
            for c in range(3):
                plane = sums[py, px, c]  # (a view)
                plane[cover] = plane[cover] + w * colour[qy, qx, c][cover]
            plane = sum_w[py, px]
            plane[cover] = plane[cover] + w
    assert sum_w.min() > 0.0
    return np.floor(sums / sum_w[..., None] + 0.5).astype(np.uint8)


def refocus(p, photo: np.ndarray, focus=0.5, focus_xy=None, aperture=32.0, max_radius=16, focus_range=0.0, space="inverse"):
    """map [h,w] and uint8 BGR photo [H,W,3] -> (refocused uint8 [H,W,3], rq uint8 [H,W], e32 fp32 [H,W])"""
    assert photo.dtype == np.uint8 and photo.ndim == 3 and photo.shape[2] == 3
    rq, e32 = defocus_planes(p, photo.shape[0], photo.shape[1], focus, focus_xy, aperture, max_radius, focus_range, space)
    return gather(photo, rq, e32), rq, e32
