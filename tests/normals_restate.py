"""fp64 numpy restatement of the surface normals and the relighting (muggled_dpt_amd.relight / mdpt_post_normals), written from the definition in
include/mdpt.h: whole-photo arrays, a neighbour is the array shifted by the step with NaN outside the photo, a Python loop over the lights; the resampler
that tests/guided_restate.py restates (through refocus_restate.map_at_pixels). Nothing of the kernel's scheme (tiles, halo, LDS) is in here.

  1. s(Y, X) = the map at the centre of photo pixel (Y, X) (bilinear, fp64 weights, rows first); a map of the photo's size is taken as it is
  2. inverse space: lo, hi = min / max of the map's finite values (+0 for a zero of either sign), v = (s - lo) / (hi - lo) if hi > lo else 0,
     z = 1 / (a + b v), a = 1 / max_depth, b = 1 / min_depth - 1 / max_depth, valid iff s is finite; depth space: z = s, valid iff s is finite and > 0
  3. x = 2 (X + 0.5) / W - 1, y = 1 - 2 (Y + 0.5) / H, P = ((z x) kx, (z y) ky, -z), kx = x_scale tan(fov / 2), ky = y_scale tan(fov / 2)
  4. per axis: A at +t (x: X + t; y: Y - t), B at -t; usable = inside and valid; both: central P_A - P_B if da <= r db and db <= r da (r = inf: always), else
     the side with the smaller depth difference; one: that side; none, or an invalid centre: invalid
  5. n = Tx x Ty, len2 = (nx^2 + ny^2) + nz^2, invalid unless finite and > 0, n / sqrt(len2); invalid: (0, 0, 0); byte = floor((c + 1) / 2 * 255 + 0.5), BGR = z, y, x
  6. per light: shade = ambient + diffuse max(0, n.l); specular > 0: view = -P / |P|, h = (l + view) / |l + view|, sp = max(0, n.h) squared shininess_log2
     times; out = min(255, floor((photo shade + 255 (specular sp)) + 0.5)); an invalid pixel keeps the photo's bytes"""
import math

import numpy as np

from tests import refocus_restate as rr

MAX_STEP = 16


def default_step(W: int, w: int) -> int:
    return min(MAX_STEP, max(1, int(math.floor(W / w + 0.5))))


def camera_scales(H: int, W: int, fov_deg: float):
    """-> (kx, ky): the mesh export's aspect rule times tan(fov / 2)"""
    tan_half = math.tan(fov_deg * 0.5 * (math.pi / 180.0))
    x_scale, y_scale = (1.0, H / W) if W > H else (W / H, 1.0)
    return x_scale * tan_half, y_scale * tan_half


def depth_plane(p, H: int, W: int, space="inverse", min_depth=50.0, max_depth=100.0) -> np.ndarray:
    """-> z fp64 [H,W], NaN where the pixel is invalid"""
    p = np.asarray(p)
    with np.errstate(all="ignore"):
        s = rr.map_at_pixels(p, H, W)
        if space == "inverse":
            finite = p[np.isfinite(p)]
            lo = np.float64(finite.min()) + 0.0 if finite.size else np.float64(0.0)
            hi = np.float64(finite.max()) + 0.0 if finite.size else np.float64(0.0)
            v = (s - lo) / (hi - lo) if finite.size and hi > lo else np.zeros_like(s)
            a, b = 1.0 / np.float64(max_depth), 1.0 / np.float64(min_depth) - 1.0 / np.float64(max_depth)
            z = 1.0 / (a + b * v)
            valid = np.isfinite(s)
        elif space == "depth":
            z = s
            valid = np.isfinite(s) & (s > 0.0)
        else:
            raise ValueError(space)
        return np.where(valid, z, np.nan)


def points(z: np.ndarray, kx: float, ky: float):
    """-> (Px, Py, Pz) of every pixel (NaN where z is)"""
    H, W = z.shape
    X, Y = np.arange(W, dtype=np.float64)[None, :], np.arange(H, dtype=np.float64)[:, None]
    x, y = 2.0 * (X + 0.5) / np.float64(W) - 1.0, 1.0 - 2.0 * (Y + 0.5) / np.float64(H)
    return (z * x) * np.float64(kx), (z * y) * np.float64(ky), -z


def shifted(a: np.ndarray, dy: int, dx: int) -> np.ndarray:
    """out[Y, X] = a[Y + dy, X + dx], NaN where that lies outside"""
    H, W = a.shape
    out = np.full((H, W), np.nan)
    ys, xs = slice(max(0, -dy), min(H, H - dy)), slice(max(0, -dx), min(W, W - dx))
    if ys.start < ys.stop and xs.start < xs.stop:
        out[ys, xs] = a[ys.start + dy:ys.stop + dy, xs.start + dx:xs.stop + dx]
    return out


def tangent(z, P, dy: int, dx: int, edge_ratio: float):
    """the tangent towards (dy, dx): A = the pixel at +(dy, dx), B the one at -(dy, dx) -> (Tx, Ty, Tz, usable)"""
    zA, zB = shifted(z, dy, dx), shifted(z, -dy, -dx)
    useA, useB = ~np.isnan(zA), ~np.isnan(zB)
    both = useA & useB
    with np.errstate(all="ignore"):
        da, db = np.abs(zA - z), np.abs(z - zB)
        central = both if np.isinf(edge_ratio) else both & (da <= np.float64(edge_ratio) * db) & (db <= np.float64(edge_ratio) * da)
        a_smaller = da < db
    takeA = np.where(both, central | a_smaller, useA)
    takeB = np.where(both, central | ~a_smaller, useB)
    T = []
    for c in range(3):
        PA, PB = np.where(takeA, shifted(P[c], dy, dx), P[c]), np.where(takeB, shifted(P[c], -dy, -dx), P[c])
        T.append(PA - PB)
    return T[0], T[1], T[2], useA | useB


def normals(p, H: int, W: int, space="inverse", fov_deg=50.0, min_depth=50.0, max_depth=100.0, step=None, edge_ratio=2.0):
    """map [h,w] -> (n fp64 [H,W,3] before its rounding, (0, 0, 0) where invalid; valid bool [H,W]; P [H,W,3])"""
    p = np.asarray(p)
    t = default_step(W, p.shape[1]) if step is None else int(step)
    kx, ky = camera_scales(H, W, fov_deg)
    z = depth_plane(p, H, W, space, min_depth, max_depth)
    P = points(z, kx, ky)
    ax, ay, az, use_x = tangent(z, P, 0, t, edge_ratio)
    bx, by, bz, use_y = tangent(z, P, -t, 0, edge_ratio)  # (up: Y - t)
    with np.errstate(all="ignore"):
        nx, ny, nz = ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx
        len2 = (nx * nx + ny * ny) + nz * nz
        valid = ~np.isnan(z) & use_x & use_y & np.isfinite(len2) & (len2 > 0.0)
        length = np.sqrt(len2)
        n = np.stack([nx / length, ny / length, nz / length], axis=-1)
    n = np.where(valid[..., None], n, 0.0)
    return n, valid, np.stack(P, axis=-1)


def encode(n: np.ndarray) -> np.ndarray:
    """fp64 normals [H,W,3] (x, y, z) -> uint8 BGR [H,W,3]"""
    return np.floor((n[..., ::-1] + 1.0) / 2.0 * 255.0 + 0.5).astype(np.uint8)


def unit_lights(light_dirs) -> np.ndarray:
    d = np.asarray(light_dirs, dtype=np.float64)
    d = d[None] if d.ndim == 1 else d
    length = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    return d / length[:, None]


def shade(photo: np.ndarray, n, valid, P, light_dirs, ambient=0.35, diffuse=0.9, specular=0.0, shininess_log2=4) -> np.ndarray:
    """uint8 BGR [H,W,3] and normals()'s results -> uint8 [V,H,W,3]"""
    colour = photo.astype(np.float64)
    frames = []
    with np.errstate(all="ignore"):
        if specular > 0.0:
            plen = np.sqrt((P[..., 0] * P[..., 0] + P[..., 1] * P[..., 1]) + P[..., 2] * P[..., 2])
            view = [-P[..., c] / plen for c in range(3)]
        for l in unit_lights(light_dirs):
            dot = (n[..., 0] * l[0] + n[..., 1] * l[1]) + n[..., 2] * l[2]
            sh = np.float64(ambient) + np.float64(diffuse) * np.where(dot > 0.0, dot, 0.0)
            spec = np.zeros_like(sh)
            if specular > 0.0:
                hv = [l[c] + view[c] for c in range(3)]
                hlen = np.sqrt((hv[0] * hv[0] + hv[1] * hv[1]) + hv[2] * hv[2])
                nh = (n[..., 0] * (hv[0] / hlen) + n[..., 1] * (hv[1] / hlen)) + n[..., 2] * (hv[2] / hlen)
                sp = np.where(nh > 0.0, nh, 0.0)
                for _ in range(int(shininess_log2)):
                    sp = sp * sp
                spec = 255.0 * (np.float64(specular) * sp)
            out = np.minimum(255.0, np.floor((colour * sh[..., None] + spec[..., None]) + 0.5))
            frames.append(np.where(valid[..., None], out, colour).astype(np.uint8))
    return np.stack(frames)


def relight(p, photo: np.ndarray, light_dirs, ambient=0.35, diffuse=0.9, specular=0.0, shininess_log2=4, **camera):
    """map [h,w] and uint8 BGR photo [H,W,3] -> (frames uint8 [V,H,W,3], normals fp32 [H,W,3], encoded uint8 [H,W,3])"""
    assert photo.dtype == np.uint8 and photo.ndim == 3 and photo.shape[2] == 3
    n, valid, P = normals(p, photo.shape[0], photo.shape[1], **camera)
    return shade(photo, n, valid, P, light_dirs, ambient, diffuse, specular, shininess_log2), n.astype(np.float32), encode(n)
