"""fp64 numpy restatement of the photo-guided upsampling (postprocess.guided_upsample_images / mdpt_post_guided_upsample), written from the
definition - plain window slices and np.linalg.solve - and not from the kernels' summation scheme (row sums, then column sums, Cholesky).

  1. cell sums: photo pixel (Y, X) belongs to cell (Y h // H, X w // W); n and the channel sums are integers; g = (S / n) / 255
  2. coefficients: window = the cells within `radius` in both axes, clipped to the grid, mean = sum / its own count;
     Sigma = mean(g g^T) - mean(g) mean(g)^T + eps I, a = Sigma^-1 (mean(g p) - mean(g) mean(p)), b = mean(p) - a . mean(g)
  3. the same window mean of (a_B, a_G, a_R, b)
  4. apply: the mean coefficients resampled bilinearly at the pixel's centre (u = (X + 0.5) w / W - 0.5 clamped, fp64 weights, rows first),
     q = a_B B / 255 + a_G G / 255 + a_R R / 255 + b, rounded to fp32 once

`real` = np.longdouble runs steps 2 to 4 in extended precision (with an elimination written out, np.linalg has no longdouble): the yardstick for
the fp64 noise of the restatement itself."""
import numpy as np


def cell_sums(photo: np.ndarray, h: int, w: int):
    """uint8 [H,W,3] -> (n int64 [h,w], S int64 [h,w,3])"""
    H, W = photo.shape[:2]
    cj, ci = (np.arange(H, dtype=np.int64) * h) // H, (np.arange(W, dtype=np.int64) * w) // W
    flat = (cj[:, None] * w + ci[None, :]).reshape(-1)
    n = np.bincount(flat, minlength=h * w).astype(np.int64).reshape(h, w)
    s = np.zeros((h * w, 3), dtype=np.int64)
    np.add.at(s, flat, photo.reshape(-1, 3).astype(np.int64))
    return n, s.reshape(h, w, 3)


def low_res_guide(photo: np.ndarray, h: int, w: int, real=np.float64) -> np.ndarray:
    n, s = cell_sums(photo, h, w)
    return (s.astype(real) / n.astype(real)[..., None]) / real(255)


def window_mean(x: np.ndarray, radius: int) -> np.ndarray:
    """[h,w,K] -> the mean over the cells within `radius` in both axes, clipped to the grid, per plane"""
    h, w = x.shape[:2]
    out = np.empty_like(x)
    for j in range(h):
        j0, j1 = max(j - radius, 0), min(j + radius, h - 1) + 1
        for i in range(w):
            i0, i1 = max(i - radius, 0), min(i + radius, w - 1) + 1
            win = x[j0:j1, i0:i1]
            out[j, i] = win.sum(axis=(0, 1)) / x.dtype.type((j1 - j0) * (i1 - i0))
    return out


def _solve3(sigma: np.ndarray, rhs: np.ndarray) -> np.ndarray:
    """[...,3,3] x = [...,3]: np.linalg.solve in fp64, Gaussian elimination with partial pivoting written out for longdouble"""
    if sigma.dtype == np.float64:
        return np.linalg.solve(sigma, rhs[..., None])[..., 0]
    out = np.empty_like(rhs)
    for idx in np.ndindex(sigma.shape[:-2]):
        a = np.concatenate([sigma[idx], rhs[idx][:, None]], axis=1)
        for c in range(3):
            piv = c + int(np.argmax(np.abs(a[c:, c])))
            a[[c, piv]] = a[[piv, c]]
            for r in range(c + 1, 3):
                a[r] = a[r] - a[c] * (a[r, c] / a[c, c])
        x = np.zeros(3, dtype=sigma.dtype)
        for c in (2, 1, 0):
            x[c] = (a[c, 3] - (a[c, c + 1:3] * x[c + 1:]).sum()) / a[c, c]
        out[idx] = x
    return out


def coefficients(p: np.ndarray, g: np.ndarray, radius: int, eps: float) -> np.ndarray:
    """map [h,w] and guide [h,w,3] -> (a_B, a_G, a_R, b) [h,w,4] before their own window mean"""
    real = g.dtype.type
    p = p.astype(g.dtype)
    mg = window_mean(g, radius)
    mgg = window_mean((g[..., :, None] * g[..., None, :]).reshape(*g.shape[:2], 9), radius).reshape(*g.shape[:2], 3, 3)
    mp = window_mean(p[..., None], radius)[..., 0]
    mgp = window_mean(g * p[..., None], radius)
    sigma = mgg - mg[..., :, None] * mg[..., None, :] + real(eps) * np.eye(3, dtype=g.dtype)
    a = _solve3(sigma, mgp - mg * mp[..., None])
    b = mp - (a * mg).sum(axis=-1)
    return np.concatenate([a, b[..., None]], axis=-1)


def bilinear_planes(m: np.ndarray, H: int, W: int) -> np.ndarray:
    """[h,w,K] resampled at the centres of an H x W grid: u = (X + 0.5) w / W - 0.5 clamped to the grid, taps x0 and min(x0 + 1, w - 1), weights in the
    planes' precision, rows first (csrc/postprocess.hip bilinear_f64_at) -> [H,W,K]"""
    h, w = m.shape[:2]
    real = m.dtype.type
    u = np.clip((np.arange(W).astype(m.dtype) + real(0.5)) * real(w) / real(W) - real(0.5), real(0), real(w - 1))
    v = np.clip((np.arange(H).astype(m.dtype) + real(0.5)) * real(h) / real(H) - real(0.5), real(0), real(h - 1))
    x0, y0 = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    ax, ay = (u - x0.astype(m.dtype))[None, :, None], (v - y0.astype(m.dtype))[:, None, None]
    top = m[y0][:, x0] * (real(1) - ax) + m[y0][:, x1] * ax
    bot = m[y1][:, x0] * (real(1) - ax) + m[y1][:, x1] * ax
    return top * (real(1) - ay) + bot * ay


def bilinear_resize(p: np.ndarray, H: int, W: int) -> np.ndarray:
    """[h,w] -> fp64 [H,W] by the rule above"""
    return bilinear_planes(np.asarray(p, dtype=np.float64)[..., None], H, W)[..., 0]


def guided_upsample(p: np.ndarray, photo: np.ndarray, radius: int, eps: float, real=np.float64):
    """map [h,w] (any float dtype; its values are taken as they are) and uint8 BGR photo [H,W,3] -> (q fp32 [H,W], mean coefficients [h,w,4] in `real`,
    q before its rounding in `real`)"""
    h, w = p.shape
    H, W = photo.shape[:2]
    assert H >= h and W >= w and photo.dtype == np.uint8 and photo.shape[2] == 3
    g = low_res_guide(photo, h, w, real)
    mean = window_mean(coefficients(np.asarray(p).astype(real), g, radius, eps), radius)
    up = bilinear_planes(mean, H, W)
    unit = photo.astype(real) / real(255)
    q = ((up[..., 0] * unit[..., 0] + up[..., 1] * unit[..., 1]) + up[..., 2] * unit[..., 2]) + up[..., 3]
    return q.astype(np.float32), mean, q
