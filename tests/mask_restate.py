"""numpy restatements of the depth masking demo (the reference's experiments/depth_masking.py) for tests/test_depth_mask_cpu.py and
tests/test_gpu_depth_mask.py: cv2.resize(INTER_LINEAR) on uint8 (the scalar fixed-point formula) and float64, CheckerPattern(), and the display and
save steps in fp64. Written independently of tests/golden/gen_depth_mask.py's cv2 stub, whose outputs the CPU tests compare them with."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F


def linear_taps(n_out: int, n_in: int):
    """per axis: (s0, s1, a) - the two source indices and the fp32 weight of the second"""
    p = (np.arange(n_out).astype(np.float64) + 0.5) * (1.0 / (float(n_out) / float(n_in))) - 0.5
    p = p.astype(np.float32)
    s = np.floor(p).astype(np.int64)
    a = (p - s.astype(np.float32)).astype(np.float32)
    lo, hi = s < 0, s >= n_in - 1
    s = np.where(lo, 0, np.where(hi, n_in - 1, s))
    a = np.where(lo | hi, np.float32(0), a).astype(np.float32)
    return s, np.where(a != 0, s + 1, s), a


def resize_u8(img: np.ndarray, wh) -> np.ndarray:
    """cv2.resize(img, wh) on uint8 HxW or HxWxC: weights round(2048 w), integer sums, (v + 2^21) >> 22"""
    w_out, h_out = int(wh[0]), int(wh[1])
    xs0, xs1, xa = linear_taps(w_out, img.shape[1])
    ys0, ys1, ya = linear_taps(h_out, img.shape[0])
    q = lambda a: np.rint(a * np.float32(2048)).astype(np.int64)  # noqa: E731
    ax0, ax1, ay0, ay1 = q(np.float32(1) - xa), q(xa), q(np.float32(1) - ya), q(ya)
    tail = (None,) * (img.ndim - 2)
    s = img.astype(np.int64)
    rows = s[:, xs0] * ax0[(None, slice(None)) + tail] + s[:, xs1] * ax1[(None, slice(None)) + tail]
    v = (rows[ys0] * ay0[(slice(None), None) + tail] + rows[ys1] * ay1[(slice(None), None) + tail] + (1 << 21)) >> 22
    return np.clip(v, 0, 255).astype(np.uint8)


def resize_f64(x: np.ndarray, wh) -> np.ndarray:
    """cv2.resize(x, wh) on a float64 HxW map: fp32 weights, fp64 sums, rows first; one tap where the weight is 0"""
    w_out, h_out = int(wh[0]), int(wh[1])
    xs0, xs1, xa = linear_taps(w_out, x.shape[1])
    ys0, ys1, ya = linear_taps(h_out, x.shape[0])

    def lerp(v0, v1, a):
        a64 = a.astype(np.float64)
        b64 = (np.float32(1) - a).astype(np.float64)
        with np.errstate(invalid="ignore"):
            return np.where(a == 0, v0, v0 * b64 + v1 * a64)

    rows = lerp(x[:, xs0], x[:, xs1], xa[None, :])
    return lerp(rows[ys0], rows[ys1], ya[:, None])


def checker(h: int, w: int) -> np.ndarray:
    """CheckerPattern().draw(h, w), one channel: 169 where ((y - t) mod 64 < 32) == ((x - l) mod 64 < 32), else 214"""
    t, l = max(h - 64, 0) // 2, max(w - 64, 0) // 2
    yy = ((np.arange(h) - t) % 64 < 32)[:, None]
    xx = ((np.arange(w) - l) % 64 < 32)[None, :]
    return np.where(yy == xx, 169, 214).astype(np.uint8)


def normalize(x):
    with np.errstate(invalid="ignore", divide="ignore"):
        return (x - x.min()) / (x.max() - x.min())


def plane(d: np.ndarray, pts: np.ndarray) -> np.ndarray:
    """plane_fit.py: SVD of the centred samples (known x / y means), the smallest right singular vector, the plane image"""
    h, w = d.shape
    z = d[pts[:, 1], pts[:, 0]].astype(np.float64)
    mean = np.array([(w - 1) * 0.5, (h - 1) * 0.5, z.mean()])
    xyz = np.hstack((pts.astype(np.float64), z[:, None]))
    _, s, vt = np.linalg.svd(xyz - mean)
    nx, ny, nz = vt[np.argmin(s)]
    dd = -(nx * mean[0] + ny * mean[1] + nz * mean[2])
    ym, xm = np.mgrid[0:h, 0:w]
    return -(dd + nx * xm + ny * ym) / nz


def prepared(pred: torch.Tensor, target_wh=None) -> np.ndarray:
    """[h,w] map in its dtype -> scale_prediction (target_wh) -> remove_inf -> normalize_01 in that dtype -> fp32 numpy; torch arithmetic on the
    map's own device, as the reference runs it on the model's device"""
    t = pred.detach()[None]
    if target_wh is not None and (target_wh[1], target_wh[0]) != tuple(t.shape[1:]):
        t = F.interpolate(t[:, None], size=(target_wh[1], target_wh[0]), mode="bilinear")[:, 0]
    t = t.clone()
    t[t.isinf()] = 0
    return ((t - t.min()) / (t.max() - t.min())).float()[0].cpu().numpy()


def plane_removed_n(d: np.ndarray, pts: np.ndarray, f: float) -> np.ndarray:
    """n = normalize_01(d - f plane) in fp64 (a NaN map stays NaN)"""
    if not np.isfinite(d).all():
        return np.full(d.shape, np.nan)
    return normalize(d - plane(d, pts) * f)


def mask_of(v: np.ndarray, tmin: float, tmax: float, invert: bool) -> np.ndarray:
    with np.errstate(invalid="ignore"):
        m = np.where((v >= tmin) & (v <= tmax), 255, 0).astype(np.uint8)
    return 255 - m if invert else m


def display(pred: torch.Tensor, img: np.ndarray, target_wh, pts, f, tmin, tmax, invert):
    """-> (mask, composite, n in fp64) of the display loop"""
    n = plane_removed_n(prepared(pred, target_wh), pts, f)
    h, w = n.shape
    m = mask_of(n, tmin, tmax, invert)
    comp = np.where(m[:, :, None] == 255, resize_u8(img, (w, h)), checker(h, w)[:, :, None])
    return m, comp, n


def save(pred: torch.Tensor, img: np.ndarray, pts, f, tmin, tmax, invert):
    """-> (cutout BGRA, mask, s in fp64) of the save step at the photo's size"""
    n = plane_removed_n(prepared(pred), pts, f)
    s = resize_f64(n, (img.shape[1], img.shape[0]))
    m = mask_of(s, tmin, tmax, invert)
    cut = np.concatenate((np.where(m[:, :, None] == 255, img, 0), m[:, :, None]), axis=2).astype(np.uint8)
    return cut, m, s
