#!/usr/bin/env python3
"""Fixtures of the depth masking demo (the reference's experiments/depth_masking.py), written to tests/golden/depth_mask.npz.

Runs the reference's own plane fit (demo_helpers/plane_fit.py), normalize_01 / scale_prediction / remove_inf_tensor (demo_helpers/postprocess.py)
and CheckerPattern (demo_helpers/toadui/helpers/checker_pattern.py) on a few small seeded depth maps and synthetic photos. The demo script opens a
window and cannot be imported, so what it does (display :189-199, :314-332; save :341-361) is restated step by step in display() and cutout(). cv2 is absent: an in-memory
stub carries what these modules call, restated from OpenCV's definitions:
  resize       INTER_LINEAR on CV_8U (fixed point: weights round(2048 w), integer row sums, (v + 2^21) >> 22 - the scalar path) and CV_64F
               (fp32 weights, fp64 sums, rows first); INTER_NEAREST_EXACT
  copyMakeBorder BORDER_WRAP;  cvtColor GRAY2BGR;  bitwise_and / bitwise_or / bitwise_not
INTER_LINEAR source taps per axis: p = float((d + 0.5) * (1 / (out / in)) - 0.5), s = floor(p), a = p - s in fp32; s < 0 -> s = 0, a = 0;
s >= in - 1 -> s = in - 1, a = 0. Only data is written.

usage: PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_depth_mask.py --reference PATH_TO_THE_REFERENCE_CHECKOUT
"""
from __future__ import annotations

import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.dont_write_bytecode = True

INTER_NEAREST, INTER_LINEAR, INTER_NEAREST_EXACT = 0, 1, 6
BORDER_WRAP = 3
COLOR_GRAY2BGR = 8


def _linear_taps(n_out: int, n_in: int):
    """cv2's per-axis INTER_LINEAR setup (resize.cpp): source index and fp32 weight of the second tap, one output position at a time"""
    scale = 1.0 / (float(n_out) / float(n_in))
    ofs = np.zeros(n_out, np.int64)
    alpha = np.zeros(n_out, np.float32)
    for d in range(n_out):
        f = np.float32((d + 0.5) * scale - 0.5)
        s = int(np.floor(f))
        f = np.float32(f - np.float32(s))
        if s < 0:
            f, s = np.float32(0.0), 0
        if s >= n_in - 1:
            f, s = np.float32(0.0), n_in - 1
        ofs[d] = s
        alpha[d] = f
    return ofs, alpha


def resize(src, dsize, interpolation=INTER_LINEAR):
    src = np.asarray(src)
    w_out, h_out = int(dsize[0]), int(dsize[1])
    h_in, w_in = src.shape[0:2]
    if interpolation == INTER_NEAREST_EXACT:
        ys = np.minimum(np.floor((np.arange(h_out) + 0.5) * (h_in / h_out)).astype(np.int64), h_in - 1)
        xs = np.minimum(np.floor((np.arange(w_out) + 0.5) * (w_in / w_out)).astype(np.int64), w_in - 1)
        return src[ys][:, xs].copy()
    assert interpolation == INTER_LINEAR, interpolation
    xo, xa = _linear_taps(w_out, w_in)
    yo, ya = _linear_taps(h_out, h_in)
    x1 = np.minimum(xo + 1, w_in - 1)
    y1 = np.minimum(yo + 1, h_in - 1)
    if src.dtype == np.uint8:
        s = src.astype(np.int64)
        ax1 = np.rint(xa * np.float32(2048)).astype(np.int64)
        ax0 = np.rint((np.float32(1) - xa) * np.float32(2048)).astype(np.int64)
        ay1 = np.rint(ya * np.float32(2048)).astype(np.int64)
        ay0 = np.rint((np.float32(1) - ya) * np.float32(2048)).astype(np.int64)
        ex = (slice(None),) + (None,) * (src.ndim - 1)
        rows = s[:, xo] * ax0[None, :][(...,) + (None,) * (src.ndim - 2)] + s[:, x1] * ax1[None, :][(...,) + (None,) * (src.ndim - 2)]
        out = (rows[yo] * ay0[ex] + rows[y1] * ay1[ex] + (1 << 21)) >> 22
        return np.clip(out, 0, 255).astype(np.uint8)
    assert src.dtype == np.float64 and src.ndim == 2, src.dtype
    out = np.empty((h_out, w_out), np.float64)
    rows = {}

    def row(r):  # the horizontal pass of one source row: S[sx] a0 + S[sx + 1] a1, one tap where a == 0 (cv2's border columns)
        if r not in rows:
            s = src[r]
            v = s[xo].copy()
            k = xa != 0
            v[k] = s[xo[k]] * (np.float32(1) - xa[k]).astype(np.float64) + s[x1[k]] * xa[k].astype(np.float64)
            rows[r] = v
        return rows[r]

    for d in range(h_out):
        a = ya[d]
        out[d] = row(yo[d]) if a == 0 else row(yo[d]) * np.float64(np.float32(1) - a) + row(y1[d]) * np.float64(a)
    return out


def copy_make_border(src, top, bottom, left, right, border_type):
    assert border_type == BORDER_WRAP
    return np.pad(src, ((top, bottom), (left, right)) + ((0, 0),) * (src.ndim - 2), mode="wrap")


def cvt_color(src, code):
    assert code == COLOR_GRAY2BGR, code
    return np.repeat(src[:, :, None], 3, axis=2)


cv2_stub = types.ModuleType("cv2")
cv2_stub.INTER_NEAREST, cv2_stub.INTER_LINEAR, cv2_stub.INTER_NEAREST_EXACT = INTER_NEAREST, INTER_LINEAR, INTER_NEAREST_EXACT
cv2_stub.BORDER_WRAP, cv2_stub.COLOR_GRAY2BGR = BORDER_WRAP, COLOR_GRAY2BGR
cv2_stub.resize = resize
cv2_stub.copyMakeBorder = copy_make_border
cv2_stub.cvtColor = cvt_color
cv2_stub.bitwise_and = np.bitwise_and
cv2_stub.bitwise_or = np.bitwise_or
cv2_stub.bitwise_not = np.bitwise_not

# map size, photo size, display size (w, h): an enlarged photo for the display and a reduced one, an unchanged one, and the reverse
CASES = (((61, 83), (90, 120), (100, 75)), ((64, 64), (64, 64), (64, 64)), ((97, 131), (45, 61), (131, 97)))
# (plane_removal, thresh_min, thresh_max, invert)
SETTINGS = ((0.0, 0.0, 1.0, False), (0.5, 0.4, 0.4, False), (1.0, 0.5, 1.0, False), (-0.5, 0.2, 0.7, False),
            (0.0, 0.5, 1.0, True), (0.5, 0.0, 1.0, True), (1.0, 0.4, 0.4, True), (-0.5, 0.5, 1.0, True))
CHECKER_SIZES = ((1, 1), (5, 9), (31, 64), (64, 64), (63, 65), (97, 131), (200, 130), (1, 300), (300, 1), (128, 129))
RESIZE_CASES = (((7, 5), (13, 11)), ((13, 11), (7, 5)), ((1, 9), (4, 17)), ((9, 1), (17, 4)), ((20, 30), (20, 30)), ((6, 6), (1, 1)), ((33, 17), (100, 3)))


def depth_map(h: int, w: int, seed: int) -> np.ndarray:
    """a tilted floor, a few blobs and noise (as gen_display_still.py draws them)"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    z = 2.0 + 0.03 * x - 0.02 * y + 0.001 * x * y / max(h, w)
    for _ in range(4):
        cy, cx, r = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(4, 14)
        z += rng.uniform(-1.5, 1.5) * np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2 * r * r))
    z += 0.02 * rng.standard_normal((h, w))
    return z.astype(np.float32)


def photo(h: int, w: int, seed: int) -> np.ndarray:
    """smooth colour ramps with a little noise: every byte value range, and it compresses"""
    rng = np.random.default_rng(100 + seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    bgr = np.stack((255 * x / max(w - 1, 1), 255 * y / max(h - 1, 1), 127.5 + 127.5 * np.sin((x + 2 * y) / 5.0)), axis=2)
    return np.clip(bgr + rng.integers(-3, 4, bgr.shape), 0, 255).astype(np.uint8)


def threshold_mask(v: np.ndarray, tmin: float, tmax: float) -> np.ndarray:
    """255 where tmin <= v <= tmax, else 0 (a NaN compares false)"""
    return np.where((v >= tmin) & (v <= tmax), 255, 0).astype(np.uint8)


def display(ref, prediction, img_bgr, display_wh, f, tmin, tmax, invert, seed, checker):
    """the demo's display steps for one image (depth_masking.py:189-199, 315-332) -> (mask, composite); np.random seeded for the plane fit"""
    np.random.seed(seed)
    resized = ref.pp.scale_prediction(prediction, display_wh)
    ref.pp.remove_inf_tensor(resized)  # (in place: the demo normalizes the resized map itself after this call)
    d = ref.pp.normalize_01(resized).float().cpu().numpy().squeeze()
    n = ref.pp.normalize_01(d - ref.plane_fit.estimate_plane_of_best_fit(d) * f)
    mask = threshold_mask(n, tmin, tmax)
    mask = ~mask if invert else mask
    return mask, checker.render_from_mask(resize(img_bgr, display_wh), mask)


def cutout(ref, prediction, img_bgr, f, tmin, tmax, invert, seed):
    """the demo's save steps for one image (depth_masking.py:343-361) at the photo's own size -> (mask, BGRA cutout)"""
    np.random.seed(seed)
    p = ref.pp.normalize_01(ref.pp.remove_inf_tensor(prediction, in_place=False)).float().cpu().numpy().squeeze()
    n = ref.pp.normalize_01(p - f * ref.plane_fit.estimate_plane_of_best_fit(p))
    ih, iw = img_bgr.shape[0:2]
    mask = threshold_mask(resize(n, (iw, ih)), tmin, tmax)
    mask = 255 - mask if invert else mask
    return mask, np.dstack((img_bgr & mask[:, :, None], mask))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of the reference project (muggled_dpt)")
    ref_path = ap.parse_args().reference
    sys.modules["cv2"] = cv2_stub
    sys.path.insert(0, ref_path)
    from muggled_dpt.demo_helpers import plane_fit
    from muggled_dpt.demo_helpers import postprocess as ref_pp
    ref = types.SimpleNamespace(pp=ref_pp, plane_fit=plane_fit)
    spec = importlib.util.spec_from_file_location("checker_pattern", os.path.join(ref_path, "muggled_dpt", "demo_helpers", "toadui", "helpers", "checker_pattern.py"))
    checker_mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(checker_mod)
    CheckerPattern = checker_mod.CheckerPattern

    out = {"settings": np.array(SETTINGS, dtype=np.float64)}
    checker = CheckerPattern()
    for h, w in CHECKER_SIZES:
        out[f"checker_{h}x{w}"] = checker.draw(h, w)[:, :, 0]
    rng = np.random.default_rng(5)
    for (ih, iw), (oh, ow) in RESIZE_CASES:
        src_u8 = rng.integers(0, 256, (ih, iw, 3), dtype=np.uint8)
        src_f64 = rng.standard_normal((ih, iw))
        out[f"resize_in_u8_{ih}x{iw}_{oh}x{ow}"] = src_u8
        out[f"resize_u8_{ih}x{iw}_{oh}x{ow}"] = resize(src_u8, (ow, oh))
        out[f"resize_in_f64_{ih}x{iw}_{oh}x{ow}"] = src_f64
        out[f"resize_f64_{ih}x{iw}_{oh}x{ow}"] = resize(src_f64, (ow, oh))

    for i, ((h, w), (ih, iw), display_wh) in enumerate(CASES):
        d = depth_map(h, w, i)
        img_bgr = photo(ih, iw, i)
        out[f"map{i}"] = d
        out[f"photo{i}"] = img_bgr
        out[f"display_wh{i}"] = np.array(display_wh, dtype=np.int32)
        prediction = torch.from_numpy(d)[None]
        for j, (f, thresh_min, thresh_max, invert) in enumerate(SETTINGS):
            seed = 10 * i + j
            mask, composite = display(ref, prediction, img_bgr, display_wh, f, thresh_min, thresh_max, invert, seed, checker)
            out[f"case{i}_{j}_display_seed"] = np.int64(seed)
            out[f"case{i}_{j}_display_mask"] = mask
            out[f"case{i}_{j}_display_composite"] = composite
            mask, cut = cutout(ref, prediction, img_bgr, f, thresh_min, thresh_max, invert, seed + 1000)
            out[f"case{i}_{j}_save_seed"] = np.int64(seed + 1000)
            out[f"case{i}_{j}_save_mask"] = mask
            out[f"case{i}_{j}_save_cutout"] = cut
    path = os.path.join(REPO, "tests", "golden", "depth_mask.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes, {len(out)} arrays)")


if __name__ == "__main__":
    main()
