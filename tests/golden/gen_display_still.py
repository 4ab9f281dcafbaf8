#!/usr/bin/env python3
"""Fixtures of the still-image display tail and the 3D viewer's edge alpha (build container only: imports /root/reference).

Runs the reference's own plane fit (demo_helpers/plane_fit.py) and the display loop of its still-image demo (run_image.py:185-195, 323-343,
350-358: scale_prediction, remove_inf_tensor, normalize_01, estimate_plane_of_best_fit, the threshold window, histogram_equalization) on a few
small seeded depth maps, and writes the results to tests/golden/display_still.npz. The viewer script cannot be imported (it starts a server), so
its edge filters (run_3dviewer.py:455-505) are restated here with torch's Conv2d on the CPU. cv2 is absent: an in-memory stub carries
equalizeHist, restated from its definition. Only data is written.

usage: PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_display_still.py
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch
from torch import nn

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = "/root/reference"
sys.dont_write_bytecode = True


def equalize_hist(x: np.ndarray) -> np.ndarray:
    """cv2.equalizeHist: first non-empty bin i; a single-valued image stays i; else lut[j] = round(float(cumsum bins i+1..j) * (255.f / (total - hist[i])))"""
    hist = np.bincount(x.ravel(), minlength=256)
    i = int(np.flatnonzero(hist)[0])
    if hist[i] == x.size:
        return np.full_like(x, i)
    scale = np.float32(255.0) / np.float32(x.size - hist[i])
    lut = np.zeros(256, np.uint8)
    s = 0
    for j in range(i + 1, 256):
        s += int(hist[j])
        lut[j] = np.clip(np.rint(np.float32(s) * scale), 0, 255)
    return lut[x]


cv2_stub = types.ModuleType("cv2")
cv2_stub.equalizeHist = equalize_hist
sys.modules["cv2"] = cv2_stub
sys.path.insert(0, REF)

from muggled_dpt.demo_helpers import plane_fit  # noqa: E402
from muggled_dpt.demo_helpers import postprocess as ref_pp  # noqa: E402

MAP_SIZES = ((61, 83), (64, 64), (97, 131))
SAMPLE_SIZES = MAP_SIZES + ((5, 9), (12, 3), (1, 20), (16, 16), (40, 7))
SEEDS = (0, 1, 7)
# (plane_removal, thresh_min, thresh_max, reverse, high_contrast)
SETTINGS = ((0.0, 0.0, 1.0, False, False), (0.5, 0.1, 0.8, True, False), (1.0, 0.0, 1.0, True, True), (0.75, 0.2, 0.7, False, True),
            (0.3, 0.4, 0.4, True, True))
SCALED_SETTINGS = SAVING_SETTINGS = (1, 2)
DISPLAY_WH = (150, 110)  # the display size of the resized case (w, h)
EDGE_CASES = ((3, 1.0), (5, 1.0), (7, 1.0), (5, 0.5), (5, 2.0))


def depth_map(h: int, w: int, seed: int) -> np.ndarray:
    """a tilted floor, a few blobs and noise: something with a plane, edges and a skewed histogram"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    z = 2.0 + 0.03 * x - 0.02 * y + 0.001 * x * y / max(h, w)
    for _ in range(4):
        cy, cx, r = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(4, 14)
        z += rng.uniform(-1.5, 1.5) * np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2 * r * r))
    z += 0.02 * rng.standard_normal((h, w))
    return z.astype(np.float32)


def edges(depth: np.ndarray, k: int, bw: float) -> np.ndarray:
    """run_3dviewer.py:455-505 restated: Gaussian blur and Sobel, Conv2d(padding_mode="reflect"), ~round(255 mag / max)"""
    ks_pad = k // 2
    ksize = 1 + 2 * ks_pad
    idx = torch.linspace(-ks_pad, ks_pad, ksize, dtype=torch.float32)
    xy = torch.stack(torch.meshgrid(idx, idx, indexing="ij"))
    g = torch.exp(-torch.sum(torch.square(xy) * (0.01 / bw), dim=0))
    blur = nn.Conv2d(1, 1, kernel_size=ksize, padding=ks_pad, padding_mode="reflect", bias=False)
    blur.weight = nn.Parameter((g / g.max())[None, None])
    sdy = torch.tensor([[[[3, 10, 3], [0, 0, 0], [-3, -10, -3]]]], dtype=torch.float32)
    sobel = nn.Conv2d(1, 2, kernel_size=3, padding=1, padding_mode="reflect", bias=False)
    sobel.weight = nn.Parameter(torch.cat((sdy.transpose(2, 3), sdy), dim=0))
    with torch.no_grad():
        d = torch.from_numpy(depth)[None]
        dxdy = sobel(blur(d))
        mag = torch.sqrt(torch.sum(torch.square(dxdy), dim=0))
        return torch.bitwise_not(torch.round(255 * mag / mag.max()).byte()).numpy()


def display(prediction: torch.Tensor, scaled_wh, f, tmin, tmax, reverse, high_contrast, seed, lut):
    """run_image.py's loop for one image (post_process_prediction, then the plane / threshold / colormap steps), with np.random seeded"""
    np.random.seed(seed)
    scaled = ref_pp.scale_prediction(prediction, scaled_wh)
    ref_pp.remove_inf_tensor(scaled)
    depth_norm = ref_pp.normalize_01(scaled).float().cpu().numpy().squeeze()
    plane = plane_fit.estimate_plane_of_best_fit(depth_norm)
    depth_1ch = ref_pp.normalize_01(depth_norm - (plane * f))
    delta = max(0.001, tmax - tmin)
    u8 = np.round(255.0 * np.clip((depth_1ch - tmin) / delta, 0.0, 1.0)).astype(np.uint8)
    if high_contrast:
        u8 = ref_pp.histogram_equalization(u8, tmin, tmax)
    if reverse:
        u8 = 255 - u8
    return lut[u8]


def for_saving(prediction: torch.Tensor, f, tmin, tmax, reverse, seed):
    np.random.seed(seed)
    npy = ref_pp.remove_inf_tensor(prediction.clone())
    npy = ref_pp.normalize_01(npy).float().cpu().numpy().squeeze()
    npy = npy - (f * plane_fit.estimate_plane_of_best_fit(npy))
    npy = ref_pp.normalize_01(npy)
    npy = np.clip((npy - tmin) / max(0.001, tmax - tmin), 0.0, 1.0)
    return 1.0 - npy if reverse else npy


def main():
    out = {}
    v = np.arange(256)
    lut = np.stack((v, 255 - v, (v * 7) % 256), axis=1).astype(np.uint8)  # BGR, no two entries alike
    out["lut"] = lut
    out["settings"] = np.array(SETTINGS, dtype=np.float64)
    out["display_wh"] = np.array(DISPLAY_WH, dtype=np.int32)
    out["edge_cases"] = np.array(EDGE_CASES, dtype=np.float64)
    for i, (h, w) in enumerate(SAMPLE_SIZES):
        for s in SEEDS:
            np.random.seed(s)
            xyz, _ = plane_fit.get_xyz_samples(np.zeros((h, w), np.float32), 16, 16)
            out[f"points_{h}x{w}_seed{s}"] = xyz[:, :2].astype(np.int32)
    for i, (h, w) in enumerate(MAP_SIZES):
        d = depth_map(h, w, i)
        out[f"map{i}"] = d
        for s in SEEDS[:2]:
            np.random.seed(s)
            out[f"map{i}_plane_seed{s}"] = plane_fit.estimate_plane_of_best_fit(d).astype(np.float32)
        dn = ref_pp.normalize_01(torch.from_numpy(d)).numpy()
        for k, bw in EDGE_CASES:
            out[f"map{i}_edges_k{k}_w{bw:g}"] = edges(dn, k, bw)
        pred = torch.from_numpy(d)[None]
        for j, (f, tmin, tmax, rev, hc) in enumerate(SETTINGS):
            seed = 10 * i + j
            out[f"map{i}_display{j}"] = display(pred, (w, h), f, tmin, tmax, rev, hc, seed, lut)
            if j in SCALED_SETTINGS:
                out[f"map{i}_display{j}_scaled"] = display(pred, DISPLAY_WH, f, tmin, tmax, rev, hc, seed + 100, lut)
            if j in SAVING_SETTINGS:
                out[f"map{i}_saving{j}"] = for_saving(pred, f, tmin, tmax, rev, seed + 200).astype(np.float32)
    path = os.path.join(REPO, "tests", "golden", "display_still.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes, {len(out)} arrays)")


if __name__ == "__main__":
    main()
