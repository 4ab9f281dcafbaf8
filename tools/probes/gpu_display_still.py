#!/usr/bin/env python3
"""Still-image display tail and 24-bit edge frames: device against host, at a 1920x1080 display size for B = 1 and B = 32 maps of 518x518.
  display  device: one postprocess.depth_to_display call (resize, plane removal 0.5, threshold (0.1, 0.9), high contrast, reverse, a LUT)
           host:   the reference's numpy path per map (run_image.py:185-195, 323-343): device resize + normalize, copy to the host, plane fit
                   (SVD), plane removal, threshold, round, thresholded histogram equalization, reverse, LUT
  u24      device: one postprocess.pack_depth_u24_frames call (edge alpha), at 518x518
           host:   the viewer's path per map: pack_depth_u24 on the device plus its torch edge filters on the device, both copied back
Device steps are timed with HIP events on the current stream (best of ROUNDS rounds of STEPS calls); host steps with perf_counter around
the whole per-map loop, synchronised. Prints one JSON line (and writes it to --out PATH when given)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
from torch import nn

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
from muggled_dpt_amd import native  # noqa: E402
from muggled_dpt_amd import postprocess as pp  # noqa: E402

STEPS, ROUNDS = 3, 3
WH = (1920, 1080)


def timed_device(fn):
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(ROUNDS):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(STEPS):
            fn()
        t1.record()
        t1.synchronize()
        best = min(best, t0.elapsed_time(t1) / STEPS)
    return best


def timed_host(fn):
    fn()
    best = float("inf")
    for _ in range(ROUNDS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, 1000 * (time.perf_counter() - t0))
    return best


def host_plane(d):
    h, w = d.shape
    pts = pp.plane_sample_points((h, w))
    z = d[pts[:, 1], pts[:, 0]].astype(np.float64)
    mean = np.array([(w - 1) * 0.5, (h - 1) * 0.5, z.mean()])
    _, s, vt = np.linalg.svd(np.hstack((pts.astype(np.float64), z[:, None])) - mean)
    nx, ny, nz = vt[np.argmin(s)]
    dd = -(nx * mean[0] + ny * mean[1] + nz * mean[2])
    ym, xm = np.mgrid[0:h, 0:w]
    return -(dd + nx * xm + ny * ym) / nz


def host_display(pred, lut):
    for b in range(pred.shape[0]):
        dn = pp.normalize_01(pp.scale_prediction(pred[b:b + 1], WH)).cpu().numpy()[0]
        v = dn - host_plane(dn) * 0.5
        v = (v - v.min()) / (v.max() - v.min())
        u8 = np.round(255.0 * np.clip((v - 0.1) / 0.8, 0.0, 1.0)).astype(np.uint8)
        counts, _ = np.histogram(u8, 1 + 230 - 26, range=(26, 230))
        cdf = counts.cumsum()
        cdf_u8 = np.uint8(255 * ((cdf - cdf.min()) / float(max(cdf.max() - cdf.min(), 1))))
        u8 = np.concatenate((np.zeros(26, np.uint8), cdf_u8, np.full(25, 255, np.uint8)))[u8]
        _ = lut[255 - u8]


def viewer_filters(dev):
    g = torch.exp(-torch.sum(torch.square(torch.stack(torch.meshgrid(*(torch.linspace(-2, 2, 5),) * 2, indexing="ij"))) * 0.01, dim=0))
    blur = nn.Conv2d(1, 1, 5, padding=2, padding_mode="reflect", bias=False)
    blur.weight = nn.Parameter((g / g.max())[None, None])
    sdy = torch.tensor([[[[3, 10, 3], [0, 0, 0], [-3, -10, -3]]]], dtype=torch.float32)
    sobel = nn.Conv2d(1, 2, 3, padding=1, padding_mode="reflect", bias=False)
    sobel.weight = nn.Parameter(torch.cat((sdy.transpose(2, 3), sdy), dim=0))
    return blur.to(dev).requires_grad_(False), sobel.to(dev).requires_grad_(False)


def host_u24(pred, blur, sobel):
    for b in range(pred.shape[0]):
        frame = pp.pack_depth_u24(pred[b:b + 1]).cpu().numpy()
        dn = pp.normalize_01(pred[b:b + 1])
        with torch.no_grad():
            mag = torch.sqrt(torch.sum(torch.square(sobel(blur(dn))), dim=0))
        frame[..., 3] = torch.bitwise_not(torch.round(255 * mag / mag.max()).byte()).cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.manual_seed(0)
    lut = np.random.default_rng(0).integers(0, 256, (256, 3), dtype=np.uint8)
    blur, sobel = viewer_filters("cuda")
    res = {"probe": "gpu_display_still", "source_hash": native.source_hash(), "display_wh": list(WH), "map_hw": [518, 518], "steps": STEPS,
           "rounds": ROUNDS}
    for b in (1, 32):
        yy, xx = torch.meshgrid(torch.arange(518.0), torch.arange(518.0), indexing="ij")
        pred = (1 + 0.002 * xx + 0.3 * torch.sin(xx / 17) * torch.cos(yy / 23))[None].repeat(b, 1, 1).cuda()
        pred += 0.01 * torch.rand_like(pred)
        res[f"display_device_ms_b{b}"] = round(timed_device(lambda: pp.depth_to_display(pred, WH, 0.5, (0.1, 0.9), True, True, lut)), 3)
        res[f"display_host_ms_b{b}"] = round(timed_host(lambda: host_display(pred, lut)), 3)
        res[f"u24_device_ms_b{b}"] = round(timed_device(lambda: pp.pack_depth_u24_frames(pred)), 3)
        res[f"u24_host_ms_b{b}"] = round(timed_host(lambda: host_u24(pred, blur, sobel)), 3)
        print(json.dumps(res), flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
