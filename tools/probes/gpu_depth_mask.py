#!/usr/bin/env python3
"""Depth masking (the reference's experiments/depth_masking.py): device against host.
  display  B = 1 and B = 32 maps of 518x518 and 3840x2160 photos, to a 1920x1080 display.
           device: one postprocess.depth_mask_display call (plane removal 0.5, threshold (0.3, 0.8)): prep, fit, min/max, mask + checker composite
           host:   the numpy restatement per map (tests/mask_restate.py stands in for cv2.resize and CheckerPattern): device
                   resize + normalize, copy to the host, plane fit (SVD), plane removal, mask, uint8 photo resize, checker composite
  cutout   64 photos in the sizes of gpu_images_throughput.py (640x480, 1280x720, 1920x1080, 1080x1920, 3024x4032, 800x800, shuffled), each cut out
           at its own size from a 518x518 map.
           device: one postprocess.depth_mask_images call on host photos (pinned staging included) and on photos already on the device
           host:   the numpy restatement per photo: device normalize, copy to the host, plane fit, cv2.resize(CV_64F) restated, mask, BGRA cutout
Device steps are timed with HIP events on the current stream (best of ROUNDS rounds of STEPS calls); host steps once with perf_counter around the
whole loop, synchronised. Prints one JSON line (and writes it to --out PATH when given)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
from muggled_dpt_amd import native  # noqa: E402
from muggled_dpt_amd import postprocess as pp  # noqa: E402
from tests import mask_restate as mr  # noqa: E402

STEPS, ROUNDS = 3, 3
WH = (1920, 1080)
PHOTO_WH = [(640, 480), (1280, 720), (1920, 1080), (1080, 1920), (3024, 4032), (800, 800)]


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
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1000 * (time.perf_counter() - t0)


def host_display(pred, photos):
    for b in range(pred.shape[0]):
        dn = pp.normalize_01(pp.scale_prediction(pred[b:b + 1], WH)).cpu().numpy()[0]
        n = mr.normalize(dn - mr.plane(dn, pp.plane_sample_points(dn.shape)) * 0.5)
        m = mr.mask_of(n, 0.3, 0.8, False)
        _ = np.where(m[:, :, None] == 255, mr.resize_u8(photos[b], WH), mr.checker(WH[1], WH[0])[:, :, None])


def host_cutout(pred, photos):
    for img in photos:
        p = pp.normalize_01(pred).cpu().numpy()[0]
        n = mr.normalize(p - mr.plane(p, pp.plane_sample_points(p.shape)) * 0.5)
        s = mr.resize_f64(n, (img.shape[1], img.shape[0]))
        m = mr.mask_of(s, 0.3, 0.8, False)
        _ = np.concatenate((np.where(m[:, :, None] == 255, img, 0), m[:, :, None]), axis=2).astype(np.uint8)


def photo(h, w, rng):
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack(((x * 255 // max(w - 1, 1)), (y * 255 // max(h - 1, 1)), ((x + y) % 256)), axis=2).astype(np.uint8)
    return base ^ rng.integers(0, 8, (h, w, 3), dtype=np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    res = {"probe": "gpu_depth_mask", "source_hash": native.source_hash(), "display_wh": list(WH), "map_hw": [518, 518], "steps": STEPS,
           "rounds": ROUNDS, "host": "numpy restatement of the cv2 steps"}
    yy, xx = torch.meshgrid(torch.arange(518.0), torch.arange(518.0), indexing="ij")
    one = (1 + 0.002 * xx + 0.3 * torch.sin(xx / 17) * torch.cos(yy / 23))[None]
    for b in (1, 32):
        pred = one.repeat(b, 1, 1).cuda()
        pred += 0.01 * torch.rand_like(pred)
        photos = [photo(2160, 3840, rng)] * b
        photos_dev = torch.from_numpy(np.stack(photos)).cuda()
        res[f"display_device_ms_b{b}"] = round(timed_device(lambda: pp.depth_mask_display(pred, photos_dev, WH, 0.5, (0.3, 0.8))), 3)
        res[f"display_host_ms_b{b}"] = round(timed_host(lambda: host_display(pred, photos)), 3)
        print(json.dumps(res), flush=True)
    order = rng.permutation(64)
    sizes = [PHOTO_WH[k % len(PHOTO_WH)] for k in order]
    cache = {wh: photo(wh[1], wh[0], rng) for wh in PHOTO_WH}
    photos = [cache[wh] for wh in sizes]
    photos_dev = [torch.from_numpy(p).cuda() for p in photos]
    preds = [(one + 0.01 * torch.rand_like(one)).cuda() for _ in photos]
    mpx = sum(w * h for w, h in sizes) / 1e6
    res["cutout_photos"] = len(photos)
    res["cutout_megapixels"] = round(mpx, 2)
    res["cutout_device_ms_host_photos"] = round(timed_device(lambda: pp.depth_mask_images(preds, photos, 0.5, (0.3, 0.8))), 3)
    res["cutout_device_ms_device_photos"] = round(timed_device(lambda: pp.depth_mask_images(preds, photos_dev, 0.5, (0.3, 0.8))), 3)
    print(json.dumps(res), flush=True)
    res["cutout_host_ms"] = round(timed_host(lambda: host_cutout(preds[0], photos)), 3)
    # the cutout kernel alone: its share of the device call (bytes moved per photo: 3 in, 4 + 1 out per pixel)
    native.load().mdpt_profile_enable(1)
    pp.depth_mask_images(preds, photos_dev, 0.5, (0.3, 0.8))
    torch.cuda.synchronize()
    buf = native.ctypes.create_string_buffer(1 << 16)
    native.load().mdpt_profile_report(buf, len(buf))
    native.load().mdpt_profile_enable(0)
    for k in json.loads(buf.value.decode()).get("kernels", []):
        if k["name"] in ("mask_cutout_kernel", "mask_display_kernel", "disp_prep_kernel", "plane_fit_kernel", "plane_minmax_kernel"):
            res[f"profile_{k['name']}_ms"] = round(k["total_ms"], 3)
    if "profile_mask_cutout_kernel_ms" in res:
        res["cutout_kernel_GBps"] = round(mpx * 1e6 * 8 / (res["profile_mask_cutout_kernel_ms"] * 1e-3) / 1e9, 1)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
