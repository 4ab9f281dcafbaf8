#!/usr/bin/env python3
"""Tiled high-resolution inference (DPTModel.inference_tiled / postprocess.stitch_tiles): device against the routes without it.
  model   ViT-L (synthetic weights), bf16, model tensor 504 x 504
  photos  3024 x 4032 (H x W) uint8 on the device, grids of 4 x 3 and 8 x 6 tiles, overlap 0.25
  fit / blend  the profiler's time of the fit launches (partials + solve) and of the blend launch alone, per call
  stitch       one postprocess.stitch_tiles call on maps that exist already, HIP events (best of ROUNDS rounds of STEPS calls), allocation included
  tiled        the whole DPTModel.inference_tiled call: one inference_regions call of 1 + T regions, then the stitch
  torch        the route without the feature on the same maps: F.interpolate of every tile to its box, the same feather weights built with torch,
               weighted accumulation and the division, all in fp32 on the device; no scale / shift fit (torch.linalg.lstsq per tile would come on top)
  host         the fp64 numpy restatement (tests/tile_restate.py stitch) on maps already on the host, perf_counter, one run
  blend GB/s   (photo bytes written + tile-map bytes read) / blend time, against HBM's 8 TB/s: the useful traffic of a kernel whose arithmetic is
               fp64 per pixel and tile (two cv2 tap computations, three lerps, the affine map, two weights, two accumulations)
Output quality on real photographs is NOT measured here: no checkpoint can be loaded, the weights are synthetic.
Prints one JSON line (and writes it to --out PATH when given)."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
from muggled_dpt_amd import make_depthanythingv2_dpt_from_original_state_dict, native, tiling  # noqa: E402
from muggled_dpt_amd import postprocess as pp  # noqa: E402
from muggled_dpt_amd.synthetic import make_synthetic_original_state_dict  # noqa: E402
from tests import tile_restate as tr  # noqa: E402

STEPS, ROUNDS, PROFILE_CALLS = 3, 3, 5
PHOTO_HW, SIDE, OVERLAP = (3024, 4032), 504, 0.25
HBM_GBS = 8000.0


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


def profiled(fn, calls):
    """-> {kernel name: ms per call} from the library's per-launch event profiler"""
    lib = native.load()
    torch.cuda.synchronize()
    lib.mdpt_profile_enable(1)
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    buf = ctypes.create_string_buffer(1 << 16)
    lib.mdpt_profile_report(buf, len(buf))
    lib.mdpt_profile_enable(0)
    return {k["name"]: k["total_ms"] / calls for k in json.loads(buf.value.decode())["kernels"]}


def torch_route(maps, boxes, hw, feather):
    """the route without the feature, on the device in fp32: resize every tile to its box, feather weights, weighted accumulation"""
    dev = maps[0].device
    num = torch.zeros(hw, device=dev)
    den = torch.zeros(hw, device=dev)
    H, W = hw

    def axis(lo, hi, n):
        c = torch.arange(lo, hi, device=dev, dtype=torch.float32)
        d = torch.full_like(c, float("inf"))
        if lo > 0:
            d = torch.minimum(d, c - lo)
        if hi < n:
            d = torch.minimum(d, (hi - 1) - c)
        return torch.clamp((d + 1) / (feather + 1), max=1.0)

    for m, (x1, y1, x2, y2) in zip(maps, boxes):
        val = F.interpolate(m.float()[None], size=(y2 - y1, x2 - x1), mode="bilinear")[0, 0]
        w = axis(y1, y2, H)[:, None] * axis(x1, x2, W)[None, :]
        num[y1:y2, x1:x2] += w * val
        den[y1:y2, x1:x2] += w
    return (num / den)[None]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip_host", action="store_true", help="leave the numpy restatement out (it takes the longest)")
    args = ap.parse_args()
    _, model = make_depthanythingv2_dpt_from_original_state_dict(make_synthetic_original_state_dict("vitl", 0))
    model = model.to("cuda", torch.bfloat16)
    yy, xx = np.mgrid[:PHOTO_HW[0], :PHOTO_HW[1]]
    base = 128 + 90 * np.sin(yy / 310.0) * np.cos(xx / 170.0)
    photo = np.clip(base[:, :, None] + np.random.default_rng(0).normal(0, 10, (*PHOTO_HW, 3)), 0, 255).astype(np.uint8)
    dev_photo = torch.from_numpy(photo).cuda()
    res = {"probe": "gpu_tiled", "source_hash": native.source_hash(), "device": torch.cuda.get_device_name(0), "gpus": 1, "model": "vitl synthetic bf16",
           "photo_hw": list(PHOTO_HW), "model_side": SIDE, "overlap": OVERLAP, "steps": STEPS, "rounds": ROUNDS,
           "quality_on_photographs": "not verified: synthetic weights, no checkpoint can be loaded", "cases": []}
    for grid in ((4, 3), (8, 6)):
        boxes = tiling.tile_grid_boxes(PHOTO_HW, grid, OVERLAP)
        feather = float(tiling.smallest_overlap(boxes))
        regions = [(0, 0, 0, PHOTO_HW[1], PHOTO_HW[0])] + [(0, *b) for b in boxes]
        maps = model.inference_regions([dev_photo], regions, SIDE)
        guide, tiles = maps[0], maps[1:]
        stitch = lambda: pp.stitch_tiles(tiles, boxes, PHOTO_HW, guide=guide)  # noqa: E731
        ms_stitch = timed_device(stitch)
        ms_regions = timed_device(lambda: model.inference_regions([dev_photo], regions, SIDE))
        ms_tiled = timed_device(lambda: model.inference_tiled(dev_photo, tiles=grid, overlap=OVERLAP, max_side_length=SIDE))
        ms_torch = timed_device(lambda: torch_route(tiles, boxes, PHOTO_HW, feather))
        prof = profiled(stitch, PROFILE_CALLS)
        ms_fit = prof.get("tile_fit_partial_kernel", 0.0) + prof.get("tile_fit_solve_kernel", 0.0)
        ms_blend = prof.get("tile_blend_kernel", 0.0)
        useful = PHOTO_HW[0] * PHOTO_HW[1] * 4 + sum(m.numel() * m.element_size() for m in tiles)
        case = {"grid": list(grid), "tiles": len(boxes), "tile_box_hw": [boxes[0][3] - boxes[0][1], boxes[0][2] - boxes[0][0]], "feather": feather,
                "fit_ms": round(ms_fit, 4), "blend_ms": round(ms_blend, 4), "stitch_call_ms": round(ms_stitch, 4),
                "inference_regions_ms": round(ms_regions, 3), "inference_tiled_ms": round(ms_tiled, 3), "torch_resize_accumulate_ms": round(ms_torch, 3),
                "blend_useful_bytes": useful, "blend_gb_s": round(useful / ms_blend / 1e6, 1) if ms_blend else None,
                "blend_share_of_hbm": round(useful / ms_blend / 1e6 / HBM_GBS, 4) if ms_blend else None}
        got = stitch()
        ref32 = torch_route(tiles, boxes, PHOTO_HW, feather)
        fit = pp.stitch_tiles(tiles, boxes, PHOTO_HW, guide=guide, return_fit=True)[1]
        case["fit_scale_range"] = [float(fit[:, 0].min()), float(fit[:, 0].max())]
        case["max_abs_diff_to_unaligned_torch_route"] = float((got - ref32).abs().max())
        if not args.skip_host and grid == (4, 3):
            host_maps = [m[0].float().cpu().numpy() for m in tiles]
            host_guide = guide[0].float().cpu().numpy()
            t0 = time.perf_counter()
            want = tr.stitch(host_maps, boxes, PHOTO_HW, host_guide, feather)[0]
            case["host_numpy_restatement_ms"] = round(1000 * (time.perf_counter() - t0), 1)
            g = got[0].cpu().numpy()
            same_nan = bool(np.array_equal(np.isnan(g), np.isnan(want)))
            case["max_ulp_to_restatement"] = int(np.abs(g.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64)).max()) if same_nan else -1
        res["cases"].append(case)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
