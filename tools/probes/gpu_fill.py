#!/usr/bin/env python3
"""Hole filling of rendered views (postprocess.fill_holes, depth-banded push-pull): the device call, its launches, and the routes without it.
  views   one 518x518 frame at the viewer's default mesh density (as tools/probes/gpu_render.py), rendered to 1280x720 and 1920x1080, 1 view (the
          start pose) and a 32-view swing: render_mesh's colour and depth are the inputs
  device  one postprocess.fill_holes call (colour and depth out), HIP events on the current stream (best of ROUNDS rounds of STEPS calls), output and
          scratch allocation included; the profiler's split over the launches from calls of its own; render_mesh alone and with fill_holes=
  bytes   the model of one call: the inputs read twice (8 bytes per pixel by the first push and again by the last pull), the outputs written once
          (8), the scratch written by the push and read by the pull (2 x 16 / 3) -> GB/s of the call's time, against HBM's rate
  torch   the same pyramid in torch on the device: masked avg_pool2d up, F.interpolate (bilinear) down, fp32, no depth band
  host    the numpy restatement (tests/fill_restate.py) on one 1280x720 view; the device on the same, compared on the safe pixels
Prints one JSON line (and writes it to --out PATH when given)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
from muggled_dpt_amd import native  # noqa: E402
from muggled_dpt_amd import orbit_camera as oc  # noqa: E402
from muggled_dpt_amd import postprocess as pp  # noqa: E402
from tests import fill_restate as fr  # noqa: E402

STEPS, ROUNDS, PROFILE_CALLS = 3, 3, 3
SIDE, BAND, HBM_GBPS = 518, 0.1, 8000.0


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


def torch_push_pull(color, depth):
    """[N,h,w,4] uint8, [N,h,w] fp32 -> filled colour uint8 [N,h,w,4], depth [N,h,w]: plain push-pull, every valid contributor kept"""
    valid = (color[..., 3] != 0) & (depth > 0) & torch.isfinite(depth)
    m = valid[:, None].float()
    x = torch.cat([color[..., :3].permute(0, 3, 1, 2).float(), torch.where(valid, depth, torch.zeros_like(depth))[:, None]], dim=1) * m
    levels = [(x, m)]
    while x.shape[-2:] != (1, 1):
        den = F.avg_pool2d(m, 2, ceil_mode=True)
        x = F.avg_pool2d(x * m, 2, ceil_mode=True) / den.clamp_min(1e-12)
        m = (den > 0).float()
        levels.append((x, m))
    up = levels[-1][0]
    for x, m in reversed(levels[:-1]):
        up = torch.where(m > 0, x, F.interpolate(up, size=x.shape[-2:], mode="bilinear", align_corners=False))
    out = torch.cat([torch.floor(up[:, :3] + 0.5).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1), torch.full_like(color[..., :1], 255)], dim=-1)
    return out, up[:, 3]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = {"probe": "gpu_fill", "source_hash": native.source_hash(), "device": torch.cuda.get_device_name(0), "gpus": 1, "frame_hw": [SIDE, SIDE],
           "band": BAND, "steps": STEPS, "rounds": ROUNDS, "hbm_GBps_assumed": HBM_GBPS, "cases": []}
    yy, xx = torch.meshgrid(torch.arange(float(SIDE)), torch.arange(float(SIDE)), indexing="ij")
    depth = (1 + 0.002 * xx + 0.3 * torch.sin(xx / 17) * torch.cos(yy / 23) + (xx > 300) * 0.4)[None].cuda()
    photo = np.random.default_rng(0).integers(0, 256, (SIDE, SIDE, 3), dtype=np.uint8)
    tex = torch.from_numpy(photo).cuda()
    xyz, uv, faces, counts, _ = pp.depth_frames_to_mesh(pp.pack_depth_u24_frames(depth), (SIDE, SIDE))
    lib = native.load()
    host_input = None
    for w, h in ((1280, 720), (1920, 1080)):
        for n_views in (1, 32):
            views = oc.viewer_view_proj(aspect=w / h)[None] if n_views == 1 else oc.swing_views(n_views, 8.0, 4.0, aspect=w / h)
            dviews = torch.from_numpy(views).cuda()
            color, vdepth = pp.render_mesh(xyz, uv, faces, counts, [tex], dviews, (w, h), return_depth=True)
            if host_input is None and n_views == 32:
                host_input = (color[0, 8].cpu().numpy(), vdepth[0, 8].cpu().numpy())

            def call():
                return pp.fill_holes(color, vdepth, BAND, return_depth=True)

            ms_fill = timed_device(call)
            ms_render = timed_device(lambda: pp.render_mesh(xyz, uv, faces, counts, [tex], dviews, (w, h), return_depth=True))
            ms_both = timed_device(lambda: pp.render_mesh(xyz, uv, faces, counts, [tex], dviews, (w, h), return_depth=True, fill_holes=BAND))
            ms_torch = timed_device(lambda: torch_push_pull(color[0], vdepth[0]))
            torch.cuda.synchronize()
            lib.mdpt_profile_enable(1)
            for _ in range(PROFILE_CALLS):
                call()
            torch.cuda.synchronize()
            buf = native.ctypes.create_string_buffer(1 << 16)
            lib.mdpt_profile_report(buf, len(buf))
            lib.mdpt_profile_enable(0)
            prof = {k["name"]: k["total_ms"] / PROFILE_CALLS for k in json.loads(buf.value.decode()).get("kernels", []) if k["name"].startswith("fill_")}
            filled = call()[0]
            t_c, _ = torch_push_pull(color[0], vdepth[0])
            holes = color[0][..., 3] == 0
            bytes_model = n_views * w * h * (2 * 8 + 8 + 2 * 16 / 3)
            res["cases"].append({
                "out_wh": [w, h], "views": n_views, "hole_share": round(float(holes.float().mean()), 4), "fill_holes_ms": round(ms_fill, 4),
                "ms_per_view": round(ms_fill / n_views, 4), "profile_ms": {k: round(v, 4) for k, v in prof.items()},
                "profile_sum_ms": round(sum(prof.values()), 4), "render_mesh_ms": round(ms_render, 4), "render_mesh_with_fill_ms": round(ms_both, 4),
                "fill_share_of_render": round((ms_both - ms_render) / ms_render, 3), "bytes_model": int(bytes_model),
                "GBps_of_call": round(bytes_model / (ms_fill * 1e-3) / 1e9, 1), "share_of_hbm_rate": round(bytes_model / (ms_fill * 1e-3) / 1e9 / HBM_GBPS, 3),
                "torch_push_pull_ms": round(ms_torch, 4), "torch_over_device": round(ms_torch / ms_fill, 2),
                "all_opaque": bool((filled[..., 3] == 255).all()),
                "torch_mean_abs_colour_diff_on_holes": round(float((t_c[holes][:, :3].float() - filled[0][holes][:, :3].float()).abs().mean()), 3)})
            del color, vdepth, filled
    c, d = host_input
    t0 = time.perf_counter()
    ref = fr.fill(c, d, BAND)
    host_s = time.perf_counter() - t0
    dc, dd = torch.from_numpy(c).cuda(), torch.from_numpy(d).cuda()
    ms_dev = timed_device(lambda: pp.fill_holes(dc, dd, BAND, return_depth=True))
    got_c, got_d = (t.cpu().numpy() for t in pp.fill_holes(dc, dd, BAND, return_depth=True))
    safe = ref["safe"]
    res["host"] = {"what": "numpy restatement (tests/fill_restate.py), one 1280x720 view of the swing", "host_ms": round(host_s * 1e3, 1),
                   "device_ms": round(ms_dev, 4), "speedup": round(host_s * 1e3 / ms_dev, 1), "unsafe_share": round(float((~safe).mean()), 6),
                   "equal_on_safe_pixels": bool((got_c[safe] == ref["color"][safe]).all() and
                                                (got_d.view(np.uint32)[safe] == ref["depth"].view(np.uint32)[safe]).all())}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
