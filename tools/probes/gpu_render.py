#!/usr/bin/env python3
"""Rendering of depth meshes (the reference's 3D viewer draws them with WebGL in a browser): the device call, its four launches, and what a headless
node has without it.
  mesh    one 518x518 frame from postprocess.pack_depth_u24_frames (24-bit depth, edge alpha) at the viewer's default density
          (MESH_TARGET_FACES), photo 518x518 as the texture, the viewer's start controls
  views   1 view (the start pose) and a 32-view swing, rendered to 1280x720 and 1920x1080
  device  one postprocess.render_mesh call (clear, vertex stage, raster, resolve), HIP events on the current stream (best of ROUNDS rounds of
          STEPS calls), output and scratch allocation included; the profiler's split over the four launches
  raster  fragments tested = the pixels of the kept, unculled faces' clipped bounding boxes (from a torch restatement of the vertex stage, which
          is also the torch comparison below); per output pixel that is the overdraw. Every tested fragment costs three int64 edge functions; a
          covered one whose key is below the z-buffer's word issues one 64-bit atomic min. The atomics themselves are not counted (no counter run):
          tested fragments per second bound them from above. zbuf bytes = 8 per pixel and view, against the raster launch's time.
  torch   the vertex stage only - the matrix product, the divide and the snap, fp64, the part torch can express - for the same mesh and views
  host    the numpy restatement (tests/render_restate.py) on a case it can finish: a HOST_FACES-face mesh, one view, HOST_WH; the device on the same
Prints one JSON line (and writes it to --out PATH when given)."""
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
from muggled_dpt_amd import orbit_camera as oc  # noqa: E402
from muggled_dpt_amd import postprocess as pp  # noqa: E402
from tests import render_restate as rr  # noqa: E402

STEPS, ROUNDS, PROFILE_CALLS = 3, 3, 3
SIDE, HOST_FACES, HOST_WH = 518, 20_000, (320, 180)


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


def torch_vertex_stage(xyz, views, w, h):
    """[nv,3] fp32, [V,16] fp64 on the device -> snapped x, y int64 [V,nv] (unusable: x = -2^31), 1 / w, z01"""
    p = torch.cat([xyz.double(), torch.ones_like(xyz[:, :1], dtype=torch.float64)], dim=1)
    clip = p @ views.reshape(-1, 4, 4)
    cw = clip[..., 3]
    sx = torch.round((clip[..., 0] / cw + 1.0) * 0.5 * w * 256.0)
    sy = torch.round((1.0 - clip[..., 1] / cw) * 0.5 * h * 256.0)
    ok = (cw > 0) & (sx.abs() < 2.0 ** 30) & (sy.abs() < 2.0 ** 30)
    return torch.where(ok, sx, torch.full_like(sx, -2.0 ** 31)).long(), torch.where(ok, sy, torch.zeros_like(sy)).long(), 1.0 / cw, (clip[..., 2] / cw + 1.0) * 0.5


def fragments_tested(xyz, faces, views, w, h):
    X, Y, _, _ = torch_vertex_stage(xyz, views, w, h)
    f = faces.long()
    xs, ys = X[:, f], Y[:, f]  # [V,nf,3]
    usable = (xs != -2 ** 31).all(dim=-1)
    area = (xs[..., 1] - xs[..., 0]) * (ys[..., 2] - ys[..., 0]) - (ys[..., 1] - ys[..., 0]) * (xs[..., 2] - xs[..., 0])
    x0, x1 = ((xs.amin(-1) + 127) >> 8).clamp(min=0), ((xs.amax(-1) - 128) >> 8).clamp(max=w - 1)
    y0, y1 = ((ys.amin(-1) + 127) >> 8).clamp(min=0), ((ys.amax(-1) - 128) >> 8).clamp(max=h - 1)
    box = (x1 - x0 + 1).clamp(min=0) * (y1 - y0 + 1).clamp(min=0)
    box = torch.where(usable & (area < 0), box, torch.zeros_like(box))
    return int(box.sum()), int((box > rr.SMALL_BOX).sum()), int(((box > 0) & (box <= rr.SMALL_BOX)).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = {"probe": "gpu_render", "source_hash": native.source_hash(), "device": torch.cuda.get_device_name(0), "gpus": 1, "frame_hw": [SIDE, SIDE],
           "steps": STEPS, "rounds": ROUNDS, "cases": []}
    yy, xx = torch.meshgrid(torch.arange(float(SIDE)), torch.arange(float(SIDE)), indexing="ij")
    depth = (1 + 0.002 * xx + 0.3 * torch.sin(xx / 17) * torch.cos(yy / 23) + (xx > 300) * 0.4)[None].cuda()
    photo = np.random.default_rng(0).integers(0, 256, (SIDE, SIDE, 3), dtype=np.uint8)
    tex = torch.from_numpy(photo).cuda()
    frames = pp.pack_depth_u24_frames(depth)
    xyz, uv, faces, counts, _ = pp.depth_frames_to_mesh(frames, (SIDE, SIDE))
    kv, kf = counts[0].tolist()
    res["mesh"] = {"target_faces": pp.MESH_TARGET_FACES, "vertices": kv, "faces": kf}
    lib = native.load()
    for w, h in ((1280, 720), (1920, 1080)):
        for n_views in (1, 32):
            views = oc.viewer_view_proj(aspect=w / h)[None] if n_views == 1 else oc.swing_views(n_views, 8.0, 4.0, aspect=w / h)
            dviews = torch.from_numpy(views).cuda()

            def call():
                return pp.render_mesh(xyz, uv, faces, counts, [tex], dviews, (w, h))

            ms_call = timed_device(call)
            torch.cuda.synchronize()
            lib.mdpt_profile_enable(1)
            for _ in range(PROFILE_CALLS):
                call()
            torch.cuda.synchronize()
            buf = native.ctypes.create_string_buffer(1 << 16)
            lib.mdpt_profile_report(buf, len(buf))
            lib.mdpt_profile_enable(0)
            prof = {k["name"]: k["total_ms"] / PROFILE_CALLS for k in json.loads(buf.value.decode()).get("kernels", []) if k["name"].startswith("render_")}
            tested, big, small = fragments_tested(xyz[0, :kv], faces[0, :kf], dviews, w, h)
            ms_torch = timed_device(lambda: torch_vertex_stage(xyz[0, :kv], dviews, w, h))
            color = call()
            raster = prof.get("render_raster_kernel")
            case = {"out_wh": [w, h], "views": n_views, "render_mesh_ms": round(ms_call, 4), "ms_per_view": round(ms_call / n_views, 4),
                    "profile_ms": {k: round(v, 4) for k, v in prof.items()}, "covered_share": round(float((color[..., 3] > 0).float().mean()), 4),
                    "fragments_tested": tested, "overdraw_tested_per_pixel": round(tested / (n_views * w * h), 3), "faces_cooperative": big,
                    "faces_single_lane": small, "zbuf_bytes": 8 * n_views * w * h, "torch_vertex_stage_ms": round(ms_torch, 4),
                    "device_vertex_stage_ms": round(prof.get("render_vertex_kernel", float("nan")), 4)}
            if raster:
                case["fragments_tested_per_s"] = round(tested / (raster * 1e-3), 1)
                case["zbuf_GBps_of_raster_time"] = round(8 * n_views * w * h / (raster * 1e-3) / 1e9, 2)
            res["cases"].append(case)
            del color
    # the host: the numpy restatement on a case it can finish
    hx, hu, hf, hc, _ = pp.depth_frames_to_mesh(frames, (SIDE, SIDE), target_num_faces=HOST_FACES)
    hv, hk = hc[0].tolist()
    view = oc.viewer_view_proj(aspect=HOST_WH[0] / HOST_WH[1])
    t0 = time.perf_counter()
    ref = rr.render(hx[0, :hv].cpu().numpy(), hu[0, :hv].cpu().numpy(), hf[0, :hk].cpu().numpy(), photo, view, HOST_WH)
    host_s = time.perf_counter() - t0
    ms_dev = timed_device(lambda: pp.render_mesh(hx, hu, hf, hc, [tex], view[None], HOST_WH))
    got = pp.render_mesh(hx, hu, hf, hc, [tex], view[None], HOST_WH, return_face_ids=True)[1][0, 0].cpu().numpy()
    res["host"] = {"what": "numpy restatement (tests/render_restate.py), one view", "faces": hk, "out_wh": list(HOST_WH), "host_ms": round(host_s * 1e3, 1),
                   "device_ms": round(ms_dev, 4), "speedup": round(host_s * 1e3 / ms_dev, 1),
                   "face_ids_equal_on_safe_pixels": bool((got[ref["safe"]] == ref["ids"][ref["safe"]]).all())}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
