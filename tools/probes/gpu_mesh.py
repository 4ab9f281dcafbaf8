#!/usr/bin/env python3
"""Depth-to-mesh export (the reference's 3D viewer "Save 3D Model", JavaScript on the CPU there): device against host.
  frames  B = 1 and B = 32 frames of 518x518 from postprocess.pack_depth_u24_frames (24-bit depth, edge alpha), photo 518x518, edge threshold 0.503
  grids   the viewer's grid for about 250 k and 2 M target faces
  device  one postprocess.depth_frames_to_mesh call (five launches: flags, face counts, scan, vertices, faces), timed with HIP events on the current
          stream (best of ROUNDS rounds of STEPS calls), output allocation included
  host    the vectorised fp64 numpy restatement (tests/mesh_restate.py mesh_of_frame) per frame on frames already on the host, perf_counter; at most
          HOST_FRAMES frames are run and the per-frame time is reported
  GB/s    (frame bytes read + kept xyz / uv / face bytes written) / device time: the useful traffic. The vertex map, its re-read by the face passes
          and the second read of the frames are on top, so the kernels move more than this figure says.
  fp64    the profiler's time of the two kernels that do fp64 arithmetic (flags, vertices) at B = 32 and 2 M faces, against the same kernels in
          float from a library built with MDPT_EXTRA_HIPCC_FLAGS=-DMDPT_DEBUG_SWITCHES (MDPT_MESH_FP32=1): whether the fp64 bounds them.
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
from muggled_dpt_amd import postprocess as pp  # noqa: E402
from tests import mesh_restate as ms  # noqa: E402

STEPS, ROUNDS, HOST_FRAMES, PROFILE_CALLS = 3, 3, 2, 5
SIDE = 518
CAMERA = dict(fov_deg=50.0, min_depth=0.5, max_depth=20.0)
THRESHOLD = 0.503  # (off the half steps an interpolated alpha byte can land on exactly)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.manual_seed(0)
    res = {"probe": "gpu_mesh", "source_hash": native.source_hash(), "device": torch.cuda.get_device_name(0), "gpus": 1, "frame_hw": [SIDE, SIDE],
           "edge_threshold": THRESHOLD, "steps": STEPS, "rounds": ROUNDS, "host": "vectorised fp64 numpy restatement, per frame", "cases": []}
    yy, xx = torch.meshgrid(torch.arange(float(SIDE)), torch.arange(float(SIDE)), indexing="ij")
    one = (1 + 0.002 * xx + 0.3 * torch.sin(xx / 17) * torch.cos(yy / 23) + (xx > 300) * 0.4)[None]
    for target in (250_000, 2_000_000):
        nx, ny, _ = pp.mesh_plane_grid((SIDE, SIDE), target)
        for b in (1, 32):
            pred = one.repeat(b, 1, 1).cuda()
            pred += 0.01 * torch.rand_like(pred)
            frames = pp.pack_depth_u24_frames(pred)
            call = lambda: pp.depth_frames_to_mesh(frames, (SIDE, SIDE), edge_threshold=THRESHOLD, target_num_faces=target, **CAMERA)  # noqa: E731
            ms_dev = timed_device(call)
            counts = call()[3].cpu().numpy().astype(np.int64)
            useful = frames.numel() + int(counts[:, 0].sum()) * 20 + int(counts[:, 1].sum()) * 12
            host_frames = frames[:HOST_FRAMES].cpu().numpy()
            t0 = time.perf_counter()
            for f in host_frames:
                ms.mesh_of_frame(f, (SIDE, SIDE), nx, ny, edge_threshold=THRESHOLD, **CAMERA)
            ms_host = 1000 * (time.perf_counter() - t0) / len(host_frames)
            res["cases"].append({"target_faces": target, "grid": [nx, ny], "batch": b, "kept_vertices": int(counts[:, 0].sum()),
                                 "kept_faces": int(counts[:, 1].sum()), "device_ms": round(ms_dev, 3), "device_ms_per_frame": round(ms_dev / b, 4),
                                 "host_ms_per_frame": round(ms_host, 1), "speedup_per_frame": round(ms_host / (ms_dev / b), 1),
                                 "useful_GBps": round(useful / (ms_dev * 1e-3) / 1e9, 1)})
            print(json.dumps(res["cases"][-1]), flush=True)
    # the launches alone (no allocation, no Python): the profiler's record of B = 32, 2 M-face calls
    lib = native.load()

    def profile(calls=PROFILE_CALLS):
        call()  # (not recorded)
        torch.cuda.synchronize()
        lib.mdpt_profile_enable(1)
        for _ in range(calls):
            call()
        torch.cuda.synchronize()
        buf = native.ctypes.create_string_buffer(1 << 16)
        lib.mdpt_profile_report(buf, len(buf))
        lib.mdpt_profile_enable(0)
        return {k["name"]: k["total_ms"] / calls for k in json.loads(buf.value.decode()).get("kernels", []) if k["name"].startswith("mesh_")}

    prof = profile()
    res["profile_b32_2M_ms"] = {k: round(v, 4) for k, v in prof.items()}
    if prof:
        res["profile_b32_2M_total_ms"] = round(sum(prof.values()), 4)
        res["profile_b32_2M_useful_GBps"] = round(useful / (sum(prof.values()) * 1e-3) / 1e9, 1)
    nv32, kept32 = 32 * nx * ny, int(counts[:, 0].sum())
    # the bytes each fp64 kernel has to move: flags = 4 B map written per vertex; vertices = 4 B map read per vertex, 20 B of xyz / uv and 4 B of
    # map written per kept vertex; both read the frames once from memory (the other taps come from cache)
    traffic = {"mesh_flag_kernel": nv32 * 4 + frames.numel(), "mesh_vertex_kernel": nv32 * 4 + kept32 * 24 + frames.numel()}
    res["profile_kernel_GBps"] = {k: round(traffic[k] / (prof[k] * 1e-3) / 1e9, 1) for k in traffic if k in prof}
    # what the fp64 costs: the same two kernels in float (a -DMDPT_DEBUG_SWITCHES library has them behind MDPT_MESH_FP32=1; wrong results, same
    # traffic). A release library ignores the variable, no kernel reports as <float>, and the comparison is recorded as not made.
    os.environ["MDPT_MESH_FP32"] = "1"
    try:
        prof32 = profile()
    finally:
        del os.environ["MDPT_MESH_FP32"]
    if "mesh_vertex_kernel<float>" in prof32 and "mesh_flag_kernel<float>" in prof32:
        ab = {}
        for k in traffic:
            ab[k] = {"fp64_ms": round(prof[k], 4), "fp32_ms": round(prof32[k + "<float>"], 4), "fp64_over_fp32": round(prof[k] / prof32[k + "<float>"], 2),
                     "fp32_GBps": round(traffic[k] / (prof32[k + "<float>"] * 1e-3) / 1e9, 1)}
        fp64_ms, fp32_ms = (sum(v[key] for v in ab.values()) for key in ("fp64_ms", "fp32_ms"))
        res["fp64_vs_fp32"] = {"kernels": ab, "whole_call_fp64_ms": round(sum(prof.values()), 4), "whole_call_fp32_ms": round(sum(prof32.values()), 4),
                               "fp64_bounds_the_kernels": bool(fp64_ms > 1.1 * fp32_ms)}
    else:
        res["fp64_vs_fp32"] = "not measured: the library has no float kernels (build it with MDPT_EXTRA_HIPCC_FLAGS=-DMDPT_DEBUG_SWITCHES)"
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
