#!/usr/bin/env python3
"""Surface normals and relighting (relight.depth_normals / relight_images): the device call, its per-launch split, and the route a user has without it.
  maps     ViT-L (synthetic weights), bf16, photos of 504 x 504 -> maps of 504 x 504 (the model's own size)
  photos   uint8 BGR on the device, random, 1280 x 720 and 3024 x 4032; 1 and 32 pairs; step 1 and the default step (3 and 8); V = 1 and V = 16 lights
           (light_sweep), inverse space, no highlight
  device   ONE relight_images call over the pairs: HIP events, best of ROUNDS rounds of STEPS calls, table upload and allocation included; the library
           profiler's time per launch; and one depth_normals call (12 bytes a pixel of normals, no frames)
  traffic  the tile kernel's useful traffic against HBM's 8 TB/s: photo bytes read + V frames written (+ 12 B a pixel of normals where asked); the map
           (504 x 504 x 2 bytes) stays in cache and is not counted
  restated the numpy restatement (tests/normals_restate.py) on a 96 x 128 photo on the host: the yardstick of the arithmetic; its output must equal the device's
  torch    what a user can do today in torch on the device, fp32: F.interpolate to the photo, the unprojection, torch.gradient, cross, normalize, the
           Lambert mix per light. NOT the same arithmetic (central differences only, fp32): its time and its peak extra memory are reported, 1 pair only.
No counter run is made here: what bounds the tile kernel is not separated.
Three steps, each a child process under its own time limit; a step that fails ends the probe. Prints one JSON line (and writes --out PATH)."""
import argparse
import ctypes
import json
import math
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

STEPS, ROUNDS, PROFILE_CALLS, MAPS = 3, 3, 3, 32
PHOTO_HWS = [(720, 1280), (3024, 4032)]
PAIR_COUNTS = [1, 32]
LIGHT_COUNTS = [1, 16]
HBM_BYTES_PER_S = 8e12
STEP_LIMITS = {"maps": 400, "device": 500, "torch": 300}  # seconds


def step_maps(work):
    import torch
    from muggled_dpt_amd import make_depthanythingv2_dpt_from_original_state_dict
    from muggled_dpt_amd.synthetic import make_synthetic_original_state_dict
    _, model = make_depthanythingv2_dpt_from_original_state_dict(make_synthetic_original_state_dict("vitl", 0))
    model = model.to("cuda", torch.bfloat16)
    rng = np.random.default_rng(0)
    photos = [rng.integers(0, 256, (504, 504, 3), dtype=np.uint8) for _ in range(MAPS)]
    maps = model.inference_images(photos, 504, True, 32)
    torch.save(torch.stack([m[0] for m in maps]).cpu(), os.path.join(work, "maps.pt"))


def _timed(fn):
    import torch
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


def step_device(work):
    import torch
    from muggled_dpt_amd import native, relight
    from tests import normals_restate as nr
    all_maps = torch.load(os.path.join(work, "maps.pt")).cuda()
    lib = native.load()

    def profiled(fn):
        torch.cuda.synchronize()
        lib.mdpt_profile_enable(1)
        for _ in range(PROFILE_CALLS):
            fn()
        torch.cuda.synchronize()
        buf = ctypes.create_string_buffer(1 << 16)
        lib.mdpt_profile_report(buf, len(buf))
        lib.mdpt_profile_enable(0)
        ks = json.loads(buf.value.decode())["kernels"]
        return {k["name"]: round(k["total_ms"] / PROFILE_CALLS, 4) for k in ks}, sum(k["launches"] for k in ks) / PROFILE_CALLS

    rng = np.random.default_rng(3)
    small = rng.integers(0, 256, (96, 128, 3), dtype=np.uint8)
    small_map = all_maps[0].float()[::6, ::6].contiguous()
    ring = relight.light_sweep(4, 35.0)
    t0 = time.perf_counter()
    want, want_n, _ = nr.relight(small_map.cpu().numpy(), small, ring)
    restated_s = time.perf_counter() - t0
    got, got_n = relight.relight_images([small_map], [small], ring, return_normals=True)
    restated = {"photo_hw": [96, 128], "lights": 4, "numpy_host_ms": round(1000 * restated_s, 1), "differing_bytes": int((got[0].cpu().numpy() != want).sum()),
                "differing_normal_words": int((got_n[0].cpu().numpy().view(np.uint32) != want_n.view(np.uint32)).sum()),
                "device_call_ms": round(_timed(lambda: relight.relight_images([small_map], [torch.from_numpy(small).cuda()], ring)), 4)}

    g = torch.Generator(device="cuda").manual_seed(1)
    results = []
    for hw in PHOTO_HWS:
        for pairs in PAIR_COUNTS:
            maps = [m for m in all_maps[:pairs]]
            photos = [torch.randint(0, 256, (*hw, 3), device="cuda", dtype=torch.uint8, generator=g) for _ in range(pairs)]
            px = pairs * hw[0] * hw[1]
            for step in (1, None):
                for V in LIGHT_COUNTS:
                    if pairs * V * hw[0] * hw[1] * 3 > 8 << 30:  # (32 photos of 12 Mpixel x 16 frames: 18 GB of output; not run)
                        continue
                    lights = relight.light_sweep(V, 35.0)
                    call = lambda: relight.relight_images(maps, photos, lights, step=step)  # noqa: E731
                    kernels, launches = profiled(call)
                    tile_ms = kernels.get("normals_tile_kernel", 0.0)
                    call_ms, useful = _timed(call), 3 * px * (1 + V)
                    results.append({"call": "relight_images", "photo_hw": list(hw), "pairs": pairs, "step": relight.default_step(hw[1], 504) if step is None else step,
                                    "lights": V, "call_ms": round(call_ms, 4), "kernels": kernels, "launches_per_call": launches, "useful_bytes": useful,
                                    "tile_kernel_share_of_hbm": round(useful / (tile_ms * 1e-3) / HBM_BYTES_PER_S, 4) if tile_ms > 0 else None,
                                    "megapixels_per_s": round(px / call_ms / 1e3, 2)})
                call = lambda: relight.depth_normals(maps, None, photos, step=step)  # noqa: E731
                kernels, launches = profiled(call)
                tile_ms = kernels.get("normals_tile_kernel", 0.0)
                call_ms, useful = _timed(call), 12 * px
                results.append({"call": "depth_normals", "photo_hw": list(hw), "pairs": pairs, "step": relight.default_step(hw[1], 504) if step is None else step,
                                "call_ms": round(call_ms, 4), "kernels": kernels, "launches_per_call": launches, "useful_bytes": useful,
                                "tile_kernel_share_of_hbm": round(useful / (tile_ms * 1e-3) / HBM_BYTES_PER_S, 4) if tile_ms > 0 else None,
                                "megapixels_per_s": round(px / call_ms / 1e3, 2)})
            del photos
            torch.cuda.empty_cache()
    with open(os.path.join(work, "device.json"), "w") as fh:
        json.dump({"restated": restated, "configs": results}, fh)


def torch_route(m, photo, lights, fov_deg=50.0, min_depth=50.0, max_depth=100.0, ambient=0.35, diffuse=0.9):
    """the route a user has today: one bf16 map [h,w], one uint8 photo [H,W,3], fp64 lights [V,3] on the device -> uint8 [V,H,W,3]"""
    import torch
    import torch.nn.functional as F
    H, W = photo.shape[:2]
    s = F.interpolate(m.float()[None, None], (H, W), mode="bilinear", align_corners=False)[0, 0]
    v = (s - s.min()) / (s.max() - s.min())
    z = 1.0 / (1.0 / max_depth + (1.0 / min_depth - 1.0 / max_depth) * v)
    t = math.tan(math.radians(fov_deg) / 2)
    kx, ky = (t, t * H / W) if W > H else (t * W / H, t)
    x = (2 * (torch.arange(W, device=m.device) + 0.5) / W - 1)[None, :]
    y = (1 - 2 * (torch.arange(H, device=m.device) + 0.5) / H)[:, None]
    P = torch.stack([z * x * kx, z * y * ky, -z], dim=-1)
    dy, dx = torch.gradient(P, dim=(0, 1))
    n = F.normalize(torch.cross(dx, -dy, dim=-1), dim=-1)
    img = photo.float()
    frames = [(img * (ambient + diffuse * (n @ l).clamp_min(0))[..., None] + 0.5).floor().clamp(0, 255).to(torch.uint8) for l in lights.float()]
    return torch.stack(frames)


def step_torch(work):
    import torch
    from muggled_dpt_amd import relight
    all_maps = torch.load(os.path.join(work, "maps.pt")).cuda()
    g = torch.Generator(device="cuda").manual_seed(1)
    results = []
    for hw in PHOTO_HWS:
        photo = torch.randint(0, 256, (*hw, 3), device="cuda", dtype=torch.uint8, generator=g)
        for V in LIGHT_COUNTS:
            lights = torch.from_numpy(relight.light_sweep(V, 35.0)).cuda()
            got = relight.relight_images(all_maps[:1], [photo], lights, step=1)[0]
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            ref = torch_route(all_maps[0], photo, lights)
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated() - base
            results.append({"photo_hw": list(hw), "pairs": 1, "lights": V, "torch_fp32_ms": round(_timed(lambda: torch_route(all_maps[0], photo, lights)), 3),
                            "torch_peak_extra_bytes": int(peak), "mean_abs_diff_to_device_bytes": float((got.float() - ref.float()).abs().mean())})
            del ref, got
        del photo
        torch.cuda.empty_cache()
    with open(os.path.join(work, "torch.json"), "w") as fh:
        json.dump(results, fh)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, choices=list(STEP_LIMITS))
    ap.add_argument("--work", default=None)
    args = ap.parse_args()
    if args.step:
        return {"maps": step_maps, "device": step_device, "torch": step_torch}[args.step](args.work)
    from muggled_dpt_amd import native
    with tempfile.TemporaryDirectory() as work:
        for step, limit in STEP_LIMITS.items():  # (a fault, an abort or a time limit in one step: nothing more is started)
            r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step, "--work", work])
            if r.returncode != 0:
                raise SystemExit(f"gpu_normals: step '{step}' ended with status {r.returncode}; stopping")
        device = json.load(open(os.path.join(work, "device.json")))
        res = {"probe": "gpu_normals", "source_hash": native.source_hash(), "gpus": 1, "model": "vitl synthetic bf16", "map_hw": [504, 504], "space": "inverse",
               "steps": STEPS, "rounds": ROUNDS, "hbm_bytes_per_s": HBM_BYTES_PER_S, "counter_run": "none: what bounds the tile kernel is not separated",
               "restated": device["restated"], "configs": device["configs"],
               "torch_route": {"note": "not the same arithmetic: central differences only, fp32", "configs": json.load(open(os.path.join(work, "torch.json")))}}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
