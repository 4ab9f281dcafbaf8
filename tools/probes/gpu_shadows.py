#!/usr/bin/env python3
"""Cast shadows and ambient occlusion for the relighting (relight.shade_images): the device call, its per-launch split, and two yardsticks.
  maps     ViT-L (synthetic weights), bf16, photos of 504 x 504 -> maps of 504 x 504 (the model's own size), which are the working grids (grid_hw=None)
  photos   uint8 BGR on the device, random, 1280 x 720 and 3024 x 4032; 1 and 32 pairs; V = 1 and V = 16 lights (light_sweep); shadow_reach 8 and 32 (ao_reach 8);
           inverse space, no highlight
  device   ONE shade_images call over the pairs: HIP events, best of ROUNDS rounds of STEPS calls, table upload and allocation included; the library
           profiler's time per launch (min/max, state, grid kernel, shade kernel)
  relight  yardstick 1, never the code under test: relight_images on the same pairs (normals_tile_kernel, whose arithmetic is the parent commit's) -
           call_ms - relight_ms is what the feature adds
  torch    yardstick 2: the route a user has today in torch on the device, fp32: the map as a height field, per light a loop over k of shifted compares
           (torch.roll along the light's rounded screen direction, the ray's depth taken linear in k). NOT the same arithmetic (one direction per light for
           the whole image, no perspective, fp32): its time and its peak extra memory are reported, 1 pair only.
No counter run is made here and no tracing: the LDS bank behaviour of the grid kernel is not measured by this probe.
Three steps, each a child process under its own time limit; a step that fails ends the probe. Prints one JSON line (and writes --out PATH)."""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

STEPS, ROUNDS, PROFILE_CALLS, MAPS = 3, 3, 3, 32
PHOTO_HWS = [(720, 1280), (3024, 4032)]
PAIR_COUNTS = [1, 32]
LIGHT_COUNTS = [1, 16]
REACHES = [8, 32]
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

    g = torch.Generator(device="cuda").manual_seed(1)
    results = []
    for hw in PHOTO_HWS:
        for pairs in PAIR_COUNTS:
            maps = [m for m in all_maps[:pairs]]
            photos = [torch.randint(0, 256, (*hw, 3), device="cuda", dtype=torch.uint8, generator=g) for _ in range(pairs)]
            px = pairs * hw[0] * hw[1]
            for V in LIGHT_COUNTS:
                if pairs * V * hw[0] * hw[1] * 3 > 8 << 30:  # (32 photos of 12 Mpixel x 16 frames: 18 GB of output; not run)
                    continue
                lights = relight.light_sweep(V, 35.0)
                relight_ms = _timed(lambda: relight.relight_images(maps, photos, lights))
                for reach in REACHES:
                    call = lambda: relight.shade_images(maps, photos, lights, shadow_reach=reach)  # noqa: E731
                    kernels, launches = profiled(call)
                    call_ms = _timed(call)
                    results.append({"photo_hw": list(hw), "pairs": pairs, "lights": V, "shadow_reach": reach, "ao_reach": 8, "call_ms": round(call_ms, 4),
                                    "relight_images_ms": round(relight_ms, 4), "added_ms": round(call_ms - relight_ms, 4), "kernels": kernels,
                                    "launches_per_call": launches, "megapixels_per_s": round(px / call_ms / 1e3, 2)})
            del photos
            torch.cuda.empty_cache()
    with open(os.path.join(work, "device.json"), "w") as fh:
        json.dump(results, fh)


def torch_route(m, lights, reach, min_depth=50.0, max_depth=100.0, bias=0.02):
    """the route a user has today: one bf16 map [h,w], fp64 lights [V,3] on the device -> vis fp32 [V,h,w] by shifted compares over k, fp32"""
    import torch
    s = m.float()
    v = (s - s.min()) / (s.max() - s.min())
    z = 1.0 / (1.0 / max_depth + (1.0 / min_depth - 1.0 / max_depth) * v)
    cell = 2.0 * z.mean() * 0.466 / z.shape[1]  # world units a node, at the mean depth
    planes = []
    for l in lights.float().tolist():
        m_ = max(abs(l[0]), abs(l[1]), 1e-6)
        sx, sy = l[0] / m_, -l[1] / m_
        vis = torch.ones_like(z)
        for k in range(1, reach + 1):
            dj, di = int(np.floor(k * sx + 0.5)), int(np.floor(k * sy + 0.5))
            zq = torch.roll(z, shifts=(-di, -dj), dims=(0, 1))
            zr = z - (k * cell / m_) * l[2]
            vis = torch.where((zq < zr * (1.0 - bias)) & (zr > 0), torch.zeros_like(vis), vis)
        planes.append(vis)
    return torch.stack(planes)


def step_torch(work):
    import torch
    from muggled_dpt_amd import relight
    all_maps = torch.load(os.path.join(work, "maps.pt")).cuda()
    results = []
    for V in LIGHT_COUNTS:
        lights = torch.from_numpy(relight.light_sweep(V, 35.0)).cuda()
        for reach in REACHES:
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            ref = torch_route(all_maps[0], lights, reach)
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated() - base
            planes_ms = _timed(lambda: relight.light_occlusion(all_maps[:1], lights, shadow_reach=reach, ao_reach=0))
            results.append({"grid_hw": [504, 504], "pairs": 1, "lights": V, "shadow_reach": reach,
                            "torch_fp32_ms": round(_timed(lambda: torch_route(all_maps[0], lights, reach)), 3), "torch_peak_extra_bytes": int(peak),
                            "light_occlusion_shadows_only_ms": round(planes_ms, 4), "torch_share_in_shadow": float((ref == 0).float().mean())})
            del ref
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
                raise SystemExit(f"gpu_shadows: step '{step}' ended with status {r.returncode}; stopping")
        res = {"probe": "gpu_shadows", "source_hash": native.source_hash(), "gpus": 1, "model": "vitl synthetic bf16", "map_hw": [504, 504], "grid": "the map's own",
               "space": "inverse", "steps": STEPS, "rounds": ROUNDS, "counter_run": "none", "configs": json.load(open(os.path.join(work, "device.json"))),
               "torch_route": {"note": "not the same arithmetic: one screen direction per light, no perspective, fp32",
                               "configs": json.load(open(os.path.join(work, "torch.json")))}}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
