#!/usr/bin/env python3
"""Synthetic depth of field (refocus.refocus_images): the device call, its per-launch split, and the route a user has without it.
  maps     ViT-L (synthetic weights), bf16, photos of 504 x 504 -> maps of 504 x 504 (the model's own size)
  photos   uint8 BGR on the device, random, 1280 x 720 and 3024 x 4032 (H x W = 720 x 1280 and 3024 x 4032); 1 and 32 pairs; max_radius 8 and 32,
           inverse space, focus 0.5, aperture = 2 max_radius per unit of defocus (half the map's range away reaches max_radius)
  device   ONE refocus_images call over the pairs: HIP events, best of ROUNDS rounds of STEPS calls, table upload and allocation included; the library
           profiler's time per launch; launch_and_host_share = 1 - (sum of the kernels) / (the call): what of a call is not kernel time
  taps     the taps the gather TESTS: per 32 x 32 tile, its pixels times the lattice points of the disc of the tile's largest k over tile and halo
           (computed here from the rq planes with a max pool); divided by the gather's time -> taps per second. taps_covering_bound = the taps a
           pixel's own disc holds, summed: a lower bound of the taps that add something
  restated the numpy restatement (tests/refocus_restate.py) on a 96 x 128 photo, max_radius 8, on the host: the yardstick of the arithmetic, and its
           output must equal the device's on every byte
  torch    what a user can do today in torch on the device, fp32: the radius quantised into LAYERS layers, one disc conv2d per layer on the
           premultiplied photo and the layer's mask, the layers composited back to front by their mean defocus. NOT the same arithmetic (no
           per-pixel radius, no per-pixel depth order, fp32): its difference to the device's result is reported, not bounded. 1280 x 720, 1 pair only.
No counter run is made here: what bounds the gather is not separated.
Three steps, each a child process under its own time limit; a step that fails ends the probe. Prints one JSON line (and writes --out PATH)."""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

STEPS, ROUNDS, PROFILE_CALLS, MAPS, LAYERS = 3, 3, 3, 32, 5
PHOTO_HWS = [(720, 1280), (3024, 4032)]
PAIR_COUNTS = [1, 32]
RADII = [8, 32]
FOCUS = 0.5
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


def taps_of(rq, max_radius):
    """rq uint8 [H,W] on the device -> (taps the gather tests, taps of the pixels' own discs)"""
    import torch
    import torch.nn.functional as F
    from tests.refocus_restate import lattice_counts
    counts = torch.from_numpy(np.array(lattice_counts())).to(rq.device)
    k = (rq.to(torch.int64) ** 2) >> 4
    tile, (H, W) = 32, rq.shape
    padded = F.pad(k.float()[None, None], (0, -W % tile, 0, -H % tile))
    reach = F.max_pool2d(padded, tile + 2 * max_radius, tile, max_radius).long()[0, 0] if max_radius else F.max_pool2d(padded, tile, tile).long()[0, 0]
    pixels = F.avg_pool2d(F.pad(torch.ones(1, 1, H, W, device=rq.device), (0, -W % tile, 0, -H % tile)), tile, tile, divisor_override=1)[0, 0].long()
    tested = torch.where(reach > 0, counts[reach], torch.zeros_like(reach)) * pixels  # (a tile whose largest k is 0 copies its pixels)
    return int(tested.sum()), int(counts[k].sum())


def step_device(work):
    import torch
    from muggled_dpt_amd import native, refocus
    from tests import refocus_restate as rr
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

    # the restatement on a small photo: the arithmetic's yardstick
    rng = np.random.default_rng(3)
    small = rng.integers(0, 256, (96, 128, 3), dtype=np.uint8)
    small_map = all_maps[0].float()[::6, ::6].contiguous()
    t0 = time.perf_counter()
    want, _, _ = rr.refocus(small_map.cpu().numpy(), small, FOCUS, None, 16.0, 8)
    restated_s = time.perf_counter() - t0
    got = refocus.refocus_images([small_map], [small], FOCUS, None, 16.0, 8)[0].cpu().numpy()
    restated = {"photo_hw": [96, 128], "max_radius": 8, "numpy_host_ms": round(1000 * restated_s, 1), "differing_bytes": int((got != want).sum()),
                "device_call_ms": round(_timed(lambda: refocus.refocus_images([small_map], [torch.from_numpy(small).cuda()], FOCUS, None, 16.0, 8)), 4)}

    g = torch.Generator(device="cuda").manual_seed(1)
    results = []
    for hw in PHOTO_HWS:
        for pairs in PAIR_COUNTS:
            maps = [m for m in all_maps[:pairs]]
            photos = [torch.randint(0, 256, (*hw, 3), device="cuda", dtype=torch.uint8, generator=g) for _ in range(pairs)]
            for radius in RADII:
                call = lambda: refocus.refocus_images(maps, photos, FOCUS, None, 2.0 * radius, radius)  # noqa: E731
                kernels, launches = profiled(call)
                gather_ms = sum(v for k, v in kernels.items() if k.startswith("refocus_gather_kernel"))
                planes = refocus.defocus_planes(maps, photos, FOCUS, None, 2.0 * radius, radius)
                tested, own = (sum(v) for v in zip(*(taps_of(rq, radius) for rq, _ in planes)))
                mean_r = float(sum(float(rq.float().mean()) for rq, _ in planes) / pairs / 4.0)
                del planes
                call_ms, kernels_ms = _timed(call), sum(kernels.values())
                results.append({
                    "photo_hw": list(hw), "pairs": pairs, "max_radius": radius, "aperture": 2.0 * radius, "call_ms": round(call_ms, 4),
                    "kernels_ms": round(kernels_ms, 4), "kernels": kernels, "launches_per_call": launches,
                    "launch_and_host_share": round(max(0.0, 1.0 - kernels_ms / call_ms), 4), "mean_radius_px": round(mean_r, 3), "taps_tested": tested,
                    "taps_covering_bound": own, "gather_taps_tested_per_s": round(tested / gather_ms * 1e3, 1) if gather_ms > 0 else None,
                    "megapixels_per_s": round(pairs * hw[0] * hw[1] / call_ms / 1e3, 2),
                })
            del photos
            torch.cuda.empty_cache()
    with open(os.path.join(work, "device.json"), "w") as fh:
        json.dump({"restated": restated, "configs": results}, fh)


def torch_layers(photo, rq, e32, max_radius):
    """the layered route: uint8 [H,W,3], rq, e32 on the device -> fp32 [H,W,3]"""
    import torch
    import torch.nn.functional as F
    img = photo.permute(2, 0, 1).float()
    level = torch.round(rq.float() / 4.0 / max_radius * (LAYERS - 1)).long()
    order = sorted(range(LAYERS), key=lambda l: float(e32[level == l].mean()) if bool((level == l).any()) else float("-inf"))  # back to front
    out = torch.zeros_like(img)
    for l in order:
        mask = (level == l).float()[None]
        if not bool(mask.any()):
            continue
        r = int(round(max_radius * l / (LAYERS - 1)))
        d = torch.arange(-r, r + 1, device=photo.device)
        disc = ((d[:, None] ** 2 + d[None, :] ** 2) <= r * r).float()
        disc = (disc / disc.sum())[None, None].expand(4, 1, -1, -1).contiguous()
        both = F.conv2d(torch.cat([img * mask, mask])[None], disc, padding=r, groups=4)[0]
        out = out * (1.0 - both[3:]) + both[:3]
    return out.permute(1, 2, 0)


def step_torch(work):
    import torch
    from muggled_dpt_amd import refocus
    all_maps = torch.load(os.path.join(work, "maps.pt")).cuda()
    g = torch.Generator(device="cuda").manual_seed(1)
    hw = PHOTO_HWS[0]
    photo = torch.randint(0, 256, (*hw, 3), device="cuda", dtype=torch.uint8, generator=g)
    results = []
    for radius in RADII:
        got, planes = refocus.refocus_images(all_maps[:1], [photo], FOCUS, None, 2.0 * radius, radius, return_radius=True)
        rq, e32 = planes[0]
        ref = torch_layers(photo, rq, e32, radius)
        results.append({"photo_hw": list(hw), "pairs": 1, "max_radius": radius, "layers": LAYERS,
                        "torch_fp32_layered_ms": round(_timed(lambda: torch_layers(photo, rq, e32, radius)), 3),
                        "mean_abs_diff_to_device_bytes": float((got[0].float() - ref).abs().mean()), "max_abs_diff_to_device_bytes": float((got[0].float() - ref).abs().max())})
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
                raise SystemExit(f"gpu_refocus: step '{step}' ended with status {r.returncode}; stopping")
        device = json.load(open(os.path.join(work, "device.json")))
        res = {"probe": "gpu_refocus", "source_hash": native.source_hash(), "gpus": 1, "model": "vitl synthetic bf16", "map_hw": [504, 504], "space": "inverse",
               "focus": FOCUS, "steps": STEPS, "rounds": ROUNDS, "counter_run": "none: what bounds the gather is not separated",
               "restated": device["restated"], "configs": device["configs"],
               "torch_route": {"note": "not the same arithmetic: radius quantised into layers, layers composited back to front, fp32",
                               "configs": json.load(open(os.path.join(work, "torch.json")))}}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
