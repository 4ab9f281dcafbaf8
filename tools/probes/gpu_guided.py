#!/usr/bin/env python3
"""Photo-guided upsampling (postprocess.guided_upsample_images): the device call against the routes without it.
  maps     ViT-L (synthetic weights), bf16, photos of 504 x 504 -> maps of 504 x 504 (the model's own size)
  photos   uint8 BGR on the device, random, 1280 x 720 and 3024 x 4032 (H x W = 720 x 1280 and 3024 x 4032); 1 and 32 pairs; radius 4 and 16, eps 1e-4
  device   ONE guided_upsample_images call over the pairs: HIP events, best of ROUNDS rounds of STEPS calls, table upload and allocation included;
           and the library profiler's time per launch
  bilinear postprocess.scale_prediction_images on the same maps: the route every caller takes today (no guide)
  torch    the same filter in torch on the device, fp32, per image: adaptive_avg_pool2d of the photo to map size, avg_pool2d box means
           (count_include_pad=False), torch.linalg.solve, F.interpolate of the four mean coefficients, the sum at photo size
  bytes    what the two photo passes must move at least: the cell sums read 3 B per photo pixel, apply reads 3 B and writes 4 B per photo pixel (the
           coefficients stay in cache); against HBM's 8 TB/s. No counter run is made here: what bounds a kernel is not separated.
Two steps, each a child process under its own time limit; a step that fails ends the probe. Prints one JSON line (and writes --out PATH)."""
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
RADII = [4, 16]
EPS = 1e-4
HBM_GBS = 8000.0
STEP_LIMITS = {"maps": 400, "device": 500}  # seconds


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


def torch_guided(maps, photos, radius, eps):
    import torch
    import torch.nn.functional as F
    k = 2 * radius + 1
    box = lambda x: F.avg_pool2d(x, k, 1, radius, count_include_pad=False)  # noqa: E731
    out = []
    for m, f in zip(maps, photos):
        h, w = m.shape
        full = f.permute(2, 0, 1).float()[None] / 255.0
        g = F.adaptive_avg_pool2d(full, (h, w))
        p = m.float()[None, None]
        mg, mp = box(g), box(p)
        gg = box((g[:, :, None] * g[:, None]).reshape(1, 9, h, w)).reshape(3, 3, h, w)
        sigma = gg - mg[0, :, None] * mg[0, None] + eps * torch.eye(3, device=m.device)[:, :, None, None]
        rhs = box(g * p)[0] - mg[0] * mp[0]
        a = torch.linalg.solve(sigma.permute(2, 3, 0, 1), rhs.permute(1, 2, 0)[..., None])[..., 0].permute(2, 0, 1)
        b = mp[0] - (a * mg[0]).sum(0, keepdim=True)
        up = F.interpolate(box(torch.cat([a, b])[None]), size=f.shape[:2], mode="bilinear")[0]
        out.append((up[:3] * full[0]).sum(0) + up[3])
    return out


def step_device(work):
    import torch
    from muggled_dpt_amd import native
    from muggled_dpt_amd import postprocess as pp
    all_maps = torch.load(os.path.join(work, "maps.pt")).cuda()
    lib = native.load()

    def timed(fn):
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
            whs = [(hw[1], hw[0])] * pairs
            pixels = pairs * hw[0] * hw[1]
            bilinear_ms = timed(lambda: pp.scale_prediction_images(maps, whs))
            for radius in RADII:
                call = lambda: pp.guided_upsample_images(maps, photos, radius, EPS)  # noqa: E731
                kernels, launches = profiled(call)
                cell_ms, apply_ms = kernels["guided_cell_sum_kernel"], kernels["guided_apply_kernel"]
                ref = torch_guided(maps[:1], photos[:1], radius, EPS)[0]
                got = call()[0][0]
                results.append({
                    "photo_hw": list(hw), "pairs": pairs, "radius": radius, "call_ms": round(timed(call), 4), "kernels_ms": round(sum(kernels.values()), 4),
                    "kernels": kernels, "launches_per_call": launches, "bilinear_scale_prediction_images_ms": round(bilinear_ms, 4),
                    "torch_fp32_same_filter_ms": round(timed(lambda: torch_guided(maps, photos, radius, EPS)), 3),
                    "cell_sum_gb_s": round(3 * pixels / cell_ms / 1e6, 1), "cell_sum_share_of_hbm": round(3 * pixels / cell_ms / 1e6 / HBM_GBS, 4),
                    "apply_gb_s": round(7 * pixels / apply_ms / 1e6, 1), "apply_share_of_hbm": round(7 * pixels / apply_ms / 1e6 / HBM_GBS, 4),
                    "max_abs_diff_to_torch_route": float((got - ref).abs().max()),  # (torch: fp32, cells by adaptive pooling)
                })
                del ref, got
            del photos
            torch.cuda.empty_cache()
    with open(os.path.join(work, "device.json"), "w") as fh:
        json.dump(results, fh)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, choices=list(STEP_LIMITS))
    ap.add_argument("--work", default=None)
    args = ap.parse_args()
    if args.step:
        return {"maps": step_maps, "device": step_device}[args.step](args.work)
    from muggled_dpt_amd import native
    with tempfile.TemporaryDirectory() as work:
        for step, limit in STEP_LIMITS.items():  # (a fault, an abort or a time limit in one step: nothing more is started)
            r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step, "--work", work])
            if r.returncode != 0:
                raise SystemExit(f"gpu_guided: step '{step}' ended with status {r.returncode}; stopping")
        res = {"probe": "gpu_guided", "source_hash": native.source_hash(), "gpus": 1, "model": "vitl synthetic bf16", "map_hw": [504, 504], "eps": EPS,
               "steps": STEPS, "rounds": ROUNDS, "hbm_gb_s": HBM_GBS, "counter_run": "none: what bounds the kernels is not separated",
               "configs": json.load(open(os.path.join(work, "device.json")))}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
