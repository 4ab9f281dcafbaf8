#!/usr/bin/env python3
"""Depth segmentation (segment.segment_depth, segment.region_cutouts): the device calls, their per-launch split, and the routes a user has without them.
  maps     ViT-L (synthetic weights), bf16, photos of 504 x 504 -> maps of 504 x 504; 1 and 32 maps per call; inverse space, 4-connectivity, min_area 16
  steps    LOW_STEP gives many regions, HIGH_STEP a few large ones: the contended-atomics case of the relabel + statistics launch. Reported per
           setting: the regions, the largest region's share of the nodes, and relabel_ms_high_over_low = how that launch moves between the two
  device   ONE segment_depth call over the maps: HIP events, best of ROUNDS rounds of STEPS calls, table upload and allocation included; the library
           profiler's time per launch in a run of its own; per launch the bytes it must move at least (bytes_min: the map in its dtype, the int32
           planes, the link bytes) and bytes_min / time against HBM's 8 TB/s
  cutouts  ONE region_cutouts call to device photos of 1280 x 720 and 3024 x 4032, the centre point picked; 3 B in + 5 B out per pixel against 8 TB/s
  restated the numpy restatement (tests/segment_restate.py) of a 126 x 126 crop on the host: the yardstick of the definition; its labels must equal the device's
  torch    the route a user has today in torch on the device: labels = node indices, iterated masked min-propagation over the four links with a
           convergence read-back per round (torch.equal), on ONE map; its components must equal the device's (as partitions of the nodes)
No ratio is fixed in advance. No counter run is made here: what bounds each kernel is not separated.
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

STEPS, ROUNDS, PROFILE_CALLS, MAPS = 3, 3, 3, 32
LOW_STEP, HIGH_STEP, MIN_AREA = 0.002, 0.05, 16
MAP_COUNTS = [1, 32]
PHOTO_HWS = [(720, 1280), (3024, 4032)]
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


def bytes_min(n, elt):
    """per launch of segment_depth, the bytes n nodes of `elt`-byte values must move at least (tables and partials left out)"""
    return {"segment_minmax_kernel": n * elt, "segment_tile_kernel": n * (elt + 4 + 4 + 1), "segment_merge_kernel": 0, "segment_flatten_kernel": n * 8,
            "segment_flag_kernel": n * 8, "segment_scatter_kernel": n * 8, "segment_relabel_kernel": n * (8 + elt)}


def step_device(work):
    import torch
    from muggled_dpt_amd import native, segment
    from tests import segment_restate as sr
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

    crop = all_maps[0, :126, :126].contiguous()
    v32 = crop.float().cpu().numpy()
    t0 = time.perf_counter()
    want = sr.segment(v32, step=HIGH_STEP, min_area=MIN_AREA)
    restated_s = time.perf_counter() - t0
    got = segment.segment_depth([crop], step=HIGH_STEP, min_area=MIN_AREA)
    restated = {"map_hw": [126, 126], "step": HIGH_STEP, "numpy_host_ms": round(1000 * restated_s, 1), "regions": want["count"],
                "differing_labels": int((got.labels[0].cpu().numpy() != want["labels"]).sum()),
                "device_call_ms": round(_timed(lambda: segment.segment_depth([crop], step=HIGH_STEP, min_area=MIN_AREA)), 4)}

    configs = []
    for count in MAP_COUNTS:
        maps = [m for m in all_maps[:count]]
        n = sum(m.numel() for m in maps)
        per_step = {}
        for name, step in (("low", LOW_STEP), ("high", HIGH_STEP)):
            call = lambda: segment.segment_depth(maps, step=step, min_area=MIN_AREA)  # noqa: E731
            kernels, launches = profiled(call)
            rows = call().region_views()
            call_ms, kernels_ms = _timed(call), sum(kernels.values())
            need = bytes_min(n, maps[0].element_size())
            per_step[name] = {"step": step, "regions": sum(r["count"] for r in rows), "call_ms": round(call_ms, 4), "kernels_ms": round(kernels_ms, 4),
                              "largest_region_share": round(max((int(r["area"].max()) if r["count"] else 0) / maps[0].numel() for r in rows), 4),
                              "kernels": kernels, "launches_per_call": launches, "launch_and_host_share": round(max(0.0, 1.0 - kernels_ms / call_ms), 4),
                              "bytes_min": need, "share_of_hbm_peak": {k: round(b / (kernels[k] * 1e-3) / HBM_BYTES_PER_S, 4) for k, b in need.items()
                                                                       if kernels.get(k, 0) > 0 and b},
                              "meganodes_per_s": round(n / call_ms / 1e3, 2)}
        lo_ms, hi_ms = (per_step[k]["kernels"].get("segment_relabel_kernel", 0.0) for k in ("low", "high"))
        configs.append({"maps": count, "map_hw": [504, 504], **per_step, "relabel_ms_high_over_low": round(hi_ms / lo_ms, 3) if lo_ms > 0 else None})

    cutouts = []
    g = torch.Generator(device="cuda").manual_seed(1)
    for hw in PHOTO_HWS:
        for count in MAP_COUNTS:
            seg = segment.segment_depth([m for m in all_maps[:count]], step=HIGH_STEP, min_area=MIN_AREA)
            photos = [torch.randint(0, 256, (*hw, 3), device="cuda", dtype=torch.uint8, generator=g) for _ in range(count)]
            call = lambda: segment.region_cutouts(seg, photos, points=[[(0.5, 0.5)]] * count)  # noqa: E731
            kernels, _ = profiled(call)
            call_ms, px = _timed(call), count * hw[0] * hw[1]
            cut_ms = kernels.get("segment_cutout_kernel", 0.0)
            cutouts.append({"photo_hw": list(hw), "photos": count, "call_ms": round(call_ms, 4), "kernels": kernels,
                            "cutout_share_of_hbm_peak": round(8 * px / (cut_ms * 1e-3) / HBM_BYTES_PER_S, 4) if cut_ms > 0 else None,
                            "megapixels_per_s": round(px / call_ms / 1e3, 2)})
            del photos
            torch.cuda.empty_cache()
    with open(os.path.join(work, "device.json"), "w") as fh:
        json.dump({"restated": restated, "configs": configs, "cutouts": cutouts}, fh)


def torch_components(v, step):
    """iterated masked min-propagation, fp32 map [h,w] on the device -> int64 roots [h,w] (4-connectivity, inverse space, finite values)"""
    import torch
    h, w = v.shape
    d = v.double()
    thr = step * (d.max() - d.min())
    east, south = (d[:, 1:] - d[:, :-1]).abs() <= thr, (d[1:] - d[:-1]).abs() <= thr
    lab, rounds = torch.arange(h * w, device=v.device).view(h, w), 0
    while True:
        new = lab.clone()
        new[:, :-1] = torch.where(east, torch.minimum(new[:, :-1], lab[:, 1:]), new[:, :-1])
        new[:, 1:] = torch.where(east, torch.minimum(new[:, 1:], lab[:, :-1]), new[:, 1:])
        new[:-1] = torch.where(south, torch.minimum(new[:-1], lab[1:]), new[:-1])
        new[1:] = torch.where(south, torch.minimum(new[1:], lab[:-1]), new[1:])
        new = new.view(-1)[new.view(-1)].view(h, w)  # pointer jumping
        rounds += 1
        if torch.equal(new, lab):  # the convergence read-back
            return lab, rounds
        lab = new


def step_torch(work):
    import torch
    from muggled_dpt_amd import segment
    m = torch.load(os.path.join(work, "maps.pt"))[0].cuda()
    results = []
    for step in (LOW_STEP, HIGH_STEP):
        roots, rounds = torch_components(m.float(), step)
        seg = segment.segment_depth([m], step=step, min_area=1)
        first = seg.region_views()[0]["first"].long()
        same = bool(torch.equal(first[seg.labels[0].long()], roots)) if torch.isfinite(m.float()).all() else None
        results.append({"step": step, "rounds": rounds, "torch_min_propagation_ms": round(_timed(lambda: torch_components(m.float(), step)), 3),
                        "device_call_ms": round(_timed(lambda: segment.segment_depth([m], step=step, min_area=1)), 4), "same_components": same})
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
                raise SystemExit(f"gpu_segment: step '{step}' ended with status {r.returncode}; stopping")
        device = json.load(open(os.path.join(work, "device.json")))
        res = {"probe": "gpu_segment", "source_hash": native.source_hash(), "gpus": 1, "model": "vitl synthetic bf16", "space": "inverse", "connectivity": 4,
               "min_area": MIN_AREA, "steps": STEPS, "rounds": ROUNDS, "counter_run": "none: what bounds each kernel is not separated",
               "restated": device["restated"], "configs": device["configs"], "cutouts": device["cutouts"],
               "torch_route": {"note": "one 504 x 504 map, 4-connectivity, min_area 1: iterated min-propagation with pointer jumping, torch.equal per round",
                               "configs": json.load(open(os.path.join(work, "torch.json")))}}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
