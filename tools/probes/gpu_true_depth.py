#!/usr/bin/env python3
"""True depth from ground truth (postprocess.fit_true_depth / depth_metrics / true_depth): the device calls against the routes without them.
  model    ViT-L (synthetic weights), bf16, 64 photos of 518 x 518 -> 64 maps
  truths   fp32 on the device at mixed photo sizes up to 3024 x 4032 (SIZES in turn), about 30 % of the pixels measured (the rest zero),
           truth = 1 / (0.37 v + 0.25 + noise) of the resized map, so both fits have something to find
  device   each of fit (lstsq), fit (median), metrics and true_depth as ONE call over the 64 pairs: HIP events, best of ROUNDS rounds of STEPS
           calls, table upload and allocation included; and the library profiler's kernel times and launch counts per call
  torch    the route without the feature on the same maps, on the device, per image: F.interpolate to the truth's size, boolean indexing
           (which synchronises), masked sums or torch.median, one reduction per metric, the reciprocal map
  numpy    the same on the host for the first HOST_IMAGES pairs, maps and truths already on the host (perf_counter)
  bytes    what a call must move at least: 4 B of truth per pixel and sample pass (the prediction stays in cache), 4 B written per pixel by
           true_depth; against HBM's 8 TB/s. No counter run is made here: what bounds a kernel is not separated.
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

STEPS, ROUNDS, PROFILE_CALLS, IMAGES, HOST_IMAGES = 3, 3, 3, 64, 4
SIZES = [(3024, 4032), (1080, 1920), (480, 640), (2160, 3840), (768, 1024), (4032, 3024), (1200, 1600), (720, 1280)]
HBM_GBS = 8000.0
STEP_LIMITS = {"maps": 400, "device": 300, "host": 300}  # seconds


def truth_hws():
    return [SIZES[k % len(SIZES)] for k in range(IMAGES)]


def step_maps(work):
    import torch
    from muggled_dpt_amd import make_depthanythingv2_dpt_from_original_state_dict
    from muggled_dpt_amd.synthetic import make_synthetic_original_state_dict
    _, model = make_depthanythingv2_dpt_from_original_state_dict(make_synthetic_original_state_dict("vitl", 0))
    model = model.to("cuda", torch.bfloat16)
    rng = np.random.default_rng(0)
    photos = [rng.integers(0, 256, (518, 518, 3), dtype=np.uint8) for _ in range(IMAGES)]
    maps = model.inference_images(photos, 518, True, 32)
    torch.save(torch.stack([m[0] for m in maps]).cpu(), os.path.join(work, "maps.pt"))


def make_truths(maps):
    import torch
    import torch.nn.functional as F
    g = torch.Generator(device="cuda").manual_seed(1)
    lo, hi = float(maps.float().min()), float(maps.float().max())
    out = []
    for m, hw in zip(maps, truth_hws()):
        v = (F.interpolate(m.float()[None, None], size=hw, mode="bilinear")[0, 0] - lo) / max(hi - lo, 1e-6) + 1.0  # in [1, 2]
        t = 1.0 / (0.37 * v + 0.25 + 0.01 * torch.randn(hw, device="cuda", generator=g))
        t[torch.rand(hw, device="cuda", generator=g) > 0.3] = 0.0
        out.append(t)
    return out


def normalised(maps):
    """the maps shifted into [1, 2] in their own dtype, so that 0.37 v + 0.25 is positive whatever the synthetic weights give"""
    lo, hi = float(maps.float().min()), float(maps.float().max())
    return ((maps.float() - lo) / max(hi - lo, 1e-6) + 1.0).to(maps.dtype)


def torch_fit(maps, truths, median):
    import torch
    import torch.nn.functional as F
    out = []
    for m, t in zip(maps, truths):
        up = F.interpolate(m.float()[None, None], size=t.shape, mode="bilinear")[0, 0]
        keep = torch.isfinite(t) & (t > 0)
        v, y = up[keep].double(), 1.0 / t[keep].double()  # (boolean indexing reads the count back)
        if median:
            mv, my = torch.median(v), torch.median(y)
            a = (y - my).abs().mean() / (v - mv).abs().mean()
            out.append((a, my - a * mv))
        else:
            n, sv, sy = v.numel(), v.sum(), y.sum()
            a = (n * (v * y).sum() - sv * sy) / (n * (v * v).sum() - sv * sv)
            out.append((a, (sy - a * sv) / n))
    return out


def torch_metrics(maps, truths, fits):
    import torch
    import torch.nn.functional as F
    out = []
    for m, t, (a, b) in zip(maps, truths, fits):
        up = F.interpolate(m.float()[None, None], size=t.shape, mode="bilinear")[0, 0]
        keep = torch.isfinite(t) & (t > 0)
        g = t[keep].double()
        d = 1.0 / (a * up[keep].double() + b)
        r = torch.maximum(d / g, g / d)
        e = torch.log(d) - torch.log(g)
        out.append(torch.stack([((d - g).abs() / g).mean(), ((d - g) ** 2 / g).mean(), ((d - g) ** 2).mean().sqrt(), (e * e).mean().sqrt(),
                                (torch.log10(d) - torch.log10(g)).abs().mean(), (r < 1.25).double().mean(), (r < 1.25 ** 2).double().mean(),
                                (r < 1.25 ** 3).double().mean(), 100.0 * ((e * e).mean() - e.mean() ** 2).sqrt()]))
    return out


def torch_apply(maps, hws, fits):
    import torch.nn.functional as F
    return [1.0 / (a * F.interpolate(m.float()[None, None], size=hw, mode="bilinear")[0, 0].double() + b).float() for m, hw, (a, b) in zip(maps, hws, fits)]


def step_device(work):
    import torch
    from muggled_dpt_amd import native
    from muggled_dpt_amd import postprocess as pp
    maps = normalised(torch.load(os.path.join(work, "maps.pt")).cuda())
    truths = make_truths(maps)
    hws = truth_hws()
    pixels = sum(h * w for h, w in hws)

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
        lib = native.load()
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

    fit = pp.fit_true_depth(maps, truths)
    fit_med = pp.fit_true_depth(maps, truths, method="median")
    calls = {"fit_lstsq": (lambda: pp.fit_true_depth(maps, truths), 1), "fit_median": (lambda: pp.fit_true_depth(maps, truths, method="median"), 5),
             "metrics": (lambda: pp.depth_metrics(maps, truths, fit), 1), "true_depth": (lambda: pp.true_depth(maps, fit, hws), 1)}
    res = {"pairs": IMAGES, "truth_pixels": pixels, "valid_share": round(float(sum((t > 0).sum() for t in truths)) / pixels, 4), "calls": {}}
    for name, (fn, passes) in calls.items():
        kernels, launches = profiled(fn)
        ms_kernels = sum(kernels.values())
        moved = pixels * 4 * passes
        res["calls"][name] = {"call_ms": round(timed(fn), 4), "kernels_ms": round(ms_kernels, 4), "kernels": kernels, "launches_per_call": launches,
                              "sample_passes": passes, "least_bytes": moved, "gb_s_of_kernel_time": round(moved / ms_kernels / 1e6, 1),
                              "share_of_hbm": round(moved / ms_kernels / 1e6 / HBM_GBS, 4)}
    tf = torch_fit(maps, truths, False)
    res["torch_device_ms"] = {"fit_lstsq": round(timed(lambda: torch_fit(maps, truths, False)), 3), "fit_median": round(timed(lambda: torch_fit(maps, truths, True)), 3),
                              "metrics": round(timed(lambda: torch_metrics(maps, truths, tf)), 3), "true_depth": round(timed(lambda: torch_apply(maps, hws, tf)), 3)}
    ta = torch.stack([torch.stack(list(ab)) for ab in tf]).cpu().numpy()
    res["fit_A_range"] = [float(fit[:, 0].min()), float(fit[:, 0].max())]
    res["median_fit_A_range"] = [float(fit_med[:, 0].min()), float(fit_med[:, 0].max())]
    res["max_rel_diff_of_A_to_torch_route"] = float(np.max(np.abs(fit[:, 0].cpu().numpy() - ta[:, 0]) / np.abs(ta[:, 0])))  # (torch resizes in fp32)
    torch.save([t.cpu() for t in truths[:HOST_IMAGES]], os.path.join(work, "truths_host.pt"))
    with open(os.path.join(work, "device.json"), "w") as fh:
        json.dump(res, fh)


def step_host(work):
    import torch
    from tests import align_restate as ar
    maps = normalised(torch.load(os.path.join(work, "maps.pt")))[:HOST_IMAGES].float().numpy()
    truths = [t.numpy() for t in torch.load(os.path.join(work, "truths_host.pt"))]
    ms = {"fit_lstsq": 0.0, "fit_median": 0.0, "metrics": 0.0, "true_depth": 0.0}
    for m, t in zip(maps, truths):
        t0 = time.perf_counter()
        v = ar.resample(m, t.shape)
        keep = np.isfinite(t) & (t > 0)
        x, g = v[keep], t[keep].astype(np.float64)
        y = 1.0 / g
        t1 = time.perf_counter()
        n = x.size
        a = (n * (x * y).sum() - x.sum() * y.sum()) / (n * (x * x).sum() - x.sum() ** 2)
        b = (y.sum() - a * x.sum()) / n
        t2 = time.perf_counter()
        mx, my = np.median(x), np.median(y)
        np.abs(y - my).mean() / np.abs(x - mx).mean()
        t3 = time.perf_counter()
        d = 1.0 / (a * x + b)
        e, r = np.log(d) - np.log(g), np.maximum(d / g, g / d)
        [(np.abs(d - g) / g).mean(), ((d - g) ** 2 / g).mean(), np.sqrt(((d - g) ** 2).mean()), np.sqrt((e * e).mean()), np.abs(np.log10(d) - np.log10(g)).mean(),
         (r < 1.25).mean(), (r < 1.5625).mean(), (r < 1.953125).mean(), 100 * np.sqrt((e * e).mean() - e.mean() ** 2)]
        t4 = time.perf_counter()
        (1.0 / (a * v + b)).astype(np.float32)
        t5 = time.perf_counter()
        sample = 1000 * (t1 - t0)  # resize and masking: part of every route
        ms["fit_lstsq"] += sample + 1000 * (t2 - t1)
        ms["fit_median"] += sample + 1000 * (t3 - t2)
        ms["metrics"] += sample + 1000 * (t4 - t3)
        ms["true_depth"] += sample + 1000 * (t5 - t4)
    pixels = sum(t.size for t in truths)
    with open(os.path.join(work, "host.json"), "w") as fh:
        json.dump({"pairs": HOST_IMAGES, "truth_pixels": pixels, "numpy_host_ms": {k: round(v, 1) for k, v in ms.items()}}, fh)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, choices=list(STEP_LIMITS))
    ap.add_argument("--work", default=None)
    args = ap.parse_args()
    if args.step:
        return {"maps": step_maps, "device": step_device, "host": step_host}[args.step](args.work)
    from muggled_dpt_amd import native
    with tempfile.TemporaryDirectory() as work:
        for step, limit in STEP_LIMITS.items():  # (a fault, an abort or a time limit in one step: nothing more is started)
            r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step, "--work", work])
            if r.returncode != 0:
                raise SystemExit(f"gpu_true_depth: step '{step}' ended with status {r.returncode}; stopping")
        res = {"probe": "gpu_true_depth", "source_hash": native.source_hash(), "gpus": 1, "model": "vitl synthetic bf16", "map_hw": [518, 518],
               "truth_sizes": SIZES, "steps": STEPS, "rounds": ROUNDS, "hbm_gb_s": HBM_GBS, "counter_run": "none: what bounds the kernels is not separated",
               "device": json.load(open(os.path.join(work, "device.json"))), "host": json.load(open(os.path.join(work, "host.json")))}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
