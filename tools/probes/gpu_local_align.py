#!/usr/bin/env python3
"""Locally varying true-depth alignment (local_align.fit_true_depth_local / true_depth_local): the device calls against two yardsticks, neither of them the
code under test. The workload is gpu_true_depth.py's: 64 ViT-L maps of 518 x 518 (bf16), fp32 truths on the device at the eight photo sizes, 30 % of the pixels
measured - and a second variant with 3 % measured; grids 12 x 16 and 48 x 64, radius 1, prior 4.
  device   fit and apply as ONE call each over the 64 pairs: HIP events, best of ROUNDS rounds of STEPS calls, table upload and allocation included; and the
           library profiler's time per launch (the per-launch split) and launch count per call
  global   postprocess.fit_true_depth + true_depth on the same pairs: they read the same bytes
  torch    the same arithmetic in torch on the device, per image: F.interpolate to the truth's size, the six terms index_add_-ed into their cells under the
           mask, box sums over the windows, the solve with the prior and the fallback, the box mean, F.interpolate of the coefficients to the truth's size
  bytes    what a call must move at least: fit 4 B of truth per pixel (the prediction and the tables stay in cache), apply 4 B written per pixel; against
           HBM's 8 TB/s. No ratio is fixed in advance; no counter run is made here, so what bounds the moments kernel is a supposition: one 4-byte load a pixel
           plus four cached prediction taps and fp64 arithmetic only on measured pixels - memory-bound at 30 %, closer to the latency of the loads at 3 %.
Two steps, each a child process under its own time limit; a step that fails ends the probe. Prints one JSON line and writes --out PATH (profiles/local_align.json)."""
import argparse
import ctypes
import importlib.util
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)

STEPS, ROUNDS, PROFILE_CALLS = 3, 3, 3
SHARES = (0.3, 0.03)
GRIDS = ((12, 16), (48, 64))
RADIUS, PRIOR = 1, 4.0
HBM_GBS = 8000.0
STEP_LIMITS = {"maps": 400, "device": 500}  # seconds


def _true_depth_probe():
    spec = importlib.util.spec_from_file_location("gpu_true_depth", os.path.join(HERE, "gpu_true_depth.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_truths(td, maps, share):
    """gpu_true_depth.make_truths with `share` of the pixels measured"""
    import torch
    import torch.nn.functional as F
    g = torch.Generator(device="cuda").manual_seed(1)
    lo, hi = float(maps.float().min()), float(maps.float().max())
    out = []
    for m, hw in zip(maps, td.truth_hws()):
        v = (F.interpolate(m.float()[None, None], size=hw, mode="bilinear")[0, 0] - lo) / max(hi - lo, 1e-6) + 1.0
        t = 1.0 / (0.37 * v + 0.25 + 0.01 * torch.randn(hw, device="cuda", generator=g))
        t[torch.rand(hw, device="cuda", generator=g) > share] = 0.0
        out.append(t)
    return out


def torch_local(maps, truths, grid, radius, prior):
    """the local fit and its apply in torch, per image -> the completed maps"""
    import torch
    import torch.nn.functional as F
    gh, gw = grid
    out = []
    for m, t in zip(maps, truths):
        H, W = t.shape
        v = F.interpolate(m.float()[None, None], size=(H, W), mode="bilinear")[0, 0].double()
        keep = (torch.isfinite(t) & (t > 0)).reshape(-1)
        cell = ((torch.arange(H, device=t.device) * gh // H)[:, None] * gw + (torch.arange(W, device=t.device) * gw // W)[None, :]).reshape(-1)
        y = torch.where(keep, 1.0 / t.double().reshape(-1).clamp_min(1e-30), torch.zeros((), device=t.device, dtype=torch.float64))
        x = torch.where(keep, v.reshape(-1), torch.zeros((), device=t.device, dtype=torch.float64))
        terms = torch.stack([keep.double(), x, y, x * x, x * y, y * y], 1)
        M = torch.zeros(gh * gw, 6, device=t.device, dtype=torch.float64).index_add_(0, cell, terms).view(gh, gw, 6)
        G = M.sum((0, 1))
        k = 2 * radius + 1
        box = lambda z: F.avg_pool2d(z.permute(2, 0, 1)[None], k, 1, radius, count_include_pad=False, divisor_override=1)[0].permute(1, 2, 0)
        S = box(M)
        S = torch.where(S[..., :1] > 0, S + prior * G / G[0].clamp_min(1.0), S)
        n, sv, st, svv, svt = S.unbind(-1)[:5]
        var = n * svv - sv * sv
        a = (n * svt - sv * st) / var
        a0 = (G[0] * G[4] - G[1] * G[2]) / (G[0] * G[3] - G[1] * G[1])
        b0 = (G[2] - a0 * G[1]) / G[0]
        good = (n >= 2) & (var > 0) & torch.isfinite(a) & (a > 0)
        wf = torch.stack([torch.where(good, a, a0), torch.where(good, (st - a * sv) / n.clamp_min(1.0), b0)], -1)
        ones = torch.ones(gh, gw, 1, device=t.device, dtype=torch.float64)
        C = box(wf) / box(ones)
        ab = F.interpolate(C.permute(2, 0, 1)[None], size=(H, W), mode="bilinear")[0]
        out.append((1.0 / (ab[0] * v + ab[1])).float())
    return out


def step_device(work):
    import torch
    from muggled_dpt_amd import local_align as la
    from muggled_dpt_amd import native
    from muggled_dpt_amd import postprocess as pp
    td = _true_depth_probe()
    maps = td.normalised(torch.load(os.path.join(work, "maps.pt")).cuda())
    hws = td.truth_hws()
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

    res = {"pairs": len(hws), "truth_pixels": pixels, "radius": RADIUS, "prior": PRIOR, "hbm_gb_s": HBM_GBS, "source_hash": native.source_hash(), "variants": []}
    for share in SHARES:
        truths = make_truths(td, maps, share)
        glob = pp.fit_true_depth(maps, truths)
        base = {"fit_ms": round(timed(lambda: pp.fit_true_depth(maps, truths)), 4), "apply_ms": round(timed(lambda: pp.true_depth(maps, glob, hws)), 4)}
        for grid in GRIDS:
            fit = la.fit_true_depth_local(maps, truths, grid_hw=grid, radius=RADIUS, prior=PRIOR)
            entry = {"measured_share": share, "grid": list(grid), "global_route": base}
            for name, fn, moved in (("fit", lambda: la.fit_true_depth_local(maps, truths, grid_hw=grid, radius=RADIUS, prior=PRIOR), pixels * 4),
                                    ("apply", lambda: la.true_depth_local(maps, fit, hws), pixels * 4)):
                kernels, launches = profiled(fn)
                ms = timed(fn)
                kms = sum(kernels.values())
                entry[name] = {"call_ms": round(ms, 4), "kernels_ms": round(kms, 4), "kernels": kernels, "launches_per_call": launches, "least_bytes": moved,
                               "gb_s_of_kernel_time": round(moved / kms / 1e6, 1), "share_of_hbm": round(moved / kms / 1e6 / HBM_GBS, 4),
                               "ratio_to_global_route": round(ms / base[name + "_ms"], 3)}
            torch_ms = timed(lambda: torch_local(maps, truths, grid, RADIUS, PRIOR))
            entry["torch_route_ms"] = round(torch_ms, 3)
            entry["torch_route_over_device"] = round(torch_ms / (entry["fit"]["call_ms"] + entry["apply"]["call_ms"]), 2)
            done = la.true_depth_local(maps, fit, hws)
            ref = torch_local(maps, truths, grid, RADIUS, PRIOR)
            entry["max_rel_diff_to_torch_route"] = float(max(((a[0] - b).abs() / b.abs()).max() for a, b in zip(done, ref)))  # (torch resizes in fp32)
            res["variants"].append(entry)
    with open(os.path.join(work, "device.json"), "w") as fh:
        json.dump(res, fh)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "local_align.json"))
    ap.add_argument("--step", default=None, choices=sorted(STEP_LIMITS))
    ap.add_argument("--work", default=None)
    args = ap.parse_args()
    if args.step:
        {"maps": lambda w: _true_depth_probe().step_maps(w), "device": step_device}[args.step](args.work)
        return
    with tempfile.TemporaryDirectory() as work:
        for step in ("maps", "device"):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step, "--work", work], timeout=STEP_LIMITS[step] + 30)
            if r.returncode != 0:
                raise SystemExit(f"step {step} failed with {r.returncode}: nothing more is run")
        with open(os.path.join(work, "device.json")) as fh:
            res = json.load(fh)
    line = json.dumps(res)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
