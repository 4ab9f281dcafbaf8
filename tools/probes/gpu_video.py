#!/usr/bin/env python3
"""Temporally stable video depth (muggled_dpt_amd.video): the device stages against the route without them.
  maps     ViT-L (synthetic weights), bf16, 32 frames of 504 x 504 (one random photo under a moving brightness ramp) -> maps of 504 x 504
  clips    T = 32 and T = 1 (the one frame fitted to a state, so that the fit runs)
  device   video_fit, video_filter, video_display to 1920 x 1080 and the whole stabilize_video: HIP events, best of ROUNDS rounds of STEPS calls,
           allocation included; and the library profiler's time per launch
  torch    the route without the feature, the same arithmetic in torch on the device in fp64: per pair the masked sums and the reweighting
           rounds (vectorised over the pairs), a Python loop over the frames for the filter; postprocess.depth_to_color for the display
  bytes    what each stage must move at least - fit: (rounds + 1) passes reading two frames per pair; filter: one read of the frames, one fp32
           write; display: a read of the fp32 maps, and per display pixel 4 B written + 4 B read (resize), 1 B written + 1 B read, 3 B written -
           against HBM's 8 TB/s. No counter run is made here: what bounds a kernel is not separated.
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

STEPS, ROUNDS, PROFILE_CALLS, FRAMES = 5, 3, 3, 32
TARGET_WH = (1920, 1080)
HBM_GBS = 8000.0
STEP_LIMITS = {"maps": 400, "device": 400}  # seconds


def step_maps(work):
    import torch
    from muggled_dpt_amd import make_depthanythingv2_dpt_from_original_state_dict
    from muggled_dpt_amd.synthetic import make_synthetic_original_state_dict
    _, model = make_depthanythingv2_dpt_from_original_state_dict(make_synthetic_original_state_dict("vitl", 0))
    model = model.to("cuda", torch.bfloat16)
    rng = np.random.default_rng(0)
    photo = rng.integers(0, 200, (504, 504, 3)).astype(np.float64)
    ramp = np.linspace(0.0, 1.0, 504)[None, :, None]
    frames = [np.clip(photo + 40.0 * np.roll(ramp, 5 * t, axis=1) + rng.normal(0.0, 2.0, photo.shape), 0, 255).astype(np.uint8) for t in range(FRAMES)]
    torch.save(model.inference_batch(frames, 504, True).cpu(), os.path.join(work, "maps.pt"))


def torch_fit(x, prev, rounds=3, c=2.0):
    """the pairs' reweighted fits in torch, fp64, all pairs at once -> (a, b, s2) [T]"""
    import torch
    xs = x.double().flatten(1)
    ys = torch.cat([prev.double()[None], x[:-1].double()]).flatten(1)
    ok = torch.isfinite(xs) & torch.isfinite(ys)
    xs, ys = torch.where(ok, xs, 0.0), torch.where(ok, ys, 0.0)
    w = ok.double()
    for k in range(rounds + 1):
        n, sx, sy = w.sum(1), (w * xs).sum(1), (w * ys).sum(1)
        sxx, sxy, syy = (w * xs * xs).sum(1), (w * xs * ys).sum(1), (w * ys * ys).sum(1)
        a = (n * sxy - sx * sy) / (n * sxx - sx * sx)
        b = (sy - a * sx) / n
        s2 = ((syy - a * sxy - b * sy) / n).clamp_min(0.0)
        if k < rounds:
            r = a[:, None] * xs + b[:, None] - ys
            w = ok.double() / (1.0 + r * r / (c * c * s2[:, None]))
    return a, b, s2


def torch_filter(x, table, prev_out, alpha=0.3, tau=3.0):
    """the filter in torch, fp64, a Python loop over the frames"""
    import torch
    out, o = [], prev_out
    for t in range(x.shape[0]):
        s = table[t, 0] * x[t].double() + table[t, 1]
        d = s - o.double()
        d2 = d * d
        g = d2 / (d2 + (tau * table[t, 2]) ** 2)
        o = torch.where(table[t, 3] != 0, s, o.double() + (alpha + (1.0 - alpha) * g) * d).float()
        out.append(o)
    return torch.stack(out)


def step_device(work):
    import torch
    from muggled_dpt_amd import native, video
    from muggled_dpt_amd import postprocess as pp
    maps = torch.load(os.path.join(work, "maps.pt")).cuda()
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
        return round(best, 4)

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

    _, _, state = video.stabilize_video(maps[:1])
    results = []
    for T in (32, 1):
        x = maps[1:1 + T] if T == 1 else maps
        st = state if T == 1 else None
        table = video.video_fit(x, st)
        stable = video.video_filter(x, table, st)
        prev = state.raw if T == 1 else x[0]
        prev_out = state.out if T == 1 else torch.zeros_like(stable[0])
        px, out_px, elt = T * 504 * 504, T * TARGET_WH[0] * TARGET_WH[1], x.element_size()
        fit_k, fit_l = profiled(lambda: video.video_fit(x, st))
        fil_k, fil_l = profiled(lambda: video.video_filter(x, table, st))
        dis_k, dis_l = profiled(lambda: video.video_display(stable, table, st, TARGET_WH))
        fit_bytes, fil_bytes = 4 * 2 * px * elt, px * (elt + 4)
        dis_bytes = 2 * px * 4 + out_px * (4 + 4 + 1 + 1 + 3)
        a, b, s2 = torch_fit(x, prev)
        pairs = slice(0, T) if T == 1 else slice(1, T)
        dev_a = table[pairs, 0] / (state.ab[0] if T == 1 else torch.cat([table[:1, 0], table[:-1, 0]])[pairs])
        res = {"frames": T, "map_hw": [504, 504], "target_wh": list(TARGET_WH),
               "video_fit_ms": timed(lambda: video.video_fit(x, st)), "video_fit_kernels_ms": fit_k, "video_fit_launches": fit_l,
               "video_filter_ms": timed(lambda: video.video_filter(x, table, st)), "video_filter_kernels_ms": fil_k, "video_filter_launches": fil_l,
               "video_display_ms": timed(lambda: video.video_display(stable, table, st, TARGET_WH)), "video_display_kernels_ms": dis_k,
               "video_display_launches": dis_l, "stabilize_video_ms": timed(lambda: video.stabilize_video(x, st)),
               "torch_fit_ms": timed(lambda: torch_fit(x, prev)), "torch_filter_ms": timed(lambda: torch_filter(x, table, prev_out)),
               "depth_to_color_ms": timed(lambda: pp.depth_to_color(stable, TARGET_WH)),
               "fit_min_bytes": fit_bytes, "fit_share_of_hbm": round(fit_bytes / sum(fit_k.values()) / 1e6 / HBM_GBS, 4),
               "filter_min_bytes": fil_bytes, "filter_share_of_hbm": round(fil_bytes / sum(fil_k.values()) / 1e6 / HBM_GBS, 4),
               "display_min_bytes": dis_bytes, "display_share_of_hbm": round(dis_bytes / sum(dis_k.values()) / 1e6 / HBM_GBS, 4),
               "cuts": int(table[:, 3].sum()), "pair_scale_max_rel_diff_to_torch_route": float(((dev_a - a[pairs]) / a[pairs]).abs().max()),
               "filter_max_abs_diff_to_torch_route": float((stable - torch_filter(x, table, prev_out)).abs().max())}
        results.append(res)
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
                raise SystemExit(f"gpu_video: step '{step}' ended with status {r.returncode}; stopping")
        res = {"probe": "gpu_video", "source_hash": native.source_hash(), "gpus": 1, "model": "vitl synthetic bf16", "steps": STEPS, "rounds": ROUNDS,
               "hbm_gb_s": HBM_GBS, "counter_run": "none: what bounds the kernels is not separated", "configs": json.load(open(os.path.join(work, "device.json")))}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
