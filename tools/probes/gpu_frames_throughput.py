#!/usr/bin/env python3
"""Frame workload throughput: ViT-L bf16, 32 uint8 frames of 518 x 518 (model tensor 504 x 504), depth maps per second through
  a  a loop of inference() (the reference's per-frame call)
  b  prepare_image_bgr per frame, torch.cat, forward
  c  inference_batch from host frames (pinned staging, one mdpt_forward_bgr_batch)
  d  inference_batch from device-resident frames
  e  forward on the already prepared [32,3,504,504] tensor (bench.py's conditions)
and the display tail of the same 32 maps to 518 x 518 BGR (reverse, high contrast, a colormap LUT): depth_to_color against the host tail
(scale + uint8 on the device per map as run_video.py does, then 255 - x, equalizeHist and the LUT in numpy). Every step is timed with HIP
events on the current stream (host tail: wall clock, it ends on the host); best of ROUNDS rounds of STEPS calls each. Prints one JSON line
(and writes it to --out PATH when given)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
import bench  # noqa: E402
from muggled_dpt_amd import native  # noqa: E402
from muggled_dpt_amd import postprocess as pp  # noqa: E402

B, SIDE, STEPS, ROUNDS = 32, 518, 5, 3


def timed(fn, steps=STEPS, rounds=ROUNDS):
    """best per-call milliseconds over `rounds` rounds of `steps` calls, HIP events around each round"""
    fn()
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(rounds):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(steps):
            fn()
        t1.record()
        t1.synchronize()
        best = min(best, t0.elapsed_time(t1) / steps)
    return best


def host_equalize(x):
    hist = np.bincount(x.ravel(), minlength=256)
    i = int(np.flatnonzero(hist)[0])
    if hist[i] == x.size:
        return np.full_like(x, i)
    scale = np.float32(255.0) / np.float32(x.size - hist[i])
    cum = np.cumsum(hist) - np.cumsum(hist)[i]
    lut = np.clip(np.rint(cum.astype(np.float32) * scale), 0, 255).astype(np.uint8)
    lut[: i + 1] = 0
    return lut[x]


def box() -> str:
    """the device the numbers were taken on: name, architecture, compute units"""
    pr = torch.cuda.get_device_properties(0)
    return f"{pr.name} ({getattr(pr, 'gcnArchName', '?')}, {pr.multi_processor_count} CUs)"


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    model, _ = bench.make_model_and_weights("vitl")
    model = model.to("cuda", torch.bfloat16)
    rng = np.random.default_rng(0)
    frames = [rng.integers(0, 256, (SIDE, SIDE, 3), dtype=np.uint8) for _ in range(B)]
    dev_frames = torch.from_numpy(np.stack(frames)).cuda()
    with torch.inference_mode():
        x = torch.cat([model.prepare_image_bgr(f) for f in frames])

    def a():
        for f in frames:
            model.inference(f)

    def b():
        with torch.inference_mode():
            model(torch.cat([model.prepare_image_bgr(f) for f in frames]))

    def e():
        with torch.inference_mode():
            model(x)

    ms = {"a_inference_loop": timed(a), "b_prepare_cat_forward": timed(b), "c_inference_batch_host": timed(lambda: model.inference_batch(frames)),
          "d_inference_batch_device": timed(lambda: model.inference_batch(dev_frames)), "e_forward_prepared": timed(e)}
    # d and e once more, interleaved, so that a clock drift between their first measurements cannot decide their order
    ms["d_inference_batch_device"] = min(ms["d_inference_batch_device"], timed(lambda: model.inference_batch(dev_frames)))
    ms["e_forward_prepared"] = min(ms["e_forward_prepared"], timed(e))
    y_d, y_e = model.inference_batch(dev_frames), model(x)
    same = bool(torch.equal(y_d.view(torch.int16), y_e.view(torch.int16)))

    cmap = rng.integers(0, 256, (1, 256, 3), dtype=np.uint8)
    pred = y_e
    tail_dev = timed(lambda: pp.depth_to_color(pred, (SIDE, SIDE), True, True, cmap))

    def host_tail():
        out = []
        for i in range(B):
            u8 = pp.convert_to_uint8(pp.scale_prediction(pred[i:i + 1], (SIDE, SIDE))).cpu().numpy()[0]
            out.append(cmap[0][host_equalize(255 - u8)])
        return out

    host_tail()
    tail_host = float("inf")
    for _ in range(ROUNDS):
        torch.cuda.synchronize()
        t = time.perf_counter()
        host_tail()
        tail_host = min(tail_host, (time.perf_counter() - t) * 1e3)
    got = pp.depth_to_color(pred, (SIDE, SIDE), True, True, cmap).cpu().numpy()
    tail_same = all(np.array_equal(got[i], h) for i, h in enumerate(host_tail()))

    rec = {"probe": "gpu_frames_throughput", "model": "vitl", "dtype": "bf16", "batch": B, "frame": [SIDE, SIDE], "model_hw": list(x.shape[2:]),
           "ms_per_batch": {k: round(v, 3) for k, v in ms.items()}, "maps_per_s": {k: round(B * 1e3 / v, 1) for k, v in ms.items()},
           "d_equals_e_bits": same, "tail_ms_per_batch": {"depth_to_color": round(tail_dev, 3), "host_numpy": round(tail_host, 3)},
           "tail_equal": tail_same, "box": box(), "source_hash": native.source_hash(),
           "torch": torch.__version__}
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
