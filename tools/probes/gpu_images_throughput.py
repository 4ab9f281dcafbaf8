#!/usr/bin/env python3
"""Photo-set throughput: ViT-L bf16, a seeded set of 64 synthetic uint8 photos in common sizes (640x480, 1280x720, 1920x1080, 1080x1920,
3024x4032, 800x800, shuffled), depth maps per second, for square sizing (the default: one tensor size, 504 x 504) and aspect sizing (a few
groups), each three ways:
  a  a loop of inference() (the reference's run_image.py calls it once per file)
  b  inference_images from host arrays (one pinned staging copy and one mdpt_forward_bgr_frames call per chunk of 32)
  c  inference_images from device-resident images
and the display tail of the square-sized maps back to every photo's own size (reverse, high contrast, a colormap LUT): a loop of
depth_to_color against one depth_to_color_images call. Every step is timed with HIP events on the current stream; best of ROUNDS rounds of
STEPS calls each. Prints one JSON line (and writes it to --out PATH when given)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
import bench  # noqa: E402
from muggled_dpt_amd import native  # noqa: E402
from muggled_dpt_amd import postprocess as pp  # noqa: E402
from muggled_dpt_amd.dpt_model import image_chunks  # noqa: E402

N, STEPS, ROUNDS = 64, 2, 3
PHOTO_WH = [(640, 480), (1280, 720), (1920, 1080), (1080, 1920), (3024, 4032), (800, 800)]


def timed(fn, steps=STEPS, rounds=ROUNDS):
    """best per-call milliseconds over `rounds` rounds of `steps` calls, HIP events around each round"""
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


def box() -> str:
    """the device the numbers were taken on: name, architecture, compute units"""
    pr = torch.cuda.get_device_properties(0)
    return f"{pr.name} ({getattr(pr, 'gcnArchName', '?')}, {pr.multi_processor_count} CUs)"


def photos(seed=0):
    """N uint8 BGR images, the sizes of PHOTO_WH in turn, shuffled; smooth gradients plus noise (not that the forward cares)"""
    rng = np.random.default_rng(seed)
    whs = [PHOTO_WH[i % len(PHOTO_WH)] for i in range(N)]
    rng.shuffle(whs)
    out = []
    for w, h in whs:
        base = rng.integers(0, 256, (h // 8 + 1, w // 8 + 1, 3), dtype=np.uint8)
        img = np.repeat(np.repeat(base, 8, axis=0), 8, axis=1)[:h, :w]
        out.append(np.ascontiguousarray(img ^ rng.integers(0, 32, (h, w, 3), dtype=np.uint8)))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    model, _ = bench.make_model_and_weights("vitl")
    model = model.to("cuda", torch.bfloat16)
    images = photos()
    dev_images = [torch.from_numpy(f).cuda() for f in images]
    pe = model.patch_embed
    rec = {"probe": "gpu_images_throughput", "model": "vitl", "dtype": "bf16", "images": N, "photo_wh": PHOTO_WH, "batch_size": 32}
    ms, groups, same = {}, {}, {}
    for name, square in (("square", True), ("aspect", False)):
        plan = image_chunks([f.shape[:2] for f in images], lambda h, w: pe._scaled_hw(h, w, None, square), 32)
        groups[name] = [[list(hw), len(idx)] for hw, idx in plan]

        def loop(square=square):
            for f in images:
                model.inference(f, use_square_sizing=square)

        ms[f"{name}_a_inference_loop"] = timed(loop)
        ms[f"{name}_b_images_host"] = timed(lambda: model.inference_images(images, use_square_sizing=square))
        ms[f"{name}_c_images_device"] = timed(lambda: model.inference_images(dev_images, use_square_sizing=square))
        y_b = model.inference_images(images, use_square_sizing=square)
        y_c = model.inference_images(dev_images, use_square_sizing=square)
        same[name] = all(torch.equal(a.view(torch.int16), model.inference(images[i], use_square_sizing=square).view(torch.int16)) and
                         torch.equal(a.view(torch.int16), c.view(torch.int16)) for i, (a, c) in enumerate(zip(y_b, y_c)))
    cmap = np.random.default_rng(1).integers(0, 256, (1, 256, 3), dtype=np.uint8)
    preds = model.inference_images(dev_images)
    whs = [(f.shape[1], f.shape[0]) for f in images]

    def tail_loop():
        for p, wh in zip(preds, whs):
            pp.depth_to_color(p, wh, True, True, cmap)

    tail = {"depth_to_color_loop": timed(tail_loop), "depth_to_color_images": timed(lambda: pp.depth_to_color_images(preds, whs, True, True, cmap))}
    got = pp.depth_to_color_images(preds, whs, True, True, cmap)
    tail_same = all(torch.equal(g, pp.depth_to_color(p, wh, True, True, cmap)) for g, p, wh in zip(got, preds, whs))
    rec.update({"groups": groups, "ms_per_set": {k: round(v, 3) for k, v in ms.items()}, "maps_per_s": {k: round(N * 1e3 / v, 1) for k, v in ms.items()},
                "equal_to_inference_bits": same, "tail_ms_per_set": {k: round(v, 3) for k, v in tail.items()},
                "tail_images_per_s": {k: round(N * 1e3 / v, 1) for k, v in tail.items()}, "tail_equal": tail_same, "box": box(),
                "source_hash": native.source_hash(), "torch": torch.__version__})
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
