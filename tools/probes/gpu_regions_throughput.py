#!/usr/bin/env python3
"""Region throughput: ViT-L bf16, 64 seeded boxes of mixed sizes (sides 200 to 2000 px) out of eight synthetic 3024x4032 uint8 photos, depth
maps per second, from host photos and from device-resident photos, each three ways:
  a  a packed copy of every box, then inference_images (the route without region inference)
  b  a loop of inference() on packed copies (device photos: inference_batch on a one-frame packed copy; inference takes host arrays)
  c  inference_regions (boxes read in place on the device; host boxes staged one by one)
The copies of a and b are inside the timed step: they are what those routes cost. Square sizing (one tensor size, 504 x 504), chunks of 32.
Every step is timed with HIP events on the current stream; best of ROUNDS rounds of STEPS calls each. Prints one JSON line (and writes it
to --out PATH when given)."""
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

PHOTOS, PHOTO_HW, N, STEPS, ROUNDS = 8, (3024, 4032), 64, 2, 3


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
    """PHOTOS uint8 BGR photos of PHOTO_HW: smooth gradients plus noise (not that the forward cares)"""
    rng = np.random.default_rng(seed)
    h, w = PHOTO_HW
    out = []
    for _ in range(PHOTOS):
        base = rng.integers(0, 256, (h // 8 + 1, w // 8 + 1, 3), dtype=np.uint8)
        img = np.repeat(np.repeat(base, 8, axis=0), 8, axis=1)[:h, :w]
        out.append(np.ascontiguousarray(img ^ rng.integers(0, 32, (h, w, 3), dtype=np.uint8)))
    return out


def boxes(seed=1):
    """N (image, x1, y1, x2, y2) boxes, eight per photo, sides 200 .. 2000 px (log-uniform, so small and large boxes both occur), anywhere"""
    rng = np.random.default_rng(seed)
    h, w = PHOTO_HW
    out = []
    for k in range(N):
        bw, bh = (int(round(200 * 10 ** rng.uniform(0, 1))) for _ in range(2))
        x1, y1 = int(rng.integers(0, w - bw + 1)), int(rng.integers(0, h - bh + 1))
        out.append((k % PHOTOS, x1, y1, x1 + bw, y1 + bh))
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
    regions = boxes()
    box_bytes = sum(3 * (x2 - x1) * (y2 - y1) for _, x1, y1, x2, y2 in regions)

    def host_copies():
        return [np.ascontiguousarray(images[i][y1:y2, x1:x2]) for i, x1, y1, x2, y2 in regions]

    def dev_copies():
        return [dev_images[i][y1:y2, x1:x2].contiguous() for i, x1, y1, x2, y2 in regions]

    def host_loop():
        for f in host_copies():
            model.inference(f)

    def dev_loop():
        for f in dev_copies():
            model.inference_batch(f[None])

    ms = {"host_a_copies_then_images": timed(lambda: model.inference_images(host_copies())),
          "host_b_inference_loop": timed(host_loop),
          "host_c_regions": timed(lambda: model.inference_regions(images, regions)),
          "device_a_copies_then_images": timed(lambda: model.inference_images(dev_copies())),
          "device_b_inference_loop": timed(dev_loop),
          "device_c_regions": timed(lambda: model.inference_regions(dev_images, regions))}
    want = model.inference_images(host_copies())
    same = {"host": all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in zip(model.inference_regions(images, regions), want)),
            "device": all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in zip(model.inference_regions(dev_images, regions), want))}
    rec = {"probe": "gpu_regions_throughput", "model": "vitl", "dtype": "bf16", "photos": PHOTOS, "photo_hw": list(PHOTO_HW), "regions": N,
           "box_side_px": [min(min(r[3] - r[1], r[4] - r[2]) for r in regions), max(max(r[3] - r[1], r[4] - r[2]) for r in regions)],
           "box_megabytes": round(box_bytes / 1e6, 1), "photo_megabytes": round(PHOTOS * 3 * PHOTO_HW[0] * PHOTO_HW[1] / 1e6, 1), "batch_size": 32,
           "tensor_hw": list(want[0].shape[1:]), "ms_per_set": {k: round(v, 3) for k, v in ms.items()},
           "maps_per_s": {k: round(N * 1e3 / v, 1) for k, v in ms.items()},
           "c_over_a": {"host": round(ms["host_a_copies_then_images"] / ms["host_c_regions"], 3),
                        "device": round(ms["device_a_copies_then_images"] / ms["device_c_regions"], 3)},
           "equal_to_packed_copies_bits": same, "box": box(), "source_hash": native.source_hash(), "torch": torch.__version__}
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
