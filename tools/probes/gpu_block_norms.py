#!/usr/bin/env python3
"""Block norm maps (the reference's experiments/block_norm_visualization.py): what reading them costs on top of the encoder.
ViT-L (synthetic weights), bf16, 504x504, batch 1 and 32; the same patch tokens go through
  a  encoder   the unhooked encoder (model.imgencoder), the baseline
  b  hooks     a forward hook on every block (the encoder exports every block's fp32 [B, 1 + gh gw, F] tensor), then per block
               tensor.norm(dim=-1) in torch, the cls token dropped, the map copied to the host and normalised there by its own min / max to
               uint8 per image - the script's capture and BlockData.__init__
  c  native    imgencoder.block_norms (norms written inside the encoder pass) + postprocess.block_norm_display (tiles and min / max on the device)
All three run in this one process, one after the other; an exception in one ends the run. Times are HIP events on the current stream around
STEPS calls, best of ROUNDS (b includes its host part: the last host copy synchronises, the events bracket it). Memory is torch's peak allocated
bytes above the level before the call (the library's own workspace is a torch allocation too; it is warm before the measurement).
Prints one JSON line (and writes it to --out PATH when given). Run it under a time limit: timeout -k 10 600 python tools/probes/gpu_block_norms.py"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
from muggled_dpt_amd import native  # noqa: E402
from muggled_dpt_amd import postprocess as pp  # noqa: E402

STEPS, ROUNDS = 3, 3
SIZE = 504


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


def peak_extra_mb(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    del out
    return (peak - base) / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--config", default="vitl")
    args = ap.parse_args()
    from muggled_dpt_amd import make_depthanythingv2_dpt_from_original_state_dict
    from muggled_dpt_amd.synthetic import make_synthetic_original_state_dict
    cfg, model = make_depthanythingv2_dpt_from_original_state_dict(make_synthetic_original_state_dict(args.config, 0))
    model = model.to("cuda", torch.bfloat16)
    nb = cfg["num_blocks"]
    bps = nb // 4
    blocks = [model.imgencoder.stages[i // bps].blocks[i % bps] for i in range(nb)]
    res = {"probe": "gpu_block_norms", "source_hash": native.source_hash(), "config": args.config, "dtype": "bf16", "size": SIZE, "blocks": nb,
           "steps": STEPS, "rounds": ROUNDS}

    def hooked(tokens, hw):
        got = []
        handles = [blk.register_forward_hook(lambda mod, a, out: got.append(out)) for blk in blocks]
        try:
            model.imgencoder(tokens, hw)
        finally:
            for h in handles:
                h.remove()
        tiles = []
        for t in got:
            n = t.norm(dim=-1)[:, 1:].reshape(t.shape[0], hw[0], hw[1]).float().cpu().numpy()
            for img in n:
                lo, hi = img.min(), img.max()
                tiles.append(np.round(((img - lo) / (hi - lo)) * 255).astype(np.uint8))
        return got, tiles

    def captured(tokens, hw):
        _, norms = model.imgencoder.block_norms(tokens, hw)
        return norms, pp.block_norm_display(norms)

    with torch.inference_mode():
        for b in (1, 32):
            x = torch.randn(b, 3, SIZE, SIZE, generator=torch.Generator().manual_seed(b)).to("cuda", torch.bfloat16)
            tokens, hw = model.patch_embed(x)
            model.imgencoder(tokens, hw)  # engine and workspace exist
            torch.cuda.synchronize()
            for name, fn in (("a_encoder", lambda: model.imgencoder(tokens, hw)), ("b_hooks", lambda: hooked(tokens, hw)),
                             ("c_native", lambda: captured(tokens, hw))):
                res[f"{name}_ms_b{b}"] = round(timed(fn), 3)
                res[f"{name}_peak_extra_mb_b{b}"] = round(peak_extra_mb(fn), 1)
                print(json.dumps(res), flush=True)
            a, c = res[f"a_encoder_ms_b{b}"], res[f"c_native_ms_b{b}"]
            res[f"c_minus_a_ms_b{b}"] = round(c - a, 3)
            res[f"c_minus_a_pct_b{b}"] = round(100 * (c - a) / a, 2)
            res[f"b_minus_a_ms_b{b}"] = round(res[f"b_hooks_ms_b{b}"] - a, 3)
            # the two kernels alone
            lib = native.load()
            lib.mdpt_profile_enable(1)
            captured(tokens, hw)
            torch.cuda.synchronize()
            buf = native.ctypes.create_string_buffer(1 << 16)
            lib.mdpt_profile_report(buf, len(buf))
            lib.mdpt_profile_enable(0)
            for k in json.loads(buf.value.decode()).get("kernels", []):
                if k["name"] in ("row_norm_kernel", "block_norm_tiles_kernel"):
                    res[f"profile_{k['name']}_ms_b{b}"] = round(k["total_ms"], 4)
                    res[f"profile_{k['name']}_launches_b{b}"] = k["launches"]
            if f"profile_row_norm_kernel_ms_b{b}" in res:
                read = nb * b * hw[0] * hw[1] * cfg["features_per_token"] * 4
                res[f"row_norm_GBps_b{b}"] = round(read / (res[f"profile_row_norm_kernel_ms_b{b}"] * 1e-3) / 1e9, 1)
            del tokens, x
            torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
