#!/usr/bin/env python3
"""Headline benchmark: depth-maps/sec of the DPT path on MI355X.

    python bench.py --gpus N --steps K --warmup W                          # BASELINE configs[2]: DA-V2 ViT-L, 518x518 (-> 504), batch 32, bf16
    python bench.py --gpus N --steps K --warmup W --full                   # + roofline, CPU baseline, other modes, other configurations
    python bench.py --precision bf16x3 --steps 20                          # the same workload in the mode that meets the 1e-3 tolerance
    python bench.py --size 1036 --batch 8                                  # the other north-star size (1036x1036, 5477 tokens)
    python bench.py --model beitl   (or swinl)                             # BASELINE configs[4]: MiDaS v3.1 BEiT-L / SwinV2-L, 384x384, batch 16
    python bench.py ... --dump-outputs DIR                                 # + DIR/depth.npy: the depth maps of the last timed step (float32)
    (N>1: python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...)

One "step" = one pass of the hot path (mdpt_forward through the C ABI) over one batch of synthetic images per GPU,
followed (N>1) by the RCCL all-gather of the depth maps. Default workload = BASELINE.json configs[2]/[3]:
ViT-L, "518x518" images (= 504x504 model tensor, the reference's own size snapping), bf16 MFMA with fp32 accumulate,
batch 32 per GPU (weak scaling: global batch 32*N), seeded synthetic weights and inputs already resident in HBM.
Rank 0 prints ONE JSON line (see DESIGN.md "Measurement" for every field).

A plain run sets up, warms up, times the steps, writes --dump-outputs and prints the line; everything else it can measure or check
(per-kernel profile passes and roofline, the H2D-inclusive rate, the CPU baseline and error, the other arithmetic modes, the other
BASELINE configurations under `secondary`, the N-rank gather self-check) runs only with --full, after the timed region.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

import torch
import torch.distributed as dist

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

from muggled_dpt_amd import native  # noqa: E402
from muggled_dpt_amd.parallel import DataParallelDepth, init_distributed  # noqa: E402

# algorithmic GFLOP per depth map of the reference graph (2 FLOP/MAC), SURVEY §8(d) / BASELINE.md §4
GFLOP_PER_MAP = {("vitl", 504): 1224.9, ("vitl", 532): 1385.8, ("vitl", 1036): 7424.0,
                 ("vits", 504): 107.3, ("vits", 532): 123.5, ("vits", 1036): 875.2,
                 ("beitl", 384): 516.4, ("swinl", 384): 343.7}
PEAK_BF16_TFLOPS = 2500.0  # MI355X dense bf16 MFMA (MI355X_MICROARCH.md)
# what a loop of nothing but bf16 MFMAs on random operands sustains on this part (power limit: 1.93 GHz of the 2.4 GHz the nominal peak is
# quoted at; tools/probes/mfma_power.hip, profiles/r03_mfma_power_probe.txt). Context for `roofline.frac`, never its denominator.
SUSTAINED_BF16_TFLOPS = 2030.0
DUMP_BYTES = 64 << 20  # --dump-outputs cap
FAMILY = {"vitl": "Depth-Anything-V2 ViT-L", "vits": "Depth-Anything-V2 ViT-S", "vitb": "Depth-Anything-V2 ViT-B",
          "beitl": "MiDaS v3.1 BEiT-L-384", "swinl": "MiDaS v3.1 SwinV2-L-384"}
SYNTH_NAME = {"beitl": "beit_large_384", "swinl": "swin2_large_384"}


def make_model_and_weights(name: str, want_weights: bool = False, enable_cache: bool = False):
    """(model on CPU, (cfg, flat weight dict) for the oracle or None). Seeded synthetic checkpoints in the ORIGINAL key layout go
    through the same factories a real .pth would (make_*_dpt_from_*_state_dict)."""
    from muggled_dpt_amd.state_dict_conversion import flatten_components
    if name == "beitl":
        from muggled_dpt_amd import make_beit_dpt_from_midas_v31_state_dict as make
        from muggled_dpt_amd import state_dict_conversion_beit as conv
        from muggled_dpt_amd.synthetic import make_synthetic_beit_state_dict as synth
        osd = synth(SYNTH_NAME[name], 0)
    elif name == "swinl":
        from muggled_dpt_amd import make_swinv2_dpt_from_midas_v31_state_dict as make
        from muggled_dpt_amd import state_dict_conversion_swinv2 as conv
        from muggled_dpt_amd.synthetic import make_synthetic_swinv2_state_dict as synth
        osd = synth(SYNTH_NAME[name], 0)
    else:
        from muggled_dpt_amd import make_depthanythingv2_dpt_from_original_state_dict as make
        from muggled_dpt_amd import state_dict_conversion as conv
        from muggled_dpt_amd.synthetic import make_synthetic_original_state_dict as synth
        osd = synth(name, 0)
    cfg, model = make(osd, enable_cache)  # (run_video.py:144 builds its model with the cache on; run_image.py:129 without)
    ow = None
    if want_weights:
        ocfg = conv.get_model_config_from_state_dict(osd) if hasattr(conv, "get_model_config_from_state_dict") and name not in SYNTH_NAME else cfg
        ow = (ocfg, flatten_components(conv.convert_state_dict_keys(ocfg, osd)))
    return model, ow


def cpu_name() -> str:
    try:
        for ln in open("/proc/cpuinfo"):
            if ln.startswith("model name"):
                return ln.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown CPU"


def cpu_baseline(args, x_cpu: torch.Tensor, gpu_out: torch.Tensor | None, sweep: bool = True):
    """Oracle (CPU restatement of the reference, kind="port") timed on this box's host cores on a bounded sample (~10-30 s).
    `value` is the BEST arm of a short thread sweep (the reference's own policy, os.cpu_count()//2 threads
    - demo_helpers/misc.py:161-166 -, oversubscribes a quota-limited container and understates the host); the policy arm is reported
    beside it as `policy_value`."""
    from oracle import dpt_oracle

    ncpu = os.cpu_count() or 2
    policy = max(1, ncpu // 2)
    _, (cfg, w) = make_model_and_weights(args.model, want_weights=True)
    n_img = 8 if args.model == "vits" else (1 if args.size > 600 else 2)

    def time_arm(threads: int, n: int, warm: bool):
        torch.set_num_threads(threads)
        if warm:
            dpt_oracle.forward(w, cfg, x_cpu[:1])  # thread pool, oneDNN primitive caches
        t0 = time.perf_counter()
        first = None
        for i in range(n):
            y = dpt_oracle.forward(w, cfg, x_cpu[i % x_cpu.shape[0]: i % x_cpu.shape[0] + 1])
            if i == 0:
                first = y
        return n / (time.perf_counter() - t0), first

    arms = {}
    pol_rate, ref = time_arm(policy, n_img, True)
    arms[policy] = pol_rate
    if sweep:
        for t in (8, 16, 32, 64):
            if t < ncpu and t != policy:
                arms[t], _ = time_arm(t, 1, True)
    best = max(arms, key=arms.get)
    if best != policy:  # confirm the winner on the full sample
        arms[best] = max(arms[best], time_arm(best, n_img, False)[0])
    torch.set_num_threads(policy)
    out = {"value": round(arms[best], 4), "unit": "depth-maps/s", "cores": best, "kind": "port", "cpu": cpu_name(),
           "policy_value": round(pol_rate, 4), "policy_cores": policy, "thread_sweep": {str(k): round(v, 4) for k, v in sorted(arms.items())},
           "sample": f"{n_img} images of the same workload one at a time (batch 1: the reference's run_image.py path), fp32, torch {torch.__version__} CPU; "
                     f"value = best arm of a thread sweep {sorted(arms)} (one image per arm after a warm-up, winner re-timed on the sample), "
                     f"policy_value = os.cpu_count()//2 = {policy} threads (the reference's thread policy; os.cpu_count()={ncpu})"}
    return out, error_vs(ref, gpu_out), ref


def error_vs(ref: torch.Tensor, gpu_out: torch.Tensor | None):
    """The north-star error figure of image 0: max|y - y_cpu| and the same relative to max|y_cpu|."""
    if gpu_out is None:
        return None
    d = (gpu_out[:1].double().cpu() - ref.double()).abs().max()
    return {"max_abs": float(d), "rel_to_max": float(d / ref.double().abs().max())}


def hbm_traffic(args, kernel_name: str):
    """HBM bytes per launch of `kernel_name` from the committed PMC passes (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE on this exact workload,
    corrected per MI355X_MICROARCH.md; tools/collect_profiles.sh + tools/summarize_pmc.py). bench.py cannot run PMC passes itself, so the
    summary is stamped with a hash of the kernel sources it was taken on and is reported only while that hash still matches (else null)."""
    if args.model != "vitl" or args.batch != 32 or args.size != 504 or args.precision != "bf16":
        return None
    sha = native.source_hash()
    for tag in ("r06", "r05", "r04", "r03", "r02", "r01"):
        path = os.path.join(REPO, "profiles", f"{tag}_hbm_traffic.json")
        if not os.path.exists(path):
            continue
        rows = json.load(open(path))
        if rows.get("_meta", {}).get("csrc_sha") != sha:
            continue
        # (rocprofv3 prints every template argument - since round 6 the 16-bit forms end in ", false" (no fp8 cross terms) - the library's own profiler the short name)
        rec = rows.get(kernel_name) or (rows.get(kernel_name[:-1] + ", false>") if kernel_name.endswith(">") else None)
        return None if rec is None else int((rec["fetch_mb_per_launch"] + rec["write_mb_per_launch"]) * 1e6)
    return None


def roofline(args, pr, how):
    """Dominant GEMM kernel (by accumulated time) of a profiler report. `gflop` in the report is ALGORITHMIC (2 M N K, one pass); in the
    bf16x3 mode every product runs as three MFMA passes, so the executed-MFMA fraction is three times the algorithmic one."""
    gemms = [k for k in pr["kernels"] if k["gflop"] > 0 and k["name"].startswith("gemm")]
    dom = max(gemms, key=lambda k: k["total_ms"]) if gemms else pr["kernels"][0]
    r = {"bound": "mfma", "achieved": dom["tflops"], "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
         "frac": round(dom["tflops"] / PEAK_BF16_TFLOPS, 4), "traffic": hbm_traffic(args, dom["name"]), "kernel": dom["name"],
         "launches": dom["launches"], "avg_us": dom["avg_us"], "gflop_per_launch": round(dom["gflop"] / dom["launches"], 3), "measured": how}
    r["sustained_mfma_tflops"] = SUSTAINED_BF16_TFLOPS  # measured ceiling for random-data bf16 MFMA; frac stays against the nominal peak
    x3 = args.precision in ("bf16x3", "fp16x3")  # (mixed: the dominant kernel is a single-pass encoder GEMM)
    r["frac_of_sustained"] = round((3 if x3 else 1) * dom["tflops"] / SUSTAINED_BF16_TFLOPS, 4)
    if x3:
        r["executed_mfma_tflops"] = round(3 * dom["tflops"], 2)
        r["executed_mfma_frac"] = round(3 * dom["tflops"] / PEAK_BF16_TFLOPS, 4)
        r["note"] = "achieved/frac are algorithmic (one product per MAC); the x3 modes execute three MFMA passes per product"
    return r


def set_alone(lib, handle, alone: bool):
    """`alone` = nothing runs on the library's side stream: the two-stream half-batch split off AND the reassembly branches behind the
    encoder instead of beside it (mdpt_debug_set_reassemble_overlap 0; the default rule queues them on the side stream for every unsplit
    forward of a wide encoder, so `mdpt_set_batch_split(0)` alone leaves launches 47+ of a ViT-L forward sharing the GPU - VERDICT r05).
    Every per-kernel roofline figure is taken in this state; the timed region runs the library's defaults."""
    native.check(lib, lib.mdpt_set_batch_split(handle, 0 if alone else 8))
    native.check(lib, lib.mdpt_debug_set_reassemble_overlap(handle, 0 if alone else 1))


def profile_pass(lib, fn, steps):
    torch.cuda.synchronize()
    lib.mdpt_profile_enable(1)
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    buf = ctypes.create_string_buffer(1 << 16)
    prof = json.loads(buf.value.decode()) if lib.mdpt_profile_report(buf, len(buf)) == 0 else None
    lib.mdpt_profile_enable(0)
    return prof


PRECISION_DTYPE = {"bf16": "bf16", "bf16x3": "bf16x3 (hi/lo split bf16 MFMA operands, 3 passes, fp32 accumulate)",
                   "fp16": "fp16 (fp16 MFMA operands, single pass, fp32 accumulate)",
                   "fp16x3": "fp16x3 (hi/lo split fp16 MFMA operands, 3 passes, fp32 accumulate)",
                   "mixed": "mixed (fp16 MFMA operands; decoder classes as split products A_hi W_hi + A_lo W_hi [+ A_hi W_lo] with the cross terms on fp8 planes "
                            "through the block-scaled MFMA: reassembly, fusion convs, 1x1 fusion projections and head conv 1 3 terms; patch embed 3 fp16 "
                            "passes, head tail 2; encoder 1 pass + token-mean compensation; fp32 accumulate)"}


def model_for_precision(name: str, precision: str, dev):
    """bf16 / fp16: a model of that torch dtype (16-bit tensors at the C ABI, the reference's GPU dtypes, demo_helpers/misc.py:61-77);
    bf16x3 / fp16x3 / mixed: a float32 model (fp32 tensors at the boundary) with the operand arithmetic selected by set_precision."""
    model, _ = make_model_and_weights(name)
    if precision in ("bf16", "fp16"):
        return model.to(dev, torch.bfloat16 if precision == "bf16" else torch.float16)
    model = model.to(dev, torch.float32)
    model.set_precision(precision)
    return model


def parity_mode_legs(args, dev, x_cpu, ref, lib):
    """The same workload in the other arithmetic modes, on ONE float32 model whose operand arithmetic is switched with set_precision
    (fp32 tensors at the boundary, so `error_vs_cpu_fp32` is the operand arithmetic's error alone):
      mixed_mode       fp16 operands, 3 passes where the error budget says so: the operating point that meets the north star's 1e-3
      fp16_mode        single-pass fp16 operands (what a torch.float16 model runs)
      fp32_class_mode  bf16x3: every product in 3 passes (fp32-class accuracy)
    Reported beside the headline bf16 number, never instead of it; `bench.py --precision <mode>` is the same measurement as a first-class
    run (full step count)."""
    model, _ = make_model_and_weights(args.model)
    model = model.to(dev, torch.float32)
    x = x_cpu.to(dev)
    steps = max(2, min(args.steps, 10))
    out = {}
    for key, prec in (("mixed_mode", "mixed"), ("fp16_mode", "fp16"), ("fp32_class_mode", "bf16x3")):
        model.set_precision(prec)
        dt, y = time_model(model, x, steps)
        with torch.inference_mode():
            handle = model._get_engine().handle
            set_alone(lib, handle, True)
            model(x)
            prof = profile_pass(lib, lambda: model(x), 2)
            set_alone(lib, handle, False)
        sub = argparse.Namespace(**{**vars(args), "precision": prec})
        rec = {"value": round(args.batch / dt, 3), "unit": "depth-maps/s", "ms_per_step": round(dt * 1e3, 3), "steps": steps,
               "dtype": PRECISION_DTYPE[prec], "boundary": "fp32 image in, fp32 depth out", "error_vs_cpu_fp32": error_vs(ref, y.float())}
        if prof and prof["kernels"]:
            rec["roofline"] = roofline(sub, prof, "HIP events, batch split off, 2 steps")
        out[key] = rec
        del y
    return out


def time_model(model, x, steps, warmup=2, warmup_seconds=0.3):
    """Mean step time over `steps` steps after at least `warmup` steps AND `warmup_seconds` of back-to-back work: a leg that starts after
    seconds of GPU idle time (model construction, the CPU baseline) otherwise times the clock ramp - seen once as 3.8 ms instead of 1.15 ms
    per step on the batch-1 leg, whose two warm-up steps were 2 ms of work."""
    with torch.inference_mode():
        t_w = time.perf_counter()
        n_w = 0
        while n_w < warmup or time.perf_counter() - t_w < warmup_seconds:
            y = model(x)
            n_w += 1
            if n_w % 8 == 0:
                torch.cuda.synchronize()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            y = model(x)
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps, y


def time_inference(model, side: int, steps: int) -> dict:
    """DPTModel.inference(image_bgr) on a `side` x `side` uint8 host image: ms per call with the host waiting for every depth map
    (`ms_per_call_sync`: the latency a frame-by-frame caller sees, run_video.py:344) and with `steps` calls queued back to back
    (`ms_per_call_pipelined`)."""
    import numpy as np
    img = np.random.default_rng(5).integers(0, 256, (side, side, 3), dtype=np.uint8)
    for _ in range(20):
        y = model.inference(img)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        y = model.inference(img)
        torch.cuda.synchronize()
    t_sync = (time.perf_counter() - t0) / steps
    t0 = time.perf_counter()
    for _ in range(steps):
        y = model.inference(img)
    torch.cuda.synchronize()
    t_pipe = (time.perf_counter() - t0) / steps
    return {"ms_per_call_sync": round(t_sync * 1e3, 3), "ms_per_call_pipelined": round(t_pipe * 1e3, 3), "output": f"{tuple(y.shape)} {str(y.dtype).replace('torch.', '')} on the device"}


def secondary_legs(args, dev, lib, vitl_model):
    """The other BASELINE.json configurations inside the default run (the driver only runs the default command): configs[1] ViT-S
    518x518 batch 1, the 1036x1036 north-star size (ViT-L, batch 8), configs[4] BEiT-L and SwinV2-L 384x384 batch 16 - each with
    >= 10 timed steps, the roofline of ITS dominant GEMM kernel (HIP events, split off) and the error against the CPU oracle on
    image 0 where that oracle run takes about ten seconds or less. Same JSON fields as `bench.py --model ... --size ...`."""
    out = {}
    legs = [("vits_504_b1", "vits", 504, 1, True), ("vitl_504_b1", "vitl", 504, 1, False), ("vitl_1036_b8", "vitl", 1036, 8, True),
            ("beitl_384_b16", "beitl", 384, 16, True), ("swinl_384_b16", "swinl", 384, 16, True)]
    for key, name, size, batch, want_err in legs:
        t_leg = time.perf_counter()
        try:
            sub = argparse.Namespace(**{**vars(args), "model": name, "size": size, "batch": batch})
            # batch 1 = the reference's frame-by-frame workload (run_video.py:336-349), whose model is built with enable_cache=True (:144): per-grid
            # constants are computed by the first frame and kept (mdpt_set_grid_cache)
            own_model = not (name == "vitl" and batch != 1)
            if not own_model:
                model, ow = vitl_model, None
                if want_err:  # (the oracle's weights: the same seeded checkpoint converted for the CPU restatement)
                    _, ow = make_model_and_weights(name, want_weights=True)
            else:
                model, ow = make_model_and_weights(name, want_weights=want_err, enable_cache=batch == 1)
                model = model.to(dev, torch.bfloat16)
            x_cpu = torch.randn(batch, 3, size, size, generator=torch.Generator().manual_seed(11))
            x = x_cpu.to(dev).to(torch.bfloat16)
            steps = 200 if batch == 1 else 10  # ~0.25 s of timed work at ~1.2 ms per step
            dt, y = time_model(model, x, steps)
            handle = model._get_engine().handle
            with torch.inference_mode():
                set_alone(lib, handle, True)
                model(x)
                prof = profile_pass(lib, lambda: model(x), 3)
                set_alone(lib, handle, False)
            gflop = GFLOP_PER_MAP.get((name, size))
            rec = {"metric": f"depth-maps/sec @{size}x{size}, {FAMILY[name]}", "value": round(batch / dt, 3), "unit": "depth-maps/s",
                   "ms_per_step": round(dt * 1e3, 3), "steps": steps, "dtype": "bf16", "config": {"workload": f"{FAMILY[name]} ({name}), {size}x{size} tensor, batch {batch}, bf16", "enable_cache": batch == 1}}
            if gflop:
                rec["path_frac_of_mfma_peak"] = round(batch / dt * gflop / 1e3 / PEAK_BF16_TFLOPS, 4)
            if prof and prof["kernels"]:
                rec["roofline"] = roofline(sub, prof, "HIP events, batch split off, 3 steps")
                if gflop:
                    rec["roofline"]["path_frac"] = rec["path_frac_of_mfma_peak"]
            if batch == 1:  # the opt-in latency mode (mdpt_set_latency_mode: small launches may use forms that are not batch-invariant in the last bit)
                model.set_latency_mode(True)
                dt_l, _ = time_model(model, x, steps)
                inf_l = time_inference(model, size + 14, steps)
                model.set_latency_mode(False)
                rec["latency_mode"] = {"ms_per_step": round(dt_l * 1e3, 3), "value": round(batch / dt_l, 3)}
                # what every caller of the reference actually runs (run_image.py:204-207, run_video.py:344): DPTModel.inference on a uint8 HOST
                # image - pageable numpy -> pinned staging -> H2D -> mdpt_forward_bgr (prepare_image fused into the patch embedding's im2col kernel), depth left on the device
                rec["inference_b1"] = {"input": f"uint8 host image {size + 14}x{size + 14}x3 (BGR) -> {size}x{size} tensor", **time_inference(model, size + 14, steps),
                                       "latency_mode": inf_l}
            y_m = dt_m = None
            if (name in SYNTH_NAME or size == 1036) and want_err and ow is not None:
                # BASELINE configs[4] in the mixed-pass mode too (fp32 tensors at the boundary; SwinV2's window-major encoder runs it
                # without the token-mean compensation). (Timed before the CPU oracle so that all GPU timing of a leg is done when the CPU work starts.)
                if own_model:
                    del model  # (a float32 model built afresh: casting the bf16 model back would keep its bf16-rounded parameters)
                torch.cuda.empty_cache()
                model, _ = make_model_and_weights(name)
                m32 = model.to(dev, torch.float32)
                m32.set_precision("mixed")
                dt_m, y_m = time_model(m32, x_cpu.to(dev), steps)
                y_m = y_m.float().cpu()
                del m32
                if not own_model:
                    del model
                    model = vitl_model
            if want_err and ow is not None:
                from oracle import dpt_oracle
                torch.set_num_threads(max(1, min(32, (os.cpu_count() or 2) // 2)))
                ref = dpt_oracle.forward(ow[1], ow[0], x_cpu[:1])
                rec["error_vs_cpu_fp32"] = error_vs(ref, y.float())
                if y_m is not None:
                    rec["mixed_mode"] = {"value": round(batch / dt_m, 3), "ms_per_step": round(dt_m * 1e3, 3), "error_vs_cpu_fp32": error_vs(ref, y_m)}
            else:
                rec["error_vs_cpu_fp32"] = None
            rec["leg_seconds"] = round(time.perf_counter() - t_leg, 1)
            out[key] = rec
            if own_model:
                del model
            del x, y
            torch.cuda.empty_cache()
        except Exception as e:  # a secondary leg must never take the headline line down with it
            out[key] = {"error": f"{type(e).__name__}: {e}"[:300]}
    return out


def dump_outputs(out_dir: str, y: torch.Tensor) -> None:
    """DIR/depth.npy = what a caller of the timed path receives (the [B,H,W] depth maps of the last step; N>1: the gathered global batch)
    as float32. Above DUMP_BYTES: the maps at a fixed seeded choice of batch indices, in index order, as many as fit."""
    import numpy as np
    y = y.detach().float()
    keep = DUMP_BYTES // (y[0].numel() * 4)
    if keep == 0:
        raise SystemExit(f"--dump-outputs: one depth map {tuple(y.shape[1:])} is larger than {DUMP_BYTES >> 20} MB")
    if keep < y.shape[0]:
        idx = torch.randperm(y.shape[0], generator=torch.Generator().manual_seed(0))[:keep].sort().values
        y = y[idx.to(y.device)]
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "depth.npy"), y.cpu().numpy())


def rccl_version() -> str | None:
    try:
        v = torch.cuda.nccl.version()
        return ".".join(str(i) for i in v) if isinstance(v, tuple) else str(v)
    except Exception:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--model", default="vitl", choices=sorted(FAMILY))
    ap.add_argument("--batch", type=int, default=0, help="images per GPU per step (default: 32; 8 at --size 1036; 16 for beitl / swinl)")
    ap.add_argument("--size", type=int, default=0, help="model tensor side (default 504 = what a 518x518 image is processed at; 384 for beitl / swinl)")
    ap.add_argument("--precision", default="bf16", choices=["bf16", "bf16x3", "fp16", "fp16x3", "mixed"],
                    help="MFMA operand arithmetic (include/mdpt.h MDPT_PREC_*); bf16 / fp16 run a 16-bit model, the others a float32 model")
    ap.add_argument("--tile", type=int, default=0)
    ap.add_argument("--full", action="store_true", help="behind the timed region also run the per-kernel profile passes (roofline), the H2D-inclusive "
                    "rate, the CPU baseline and the other arithmetic modes, the other BASELINE configurations (`secondary`, default workload) and the "
                    "N-rank gather self-check; a plain run does none of them")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write the depth maps the timed path returned in its last step to DIR/depth.npy (float32; "
                    f"above {DUMP_BYTES >> 20} MB a fixed, seeded sample of whole maps)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline and the other arithmetic modes")
    ap.add_argument("--no-profile", action="store_true", help="with --full: skip the per-launch HIP-event passes behind the timed region (no roofline object)")
    ap.add_argument("--no-split", action="store_true", help="nothing on the library's side stream: no two-stream half-batch split inside mdpt_forward, reassembly branches behind the encoder (every kernel alone on the GPU)")
    ap.add_argument("--no-secondary", action="store_true", help="with --full: skip the other BASELINE configurations the default run reports under `secondary`")
    ap.add_argument("--fake-model", action="store_true", help="test hook (tests/test_parallel.py): run the N-rank control flow - barriers, timed region, "
                    "max-over-ranks reduction, rank-0 JSON line - on CPU tensors with a stand-in model and the gloo backend; measures nothing")
    args = ap.parse_args()
    if not args.full:
        args.no_profile = args.no_cpu_baseline = args.no_secondary = True
    midas = args.model in SYNTH_NAME
    default_run = args.model == "vitl" and not args.size and not args.batch and args.precision == "bf16" and not args.tile and not args.no_split
    if not args.size:
        args.size = 384 if midas else 504
    if not args.batch:
        args.batch = 16 if midas else (8 if args.size > 600 else 32)

    rank, world, local_rank = init_distributed("gloo" if args.fake_model else None)
    if args.gpus != world:
        if world == 1 and args.gpus > 1:
            raise SystemExit("--gpus N>1 must be launched with torch.distributed.run (one process per GPU)")
    # N ranks synthesise 1.3 GB of ViT-L weights at the same time: share the host cores instead of N x cpu_count()//2 threads
    torch.set_num_threads(max(1, (os.cpu_count() or 2) // (2 * world)))
    lib = None
    if args.fake_model:
        dev = torch.device("cpu")
        dtype = torch.float32

        class _Fake(torch.nn.Module):  # [B,3,H,W] -> [B,H,W], per image (like the real path: no cross-sample op, same function on every rank)
            def forward(self, x):
                return x.mean(dim=1)

        model = _Fake()
        args.no_profile = args.no_cpu_baseline = args.no_secondary = True
        args.batch, args.size = 2, 16
    else:
        if not torch.cuda.is_available():
            raise SystemExit("bench.py needs an MI355X: no GPU visible (there is no CPU fallback)")
        torch.cuda.set_device(local_rank)
        dev = torch.device("cuda", local_rank)
        if world > 1:  # one process per node checks / builds libmdpt.so, the others load the finished file
            if local_rank == 0:
                native.load()
            dist.barrier()
        dtype = {"bf16": torch.bfloat16, "fp16": torch.float16}.get(args.precision, torch.float32)
        model = model_for_precision(args.model, args.precision, dev)
        lib = native.load()
        if args.tile:
            model.set_gemm_tile(args.tile)
        if args.no_split:
            set_alone(lib, model._get_engine().handle, True)
    x_cpu = torch.randn(args.batch, 3, args.size, args.size, generator=torch.Generator().manual_seed(1 + rank))
    x = x_cpu.to(dev).to(dtype)
    dp = DataParallelDepth(model, rank, world)

    def device_sync():
        if dev.type == "cuda":
            torch.cuda.synchronize()

    def barrier():
        if world > 1:
            dist.barrier()

    with torch.inference_mode():
        for _ in range(args.warmup):
            y = dp.forward_shard(x)
        device_sync()
        barrier()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            y = dp.forward_shard(x)
        device_sync()
        barrier()
        elapsed = time.perf_counter() - t0
    # max over ranks FIRST: every rank takes part in this collective right behind the timed region; only then does rank 0 go on to its
    # (rank-local, collective-free) profile / baseline legs, so no rank is left parked in a collective while rank 0 is busy elsewhere
    n_ranks_seen = 1
    per_rank_elapsed = [elapsed]
    gather_bitwise_ok = None
    if world > 1:
        own = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        every = torch.empty(world, device=dev, dtype=torch.float64)
        dist.all_gather_into_tensor(every, own)  # every rank's own clock: a slow rank is visible in the line, the max is `elapsed`
        per_rank_elapsed = [float(v) for v in every.tolist()]
        elapsed = max(per_rank_elapsed)
        n_ranks_seen = dist.get_world_size()
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, y)
    if world > 1:
        # Self-check of the gathered tensor ("gathered result == concatenation of single-GPU results bit-for-bit"):
        # rank 0 recomputes the LAST rank's shard locally (same seed rule, 1 + rank) and compares it bitwise with its slice of what the
        # all-gather delivered; its own slice must equal its own local forward. Collective-free, after the timed region.
        if rank == 0 and args.full:
            with torch.inference_mode():
                last = world - 1
                x_last = torch.randn(args.batch, 3, args.size, args.size, generator=torch.Generator().manual_seed(1 + last)).to(dev).to(dtype)
                y_last = model(x_last)
                y_own = model(x)
                b = args.batch
                gather_bitwise_ok = bool(torch.equal(y[last * b:(last + 1) * b], y_last)) and bool(torch.equal(y[:b], y_own))
                del x_last, y_last, y_own
    # Per-kernel measurements are taken AFTER the timed region, in extra passes of the same steps on rank 0 (local forward only, no
    # collective): HIP events around every launch cost host time per launch, which would otherwise be charged to `value` (visibly so for
    # the many-small-kernel models). Pass 1: as timed (two-stream half-batch split: kernels of the two halves overlap, so a launch's
    # begin->end duration includes sharing). Pass 2: split off (every kernel alone on the GPU) - the per-kernel roofline.
    prof = prof_alone = None
    if not args.no_profile and rank == 0:
        handle = model._get_engine().handle
        with torch.inference_mode():
            prof = profile_pass(lib, lambda: model(x), args.steps)
            if not args.no_split:
                set_alone(lib, handle, True)
                model(x)
                prof_alone = profile_pass(lib, lambda: model(x), args.steps)
                set_alone(lib, handle, False)

    if rank == 0:
        maps = world * args.batch * args.steps
        value = maps / elapsed
        gflop = GFLOP_PER_MAP.get((args.model, args.size))
        img = {504: "518x518 (504x504 model tensor)", 1036: "1036x1036"}.get(args.size, f"{args.size}x{args.size}")
        line = {
            "metric": f"depth-maps/sec @{img}, {FAMILY[args.model]}",
            "value": round(value, 3), "unit": "depth-maps/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 3), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": PRECISION_DTYPE[args.precision], "data": "synthetic",
            "config": {"workload": f"{FAMILY[args.model]} ({args.model}), {'518x518 image -> ' if args.size == 504 else ''}{args.size}x{args.size} tensor, batch "
                                   f"{args.batch}/GPU, {args.precision} MFMA operands + fp32 accumulate, mdpt_forward via C ABI"
                                   + (", RCCL all-gather of depth maps" if world > 1 else ""),
                       "global_batch": world * args.batch, "tensor_hw": [args.size, args.size], "parallelism": f"dp{world}",
                       "gemm_tile": args.tile, "batch_split": not args.no_split},
            "n_ranks_seen": n_ranks_seen, "rccl_version": rccl_version() if world > 1 and not args.fake_model else None,
            "gathered_shape": list(y.shape), "gather_bitwise_ok": gather_bitwise_ok,
            "per_rank_maps_per_s": {"min": round(args.batch * args.steps / max(per_rank_elapsed), 3),
                                    "max": round(args.batch * args.steps / min(per_rank_elapsed), 3)},
        }
        if world == 1 and dev.type == "cuda" and args.full:
            # the rate with the H2D copy of each batch inside the loop (SURVEY §8(d) "report both"; the C ABI takes device pointers, only
            # DPTModel.inference starts from a host image): pinned host batch in the model dtype, one extra pass, never `value`
            x_host = x_cpu.to(dtype).pin_memory()
            with torch.inference_mode():
                for _ in range(2):
                    model(x_host.to(dev, non_blocking=True))
                torch.cuda.synchronize()
                t_h = time.perf_counter()
                for _ in range(args.steps):
                    model(x_host.to(dev, non_blocking=True))
                torch.cuda.synchronize()
            line["value_incl_h2d"] = round(args.batch * args.steps / (time.perf_counter() - t_h), 3)
            del x_host
        if gflop:
            line["path_tflops"] = round(value * gflop / 1e3, 2)
            line["path_frac_of_mfma_peak"] = round(value * gflop / 1e3 / (PEAK_BF16_TFLOPS * world), 4)
        if prof and prof["kernels"]:
            if prof_alone and prof_alone["kernels"]:
                line["roofline"] = roofline(args, prof_alone, "HIP events, extra pass of the same steps after the timed region with the batch split AND the reassembly-beside-encoder overlap off (nothing on the side "
                                                              "stream: kernel alone on the GPU; `bench.py --no-split` + rocprofv3 reproduce it)")
                line["roofline_in_timed_region"] = roofline(args, prof, "HIP events, extra pass of the same steps as timed (batch split on): two half-batch kernels overlap, "
                                                                        "durations include sharing")
                shares = prof_alone
            else:
                line["roofline"] = roofline(args, prof, "HIP events, extra pass of the same steps after the timed region")
                shares = prof
            tot = sum(k["total_ms"] for k in shares["kernels"])
            line["kernel_time_share"] = {k["name"]: round(k["total_ms"] / tot, 4) for k in shares["kernels"][:12]}
            line["kernel_frac_of_mfma_peak"] = {k["name"]: round(k["tflops"] / PEAK_BF16_TFLOPS, 4) for k in shares["kernels"][:12] if k["gflop"] > 0}
            if gflop:  # the fraction tied to `ms_per_step` (whole path, algorithmic FLOPs per map / timed region), beside the per-kernel one
                line["roofline"]["path_frac"] = line["path_frac_of_mfma_peak"]
        else:
            line["roofline"] = None
        if world == 1 and not args.no_cpu_baseline:
            base, err, ref = cpu_baseline(args, x_cpu, y.float())
            line["cpu_baseline"] = base
            line["error_vs_cpu_fp32"] = err
            if args.precision == "bf16":
                del y
                line.update(parity_mode_legs(args, dev, x_cpu, ref, lib))
        else:
            line["cpu_baseline"] = None
        if world == 1 and default_run and not args.no_secondary:
            line["secondary"] = secondary_legs(args, dev, lib, model)
        print(json.dumps(line), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
