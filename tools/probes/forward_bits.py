#!/usr/bin/env python3
"""Forwards of every model family on seeded inputs through the public Python API (and mdpt_forward_bgr for the bicubic fused route), their results
hashed: two builds of libmdpt.so whose kernels compute the same must give equal hashes. Made to reach every kernel of csrc/elementwise.hip and
csrc/swin.hip that runs under a profiler label (the `kernels` map of the result shows which were reached): the tiny fixtures of each family (DA-V2
square and rectangular, DA-V1, giant / SwiGLU, BEiT, SwinV2) with their stage taps in every precision mode and in the 16-bit model dtypes, the fp8
cross-term classes, the stage entry points, inference (bilinear and bicubic preparation, alone, fused, and a batch of frames), latency mode (also on
ViT-S, whose fc2 is long enough for the K split), weight-rounding compensation, block_norms, an image with a NaN pixel, and one ViT-S forward whose
fusion upsample is large enough for the LDS-tiled kernel; the "extras" (--only extras runs them alone): ViT-B at 252 x 252 in latency mode, whose
long-K decoder convs split into K ranges with ksplit_finish_kernel behind them, and mdpt_launch_swin_cpb called directly (the non-batch
swin_cpb_kernel: no route of the library launches it any more, every caller uses the batched form). A case a build rejects is recorded with its error
text (equal on both sides too). The in-library profiler runs throughout: `kernels` lists every profiled kernel label reached, with its launch count.
--timing adds per-kernel times on the benchmark workload (ViT-L, batch 32, 504 x 504, bf16; the same batch as uint8 frames for the fused kernel): REPEATS
profile passes, the average microseconds per launch of each named kernel per pass.
Writes {cases: {name: {sha256, bytes, tensors}}, kernels, source_hash[, timing_us]} to --out. --compare PARENT NEW [PARENT NEW ...] merges such
results of the parent commit and of this one (runs alternating between them) into the records kept under profiles/; A.json+B.json names one run whose
cases were taken in two processes (disjoint case names)."""
import argparse
import ctypes
import hashlib
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
import muggled_dpt_amd as mda  # noqa: E402
from muggled_dpt_amd import native  # noqa: E402
from muggled_dpt_amd import synthetic as syn  # noqa: E402

GOLDEN = os.path.join(REPO, "tests", "golden")
RESULTS: dict = {}
TIMED = ("layernorm_kernel", "upsample_kernel", "upsample_bf16src_kernel", "prepare_patchify_kernel", "patchify_kernel")
REPEATS = 5


def leaves(x):
    if isinstance(x, (torch.Tensor, np.ndarray)):
        yield x
    elif isinstance(x, dict):
        for k in sorted(x):
            yield from leaves(x[k])
    elif isinstance(x, (list, tuple)):
        for v in x:
            yield from leaves(v)
    elif x is not None:
        yield np.asarray(x)


def record(name: str, fn):
    """run fn() and add the tensors of its result (any nesting) to the hash of case `name`; an exception is hashed as its text"""
    entry = RESULTS.setdefault(name, {"h": hashlib.sha256(), "bytes": 0, "tensors": 0})
    try:
        with torch.inference_mode():
            result = fn()
        torch.cuda.synchronize()
    except (RuntimeError, ValueError, AssertionError, native.MdptError) as e:
        entry["h"].update(f"error: {type(e).__name__}: {e}".encode())
        entry["error"] = f"{type(e).__name__}: {e}"[:200]
        return None
    for t in leaves(result):
        if isinstance(t, torch.Tensor):
            t = t.detach().contiguous().cpu()
            t = (t.view(torch.int16) if t.dtype in (torch.bfloat16, torch.float16) else t).numpy()
        raw = np.ascontiguousarray(t).tobytes()
        entry["h"].update(f"{t.dtype}{tuple(t.shape)}".encode())
        entry["h"].update(raw)
        entry["bytes"] += len(raw)
        entry["tensors"] += 1
    return result


def golden(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def fixtures():
    """(tag, build() -> model on the CPU, [input tensors])"""
    g = {n: golden(n) for n in ("tiny_full", "tiny_rect", "tiny_v1", "tiny_giant", "beit_tiny", "swin2_tiny")}
    seed = lambda n: int(g[n]["weight_seed"]) if "weight_seed" in g[n].files else 0  # noqa: E731
    t = lambda a: torch.from_numpy(np.asarray(a)).float()  # noqa: E731
    yield "dav2", lambda: mda.make_depthanythingv2_dpt_from_original_state_dict(syn.make_synthetic_original_state_dict("tiny", seed("tiny_full")))[1], \
        [t(g["tiny_full"]["input"]), t(g["tiny_rect"]["input"])]
    v1 = dict(syn.STANDARD_CONFIGS["tiny"], num_blocks=int(g["tiny_v1"]["num_blocks"]))
    yield "dav1", lambda: mda.make_depthanythingv1_dpt_from_original_state_dict(syn.make_synthetic_original_state_dict(v1, seed("tiny_v1")))[1], [t(g["tiny_v1"]["input"])]
    yield "giant", lambda: mda.make_depthanythingv2_dpt_from_original_state_dict(syn.make_synthetic_original_state_dict("tiny_giant", seed("tiny_giant")))[1], \
        [t(g["tiny_giant"]["input"])]
    yield "beit", lambda: mda.make_beit_dpt_from_midas_v31_state_dict(syn.make_synthetic_beit_state_dict("beit_tiny", seed("beit_tiny")))[1], \
        [t(g["beit_tiny"]["base_input"]), t(g["beit_tiny"]["wide_input"])]
    yield "swin", lambda: mda.make_swinv2_dpt_from_midas_v31_state_dict(syn.make_synthetic_swinv2_state_dict("swin2_tiny", seed("swin2_tiny")))[1], \
        [t(g["swin2_tiny"]["base_input"]), t(g["swin2_tiny"]["tall_input"])]


def forward_and_taps(model, x):
    y = model(x)
    return [y, model.debug_taps(x.shape[0], tuple(x.shape[2:]))]


def stage_entries(model, x):
    """each sub-module on the previous one's output (simple_examples/internal_features.py usage)"""
    tok, hw = model.patch_embed(x)
    enc = model.imgencoder(tok, hw)
    rs = model.reassemble(*enc, hw)
    fu = model.fusion(*rs)
    return [tok, list(enc), list(rs), fu, model.head(fu)]


def families():
    for tag, build, inputs in fixtures():
        model = build()
        # every arithmetic mode on the fp32 model, then the 16-bit model dtypes with their default mode
        for mode in sorted(native.PRECISIONS):
            m = model.to("cuda", torch.float32)
            m.set_precision(mode)
            for i, x in enumerate(inputs):
                record(f"{tag}/{mode}/forward{i}", lambda: forward_and_taps(m, x.cuda()))
        model.set_precision(None)
        for dtype in (torch.bfloat16, torch.float16):
            m = model.to("cuda", dtype)
            name = str(dtype).split(".")[1]
            record(f"{tag}/{name}/forward", lambda: forward_and_taps(m, inputs[-1].to("cuda", dtype)))
            record(f"{tag}/{name}/stages", lambda: stage_entries(m, inputs[0].to("cuda", dtype)))
            record(f"{tag}/{name}/block_norms", lambda: m.block_norms(inputs[0].to("cuda", dtype), channels=1))
        # fp16 operands with the fp8 cross-term classes (the fp8 forms of the plane stores), and weight-rounding compensation forced on
        m = model.to("cuda", torch.float32)
        m.set_precision("fp16")
        m.set_class_passes({c: native.PASSES_3F8 for c in native.F8_CLASSES})
        record(f"{tag}/fp16+3f8/forward", lambda: forward_and_taps(m, inputs[0].cuda()))
        record(f"{tag}/fp16+3f8/stages", lambda: stage_entries(m, inputs[0].cuda()))
        m.set_class_passes({c: native.PASSES_2F8 for c in native.F8_CLASSES})
        record(f"{tag}/fp16+2f8/stages", lambda: stage_entries(m, inputs[-1].cuda()))
        m.set_class_passes(None)
        m.set_weight_rounding_compensation(True)
        record(f"{tag}/fp16+wrc/forward", lambda: m(inputs[0].cuda()))
        m.set_weight_rounding_compensation(None)
        m.set_precision(None)
        # latency mode at batch 1 (these fixtures are too small for a K split: ViT-S and ViT-B below take it), and an image with a NaN pixel in a batch of two
        m = model.to("cuda", torch.bfloat16)
        m.set_latency_mode(True)
        record(f"{tag}/latency/forward", lambda: forward_and_taps(m, inputs[0][:1].to("cuda", torch.bfloat16)))
        m.set_latency_mode(False)
        bad = inputs[0][:2].clone()
        bad[0, 1, 3, 4] = float("nan")
        record(f"{tag}/nan_pixel/forward", lambda: m(bad.to("cuda", torch.bfloat16)))
        yield tag, model


def bgr_direct(model, image, interp):
    """mdpt_forward_bgr with an explicit interpolation (DPTModel.inference is bilinear only): the fused prepare + patchify kernel"""
    pe = model.patch_embed
    scaled_hw, _, p, img_dtype = pe._prepare_plan(image, None, True, "bilinear")
    eng = model._get_engine()
    h, w = scaled_hw
    with torch.cuda.device(p.device):
        src = pe._stage_host_image(image, p.device)
        out = torch.empty((1, h, w), device=p.device, dtype=eng.dtype)
        mean3, std3 = pe._norm_constants()
        eng.call_checked("mdpt_forward_bgr", src, image.shape[0], image.shape[1], native.dtype_code(img_dtype), h, w, mean3, std3, interp, out,
                         native.dtype_code(out.dtype), size_hw=(h, w), batch=1)
    return out


def inference(tag, model):
    rs = np.random.RandomState(17)
    photo = rs.randint(0, 256, (90, 120, 3)).astype(np.uint8)
    frames = rs.randint(0, 256, (3, 61, 83, 3)).astype(np.uint8)
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        m = model.to("cuda", dtype)
        name = str(dtype).split(".")[1]
        record(f"{tag}/inference/{name}", lambda: [m.inference(photo), m.inference(photo, max_side_length=70, use_square_sizing=False), m.inference_batch(frames),
                                                   m.inference_images([photo, frames[0]])])
        for mode in ("bilinear", "bicubic"):
            record(f"{tag}/prepare_{mode}/{name}", lambda: (lambda x: [x, m(x)])(m.prepare_image_bgr(photo, interpolation_mode=mode)))
        record(f"{tag}/forward_bgr_bicubic/{name}", lambda: bgr_direct(m, photo, native.INTERP_BICUBIC))


def tiled_upsample():
    """ViT-S (64 fusion channels) at 448 x 448: the last fusion upsample writes 256 x 256 pixels of 64 channels as operand planes - the tiled kernel"""
    _, model = mda.make_depthanythingv2_dpt_from_original_state_dict(syn.make_synthetic_original_state_dict("vits", 0))
    x = torch.randn(1, 3, 448, 448, generator=torch.Generator().manual_seed(5))
    for dtype in (torch.bfloat16, torch.float16):
        m = model.to("cuda", dtype)
        record(f"vits448/{str(dtype).split('.')[1]}/forward", lambda: m(x.to("cuda", dtype)))
    m = model.to("cuda", torch.bfloat16)
    m.set_latency_mode(True)  # K = 1536 of fc2 is past the K-split threshold at batch 1: layernorm_addp_kernel
    record("vits448/latency/forward", lambda: m(x.to("cuda", torch.bfloat16)))
    m.set_latency_mode(False)
    m = model.to("cuda", torch.float32)
    record("vits448/float32/forward", lambda: m(x.cuda()))
    m.set_precision("fp16")
    m.set_class_passes({c: native.PASSES_3F8 for c in native.F8_CLASSES})
    record("vits448/fp16+3f8/forward", lambda: m(x.cuda()))


def extras(lib):
    """ksplit_finish_kernel: ViT-B-sized decoder at 252 x 252, batch 1, latency mode (mdpt_stages.cpp try_ksplit_conv: the 3x3 convs of the coarse
    levels run as K ranges that store partial planes). swin_cpb_kernel: its launcher in both operand builds on seeded MLP weights."""
    _, model = mda.make_depthanythingv2_dpt_from_original_state_dict(syn.make_synthetic_original_state_dict("vitb", 0))
    x = torch.randn(1, 3, 252, 252, generator=torch.Generator().manual_seed(35))
    for dtype in (torch.float32, torch.bfloat16):
        m = model.to("cuda", dtype)
        m.set_latency_mode(True)
        record(f"vitb252/latency/{str(dtype).split('.')[1]}", lambda: m(x.to("cuda", dtype)))
        m.set_latency_mode(False)
    heads, hidden, wh, ww = 3, 64, 4, 3
    g = torch.Generator().manual_seed(9)
    w1, b1, w2 = torch.randn(hidden, 2, generator=g).cuda(), torch.randn(hidden, generator=g).cuda(), (torch.randn(heads, hidden, generator=g) / 8).cuda()
    P, I = ctypes.c_void_p, ctypes.c_int
    for fmt in ("bf16", "f16"):
        fn = getattr(lib, f"mdpt_launch_swin_cpb_{fmt}")
        fn.restype, fn.argtypes = ctypes.c_int, [P, P, P, P, I, I, I, I, I, P]
        for pre in (0, 6):
            lut = torch.zeros(heads, (2 * wh - 1) * (2 * ww - 1), device="cuda")
            rc = fn(w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), lut.data_ptr(), heads, hidden, wh, ww, pre, torch.cuda.current_stream().cuda_stream)
            record(f"swin_cpb_direct/{fmt}/pretrained{pre}", lambda: [rc, lut])


def report(lib):
    buf = ctypes.create_string_buffer(1 << 18)
    return json.loads(buf.value.decode())["kernels"] if lib.mdpt_profile_report(buf, len(buf)) == 0 else []


def timing(lib) -> dict:
    """average microseconds per launch of the TIMED kernels on the benchmark workload, one figure per profile pass"""
    _, model = mda.make_depthanythingv2_dpt_from_original_state_dict(syn.make_synthetic_original_state_dict("vitl", 0))
    model = model.to("cuda", torch.bfloat16)
    x = torch.randn(32, 3, 504, 504, generator=torch.Generator().manual_seed(1)).to("cuda", torch.bfloat16)
    frames = torch.from_numpy(np.random.RandomState(3).randint(0, 256, (32, 518, 518, 3)).astype(np.uint8)).cuda()
    out: dict = {}
    with torch.inference_mode():
        for _ in range(2):
            model(x), model.inference_batch(frames)
        for _ in range(REPEATS):
            torch.cuda.synchronize()
            lib.mdpt_profile_enable(1)
            for _ in range(6):
                model(x), model.inference_batch(frames)
            torch.cuda.synchronize()
            for k in report(lib):
                if k["name"] in TIMED:
                    out.setdefault(k["name"], []).append(round(k["avg_us"], 3))
            lib.mdpt_profile_enable(0)
    return out


def load_run(spec):
    """one run from A.json, or from A.json+B.json: the cases of both (disjoint), launch counts added, the timing of whichever has one"""
    run = None
    for path in spec.split("+"):
        part = json.load(open(path))
        if run is None:
            run = part
            continue
        assert part["source_hash"] == run["source_hash"] and not set(part["cases"]) & set(run["cases"]), spec
        run["cases"].update(part["cases"])
        for k, n in part["kernels"].items():
            run["kernels"][k] = run["kernels"].get(k, 0) + n
        if "timing_us" in part and "timing_us" not in run:
            run["timing_us"] = part["timing_us"]
    run["kernels"] = dict(sorted(run["kernels"].items()))
    return run


def compare(paths, out, timing_out):
    runs = [load_run(p) for p in paths]
    parent, new = runs[0], runs[1]
    strip = lambda r: {n: e["sha256"] for n, e in r["cases"].items()}  # noqa: E731
    pairs_equal = [strip(a) == strip(b) == strip(parent) for a, b in zip(runs[0::2], runs[1::2])]
    cases = {n: {"equal": e["sha256"] == new["cases"].get(n, {}).get("sha256"), "bytes": e["bytes"], "tensors": e["tensors"], "sha256": e["sha256"],
                 **({"error": e["error"]} if "error" in e else {})} for n, e in parent["cases"].items()}
    result = {"parent_source_hash": parent["source_hash"], "new_source_hash": new["source_hash"], "pairs": len(pairs_equal), "pairs_equal": pairs_equal,
              "all_equal": all(pairs_equal) and set(parent["cases"]) == set(new["cases"]), "kernels_equal": parent["kernels"] == new["kernels"],
              "kernels": new["kernels"], "cases": cases}
    with open(out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    verdict = {"all_equal": result["all_equal"], "kernels_equal": result["kernels_equal"]}
    if timing_out and all("timing_us" in r for r in runs):
        med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
        pairs = []
        for a, b in zip(runs[0::2], runs[1::2]):
            pairs.append({k: {"parent": a["timing_us"][k], "new": b["timing_us"][k], "parent_slowest": max(a["timing_us"][k]), "new_median": med(b["timing_us"][k]),
                              "meets_bar": med(b["timing_us"][k]) <= max(a["timing_us"][k])} for k in a["timing_us"]})
        rec = {"what": "average microseconds per launch from mdpt_profile_report on the benchmark workload (ViT-L, batch 32, 504 x 504, bf16, and the same batch as "
                       "uint8 518 x 518 frames through inference_batch for the fused prepare + patchify kernel), five profile passes of six forwards per run, "
                       "parent build and new build alternating. meets_bar = the new median lies at or below the parent's slowest pass of the same pair",
               "parent_source_hash": parent["source_hash"], "new_source_hash": new["source_hash"], "pairs": pairs,
               "not_launched_on_this_workload": [k for k in TIMED if k not in pairs[0]],  # (their resizes are folded into the conv / head kernels at this size)
               "bar_met_in_every_pair": {k: all(p[k]["meets_bar"] for p in pairs) for k in pairs[0]}}
        with open(timing_out, "w") as fh:
            json.dump(rec, fh, indent=1)
            fh.write("\n")
        verdict["bar_met_in_every_pair"] = rec["bar_met_in_every_pair"]
    print(json.dumps(verdict))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", required=True)
    ap.add_argument("--timing", action="store_true")
    ap.add_argument("--compare", nargs="+", metavar="JSON", help="results of earlier runs as parent new [parent new ...]: write the comparison to --out (and --timing-out), no GPU")
    ap.add_argument("--timing-out")
    ap.add_argument("--only", choices=["extras"], help="run this group of cases alone")
    args = ap.parse_args()
    if args.compare:
        return compare(args.compare, args.out, args.timing_out)
    if not torch.cuda.is_available():
        raise SystemExit("forward_bits.py needs a GPU: there is no CPU implementation to hash")
    lib = native.load()
    kernels: dict = {}

    def drain():  # add what the profiler holds to `kernels` and start it afresh (enabling clears its records)
        torch.cuda.synchronize()
        for k in report(lib):
            kernels[k["name"]] = kernels.get(k["name"], 0) + k["launches"]
        lib.mdpt_profile_enable(1)

    lib.mdpt_profile_enable(1)
    if not args.only:
        for tag, model in families():
            if tag in ("dav2", "beit", "swin"):
                inference(tag, model)
            drain()
        tiled_upsample()
        drain()
    extras(lib)
    drain()
    lib.mdpt_profile_enable(0)
    result = {"source_hash": native.source_hash(), "kernels": dict(sorted(kernels.items())),
              "cases": {n: {"sha256": e["h"].hexdigest(), "bytes": e["bytes"], "tensors": e["tensors"], **({"error": e["error"]} if "error" in e else {})}
                        for n, e in sorted(RESULTS.items())}}
    if args.timing:
        result["timing_us"] = timing(lib)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    errors = {n: e["error"] for n, e in result["cases"].items() if "error" in e}
    print(json.dumps({"cases": len(RESULTS), "errors": errors, "kernels": len(kernels), "source_hash": result["source_hash"], "timing": result.get("timing_us")}))


if __name__ == "__main__":
    main()
