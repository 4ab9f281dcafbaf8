#!/usr/bin/env python3
"""Every public function of muggled_dpt_amd.postprocess called once or more on seeded inputs through the public API only, its results hashed:
two versions of the Python half over one libmdpt.so (equal native.source_hash()) must give equal hashes, because every difference then comes from the
Python. The shapes are the smallest at which the plumbing can go wrong: maps of 37x53 and 21x29, a 64x48 display, lists of three different sizes and
of 33 items (past POST_RUNS = 32), photos and truths on the host and on the device, one photo as a strided view, a list of valid maps holding None,
render / fill whole and with max_scratch_bytes=1. Only what a result defines is hashed (mesh slabs through mesh_views: the rest of a slab is not
written). --timing adds the HOST cost of a call: REPEATS repeats of CALLS un-synchronised calls after a warm-up, host clock around the enqueue loop
(a synchronise ends every repeat outside the timed window), microseconds per call.
Writes {functions: {name: {sha256, bytes, tensors}}, source_hash[, timing_us_per_call]} to --out. --compare PARENT NEW [PARENT NEW ...] merges such
results of the parent commit and of this one (runs alternating between them) into the record kept under profiles/."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
from muggled_dpt_amd import native  # noqa: E402
from muggled_dpt_amd import orbit_camera as oc  # noqa: E402
from muggled_dpt_amd import postprocess as pp  # noqa: E402

DEV = "cuda:0"
WH = (64, 48)
CALLS, REPEATS = 200, 5
RESULTS: dict = {}


def leaves(x):
    if isinstance(x, (torch.Tensor, np.ndarray)):
        yield x
    elif isinstance(x, (list, tuple)):
        for v in x:
            yield from leaves(v)
    elif x is not None:
        yield np.asarray(x)


def record(name: str, result):
    """add the tensors of `result` (any nesting of lists / tuples, host values included) to the running hash of function `name`"""
    entry = RESULTS.setdefault(name, {"h": hashlib.sha256(), "bytes": 0, "tensors": 0})
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


def inputs():
    g = torch.Generator().manual_seed(7)
    rs = np.random.RandomState(11)
    rand = lambda *s: torch.rand(*s, generator=g)  # noqa: E731
    maps = (rand(2, 37, 53) * 9 + 1).to(DEV)
    sizes = [(37, 53), (21, 29), (29, 41)]
    three = [(rand(1, h, w) * 9 + 1).to(DEV) for h, w in sizes]
    many = [(rand(1, *sizes[k % 2]) * 9 + 1).to(DEV) for k in range(33)]
    photo = lambda h, w: rs.randint(0, 256, (h, w, 3)).astype(np.uint8)  # noqa: E731
    big = photo(90, 112)
    host3 = [photo(80, 100), big[2:-2, 3:-3], photo(44, 61)]  # (the second one is a strided view)
    big_dev = torch.from_numpy(big).to(DEV)
    dev3 = [torch.from_numpy(host3[0]).to(DEV), big_dev[2:-2, 3:-3], torch.from_numpy(host3[2]).to(DEV)]
    many_photos = [photo(40 + k % 3, 56 + k % 5) for k in range(33)]
    lut = rs.randint(0, 256, (1, 256, 3)).astype(np.uint8)
    return dict(g=g, rs=rs, rand=rand, maps=maps, three=three, many=many, host3=host3, dev3=dev3, many_photos=many_photos, lut=lut)


def display(x):
    maps, three, many, lut, rs = x["maps"], x["three"], x["many"], x["lut"], x["rs"]
    record("scale_prediction", [pp.scale_prediction(maps, WH), pp.scale_prediction(maps.bfloat16(), WH)])
    record("normalize_01", pp.normalize_01(maps))
    u8 = record("convert_to_uint8", pp.convert_to_uint8(maps))
    record("scale_and_convert_to_uint8", pp.scale_and_convert_to_uint8(maps, WH))
    record("pack_depth_u24", [pp.pack_depth_u24(maps[:1]), pp.pack_depth_u24(maps[0] / 10, is_metric=True, lossy=True)])
    holes = maps.clone()
    holes[0, 3, 4], holes[1, 0, 0] = float("inf"), float("-inf")
    record("remove_inf_tensor", [pp.remove_inf_tensor(holes, 2.0, in_place=False), pp.remove_inf_tensor(holes)])
    record("equalization_range", [pp.equalization_range(), pp.equalization_range(0.2, 0.7)])
    record("threshold_bin_table", pp.threshold_bin_table(*pp.equalization_range(0.2, 0.7)))
    record("histogram_equalization", [pp.histogram_equalization(u8), pp.histogram_equalization(u8[0], 0.2, 0.7)])
    record("apply_colormap", [pp.apply_colormap(u8, lut), pp.apply_colormap(u8[1])])
    whs = [(64, 48), (31, 17), (53, 37)]
    for hc in (False, True):
        record("depth_to_color", [pp.depth_to_color(maps, WH, reverse=hc, high_contrast=hc, lut=lut), pp.depth_to_color(maps.half(), None, True, hc)])
        record("depth_to_color_images", [pp.depth_to_color_images(three, whs, reverse=not hc, high_contrast=hc, lut=lut),
                                         pp.depth_to_color_images(three, None, False, hc), pp.depth_to_color_images(maps, [WH, WH], high_contrast=hc)])
    record("depth_to_color_images", pp.depth_to_color_images(many, [(20 + k, 50 - k) for k in range(33)], high_contrast=True, lut=lut))
    record("scale_prediction_images", [pp.scale_prediction_images(three, whs), pp.scale_prediction_images(many, [(20 + k, 50 - k) for k in range(33)]),
                                       pp.scale_prediction_images(maps.bfloat16(), [WH, (5, 7)])])
    # the still-image tail: explicit sample points (plane_sample_points with a seeded generator), and the default draw after np.random.seed
    pts_map = record("plane_sample_points", np.stack([pp.plane_sample_points((37, 53), rng=rs) for _ in range(2)]))
    pts_disp = np.stack([pp.plane_sample_points((WH[1], WH[0]), rng=rs) for _ in range(2)])
    np.random.seed(5)
    record("plane_of_best_fit", [pp.plane_of_best_fit(maps, sample_xy=pts_map), pp.plane_of_best_fit(maps[0], sample_xy=torch.from_numpy(pts_map[1]).to(DEV)),
                                 pp.plane_of_best_fit(maps)])
    for hc in (False, True):
        record("depth_to_display", [pp.depth_to_display(maps, WH, 0.5, (0.2, 0.7), reverse=hc, high_contrast=hc, lut=lut, sample_xy=pts_disp),
                                    pp.depth_to_display(maps.bfloat16(), None, 1.0, (0.0, 1.0), True, hc, None, sample_xy=pts_map)])
    record("depth_to_display", pp.depth_to_display(maps, WH, 0.5, (0.2, 0.7)))
    record("depth_for_saving", [pp.depth_for_saving(maps, 0.5, (0.2, 0.7), True, sample_xy=pts_map), pp.depth_for_saving(maps, sample_xy=pts_map[0])])
    record("depth_edge_mask", [pp.depth_edge_mask(maps), pp.depth_edge_mask(maps[0], 9, 2.0)])
    alpha = (torch.from_numpy(rs.randint(0, 2, (37, 53)).astype(np.uint8)) * 255).to(DEV)
    frames = pp.pack_depth_u24_frames(maps)
    record("pack_depth_u24_frames", [frames, pp.pack_depth_u24_frames(maps, alpha=alpha), pp.pack_depth_u24_frames(maps / 10, True, True, None),
                                     pp.pack_depth_u24_frames(maps, alpha=torch.stack([alpha, 255 - alpha]))])
    return frames, pts_map, pts_disp


def masking(x, pts_map, pts_disp):
    maps, three, many, rs = x["maps"], x["three"], x["many"], x["rs"]
    photos = torch.from_numpy(rs.randint(0, 256, (2, 40, 50, 3)).astype(np.uint8)).to(DEV)
    record("depth_mask_display", [pp.depth_mask_display(maps, photos, WH, 0.5, (0.2, 0.7), sample_xy=pts_disp),
                                  pp.depth_mask_display(maps[0], photos[1], None, 0.0, (0.2, 0.7), True, sample_xy=pts_map[0])])
    sets = [pp.plane_sample_points(m.shape[-2:], rng=rs) for m in three]
    for images in (x["host3"], x["dev3"]):
        record("depth_mask_images", pp.depth_mask_images(three, images, 0.5, (0.2, 0.7), sample_xy=sets))
    record("depth_mask_images", pp.depth_mask_images(maps, x["host3"][:2], 0.0, (0.2, 0.7), True, sample_xy=pts_map))
    record("depth_mask_images", pp.depth_mask_images(many, x["many_photos"], 0.5, (0.2, 0.7), sample_xy=[pp.plane_sample_points(m.shape[-2:], rng=rs) for m in many]))
    norms = [x["rand"](2, 8, 8).to(DEV), x["rand"](2, 4, 2).to(DEV), x["rand"](2, 8, 8).to(DEV)]
    record("block_norm_display", [pp.block_norm_display(norms), pp.block_norm_display(norms, (16, 8), x["lut"]),
                                  pp.block_norm_display(torch.stack([norms[0]] * 33))])


def mesh_render_fill(x, frames):
    record("mesh_plane_grid", [pp.mesh_plane_grid((53, 37), 600)[:2], pp.mesh_plane_grid((53, 37), 600, 1.0, np.random.RandomState(3))])
    nx, ny, jittered = pp.mesh_plane_grid((53, 37), 600, 0.5, np.random.RandomState(4))
    meshes = [pp.depth_frames_to_mesh(frames, (53, 37), target_num_faces=600, edge_threshold=0.3),
              pp.depth_frames_to_mesh(frames, (53, 37), target_num_faces=600, vertex_xy=jittered),
              pp.depth_frames_to_mesh(frames[0], (53, 37), 60.0, 0.5, 10.0, True, 0.1, mode="points", grid_xy=(9, 7))]
    for m in meshes:
        record("depth_frames_to_mesh", [m[3], pp.mesh_views(*m)])
        record("mesh_views", pp.mesh_views(*m))
    views = oc.swing_views(3, 25.0, 10.0, aspect=WH[0] / WH[1])
    mesh = meshes[0][:4]
    for textures in (x["host3"][:2], x["dev3"][:2]):
        whole = record("render_mesh", pp.render_mesh(*mesh, textures, views, WH, return_depth=True, return_face_ids=True))
    record("render_mesh", [pp.render_mesh(*mesh, x["host3"][:2], views, WH, "none", return_depth=True, max_scratch_bytes=1),
                           pp.render_mesh(*mesh, x["dev3"][:2], views[:1], WH, return_depth=True, return_face_ids=True, fill_holes=0.1),
                           pp.render_mesh(*meshes[2][:4], [x["host3"][2]], torch.from_numpy(views).to(DEV), WH, point_size=2.0)])
    color, depth = whole[0], whole[1]
    record("fill_holes", [pp.fill_holes(color, depth), pp.fill_holes(color, depth, 0.5, True), pp.fill_holes(color, depth, 0.1, True, max_scratch_bytes=1),
                          pp.fill_holes(color[0, 0], depth[0, 0], 1.0)])


def tiles_align_guided(x):
    three, many, rs, rand = x["three"], x["many"], x["rs"], x["rand"]
    guide = (rand(1, 30, 40) * 9 + 1).to(DEV)
    boxes3 = [(0, 0, 70, 60), (50, 0, 120, 50), (20, 40, 120, 90)]
    record("stitch_tiles", [pp.stitch_tiles(three, boxes3, (90, 120), guide, return_fit=True), pp.stitch_tiles(three, boxes3, (90, 120), align="none"),
                            pp.stitch_tiles([m.bfloat16() for m in three], boxes3, (90, 120), guide.bfloat16(), feather=7.5)])
    boxes33 = [(8 * (k % 11), 20 * (k // 11), 8 * (k % 11) + 40, 20 * (k // 11) + 50) for k in range(33)]
    record("stitch_tiles", pp.stitch_tiles(many, boxes33, (90, 120), guide, return_fit=True))
    hws = [(80, 100), (44, 61), (50, 50)]
    truths = [(rs.rand(h, w) * 4 + 0.5).astype(np.float32) for h, w in hws]
    truths[0][::7, ::5] = 0.0
    truths_dev = [torch.from_numpy(t).to(DEV) for t in truths]
    mask = [(rs.rand(h, w) > 0.3) for h, w in hws]
    valid = [torch.from_numpy(mask[0]).to(DEV), None, torch.from_numpy(mask[2]).to(DEV)]
    fit = None
    for t, v in ((truths_dev, valid), (truths, [mask[0], None, mask[2]]), (truths_dev, None)):
        for method in ("lstsq", "median"):
            fit = record("fit_true_depth", pp.fit_true_depth(three, t, v, method=method, truth_range=(0.6, None), return_sums=True))[0]
        record("depth_metrics", [pp.depth_metrics(three, t, fit, v), pp.depth_metrics(three, t, None, v, "depth", (None, 4.0))])
    record("true_depth", [pp.true_depth(three, fit, hws), pp.true_depth(three, None, None, "depth", (2.0, 8.0)), pp.true_depth(x["maps"], fit[:2], [WH[::-1]] * 2)])
    hws33 = [(30 + k % 4, 45 + k % 3) for k in range(33)]
    truths33 = [(rs.rand(h, w) * 4 + 0.5).astype(np.float32) for h, w in hws33]
    fit33 = record("fit_true_depth", pp.fit_true_depth(many, truths33))
    record("depth_metrics", pp.depth_metrics(many, [torch.from_numpy(t).to(DEV) for t in truths33], fit33))
    record("true_depth", pp.true_depth(many, fit33, hws33))
    record("mesh_depth_range", pp.mesh_depth_range((0.02, 0.01), (1.0, 10.0)))
    for images in (x["host3"], x["dev3"]):
        record("guided_upsample_images", pp.guided_upsample_images(three, images, 3, 1e-3, return_coefficients=True))
    record("guided_upsample_images", [pp.guided_upsample_images(x["maps"], x["dev3"][:2]), pp.guided_upsample_images(many, x["many_photos"], 2)])
    return truths_dev


def timing(x, truths_dev) -> dict:
    """host microseconds per un-synchronised call: a warm-up, then REPEATS repeats of CALLS calls, the device drained between repeats"""
    whs = [(64, 48), (31, 17), (53, 37)]
    cases = {"depth_to_color": lambda: pp.depth_to_color(x["maps"], WH), "depth_to_color_images": lambda: pp.depth_to_color_images(x["three"], whs),
             "fit_true_depth": lambda: pp.fit_true_depth(x["three"], truths_dev)}
    out = {}
    for name, fn in cases.items():
        for _ in range(CALLS):
            fn()
        torch.cuda.synchronize()
        repeats = []
        for _ in range(REPEATS):
            t0 = time.perf_counter()
            for _ in range(CALLS):
                fn()
            repeats.append((time.perf_counter() - t0) / CALLS * 1e6)
            torch.cuda.synchronize()
        out[name] = [round(v, 2) for v in repeats]
    return out


def compare(paths, out, timing_out):
    """results of this probe in (parent, new) pairs -> one record: per function whether the hashes of the first pair are equal, and per pair and timed
    function whether the new median lies at or below the parent's slowest repeat"""
    runs = [json.load(open(p)) for p in paths]
    parent, new = runs[0], runs[1]
    pairs_equal = [a["source_hash"] == b["source_hash"] and a["functions"] == b["functions"] == parent["functions"] for a, b in zip(runs[0::2], runs[1::2])]
    functions = {n: {"equal": e == new["functions"].get(n), "bytes": e["bytes"], "tensors": e["tensors"], "parent_sha256": e["sha256"],
                     "new_sha256": new["functions"].get(n, {}).get("sha256")} for n, e in parent["functions"].items()}
    result = {"parent_source_hash": parent["source_hash"], "new_source_hash": new["source_hash"], "not_reached": new["not_reached"],
              "pairs_equal": pairs_equal, "all_equal": all(pairs_equal), "functions": functions, "timing_pairs": []}
    for a, b in zip(runs[0::2], runs[1::2]):
        pair = {}
        for n, reps in a.get("timing_us_per_call", {}).items():
            med = sorted(b["timing_us_per_call"][n])[len(reps) // 2]
            pair[n] = {"parent": reps, "new": b["timing_us_per_call"][n], "parent_slowest": max(reps), "new_median": med, "meets_bar": med <= max(reps)}
        result["timing_pairs"].append(pair)
    result["bar_met_in_every_pair"] = {n: all(p[n]["meets_bar"] for p in result["timing_pairs"]) for n in (result["timing_pairs"] or [{}])[0]}
    timing = {"source_hash": new["source_hash"], "unit": "host microseconds per un-synchronised call", "pairs": result.pop("timing_pairs"),
              "bar_met_in_every_pair": result.pop("bar_met_in_every_pair")}
    for path, record in ((out, result), (timing_out, timing)):
        with open(path, "w") as fh:
            json.dump(record, fh, indent=1)
            fh.write("\n")
    result["bar_met_in_every_pair"] = timing["bar_met_in_every_pair"]
    print(json.dumps({"all_equal": result["all_equal"], "bar_met_in_every_pair": result["bar_met_in_every_pair"]}))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", required=True)
    ap.add_argument("--timing", action="store_true")
    ap.add_argument("--compare", nargs="+", metavar="JSON", help="results of earlier runs as parent new [parent new ...]: write the hash comparison to --out and the timing to --timing-out, no GPU")
    ap.add_argument("--timing-out")
    args = ap.parse_args()
    if args.compare:
        return compare(args.compare, args.out, args.timing_out)
    if not torch.cuda.is_available():
        raise SystemExit("post_bits.py needs a GPU: there is no CPU implementation to hash")
    x = inputs()
    frames, pts_map, pts_disp = display(x)
    masking(x, pts_map, pts_disp)
    mesh_render_fill(x, frames)
    truths_dev = tiles_align_guided(x)
    torch.cuda.synchronize()
    missing = sorted(n for n in dir(pp) if not n.startswith("_") and callable(getattr(pp, n)) and n != "Tensor" and n not in RESULTS)
    result = {"source_hash": native.source_hash(), "not_reached": missing,
              "functions": {n: {"sha256": e["h"].hexdigest(), "bytes": e["bytes"], "tensors": e["tensors"]} for n, e in sorted(RESULTS.items())}}
    if args.timing:
        result["timing_us_per_call"] = timing(x, truths_dev)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps({"functions": len(RESULTS), "not_reached": missing, "source_hash": result["source_hash"], "timing": result.get("timing_us_per_call")}))


if __name__ == "__main__":
    main()
