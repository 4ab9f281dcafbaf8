"""The refusals of the mdpt_post_* entry points as a table: tests/test_post_refusals_cpu.py runs every case against the built library and compares the
return code and the whole mdpt_last_error() text with tests/golden/post_refusals.json (written by tests/golden/gen_post_refusals.py).

A case is (name, entry point, arguments that replace those of GOOD[entry point]): a complete call that differs from a well-formed one in exactly one
respect - or, for the "two faults" cases, in two, which pins the ORDER of the checks (the order decides which message a doubly wrong call gets). Every
case returns MDPT_E_INVALID before anything is launched, so nothing here needs a GPU: device pointers are fake constants (multiples of 4096, misaligned
where a case wants that), host tables are real numpy records of the project's own *_RECORD dtypes. ACCEPTED holds well-formed *_scratch_bytes queries,
which run on the CPU: their byte counts pin the size arithmetic."""
import ctypes

import numpy as np

from muggled_dpt_amd.postprocess._common import GUIDED_RECORD, PAIR_RECORD, TEXTURE_RECORD, TILE_RECORD
from muggled_dpt_amd.refocus import REFOCUS_RECORD  # (under their feature modules' names, which every commit has: the table also runs where the golden file is made)
from muggled_dpt_amd.relight import NORMALS_RECORD, SHADOWS_RECORD

P = 4096  # a fake device pointer; P * k are others
BIG = 1 << 40  # a scratch size that is always enough
OUT, OUT_I32 = "size_t*", "int32_t*"  # an output argument of the host: a fresh size_t / int32_t by reference
NAN, INF = float("nan"), float("inf")
HUGE_HW = (65536, 32768)  # H W = 2^31
THIN_W = (1 << 31) - 1  # a 1 x THIN_W photo has 2^26 tiles of 32 x 32: 32 of them reach the 2^31 tiles a call refuses


def _changed(r, changed):
    """records with field[name][k] = v for every name=(k, v); a tuple of such pairs changes several records"""
    for name, kv in changed.items():
        for k, v in (kv if isinstance(kv[0], tuple) else (kv,)):
            r[name][k] = v
    return r


def tiles(n=2, **changed):
    r = np.zeros(n, TILE_RECORD)
    r["map"], r["h"], r["w"], r["x1"], r["y1"], r["x2"], r["y2"] = P * (1 + np.arange(n)), 4, 5, 0, 0, 8, 6
    return _changed(r, changed)


def pairs(n=2, **changed):
    r = np.zeros(n, PAIR_RECORD)
    r["pred"], r["ph"], r["pw"], r["truth"], r["H"], r["W"] = P * (1 + np.arange(n)), 4, 5, P * (9 + np.arange(n)), 8, 9
    return _changed(r, changed)


def guided(n=3, **changed):
    r = np.zeros(n, GUIDED_RECORD)
    r["map"], r["photo"], r["out"] = P * (1 + np.arange(n)), P * (11 + np.arange(n)), P * (21 + np.arange(n))
    r["h"], r["w"], r["H"], r["W"], r["pitch"], r["scratch_off"] = 4, 5, 8, 9, 27, 4000 * np.arange(n)  # (a 4 x 5 map: 20 cells of 25 words)
    return _changed(r, changed)


def textures(n=1, **changed):
    r = np.zeros(n, TEXTURE_RECORD)
    r["bgr"], r["h"], r["w"] = P * (1 + np.arange(n)), 6, 7
    return _changed(r, changed)


def _photo_pairs(dtype, n, H, W, region, outputs, changed):
    r = np.zeros(n, dtype)
    r["map"], r["photo"], r["h"], r["w"], r["H"], r["W"], r["pitch"] = P * (1 + np.arange(n)), P * (41 + np.arange(n)), 4, 5, H, W, 3 * W
    for k, name in enumerate(outputs):
        r[name] = P * (100 * (k + 1) + np.arange(n))
    r["scratch_off"], r["tile_off"] = region * np.arange(n), ((H + 31) // 32) * ((W + 31) // 32) * np.arange(n)
    if "step" in dtype.names:
        r["step"], r["kx"], r["ky"] = 2, 0.4, 0.3
    if "gh" in dtype.names:
        r["gh"], r["gw"], r["gtile_off"] = 40, 33, 4 * np.arange(n)
    return _changed(r, changed)


def refocus(n=3, size=(70, 33), **changed):
    return _photo_pairs(REFOCUS_RECORD, n, *size, 1024 + 8 * size[0] * size[1], ("out",), changed)


def normals(n=3, size=(70, 33), **changed):
    return _photo_pairs(NORMALS_RECORD, n, *size, 1024, ("normals", "encoded", "relit"), changed)


def shadows(n=3, size=(70, 33), **changed):
    return _photo_pairs(SHADOWS_RECORD, n, *size, 1024, ("ao", "vis", "relit"), changed)


def thin(make):
    """32 records of a 1 x THIN_W photo each, well-formed but for their 2^31 tiles (the scratch regions 2^35 bytes apart)"""
    r = make(32, (1, THIN_W))
    r["scratch_off"], r["tile_off"] = (1 << 35) * np.arange(32), (1 << 26) * np.arange(32)
    return r


def ptrs(*values):
    return np.array(values, np.uint64)


def hw(*values):
    return np.array(values, np.int32)


def xy(x, y):
    return (ctypes.c_double * 2)(x, y)


# one well-formed call per entry point, arguments in the order of include/mdpt.h
GOOD = {
    "mdpt_post_minmax": dict(src=P, count=16, minmax=2 * P, scratch8=3 * P, stream=None),
    "mdpt_post_scale_prediction": dict(src=P, B=2, ih=4, iw=5, out=2 * P, oh=8, ow=9, minmax=3 * P, scratch8=4 * P, stream=None),
    "mdpt_post_normalize": dict(src=P, count=16, minmax=2 * P, out=3 * P, mode=1, lossy=0, stream=None),
    "mdpt_post_minmax_seg": dict(src=P, dtype=0, B=2, ih=4, iw=5, out=2 * P, oh=8, ow=9, parts=3 * P, hist_clear=4 * P, stream=None),
    "mdpt_post_u8_hist_seg": dict(src=P, dtype=0, B=2, count=20, parts=2 * P, reverse=0, out=3 * P, hist=4 * P, stream=None),
    "mdpt_post_histogram": dict(src=P, B=2, count=20, hist=2 * P, stream=None),
    "mdpt_post_equalize_lut": dict(hist=P, B=2, bin_of_value=2 * P, lo=0, hi=255, lut=3 * P, stream=None),
    "mdpt_post_colorize": dict(src=P, B=2, count=20, eq_lut=2 * P, cmap=3 * P, channels=3, out=4 * P, stream=None),
    "mdpt_post_display_prep": dict(src=P, dtype=0, B=2, ih=4, iw=5, out=2 * P, oh=8, ow=9, parts=3 * P, hist_clear=4 * P, stream=None),
    "mdpt_post_plane_fit": dict(src=P, dtype=0, B=2, H=8, W=9, parts=2 * P, sample_xy=3 * P, num_samples=16, xy_per_image=0, coef=4 * P, stream=None),
    "mdpt_post_plane_eval": dict(coef=P, B=2, H=8, W=9, out=2 * P, stream=None),
    "mdpt_post_plane_minmax": dict(src=P, dtype=0, B=2, H=8, W=9, parts=2 * P, coef=3 * P, factor=1.0, vparts=4 * P, stream=None),
    "mdpt_post_threshold": dict(src=P, dtype=0, B=2, H=8, W=9, parts=2 * P, coef=3 * P, factor=1.0, vparts=4 * P, tmin=0.2, tmax=0.8, mode=1, reverse=0,
                                out=5 * P, hist=6 * P, stream=None),
    "mdpt_post_edge_mag": dict(src=P, B=2, H=8, W=9, parts=2 * P, blur=np.full(25, 0.04, np.float32), ksize=5, mag=3 * P, mag_max=4 * P, stream=None),
    "mdpt_post_edge_mask": dict(mag=P, mag_max=2 * P, B=2, count=20, out=3 * P, stream=None),
    "mdpt_post_pack_u24_alpha": dict(src=P, B=2, count=20, parts=2 * P, lossy=0, mag=3 * P, mag_max=4 * P, mask=None, mask_per_image=0, out=5 * P, stream=None),
    "mdpt_post_minmax_images": dict(src=ptrs(P, 2 * P), in_hw=hw(4, 5, 3, 7), dtype=0, B=2, out=3 * P, out_hw=hw(8, 9, 6, 6), parts=4 * P, hist_clear=5 * P,
                                    stream=None),
    "mdpt_post_u8_hist_images": dict(src=ptrs(P, 2 * P), hw=hw(4, 5, 3, 7), dtype=0, B=2, parts=3 * P, reverse=0, out=4 * P, hist=5 * P, stream=None),
    "mdpt_post_colorize_images": dict(src=P, hw=hw(4, 5, 3, 7), B=2, eq_lut=2 * P, cmap=3 * P, channels=3, out=4 * P, stream=None),
    "mdpt_post_mask_display": dict(src=P, dtype=0, B=2, H=8, W=9, parts=2 * P, coef=3 * P, factor=1.0, vparts=4 * P, tmin=0.2, tmax=0.8, invert=0, images=5 * P,
                                   image_h=8, image_w=9, mask=6 * P, composite=7 * P, stream=None),
    "mdpt_post_mask_cutout_images": dict(maps=ptrs(P, 2 * P), map_hw=hw(4, 5, 3, 7), dtype=0, parts=ptrs(3 * P, 4 * P), coef=ptrs(5 * P, 6 * P),
                                         vparts=ptrs(7 * P, 8 * P), factor=1.0, images=ptrs(9 * P, 10 * P), image_hw=hw(8, 9, 6, 6),
                                         out_offsets=np.array([0, 72], np.int64), B=2, tmin=0.2, tmax=0.8, invert=0, bgra=11 * P, mask=12 * P, stream=None),
    "mdpt_post_block_norm_tiles": dict(maps=ptrs(P, 2 * P), map_hw=hw(4, 4, 8, 2), L=2, B=2, H=8, W=8, tiles=3 * P, minmax=4 * P, stream=None),
    "mdpt_post_mesh_grid": dict(w=640, h=480, target_faces=1000.0, nx=OUT_I32, ny=OUT_I32),
    "mdpt_post_mesh_scratch_bytes": dict(B=2, nx=30, ny=20, bytes=OUT),
    "mdpt_post_mesh": dict(frames=P, B=2, H=8, W=9, nx=30, ny=20, vertex_xy=None, a=1.0, b=0.0, tan_half_fov=0.5, x_scale=1.0, y_scale=1.0, edge=0.1, is_metric=0,
                           mode=0, xyz=2 * P, uv=3 * P, faces=4 * P, counts=5 * P, bounds=6 * P, scratch=7 * P, nbytes=BIG, stream=None),
    "mdpt_post_tile_scratch_bytes": dict(tiles=tiles(), T=2, bytes=OUT),
    "mdpt_post_tile_fit": dict(tiles=tiles(), dev=P, T=2, dtype=0, guide=2 * P, guide_dtype=0, gh=4, gw=4, H=16, W=16, fit=3 * P, sums=4 * P, scratch=5 * P,
                               nbytes=BIG, stream=None),
    "mdpt_post_tile_blend": dict(tiles=tiles(), dev=P, T=2, dtype=0, H=16, W=16, fit=2 * P, sums=3 * P, feather=4.0, out=4 * P, stream=None),
    "mdpt_post_align_scratch_bytes": dict(pairs=pairs(), n=2, bytes=OUT),
    "mdpt_post_align_fit": dict(pairs=pairs(), dev=P, n=2, dtype=0, space=0, method=0, tmin=0.5, tmax=80.0, fit=2 * P, sums=3 * P, scratch=4 * P, nbytes=BIG,
                                stream=None),
    "mdpt_post_align_metrics": dict(pairs=pairs(), dev=P, n=2, dtype=0, space=0, tmin=0.5, tmax=80.0, fit=2 * P, metrics=3 * P, scratch=4 * P, nbytes=BIG,
                                    stream=None),
    "mdpt_post_align_apply": dict(pairs=pairs(), dev=P, n=2, dtype=0, space=0, fit=2 * P, offsets=np.array([0, 72], np.int64), offsets_dev=3 * P, dmin=0.1,
                                  dmax=100.0, out=4 * P, stream=None),
    "mdpt_post_guided_scratch_bytes": dict(pairs=guided(), n=3, bytes=OUT),
    "mdpt_post_guided_upsample": dict(pairs=guided(), dev=P, n=3, dtype=0, radius=4, eps=1e-4, scratch=2 * P, nbytes=BIG, coeffs=3 * P, stream=None),
    "mdpt_post_render_scratch_bytes": dict(B=1, V=2, nv=100, nf=150, oh=48, ow=64, bytes=OUT),
    "mdpt_post_render": dict(xyz=P, uv=2 * P, faces=3 * P, counts=4 * P, B=1, nv=100, nf=150, mode=0, tex=textures(), tex_dev=5 * P, view_proj=6 * P, V=2, oh=48,
                             ow=64, cull_back=0, point_size=1.0, color=7 * P, depth=8 * P, face_id=9 * P, scratch=10 * P, nbytes=BIG, stream=None),
    "mdpt_post_fill_scratch_bytes": dict(N=2, H=48, W=64, bytes=OUT),
    "mdpt_post_fill_holes": dict(color=P, depth=2 * P, N=2, H=48, W=64, band=0.1, out=3 * P, out_depth=4 * P, scratch=5 * P, nbytes=BIG, stream=None),
    "mdpt_post_video_scratch_bytes": dict(T=3, h=24, w=32, oh=0, ow=0, bytes=OUT),
    "mdpt_post_video_fit": dict(frames=P, dtype=0, T=3, h=24, w=32, prev=2 * P, ab_in=3 * P, started=4 * P, rounds=2, c=0.1, cut_corr=0.5, table=5 * P,
                                ab_out=6 * P, sums=7 * P, scratch=8 * P, nbytes=BIG, stream=None),
    "mdpt_post_video_filter": dict(frames=P, dtype=0, T=3, h=24, w=32, table=2 * P, prev_out=3 * P, alpha=0.5, tau=0.1, out=4 * P, stream=None),
    "mdpt_post_video_display": dict(stable=P, T=3, h=24, w=32, table=2 * P, range_in=3 * P, started=4 * P, oh=0, ow=0, reverse=0, cmap=5 * P, range_rate=0.5,
                                    out=6 * P, ranges=7 * P, range_out=8 * P, scratch=9 * P, nbytes=BIG, stream=None),
    "mdpt_post_refocus_scratch_bytes": dict(records=refocus(), n=3, max_radius=16, bytes=OUT),
    "mdpt_post_refocus": dict(records=refocus(), dev=P, n=3, dtype=0, space=0, focus=0.5, focus_xy=None, aperture=8.0, focus_range=0.1, max_radius=16,
                              scratch=2 * P, nbytes=BIG, radius_out=None, defocus_out=None, stream=None),
    "mdpt_post_normals_scratch_bytes": dict(records=normals(), n=3, bytes=OUT),
    "mdpt_post_normals": dict(records=normals(), dev=P, n=3, dtype=0, space=0, min_depth=50.0, max_depth=100.0, edge_ratio=2.0, lights=2 * P, num_lights=2,
                              ambient=0.35, diffuse=0.9, specular=0.0, shininess_log2=4, scratch=3 * P, nbytes=BIG, stream=None),
    "mdpt_post_shadows_scratch_bytes": dict(records=shadows(), n=3, bytes=OUT),
    "mdpt_post_shadows": dict(records=shadows(), dev=P, n=3, dtype=0, space=0, min_depth=50.0, max_depth=100.0, edge_ratio=2.0, lights=2 * P, num_lights=2,
                              ambient=0.35, diffuse=0.9, specular=0.0, shininess_log2=4, shadow_reach=8, shadow_bias=0.01, shadow_thickness=INF, ao_reach=8,
                              ao_radius=0.6, ao_bias=0.01, ao_strength=1.0, scratch=3 * P, nbytes=BIG, stream=None),
}

CASES = []  # (name, entry point, the arguments that differ from GOOD[entry point])


def _add(entry, **named):
    """cases of mdpt_post_<entry>, named <entry>.<name>"""
    for name, kw in named.items():
        CASES.append((f"{entry}.{name}", "mdpt_post_" + entry, kw))


# ---- the entry points whose bodies only move: at least one refusal each; the shared check_* helpers through them, every message of each
_add("minmax", empty=dict(count=0), null=dict(src=None))
_add("scale_prediction", null=dict(out=None), minmax_without_scratch=dict(scratch8=None), size=dict(B=0))
_add("normalize", empty=dict(count=0), mode=dict(mode=3))
_add("minmax_seg", null=dict(parts=None), dtype=dict(dtype=9), size=dict(B=65536), out_size=dict(oh=0))
_add("u8_hist_seg", empty=dict(count=0), dtype=dict(dtype=-1), batch=dict(B=0), count=dict(count=1 << 31))
_add("histogram", null=dict(hist=None), batch=dict(B=70000))
_add("equalize_lut", null=dict(lut=None), batch=dict(B=0), range=dict(lo=5, hi=5))
_add("colorize", empty=dict(count=0), batch=dict(B=0), channels=dict(channels=2), count=dict(count=1 << 31))
_add("display_prep", null=dict(out=None), dtype=dict(dtype=3), in_size=dict(ih=0), out_size=dict(ow=-1), batch=dict(B=65536))  # check_batch_hw
_add("plane_fit", null=dict(sample_xy=None), dtype=dict(dtype=3), size=dict(W=0), samples=dict(num_samples=0))
_add("plane_eval", null=dict(coef=None), size=dict(B=0))
_add("plane_minmax", null=dict(vparts=None), dtype=dict(dtype=3), size=dict(H=0))
_add("threshold", null=dict(out=None), dtype=dict(dtype=3), size=dict(H=0), mode=dict(mode=2), reverse=dict(reverse=1), order=dict(tmin=0.9), nan=dict(tmax=NAN))
_add("edge_mag", null=dict(blur=None), size=dict(B=0), ksize_even=dict(ksize=4), ksize_large=dict(ksize=17), small=dict(H=2))
_add("edge_mask", empty=dict(count=0), batch=dict(B=0))
_add("pack_u24_alpha", empty=dict(count=0), mag_without_max=dict(mag_max=None), batch=dict(B=0), two_alphas=dict(mask=6 * P))
_add("minmax_images", null=dict(in_hw=None), out_without_hw=dict(out_hw=None), dtype=dict(dtype=3), batch=dict(B=0), batch_large=dict(B=65536),
     null_image=dict(src=ptrs(P, 0)), in_size=dict(in_hw=hw(4, 5, 0, 7)), out_size=dict(out_hw=hw(8, 9, 6, -6)))  # check_images
_add("u8_hist_images", null=dict(out=None), dtype=dict(dtype=3), batch=dict(B=0), null_image=dict(src=ptrs(0, P)), size=dict(hw=hw(4, 0, 3, 7)))
_add("colorize_images", null=dict(hw=None), channels=dict(channels=4), batch=dict(B=0), size=dict(hw=hw(4, 5, 3, 0)))
_add("mask_display", null=dict(images=None), dtype=dict(dtype=3), size=dict(W=0), image_size=dict(image_h=0), window_low=dict(tmin=-0.1), window_high=dict(tmax=1.5),
     window_order=dict(tmin=0.9), window_nan=dict(tmin=NAN))  # check_mask_window
_add("mask_cutout_images", null=dict(out_offsets=None), bgra=dict(bgra=11 * P + 2), dtype=dict(dtype=3), window=dict(tmax=1.5), batch=dict(B=0),
     null_map=dict(maps=ptrs(P, 0)), map_size=dict(map_hw=hw(4, 5, 3, 0)), null_image=dict(images=ptrs(0, 10 * P)), image_size=dict(image_hw=hw(0, 9, 6, 6)),
     statistics=dict(coef=ptrs(5 * P, 0)), offset=dict(out_offsets=np.array([0, -4], np.int64)))
_add("block_norm_tiles", null=dict(minmax=None), size=dict(B=0), count=dict(L=0), tile_size=dict(H=8192, W=4096, map_hw=hw(4, 4, 8, 2)),
     null_map=dict(maps=ptrs(P, 0)), map_size=dict(map_hw=hw(4, 4, 0, 2)), divide=dict(map_hw=hw(4, 4, 3, 2)))
_add("mesh_grid", null=dict(nx=None), size=dict(w=0), nan=dict(target_faces=NAN), large=dict(target_faces=1e19))
_add("mesh_scratch_bytes", null=dict(bytes=None), batch=dict(B=0), side=dict(nx=1), vertices=dict(nx=65536, ny=32768), faces=dict(nx=32769, ny=32769))  # check_mesh_grid
_add("mesh", null=dict(bounds=None), frames=dict(frames=P + 2), size=dict(H=0), side=dict(ny=1), large=dict(nx=65536, ny=32768), mode=dict(mode=2), edge=dict(edge=NAN),
     scratch=dict(nbytes=4 * 2 * (600 + 3 + 3 + 6) - 4))
_add("tile_scratch_bytes", null=dict(bytes=None), null_table=dict(tiles=None), count=dict(T=0), null_map=dict(tiles=tiles(map=(1, 0))),
     map_size=dict(tiles=tiles(h=(0, 0))), box_empty=dict(tiles=tiles(x2=(1, 0))), box_negative=dict(tiles=tiles(y1=(0, -1))),
     large=dict(tiles=tiles(h=(1, 1 << 18), w=(1, 1 << 18))))  # check_tiles
_add("tile_fit", null=dict(guide=None), dtype=dict(dtype=3), guide_dtype=dict(guide_dtype=3), size=dict(H=0), guide_size=dict(gw=0), count=dict(T=65536),
     null_table=dict(tiles=None), misaligned_map=dict(tiles=tiles(map=(1, P + 2))), map_aligned_to_its_element=dict(tiles=tiles(map=(1, P + 2)), dtype=1, scratch=P + 4),
     box_outside=dict(tiles=tiles(x2=(1, 17))), table=dict(dev=P + 4), guide=dict(guide=2 * P + 2), scratch=dict(nbytes=2 * 1 * 48 - 8))
_add("tile_blend", null=dict(out=None), dtype=dict(dtype=3), size=dict(W=0), feather=dict(feather=-1.0), feather_inf=dict(feather=INF),
     large=dict(H=1 << 19, W=1 << 19, tiles=tiles()), count=dict(T=0), box_outside=dict(tiles=tiles(y2=(0, 17))), fit=dict(fit=2 * P + 4), out=dict(out=4 * P + 2))
_add("align_scratch_bytes", null=dict(bytes=None), null_table=dict(pairs=None), count=dict(n=0), count_large=dict(n=65536), pred=dict(pairs=pairs(pred=(1, 0))),
     pred_misaligned=dict(pairs=pairs(pred=(0, P + 1))), size=dict(pairs=pairs(pw=(1, 0))), truth_size=dict(pairs=pairs(H=(0, -8))),
     truth_large=dict(pairs=pairs(H=(1, HUGE_HW[0]), W=(1, HUGE_HW[1]))))  # check_pairs
_add("align_fit", null=dict(sums=None), dtype=dict(dtype=3), space=dict(space=2), range=dict(tmin=90.0), range_nan=dict(tmax=NAN), method=dict(method=2),
     null_truth=dict(pairs=pairs(truth=(1, 0))), truth_misaligned=dict(pairs=pairs(truth=(0, 9 * P + 2))), pred_misaligned=dict(pairs=pairs(pred=(0, P + 2))),
     pointer=dict(fit=2 * P + 4), scratch=dict(nbytes=2 * 1 * 88 + 2 * 1040 * 4 - 8))  # check_align_common
_add("align_metrics", null=dict(metrics=None), dtype=dict(dtype=3), space=dict(space=-1), range=dict(tmin=90.0), null_truth=dict(pairs=pairs(truth=(0, 0))),
     pointer=dict(scratch=4 * P + 4), scratch=dict(nbytes=0))
_add("align_apply", null=dict(offsets=None), dtype=dict(dtype=3), space=dict(space=2), clamp=dict(dmin=200.0), clamp_nan=dict(dmax=NAN), count=dict(n=0),
     size=dict(pairs=pairs(ph=(0, 0))), offset=dict(offsets=np.array([0, -72], np.int64)), pointer=dict(offsets_dev=3 * P + 4), out=dict(out=4 * P + 2))
_add("render_scratch_bytes", null=dict(bytes=None), batch=dict(B=0), views=dict(V=0), product=dict(B=256, V=256), vertices=dict(nv=0), faces=dict(nf=0),
     size=dict(oh=0), side=dict(ow=32769))  # check_render_sizes
_add("render", null=dict(tex=None), views=dict(V=0), capacity=dict(nf=-1), size=dict(oh=32769), mode=dict(mode=2), points=dict(mode=1), point_size=dict(point_size=0.0),
     point_size_nan=dict(point_size=NAN), null_texture=dict(tex=textures(bgr=(0, 0))), texture_size=dict(tex=textures(w=(0, 0))), matrices=dict(view_proj=6 * P + 4),
     slab=dict(uv=2 * P + 2), scratch=dict(nbytes=1 * 2 * (100 * 24 + 48 * 64 * 8) - 8))
_add("fill_scratch_bytes", null=dict(bytes=None), count=dict(N=0), count_large=dict(N=65536), size=dict(H=0), side=dict(W=32769))  # check_fill_sizes
_add("fill_holes", null=dict(depth=None), count=dict(N=0), size=dict(W=0), band=dict(band=1.5), band_nan=dict(band=NAN), image=dict(color=P + 2), scratch16=dict(scratch=5 * P + 8),
     in_place=dict(out=P), depth_in_place=dict(out_depth=2 * P), scratch=dict(nbytes=64))
_add("video_scratch_bytes", null=dict(bytes=None), count=dict(T=0), count_large=dict(T=65536), size=dict(h=0), large=dict(h=HUGE_HW[0], w=HUGE_HW[1]),
     display_one_zero=dict(oh=48), display_negative=dict(oh=-1, ow=-1), display_large=dict(oh=HUGE_HW[0], ow=HUGE_HW[1]))  # check_video_sizes, check_video_out
_add("video_fit", null=dict(started=None), dtype=dict(dtype=3), count=dict(T=0), size=dict(w=0), rounds=dict(rounds=9), c=dict(c=0.0), c_large=dict(c=1e151),
     cut_corr=dict(cut_corr=1.5), pointer=dict(sums=7 * P + 4), flag=dict(started=4 * P + 2), frames=dict(frames=P + 2), frames_f16=dict(frames=P + 1, dtype=2),
     scratch=dict(nbytes=(3 * 1 * 6 + 3 * 4) * 8 - 8))
_add("video_filter", null=dict(prev_out=None), dtype=dict(dtype=3), size=dict(h=0), alpha=dict(alpha=0.0), tau=dict(tau=-1.0), tau_large=dict(tau=1e151),
     table=dict(table=2 * P + 4), in_place=dict(out=P), over_prev=dict(out=3 * P))
_add("video_display", null=dict(range_out=None), count=dict(T=0), display=dict(ow=64), display_large=dict(oh=HUGE_HW[0], ow=HUGE_HW[1]), rate=dict(range_rate=0.0),
     table=dict(table=2 * P + 4), scratch4=dict(scratch=9 * P + 2), scratch=dict(nbytes=2 * 3 * 64 * 2 * 4 + 3 * 24 * 32 - 1),
     scratch_resized=dict(oh=48, ow=64, nbytes=2 * 3 * 64 * 2 * 4 + 3 * 48 * 64 * 5 - 1))

# ---- the four record entry points: every refusal of each, in the order of the checks
_add("guided_scratch_bytes", null=dict(bytes=None), null_table=dict(pairs=None), count=dict(n=0), count_large=dict(n=65536), map_size=dict(pairs=guided(h=(1, 0))),
     map_large=dict(pairs=guided(h=(2, HUGE_HW[0]), w=(2, HUGE_HW[1]))))  # check_guided_sizes
_add("guided_upsample", null=dict(dev=None), null_table=dict(pairs=None), null_scratch=dict(scratch=None), dtype=dict(dtype=3), radius=dict(radius=65),
     radius_negative=dict(radius=-1), eps=dict(eps=0.0), eps_nan=dict(eps=NAN), eps_inf=dict(eps=INF), count=dict(n=0), map_size=dict(pairs=guided(w=(0, -5))),
     pointer=dict(coeffs=3 * P + 4), table=dict(dev=P + 2), null_map=dict(pairs=guided(map=(1, 0))), null_photo=dict(pairs=guided(photo=(0, 0))),
     null_out=dict(pairs=guided(out=(2, 0))), misaligned_map=dict(pairs=guided(map=(1, 2 * P + 2))), map_aligned_to_its_element=dict(pairs=guided(map=(1, 2 * P + 2), pitch=(1, 26)), dtype=2),
     misaligned_out=dict(pairs=guided(out=(0, 21 * P + 2))), shrinks=dict(pairs=guided(H=(1, 3), pitch=(1, 27))), photo_large=dict(pairs=guided(H=(2, HUGE_HW[0]), W=(2, HUGE_HW[1]), pitch=(2, 3 * HUGE_HW[1]))),
     pitch=dict(pairs=guided(pitch=(1, 26))), region_negative=dict(pairs=guided(scratch_off=(0, -8))), region_misaligned=dict(pairs=guided(scratch_off=(1, 4004))),
     region_beyond=dict(pairs=guided(scratch_off=(2, BIG + 8))), region_cut=dict(nbytes=12000 - 8), overlap=dict(pairs=guided(scratch_off=(2, 4000 + 3992))),
     same_region=dict(pairs=guided(scratch_off=(1, 0))))
_add("refocus_scratch_bytes", null=dict(bytes=None), null_table=dict(records=None), count=dict(n=0), count_large=dict(n=65536), max_radius=dict(max_radius=33),
     max_radius_negative=dict(max_radius=-1), photo_size=dict(records=refocus(H=(1, 0))), photo_large=dict(records=refocus(H=(2, HUGE_HW[0]), W=(2, HUGE_HW[1]))))
_add("refocus", null=dict(dev=None), null_table=dict(records=None), null_scratch=dict(scratch=None), dtype=dict(dtype=3), space=dict(space=2), count=dict(n=0),
     max_radius=dict(max_radius=33), photo_size=dict(records=refocus(W=(0, 0))), aperture=dict(aperture=-1.0), aperture_nan=dict(aperture=NAN),
     focus_range=dict(focus_range=INF), focus_xy=dict(focus_xy=xy(0.5, 1.5)), focus_xy_nan=dict(focus_xy=xy(NAN, 0.5)), focus_inverse=dict(focus=1.5),
     focus_depth=dict(space=1, focus=0.0), focus_depth_inf=dict(space=1, focus=INF), pointer=dict(scratch=2 * P + 4), defocus_out=dict(defocus_out=5 * P + 2),
     null_map=dict(records=refocus(map=(1, 0))), null_photo=dict(records=refocus(photo=(0, 0))), misaligned_map=dict(records=refocus(map=(2, 3 * P + 2))),
     map_size=dict(records=refocus(h=(0, 0))), map_large=dict(records=refocus(h=(1, HUGE_HW[0]), w=(1, HUGE_HW[1]))), pitch=dict(records=refocus(pitch=(2, 98))),
     region_negative=dict(records=refocus(scratch_off=(0, -8))), region_misaligned=dict(records=refocus(scratch_off=(1, 19508))),
     region_beyond=dict(records=refocus(scratch_off=(2, BIG + 8))), region_cut=dict(nbytes=3 * 19504 - 8), tile_off=dict(records=refocus(tile_off=(2, 5))),
     tile_off_first=dict(records=refocus(tile_off=(0, 1))), some_out=dict(records=refocus(out=(1, 0))), nothing_asked=dict(records=refocus(out=((0, 0), (1, 0), (2, 0)))),
     tiles=dict(records=thin(refocus), n=32, nbytes=1 << 62), overlap=dict(records=refocus(scratch_off=(1, 8))), same_region=dict(records=refocus(scratch_off=(2, 0))))
_add("normals_scratch_bytes", null=dict(bytes=None), null_table=dict(records=None), count=dict(n=0), count_large=dict(n=65536), photo_size=dict(records=normals(H=(1, 0))),
     photo_large=dict(records=normals(H=(2, HUGE_HW[0]), W=(2, HUGE_HW[1]))))
_RELIGHT = dict(  # the scalar and per-record refusals that mdpt_post_normals and mdpt_post_shadows share, under the same names
    null=dict(dev=None), null_table=dict(records=None), null_scratch=dict(scratch=None), dtype=dict(dtype=3), space=dict(space=2), count=dict(n=0), count_large=dict(n=65536),
    depth_zero=dict(min_depth=0.0), depth_order=dict(min_depth=100.0), depth_inf=dict(max_depth=INF), depth_nan=dict(min_depth=NAN), edge_ratio=dict(edge_ratio=0.5),
    edge_ratio_nan=dict(edge_ratio=NAN), lights_many=dict(num_lights=65), lights_negative=dict(num_lights=-1), ambient=dict(ambient=-1.0), diffuse=dict(diffuse=NAN),
    specular=dict(specular=INF), shininess=dict(shininess_log2=11), shininess_negative=dict(shininess_log2=-1), table=dict(dev=P + 4), lights_misaligned=dict(lights=2 * P + 4),
    scratch_misaligned=dict(scratch=3 * P + 4), no_lights=dict(num_lights=0), null_lights=dict(lights=None), region_cut=dict(nbytes=3 * 1024 - 8))
_RELIGHT_RECORDS = dict(  # ... and those of their records: name -> the changed fields
    photo_size=dict(W=(1, 0)), photo_large=dict(H=(2, HUGE_HW[0]), W=(2, HUGE_HW[1])), null_map=dict(map=(1, 0)), misaligned_map=dict(map=(2, 3 * P + 2)), map_size=dict(w=(0, 0)),
    map_large=dict(h=(1, HUGE_HW[0]), w=(1, HUGE_HW[1])), pitch=dict(pitch=(0, 98)), step_zero=dict(step=(1, 0)), step_large=dict(step=(1, 17)), kx=dict(kx=(0, 0.0)),
    ky_nan=dict(ky=(0, NAN)), kx_inf=dict(kx=(2, INF)), region_negative=dict(scratch_off=(0, -8)), region_misaligned=dict(scratch_off=(1, 1028)),
    region_beyond=dict(scratch_off=(2, BIG + 8)), tile_off=dict(tile_off=(2, 5)), tile_off_first=dict(tile_off=(0, 1)), some_relit=dict(relit=(1, 0)),
    some_photo=dict(photo=(2, 0)), overlap=dict(scratch_off=(1, 8)), same_region=dict(scratch_off=(2, 0)))
_add("normals", **_RELIGHT, **{name: dict(records=normals(**fields)) for name, fields in _RELIGHT_RECORDS.items()},
     misaligned_normals=dict(records=normals(normals=(0, 100 * P + 2))), some_normals=dict(records=normals(normals=(0, 0))), some_encoded=dict(records=normals(encoded=(2, 0))),
     nothing_asked=dict(records=normals(normals=((0, 0), (1, 0), (2, 0)), encoded=((0, 0), (1, 0), (2, 0)), relit=((0, 0), (1, 0), (2, 0)))),
     tiles=dict(records=thin(normals), n=32))
_add("shadows_scratch_bytes", null=dict(bytes=None), null_table=dict(records=None), count=dict(n=0), count_large=dict(n=65536), photo_size=dict(records=shadows(H=(1, 0))),
     photo_large=dict(records=shadows(H=(2, HUGE_HW[0]), W=(2, HUGE_HW[1]))), grid_size=dict(records=shadows(gh=(1, 0))),
     grid_large=dict(records=shadows(gh=(0, HUGE_HW[0]), gw=(0, HUGE_HW[1]))))
_add("shadows", **_RELIGHT, **{name: dict(records=shadows(**fields)) for name, fields in _RELIGHT_RECORDS.items()},
     grid_size=dict(records=shadows(gw=(2, -1))), shadow_reach=dict(shadow_reach=33), shadow_reach_negative=dict(shadow_reach=-1), ao_reach=dict(ao_reach=33),
     shadow_bias=dict(shadow_bias=1.0), shadow_bias_nan=dict(shadow_bias=NAN), shadow_thickness=dict(shadow_thickness=-0.5), ao_radius=dict(ao_radius=0.0),
     ao_radius_inf=dict(ao_radius=INF), ao_bias=dict(ao_bias=-1.0), ao_strength=dict(ao_strength=NAN), misaligned_ao=dict(records=shadows(ao=(0, 100 * P + 2))),
     misaligned_vis=dict(records=shadows(vis=(1, 200 * P + 1))), gtile_off=dict(records=shadows(gtile_off=(1, 5))), some_ao=dict(records=shadows(ao=(0, 0))),
     some_vis=dict(records=shadows(vis=(2, 0))),
     nothing_asked=dict(records=shadows(ao=((0, 0), (1, 0), (2, 0)), vis=((0, 0), (1, 0), (2, 0)), relit=((0, 0), (1, 0), (2, 0)))),
     vis_without_lights=dict(records=shadows(relit=((0, 0), (1, 0), (2, 0))), num_lights=0),
     shade_without_vis=dict(records=shadows(vis=((0, 0), (1, 0), (2, 0)))), shade_without_ao=dict(records=shadows(ao=((0, 0), (1, 0), (2, 0)))),
     tiles=dict(records=thin(shadows), n=32),
     grid_tiles=dict(records=_changed(shadows(32), dict(gh=tuple((k, 1) for k in range(32)), gw=tuple((k, THIN_W) for k in range(32)),
                                                        gtile_off=tuple((k, k << 26) for k in range(32)))), n=32))

# ---- two faults in one call: the message is that of the check that runs first
_add("guided_upsample",
     two_dtype_then_record=dict(dtype=3, pairs=guided(map=(0, 0))), two_eps_then_map_size=dict(eps=0.0, pairs=guided(h=(0, 0))),
     two_map_size_then_pointer=dict(pairs=guided(h=(2, 0)), scratch=2 * P + 4), two_pointer_then_record=dict(coeffs=3 * P + 4, pairs=guided(photo=(0, 0))),
     two_records_in_order=dict(pairs=guided(pitch=(0, 26), map=(1, 0))), two_later_check_of_an_earlier_record=dict(pairs=guided(scratch_off=(0, -8), map=(1, 0))),
     two_null_then_misaligned=dict(pairs=guided(out=((0, 21 * P + 2), (0, 0)))), two_photo_then_pitch=dict(pairs=guided(H=(1, 3), pitch=(1, 26))),
     two_region_then_overlap=dict(pairs=guided(scratch_off=((1, 0), (2, 4004)))))
_add("refocus",
     two_dtype_then_record=dict(dtype=3, records=refocus(map=(0, 0))), two_space_then_count=dict(space=2, n=0), two_photo_size_then_aperture=dict(records=refocus(H=(2, 0)), aperture=-1.0),
     two_aperture_then_focus=dict(aperture=-1.0, focus=1.5), two_focus_then_pointer=dict(focus=1.5, scratch=2 * P + 4), two_pointer_then_record=dict(dev=P + 4, records=refocus(map=(0, 0))),
     two_records_in_order=dict(records=refocus(tile_off=(0, 1), map=(1, 0))), two_later_check_of_an_earlier_record=dict(records=refocus(pitch=(0, 98), photo=(2, 0))),
     two_region_then_tile_off=dict(records=refocus(scratch_off=(1, 19508), tile_off=(1, 7))), two_tile_off_then_outputs=dict(records=refocus(tile_off=(2, 5), out=(0, 0))),
     two_outputs_then_overlap=dict(records=refocus(out=(1, 0), scratch_off=(2, 0))))
_TWO_RELIGHT = dict(
    two_dtype_then_record=dict(dtype=3, records=dict(step=(0, 0))), two_space_then_photo_size=dict(space=2, records=dict(H=(0, 0))),
    two_photo_size_then_depth=dict(records=dict(H=(2, HUGE_HW[0]), W=(2, HUGE_HW[1])), min_depth=0.0), two_depth_then_edge_ratio=dict(min_depth=0.0, edge_ratio=0.5),
    two_edge_ratio_then_record=dict(edge_ratio=0.5, records=dict(pitch=(0, 98))), two_shininess_then_pointer=dict(shininess_log2=11, lights=2 * P + 4),
    two_pointer_then_record=dict(scratch=3 * P + 4, records=dict(map=(0, 0))), two_records_in_order=dict(records=dict(step=(0, 0), map=(1, 0))),
    two_later_check_of_an_earlier_record=dict(records=dict(tile_off=(0, 1), map=(2, 0))), two_step_then_kx=dict(records=dict(step=(1, 17), kx=(1, 0.0))),
    two_region_then_tile_off=dict(records=dict(scratch_off=(1, 1028), tile_off=(1, 7))), two_outputs_then_photo=dict(records=dict(relit=(1, 0), photo=(2, 0))),
    two_photo_then_overlap=dict(records=dict(photo=(2, 0), scratch_off=(2, 0))), two_lights_then_photo=dict(num_lights=0, records=dict(photo=(0, 0))))
for _entry, _make in (("normals", normals), ("shadows", shadows)):
    _add(_entry, **{name: {k: (_make(**v) if k == "records" else v) for k, v in kw.items()} for name, kw in _TWO_RELIGHT.items()})
_add("shadows", two_reach_then_bias=dict(ao_reach=33, shadow_bias=1.0), two_ao_then_pointer=dict(ao_strength=-1.0, dev=P + 4),
     two_tile_off_then_gtile_off=dict(records=shadows(tile_off=(1, 5), gtile_off=(1, 5))), two_plane_then_region=dict(records=shadows(vis=(0, 200 * P + 2), scratch_off=(0, 4))),
     two_lights_then_shading=dict(records=shadows(vis=((0, 0), (1, 0), (2, 0))), lights=None))

# ---- accepted *_scratch_bytes queries: (name, entry point, arguments) -> the byte count
ACCEPTED = []


def _accept(entry, **named):
    for name, kw in named.items():
        ACCEPTED.append((f"{entry}.{name}", f"mdpt_post_{entry}_scratch_bytes", kw))


_accept("mesh", small=dict(B=1, nx=2, ny=2), plain=dict(), odd=dict(B=3, nx=257, ny=513), batch=dict(B=65535, nx=2, ny=3), largest=dict(B=1, nx=32768, ny=32768))
_accept("tile", plain=dict(), one=dict(tiles=tiles(1), T=1), two_chunks=dict(tiles=tiles(h=(1, 41), w=(1, 50))), largest=dict(tiles=tiles(3, h=(2, 1 << 17), w=(2, (1 << 18) - 1)), T=3))
_accept("align", plain=dict(), one=dict(pairs=pairs(1), n=1), two_chunks=dict(pairs=pairs(H=(0, 41), W=(0, 50))), no_truth=dict(pairs=pairs(truth=(0, 0))),
        largest=dict(pairs=pairs(3, H=(1, 32768), W=(1, 65535)), n=3))
_accept("guided", plain=dict(), one=dict(pairs=guided(1), n=1), mixed=dict(pairs=guided(h=(1, 37), w=(2, 1))), largest=dict(pairs=guided(h=(0, 32768), w=(0, 65535))))
_accept("render", small=dict(B=1, V=1, nv=1, nf=1, oh=1, ow=1), plain=dict(), points=dict(B=3, V=5, nv=1001, nf=1001, oh=33, ow=65), largest=dict(B=255, V=257, nv=7, nf=9, oh=32768, ow=32768))
_accept("fill", one=dict(N=1, H=1, W=1), plain=dict(), odd=dict(N=3, H=33, W=65), top=dict(N=1, H=32, W=32), past_top=dict(N=1, H=33, W=32), largest=dict(N=65535, H=32768, W=32768))
_accept("video", one=dict(T=1, h=1, w=1), plain=dict(), resized=dict(oh=48, ow=64), shrunk=dict(oh=3, ow=5), fit_larger=dict(T=2, h=2049, w=1, oh=1, ow=1),
        odd=dict(T=5, h=7, w=9), largest=dict(T=65535, h=32768, w=65535))
_accept("refocus", plain=dict(), one=dict(records=refocus(1, (1, 1)), n=1, max_radius=0), mixed=dict(records=refocus(H=(1, 9), W=(2, 1000)), max_radius=32),
        largest=dict(records=refocus(H=(0, 32768), W=(0, 65535))))
_accept("normals", plain=dict(), one=dict(records=normals(1, (1, 1)), n=1), many=dict(records=normals(65535), n=65535), largest=dict(records=normals(H=(0, 32768), W=(0, 65535))))
_accept("shadows", plain=dict(), one=dict(records=shadows(1, (1, 1)), n=1), many=dict(records=shadows(65535), n=65535),
        largest=dict(records=shadows(H=(0, 32768), W=(0, 65535), gh=(2, 65535), gw=(2, 32768))))


def run(lib, entry, changed):
    """one call of GOOD[entry] with `changed` put in -> (return code, mdpt_last_error() text, the value left in the last OUT argument or None)"""
    unknown = set(changed) - set(GOOD[entry])
    assert not unknown, (entry, unknown)
    args, outs = [], []
    for value in {**GOOD[entry], **changed}.values():
        if isinstance(value, np.ndarray):
            value = value.ctypes.data
        elif isinstance(value, str) and value in (OUT, OUT_I32):
            outs.append(ctypes.c_size_t(0) if value == OUT else ctypes.c_int32(0))
            value = ctypes.byref(outs[-1])
        args.append(value)
    rc = getattr(lib, entry)(*args)
    return rc, lib.mdpt_last_error().decode(), (outs[-1].value if outs else None)
