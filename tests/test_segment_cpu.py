"""The depth segmentation without a GPU: the properties of the restatement (tests/segment_restate.py) on scenes whose answer is known from geometry; that the
scenes of the GPU tests have the properties those tests rely on; the argument checks of muggled_dpt_amd.segment; the exported entry points, which refuse bad
arguments before they touch a device pointer; the record tables' layout; the scratch query."""
import ctypes

import numpy as np
import pytest
import torch

from muggled_dpt_amd import native, segment
from muggled_dpt_amd.postprocess import _common
from tests import segment_restate as sr
from tests import segment_scenes as sc


def test_a_plate_before_a_wall_gives_two_regions_with_their_areas_and_boxes():
    v = sc.plate_before_wall(40, 50, (8, 10, 29, 33))
    for conn in (4, 8):
        res = sr.segment(v, step=0.02, connectivity=conn, min_area=16)
        assert res["count"] == 2 and res["first"].tolist() == [0, 8 * 50 + 10]  # the wall's root is node 0: it is region 0
        assert res["area"].tolist() == [40 * 50 - 22 * 24, 22 * 24]
        assert res["bbox"].tolist() == [[0, 0, 49, 39], [10, 8, 33, 29]]
        assert res["vmin"].tolist() == [0.0, 1.0] and res["vmax"].tolist() == [0.0, 1.0] and res["mean"].tolist() == [0.0, 1.0]
        assert res["sum_q"].tolist() == [0, 22 * 24 * 2 ** 24] and (res["lo"], res["hi"]) == (0.0, 1.0)
        assert (res["labels"][8:30, 10:34] == 1).all() and (res["labels"] == 1).sum() == 22 * 24
    # depth space: the same plate at 2 m before a wall at 4 m, a ramp of 1 % per node on the wall stays one region
    d = np.where(v > 0, 2.0, 4.0).astype(np.float32) * (1.0 + 0.01 * np.arange(50, dtype=np.float32))[None, :]
    res = sr.segment(d, space="depth", step=0.02, min_area=16)
    assert res["count"] == 2 and res["area"].tolist() == [40 * 50 - 22 * 24, 22 * 24]


def test_a_flat_map_gives_one_region():
    for space, value in (("inverse", -3.5), ("inverse", 0.0), ("depth", 2.0)):
        res = sr.segment(np.full((9, 13), value, np.float32), space=space, step=0.0, min_area=1)
        assert res["count"] == 1 and res["area"].tolist() == [117] and res["bbox"].tolist() == [[0, 0, 12, 8]] and res["sum_q"].tolist() == [0]
        assert res["mean"].tolist() == [value] and res["lo"] == res["hi"] == value
    res = sr.segment(np.full((9, 13), -2.0, np.float32), space="depth", min_area=1)  # not a depth: nothing is valid
    assert res["count"] == 0 and (res["labels"] == -1).all()


def test_a_checkerboard_gives_every_node_at_4_and_two_regions_at_8():
    v = sc.checkerboard(7, 9)
    res = sr.segment(v, connectivity=4, min_area=1)
    assert res["count"] == 63 and np.array_equal(res["labels"].reshape(-1), np.arange(63)) and (res["area"] == 1).all()
    res = sr.segment(v, connectivity=8, min_area=1)
    assert res["count"] == 2 and res["area"].tolist() == [32, 31] and np.array_equal(res["labels"], (np.add.outer(np.arange(7), np.arange(9)) & 1))
    assert sr.segment(v, connectivity=4, min_area=2)["count"] == 0


def test_a_diagonal_line_is_one_region_at_8_and_its_length_at_4():
    v = sc.diagonal(11)
    assert sr.segment(v, connectivity=8, min_area=1)["count"] == 1 and sr.segment(v, connectivity=8, min_area=1)["area"].tolist() == [11]
    res = sr.segment(v, connectivity=4, min_area=1)
    assert res["count"] == 11 and res["first"].tolist() == [12 * k for k in range(11)]
    anti = np.ascontiguousarray(v[:, ::-1])  # the other diagonal direction
    assert sr.segment(anti, connectivity=8, min_area=1)["count"] == 1 and sr.segment(anti, connectivity=4, min_area=1)["count"] == 11


def test_nan_nodes_are_minus_one_and_separate_their_neighbours():
    v = np.ones((6, 9), np.float32)
    v[:, 4] = np.nan
    v[2, 1] = np.inf
    res = sr.segment(v, connectivity=8, min_area=1)
    assert res["count"] == 2 and (res["labels"][:, 4] == -1).all() and res["labels"][2, 1] == -1
    assert (res["labels"][:, :4][np.isfinite(v[:, :4])] == 0).all() and (res["labels"][:, 5:] == 1).all() and res["area"].tolist() == [23, 24]
    res = sr.segment(np.full((4, 4), np.nan, np.float32), min_area=1)
    assert res["count"] == 0 and (res["labels"] == -1).all() and (res["lo"], res["hi"]) == (0.0, 0.0)


def test_min_area_drops_exactly_the_small_ones_and_renumbers_the_rest_in_root_order():
    v = np.zeros((12, 20), np.float32)
    v[1:3, 1:4] = 1.0  # 6 nodes, root 21
    v[5:10, 5:12] = 2.0  # 35 nodes
    v[4, 15] = 3.0  # 1 node
    v[10:12, 16:20] = 4.0  # 8 nodes
    every = sr.segment(v, min_area=1)
    assert every["count"] == 5 and every["area"].tolist() == [240 - 50, 6, 1, 35, 8]
    for min_area, kept in ((2, [0, 1, 3, 4]), (7, [0, 3, 4]), (9, [0, 3]), (36, [0]), (191, [])):
        res = sr.segment(v, min_area=min_area)
        assert res["count"] == len(kept) and res["area"].tolist() == [int(every["area"][k]) for k in kept] and res["first"].tolist() == every["first"][kept].tolist()
        for new, old in enumerate(kept):
            assert np.array_equal(res["labels"] == new, every["labels"] == old)
        assert ((res["labels"] == -1) == ~np.isin(every["labels"], kept)).all()
        assert res["count"] <= min(240, 240 // min_area)  # the slab bound


def test_the_serpentine_and_the_comb_are_what_their_names_say():
    v = sc.serpentine()
    res = sr.segment(v, min_area=1)
    path = res["labels"][0, 0]
    assert path == 0 and ((res["labels"] == path) == (v == 1.0)).all() and res["bbox"][0].tolist() == [0, 0, 129, 96]
    assert res["count"] == 1 + 48  # the path and one wall per odd row
    c = sc.comb()
    res = sr.segment(c, min_area=1)
    assert res["count"] == 1 + 49 and ((res["labels"] == 0) == (c == 1.0)).all()
    assert sr.segment(c[:-1], min_area=1)["count"] == 99  # without the last row every tooth stands alone


def test_the_random_scenes_have_the_properties_the_gpu_tests_rely_on():
    for seed, h, w, noise in sc.RANDOM_SCENES:
        for space in ("inverse", "depth"):
            v = sc.piecewise(seed, h, w, noise, positive=space == "depth")
            step = 0.02 if space == "inverse" else 0.012
            res = sr.segment(v, space=space, step=step, min_area=16)
            props = sc.region_properties(res, sr.valid_nodes(v, space))
            assert props["dropped"] and props["multi_tile"], (seed, space, props)
            assert props["edges"] or noise > 0.02, (seed, space, props)  # (the quiet scene keeps regions on all four edges; the shattered one need not)
            assert res["count"] >= 3 and (~np.isfinite(v)).sum() == 2
    quiet, loud = (sr.segment(sc.piecewise(s, h, w, n), min_area=1)["count"] for s, h, w, n in sc.RANDOM_SCENES)
    assert loud > 10 * quiet  # noise above the step shatters the levels


def test_cutout_restatement_follows_the_integer_node_rule():
    lab = np.array([[0, 1], [-1, 1]], np.int32)
    photo = np.random.default_rng(0).integers(1, 256, (5, 7, 3), dtype=np.uint8)
    bgra, mask = sr.cutout(lab, photo, {1})
    want = np.zeros((5, 7), bool)
    want[:, 4:] = True  # X w // W = 1 from X = 4 on (2 X // 7)
    assert np.array_equal(mask, want * np.uint8(255)) and np.array_equal(bgra[..., 3], mask) and np.array_equal(bgra[..., :3], photo * want[..., None])
    _, inv = sr.cutout(lab, photo, {1}, invert=True)
    assert np.array_equal(inv, 255 - mask)
    assert sr.picked(lab, [(0.0, 0.0), (1.0, 1.0), (0.0, 0.99)]) == {0, 1} and sr.picked(lab, [(0.2, 0.7)]) == set()
    assert sr.colors(lab)[1, 0].tolist() == [0, 0, 0] and sr.colors(lab).min(initial=255, where=(lab >= 0)[..., None]) >= 32


def test_python_arguments_are_checked_before_anything_runs():
    maps = [torch.zeros(1, 4, 5), torch.zeros(1, 3, 3)]
    for bad in (dict(space="linear"), dict(step=-0.1), dict(step=float("nan")), dict(step=float("inf")), dict(connectivity=6), dict(connectivity=True),
                dict(min_area=0), dict(min_area=1.5), dict(min_area=True), dict(min_area=2 ** 31)):
        with pytest.raises(ValueError, match="segment_depth"):
            segment.segment_depth(maps, **bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # there is no CPU implementation: host maps raise
        segment.segment_depth(maps)
    with pytest.raises(TypeError, match="DepthSegments"):
        segment.region_cutouts(object(), [])
    with pytest.raises(TypeError, match="DepthSegments"):
        segment.label_colors(None)
    seg = segment.DepthSegments([torch.zeros(4, 5, dtype=torch.int32)], *([None] * 9), [0], [1], 16)
    for kw in (dict(points=[[(0.5, 1.5)]]), dict(points=[[(0.5,)]]), dict(points=[[(0.1, 0.1)]], labels=[[0]]), dict(labels=[[1]]), dict(labels=[[-1]]),
               dict(labels=[[0.0]]), dict(points=[]), dict(labels=[[0], [0]])):
        with pytest.raises(ValueError, match="region_cutouts"):
            segment.region_cutouts(seg, [np.zeros((8, 9, 3), np.uint8)], **kw)
    assert "not a measured optimum" in segment.segment_depth.__doc__
    for word in ("grazing", "ramp", "dropped, not merged", "unverified"):
        assert word in segment.__doc__, word


def _records(sizes, min_area=16):
    rec = np.zeros(len(sizes), dtype=_common.SEGMENT_RECORD)
    at = regions = tiles = pixels = 0
    for k, (h, w) in enumerate(sizes):
        rec[k] = (4096, h, w, 8192, at, regions, tiles, pixels)  # (not device addresses: nothing may be launched with them)
        n = h * w
        at += (1024 + 4 * n + (n + 7) // 8 * 8 + (n + 255) // 256 * 4 + 7) // 8 * 8
        regions, tiles, pixels = regions + n // min_area, tiles + ((h + 31) // 32) * ((w + 31) // 32), pixels + n
    return rec, at


def test_entry_points_are_exported_and_refuse_bad_arguments_without_a_device():
    lib = native.load()
    names = ("mdpt_segment_scratch_bytes", "mdpt_segment_depth", "mdpt_segment_colors", "mdpt_segment_cutout")
    for name in names:
        assert name in native.SYMBOLS and hasattr(lib, name)
    assert {s for s in native.SYMBOLS if s.startswith("mdpt_segment_")} == set(names)
    assert "post_segment.inc" in native.HEADERS and "mdpt_segment.cpp" in native.SOURCES and native.SEGMENT_TILE == 32
    assert lib.mdpt_abi_version() == 6 == native.ABI_VERSION
    sizes = [(70, 33), (5, 9), (64, 64)]
    rec, total = _records(sizes)
    need = ctypes.c_size_t()
    assert lib.mdpt_segment_scratch_bytes(rec.ctypes.data, 3, ctypes.byref(need)) == 0 and need.value == total
    huge, _ = _records([(65536, 32768)])
    for args, word in (((None, 1), b"records_host"), ((rec.ctypes.data, 0), b"n ="), ((rec.ctypes.data, 65536), b"n ="), ((huge.ctypes.data, 1), b"2^31")):
        assert lib.mdpt_segment_scratch_bytes(*args, ctypes.byref(need)) != 0 and word in lib.mdpt_last_error(), args
    assert lib.mdpt_segment_scratch_bytes(rec.ctypes.data, 3, None) != 0 and b"bytes" in lib.mdpt_last_error()

    p, big = 4096, 1 << 30

    def depth(r=rec, dev=p, n=3, dtype=0, space=0, step=0.02, conn=4, min_area=16, scratch=p, nbytes=big, counts=p, area=p, bbox=p, first=p, vrange=p, sum_q=p, rng=p):
        return lib.mdpt_segment_depth(None if r is None else r.ctypes.data, dev, n, dtype, space, step, conn, min_area, scratch, nbytes, counts, area, bbox, first,
                                      vrange, sum_q, rng, None)

    def changed(field, k, value, base=rec):
        r = base.copy()
        r[field][k] = value
        return r

    for kw, word in ((dict(r=None), b"records_host"), (dict(dev=None), b"records_dev"), (dict(scratch=None), b"scratch"), (dict(counts=None), b"counts"),
                     (dict(sum_q=None), b"sum_q"), (dict(rng=None), b"range"), (dict(n=0), b"n ="), (dict(n=65536), b"n ="), (dict(dtype=7), b"dtype"),
                     (dict(space=2), b"space"), (dict(step=-0.5), b"step"), (dict(step=float("nan")), b"step"), (dict(step=float("inf")), b"step"),
                     (dict(conn=6), b"connectivity"), (dict(conn=0), b"connectivity"), (dict(min_area=0), b"min_area"), (dict(min_area=-3), b"min_area"),
                     (dict(r=changed("h", 1, 0)), b"size"), (dict(r=changed("w", 0, -2)), b"size"), (dict(r=huge, n=1), b"2^31"),
                     (dict(r=changed("map", 2, 0)), b"map"), (dict(r=changed("labels", 0, 0)), b"labels"), (dict(r=changed("labels", 0, 8194)), b"labels"),
                     (dict(r=changed("map", 1, 4098), dtype=0), b"misaligned map"), (dict(nbytes=total - 8), b"scratch"),
                     (dict(r=changed("scratch_off", 1, 0)), b"overlap"), (dict(r=changed("scratch_off", 1, 4)), b"scratch"),
                     (dict(r=changed("region_off", 2, 1)), b"region_off"), (dict(r=changed("tile_off", 1, 7)), b"tile_off"),
                     (dict(r=changed("pixel_off", 2, 0)), b"pixel_off"), (dict(min_area=1), b"region_off"),  # (the rows follow min_area)
                     (dict(scratch=4100), b"misaligned"), (dict(area=4098), b"misaligned"), (dict(sum_q=4100), b"misaligned")):
        assert depth(**kw) != 0, kw
        assert word in lib.mdpt_last_error(), (kw, lib.mdpt_last_error())

    for r, args, word in ((None, (p, 3, p), b"records_host"), (rec, (None, 3, p), b"records_dev"), (rec, (p, 3, None), b"colors"), (rec, (p, 0, p), b"n ="),
                          (changed("labels", 1, 0), (p, 3, p), b"labels"), (changed("pixel_off", 1, 3), (p, 3, p), b"pixel_off"),
                          (changed("h", 2, 0), (p, 3, p), b"size")):
        assert lib.mdpt_segment_colors(None if r is None else r.ctypes.data, *args, None) != 0 and word in lib.mdpt_last_error(), (args, lib.mdpt_last_error())

    ph = np.zeros(2, dtype=_common.SEGMENT_PHOTO_RECORD)
    ph[0] = (4096, 70, 33, 8192, 3 * 120, 90, 120, 12288, 16384, 0, 144, 0)
    ph[1] = (4096, 5, 9, 8192, 3 * 7, 4, 7, 12288, 16384, 144, 2, 0)

    def cut(r=ph, dev=p, n=2, picks=p, num=3, by_label=0, selected=p, nbytes=146, invert=0):
        return lib.mdpt_segment_cutout(None if r is None else r.ctypes.data, dev, n, picks, num, by_label, selected, nbytes, invert, None)

    for kw, word in ((dict(r=None), b"records_host"), (dict(dev=None), b"records_dev"), (dict(selected=None), b"selected"), (dict(n=0), b"n ="),
                     (dict(num=-1), b"num_picks"), (dict(picks=None), b"picks_dev"), (dict(picks=4098), b"misaligned"),
                     (dict(r=changed("labels", 0, 0, ph)), b"labels"), (dict(r=changed("photo", 1, 0, ph)), b"photo"), (dict(r=changed("mask", 1, 0, ph)), b"mask"),
                     (dict(r=changed("H", 0, 0, ph)), b"photo size"), (dict(r=changed("pitch", 0, 359, ph)), b"pitch"), (dict(r=changed("pitch", 1, 20, ph)), b"pitch"),
                     (dict(r=changed("bgra", 0, 12290, ph)), b"bgra"), (dict(nbytes=145), b"selected"), (dict(r=changed("regions", 0, -1, ph)), b"selected"),
                     (dict(r=changed("w", 0, 0, ph)), b"size")):
        assert cut(**kw) != 0, kw
        assert word in lib.mdpt_last_error(), (kw, lib.mdpt_last_error())


def test_the_record_tables_have_the_layout_of_their_structs():
    r = _common.SEGMENT_RECORD
    assert r.itemsize == 56
    assert {n: r.fields[n][1] for n in r.names} == {"map": 0, "h": 8, "w": 12, "labels": 16, "scratch_off": 24, "region_off": 32, "tile_off": 40, "pixel_off": 48}
    q = _common.SEGMENT_PHOTO_RECORD
    assert q.itemsize == 72
    assert {n: q.fields[n][1] for n in q.names} == {"labels": 0, "h": 8, "w": 12, "photo": 16, "pitch": 24, "H": 32, "W": 36, "bgra": 40, "mask": 48, "region_off": 56,
                                                    "regions": 64, "pad": 68}
    header = open(native.HEADERS[-1]).read()
    assert "typedef struct mdpt_segment_image { const void* map; int32_t h, w; void* labels; int64_t scratch_off, region_off, tile_off, pixel_off; }" in header
    assert ("typedef struct mdpt_segment_photo { const void* labels; int32_t h, w; const void* photo; int64_t pitch; int32_t H, W; void* bgra; void* mask; "
            "int64_t region_off; int32_t regions, pad; }") in header
    assert "#define MDPT_SEGMENT_TILE 32" in header and "#define MDPT_ABI_VERSION 6" in header
    import muggled_dpt_amd.postprocess as package  # the new records stay out of the recorded package surface
    assert not hasattr(package, "SEGMENT_RECORD") and "SEGMENT_RECORD" not in getattr(_common, "__all__", ())


def test_scratch_bytes_grow_with_the_pixel_count():
    lib, need, last = native.load(), ctypes.c_size_t(), 0
    for h, w in ((1, 1), (7, 9), (32, 32), (33, 65), (504, 504), (1024, 2048)):
        rec, total = _records([(h, w)])
        assert lib.mdpt_segment_scratch_bytes(rec.ctypes.data, 1, ctypes.byref(need)) == 0
        assert need.value == total > last and need.value % 8 == 0 and need.value >= 1024 + 5 * h * w
        last = need.value
    rec, total = _records([(7, 9), (33, 65)])
    assert lib.mdpt_segment_scratch_bytes(rec.ctypes.data, 2, ctypes.byref(need)) == 0 and need.value == total
