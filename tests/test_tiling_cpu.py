"""Tiled high-resolution inference without a GPU: the tile layouts of muggled_dpt_amd.tiling (boxes inside the image, full cover, the promised
overlap, the counts the rule predicts), properties of the fp64 restatement tests/tile_restate.py that the GPU tests measure the kernels against,
and the argument checks of postprocess.stitch_tiles / the C entry points, which raise before anything touches a device."""
import ctypes
import math

import numpy as np
import pytest
import torch

from muggled_dpt_amd import native, tiling
from muggled_dpt_amd import postprocess as pp
from tests import tile_restate as tr

LAYOUTS = [((61, 47), (40, 32), 5), ((97, 83), (24, 24), 6), ((3024, 4032), (1008, 1008), 252), ((100, 100), (30, 45), (0, 7)), ((17, 1), (4, 4), 1),
           ((50, 60), (50, 20), 3)]


def _cover(boxes, hw):
    c = np.zeros(hw, dtype=np.int32)
    for x1, y1, x2, y2 in boxes:
        c[y1:y2, x1:x2] += 1
    return c


def _axis_overlaps(boxes):
    xs = sorted({(b[0], b[2]) for b in boxes})
    ys = sorted({(b[1], b[3]) for b in boxes})
    return [a[1] - b[0] for a, b in zip(ys, ys[1:])], [a[1] - b[0] for a, b in zip(xs, xs[1:])]


@pytest.mark.parametrize("hw,tile,ov", LAYOUTS)
def test_tile_boxes_lie_inside_cover_every_pixel_and_overlap_enough(hw, tile, ov):
    boxes = tiling.tile_boxes(hw, tile, ov)
    oy, ox = ov if isinstance(ov, tuple) else (ov, ov)
    assert all(0 <= x1 < x2 <= hw[1] and 0 <= y1 < y2 <= hw[0] for x1, y1, x2, y2 in boxes)
    assert len({(x2 - x1, y2 - y1) for x1, y1, x2, y2 in boxes}) == 1
    assert _cover(boxes, hw).min() >= 1
    got_y, got_x = _axis_overlaps(boxes)
    assert all(o >= oy for o in got_y) and all(o >= ox for o in got_x)
    assert boxes[0][:2] == (0, 0) and boxes[-1][2:] == (hw[1], hw[0])
    assert boxes == sorted(boxes, key=lambda b: (b[1], b[0]))  # row by row, left to right


def test_tile_counts_follow_the_rule():
    # n = ceil((L - ov) / (tile - ov)): (3024 - 252) / 756 = 3.67 -> 4 rows, (4032 - 252) / 756 = 5 -> 5 columns
    boxes = tiling.tile_boxes((3024, 4032), 1008, 252)
    assert len(boxes) == 20 and len({b[1] for b in boxes}) == 4 and len({b[0] for b in boxes}) == 5
    assert sorted({b[0] for b in boxes}) == [0, 756, 1512, 2268, 3024]  # exact fit: every overlap is 252
    assert sorted({b[1] for b in boxes}) == [0, 672, 1344, 2016]  # round(i 2016 / 3)
    for length, tile, ov in ((100, 30, 5), (101, 30, 5), (55, 30, 29), (31, 30, 0), (1000, 7, 3)):
        side, starts = tiling.axis_starts(length, tile, ov)
        assert side == tile and len(starts) == math.ceil((length - ov) / (tile - ov))
        assert starts[0] == 0 and starts[-1] == length - tile and all(b - a <= tile - ov for a, b in zip(starts, starts[1:]))
    assert tiling.axis_starts(101, 30, 5)[1] == [round(i * 71 / 3) for i in range(4)]


def test_a_tile_as_large_as_the_image_and_a_one_by_one_grid_give_the_whole_image():
    assert tiling.tile_boxes((61, 47), (61, 47), 5) == [(0, 0, 47, 61)]
    assert tiling.tile_boxes((61, 47), (100, 200), 99) == [(0, 0, 47, 61)]
    assert tiling.tile_boxes((61, 47), (100, 20), 4)[0] == (0, 0, 20, 61)  # one axis covered, the other tiled
    assert tiling.tile_grid_boxes((61, 47), (1, 1), 0.25) == [(0, 0, 47, 61)]
    assert tiling.tile_grid_boxes((61, 47), (1, 1), 0.0) == [(0, 0, 47, 61)]


@pytest.mark.parametrize("hw,grid,frac", [((61, 47), (2, 2), 0.25), ((97, 83), (5, 4), 0.3), ((3024, 4032), (4, 3), 0.25), ((3024, 4032), (8, 6), 0.25),
                                          ((120, 150), (2, 2), 0.0), ((9, 9), (9, 9), 0.0), ((50, 7), (3, 1), 0.5)])
def test_tile_grid_boxes(hw, grid, frac):
    boxes = tiling.tile_grid_boxes(hw, grid, frac)
    assert len(boxes) == grid[0] * grid[1] and len({b[1] for b in boxes}) == grid[0] and len({b[0] for b in boxes}) == grid[1]
    assert all(0 <= x1 < x2 <= hw[1] and 0 <= y1 < y2 <= hw[0] for x1, y1, x2, y2 in boxes)
    assert _cover(boxes, hw).min() >= 1
    th, tw = boxes[0][3] - boxes[0][1], boxes[0][2] - boxes[0][0]
    got_y, got_x = _axis_overlaps(boxes)
    # the side is ceil(L / (n - (n - 1) f)), so neighbours share f of a side up to the rounding of the side and of the starts: one pixel each
    assert all(o >= frac * th - 2 for o in got_y) and all(o >= frac * tw - 2 for o in got_x)
    assert tiling.smallest_overlap(boxes) == min(got_y + got_x, default=0)  # stitch_tiles' default feather


def test_smallest_overlap_looks_at_neighbours_only():
    # overlaps above half a side: tiles two apart still intersect, and their thin intersection must not become the default feather
    boxes = tiling.tile_boxes((40, 100), (40, 40), 30)  # one row; starts 0, 10, ..., 60: neighbours share 30, tiles two apart 20, three apart 10
    assert [b[0] for b in boxes] == [0, 10, 20, 30, 40, 50, 60] and tiling.smallest_overlap(boxes) == 30
    grid = tiling.tile_grid_boxes((90, 120), (4, 5), 0.7)
    got_y, got_x = _axis_overlaps(grid)
    assert min(got_y + got_x) > 0.5 * min(grid[0][3], grid[0][2]) and tiling.smallest_overlap(grid) == min(got_y + got_x)
    assert tiling.smallest_overlap([(0, 0, 10, 10)]) == 0 and tiling.smallest_overlap([(0, 0, 10, 10), (10, 0, 20, 10)]) == 0
    assert tiling.smallest_overlap([(0, 0, 10, 10), (7, 0, 20, 10), (0, 6, 10, 20)]) == 3  # x neighbours share 3 columns, y neighbours 4 rows


def test_layout_arguments_are_checked():
    for bad in (lambda: tiling.tile_boxes((10, 10), 4, 4), lambda: tiling.tile_boxes((10, 10), 0, 0), lambda: tiling.tile_boxes((0, 10), 4, 1),
                lambda: tiling.tile_boxes((10, 10), 4, -1), lambda: tiling.tile_grid_boxes((10, 10), (0, 1)), lambda: tiling.tile_grid_boxes((10, 10), (11, 1)),
                lambda: tiling.tile_grid_boxes((10, 10), (2, 2), 1.0), lambda: tiling.tile_boxes((10, 10, 3), 4, 1)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(TypeError):
        tiling.tile_boxes((10, 10), 4.5, 1)


# ---- the restatement itself

def _grid_case(hw=(61, 47), tile=(40, 32), ov=5, map_hw=((16, 12), (9, 21)), seed=0):
    boxes = tiling.tile_boxes(hw, tile, ov)
    rng = np.random.default_rng(seed)
    maps = [rng.uniform(1.0, 2.0, map_hw[k % len(map_hw)]).astype(np.float32) for k in range(len(boxes))]
    return boxes, maps


def test_restatement_constant_tiles_blend_to_the_constant():
    boxes, maps = _grid_case()
    for c in (0.0, 1.0, -3.25, 1e-3, float(np.float32(0.1))):
        out = tr.blend([np.full_like(m, c) for m in maps], boxes, (61, 47), feather=9.0).astype(np.float32)
        assert out.shape == (61, 47) and np.all(out == np.float32(c))
    # 8 -> 24 pixels: source positions in the first interval carry bits below 2^-24, where cv2's fp32 weights 1 - a and a do not sum to 1 and a
    # power of two would come out one ulp low (mask_restate.resize_f64 shows it); equal taps give that tap (resize_tile)
    from tests.mask_restate import resize_f64
    boxes20, maps20 = _grid_case((97, 83), 24, 4, ((8, 8), (7, 9)))
    for c in (1.0, 0.25, -3.25, 1e-30):
        out = tr.blend([np.full_like(m, c) for m in maps20], boxes20, (97, 83), feather=4.0).astype(np.float32)
        assert np.all(out == np.float32(c))
    assert (resize_f64(np.ones((8, 8)), (24, 24)).astype(np.float32) != 1).any()
    x = np.random.default_rng(2).uniform(-2, 2, (7, 9))
    assert np.array_equal(tr.resize_tile(x, (24, 24)), resize_f64(x, (24, 24)))  # no equal taps: cv2's rule unchanged
    # a hole in the cover is NaN, everything else still the constant
    out = tr.blend([np.full_like(m, 2.5) for m in maps[:3]], boxes[:3], (61, 47), feather=3.0)
    covered = _cover(boxes[:3], (61, 47)) > 0
    assert np.isnan(out[~covered]).all() and (~covered).any() and np.all(out[covered].astype(np.float32) == 2.5)


def test_restatement_weights_are_symmetric_under_flipping_the_photo():
    hw = (61, 47)
    boxes, maps = _grid_case()
    H, W = hw
    for feather in (0.0, 4.0, 11.5):
        out = tr.blend(maps, boxes, hw, feather=feather)
        # the same scene mirrored: boxes mirrored in both axes, maps flipped; the tile order changes nothing beyond the last bits of the sums
        fboxes = [(W - x2, H - y2, W - x1, H - y1) for x1, y1, x2, y2 in boxes]
        fout = tr.blend([m[::-1, ::-1] for m in maps], fboxes, hw, feather=feather)
        for (x1, y1, x2, y2), (fx1, fy1, fx2, fy2) in zip(boxes, fboxes):
            assert np.array_equal(tr.axis_weights(x1, x2, W, feather), tr.axis_weights(fx1, fx2, W, feather)[::-1])
            assert np.array_equal(tr.axis_weights(y1, y2, H, feather), tr.axis_weights(fy1, fy2, H, feather)[::-1])
        # cv2's tap positions are fp32 roundings of mirrored positions: equal up to that rounding, far below the maps' own step
        assert np.allclose(out, fout[::-1, ::-1], rtol=0, atol=1e-5)
    w = tr.axis_weights(10, 30, 100, 4.0)
    assert w[0] == 0.2 and w[4] == 1.0 and w[-1] == 0.2 and np.array_equal(w, w[::-1])
    assert np.all(tr.axis_weights(0, 30, 30, 4.0) == 1.0)  # both edges on the photo's border: no ramp
    assert tr.axis_weights(0, 30, 100, 4.0)[0] == 1.0 and tr.axis_weights(0, 30, 100, 4.0)[-1] == 0.2


def test_restatement_fit_recovers_an_exact_affine_relation_and_flags_degenerate_tiles():
    hw = (61, 47)
    boxes, maps = _grid_case()
    guide = np.random.default_rng(3).uniform(0.5, 4.0, (13, 10))
    for t, (m, b) in enumerate(zip(maps, boxes)):
        y = tr.guide_samples(guide, b, m.shape, hw)
        x = ((y - 2.5) / 0.37)  # the tile whose samples satisfy y = 0.37 x + 2.5 exactly (up to rounding)
        (s, sh), sums, _ = (v[0] for v in tr.fit([x], [b], guide, hw))
        assert abs(s - 0.37) < 1e-9 and abs(sh - 2.5) < 1e-9 and sums[0] == m.size
    flat = tr.fit([np.full((16, 12), 1.5)], [boxes[0]], guide, hw)
    assert flat[0][0, 0] == 0.0 and flat[0][0, 1] == flat[1][0, 2] / flat[1][0, 0]
    y = tr.guide_samples(guide, boxes[1], (9, 21), hw)
    neg = tr.fit([-y], [boxes[1]], guide, hw)
    assert neg[0][0, 0] == 0.0 and neg[0][0, 1] == neg[1][0, 2] / neg[1][0, 0]
    empty = tr.fit([np.full((9, 21), np.nan)], [boxes[1]], guide, hw)
    assert np.all(empty[0] == 0.0) and empty[1][0, 0] == 0
    one = np.full((9, 21), np.nan)
    one[4, 4] = 1.0
    single = tr.fit([one], [boxes[1]], guide, hw)
    assert single[1][0, 0] == 1 and single[0][0, 0] == 0.0 and single[0][0, 1] == y[4, 4]
    x = np.random.default_rng(4).uniform(1, 2, (16, 12))
    holed = x.copy()
    holed[3, 5] = np.nan
    assert tr.fit([holed], [boxes[0]], guide, hw)[1][0, 0] == x.size - 1


# ---- argument checks: nothing below reaches a device

def test_stitch_tiles_checks_its_arguments_before_touching_a_device():
    m = [torch.zeros(1, 4, 4), torch.zeros(1, 4, 4)]
    boxes = [(0, 0, 8, 8), (4, 0, 12, 8)]
    guide = torch.zeros(1, 4, 4)
    with pytest.raises(ValueError, match="guide"):
        pp.stitch_tiles(m, boxes, (8, 12))
    with pytest.raises(ValueError, match="align"):
        pp.stitch_tiles(m, boxes, (8, 12), guide, align="scale")
    with pytest.raises(ValueError, match="outside"):
        pp.stitch_tiles(m, [(0, 0, 8, 8), (4, 0, 13, 8)], (8, 12), guide)
    with pytest.raises(ValueError, match="outside"):
        pp.stitch_tiles(m, [(0, 0, 8, 8), (4, 3, 12, 3)], (8, 12), guide)
    with pytest.raises(ValueError, match="outside"):
        pp.stitch_tiles(m, [(-1, 0, 8, 8), (4, 0, 12, 8)], (8, 12), align="none")
    with pytest.raises(TypeError, match="four ints"):
        pp.stitch_tiles(m, [(0, 0, 8, 8), (4.0, 0, 12, 8)], (8, 12), guide)
    with pytest.raises(ValueError, match="2 tile maps but 1 boxes"):
        pp.stitch_tiles(m, boxes[:1], (8, 12), guide)
    with pytest.raises(ValueError, match="photo size"):
        pp.stitch_tiles(m, boxes, (0, 12), guide)
    with pytest.raises(ValueError, match="feather"):
        pp.stitch_tiles(m, boxes, (8, 12), guide, feather=-1)
    with pytest.raises(ValueError, match="feather"):
        pp.stitch_tiles(m, boxes, (8, 12), guide, feather=float("nan"))
    with pytest.raises(ValueError, match="non-empty"):
        pp.stitch_tiles([], [], (8, 12), guide)
    with pytest.raises(RuntimeError, match="CUDA"):  # host tensors: there is no CPU implementation
        pp.stitch_tiles(m, boxes, (8, 12), guide)
    with pytest.raises(RuntimeError, match="CUDA"):
        pp.stitch_tiles(m, boxes, (8, 12), align="none")


def _table(rows):
    t = np.zeros(len(rows), dtype=pp._TILE_RECORD)
    for k, r in enumerate(rows):
        t[k] = r
    return t


def test_c_entry_points_check_on_the_host_and_launch_nothing():
    """Pointers are plain numbers here: a call that got past its checks would fault, so every call must return its error first."""
    lib = native.load()
    A = 0x10000  # an aligned, non-null address that is never read
    good = _table([(A, 16, 12, 0, 0, 32, 40), (A + 4096, 9, 21, 15, 21, 47, 61)])
    need = ctypes.c_size_t()
    assert lib.mdpt_post_tile_scratch_bytes(good.ctypes.data, 2, ctypes.byref(need)) == 0
    assert need.value == 2 * 1 * 6 * 8  # one chunk of 2048 samples covers both maps
    big = _table([(A, 504, 504, 0, 0, 32, 40)])
    assert lib.mdpt_post_tile_scratch_bytes(big.ctypes.data, 1, ctypes.byref(need)) == 0 and need.value == math.ceil(504 * 504 / 2048) * 48

    def fit_rc(table, T=None, dt=native.DTYPE_F32, guide=A, gdt=native.DTYPE_F32, ghw=(13, 10), hw=(61, 47), fit=A, sums=A, scratch=A, nbytes=1 << 20, tdev=A):
        return lib.mdpt_post_tile_fit(table.ctypes.data, tdev, len(table) if T is None else T, dt, guide, gdt, ghw[0], ghw[1], hw[0], hw[1], fit, sums, scratch,
                                      nbytes, None)

    def blend_rc(table, T=None, dt=native.DTYPE_F32, hw=(61, 47), fit=A, sums=A, feather=3.0, out=A, tdev=A):
        return lib.mdpt_post_tile_blend(table.ctypes.data, tdev, len(table) if T is None else T, dt, hw[0], hw[1], fit, sums, feather, out, None)

    bad_tables = {
        "outside": _table([(A, 16, 12, 0, 0, 48, 40)]), "below": _table([(A, 16, 12, 0, 22, 32, 62)]), "negative": _table([(A, 16, 12, -1, 0, 32, 40)]),
        "empty box": _table([(A, 16, 12, 5, 0, 5, 40)]), "map size": _table([(A, 0, 12, 0, 0, 32, 40)]), "null or misaligned": _table([(0, 16, 12, 0, 0, 32, 40)]),
    }
    for word, table in bad_tables.items():
        for rc in (fit_rc(table), blend_rc(table)):
            assert rc == -1 and lib.mdpt_last_error(), word
    assert fit_rc(_table([(A + 2, 16, 12, 0, 0, 32, 40)])) == -1 and b"misaligned" in lib.mdpt_last_error()  # an fp32 map at a 2-byte address
    for kw in (dict(T=0), dict(T=70000), dict(dt=7), dict(gdt=7), dict(guide=0), dict(guide=A + 2), dict(ghw=(0, 10)), dict(hw=(61, 0)), dict(fit=0), dict(fit=A + 4),
               dict(sums=A + 4), dict(scratch=A + 4), dict(scratch=0), dict(nbytes=95), dict(tdev=0), dict(tdev=A + 4)):
        assert fit_rc(good, **kw) == -1, kw
        assert lib.mdpt_last_error()
    for kw in (dict(T=0), dict(dt=7), dict(hw=(0, 47)), dict(fit=A + 4), dict(sums=A + 4), dict(feather=-1.0), dict(feather=float("nan")), dict(feather=float("inf")),
               dict(out=0), dict(out=A + 2), dict(tdev=0), dict(tdev=A + 4)):
        assert blend_rc(good, **kw) == -1, kw
    assert lib.mdpt_post_tile_scratch_bytes(None, 2, ctypes.byref(need)) == -1 and lib.mdpt_post_tile_scratch_bytes(good.ctypes.data, 2, None) == -1
