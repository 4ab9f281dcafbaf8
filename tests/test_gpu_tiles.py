"""postprocess.stitch_tiles (mdpt_post_tile_fit / mdpt_post_tile_blend) against the fp64 restatement tests/tile_restate.py.

Inputs of the fit: the guide is 0.37 u + 2.5 with u uniform in [1, 2]; a tile sample is x = (y - 2.5 - e) / 0.37 rounded to the tile dtype, y the guide
at the sample (the restatement's sampling, used here only to BUILD inputs) and e ~ N(0, 0.05) - so y = 0.37 x + 2.5 + e, x in about [1, 2], and the
cancellation in var = n Sxx - Sx^2 is about 28 x.
Bounds: sums against math.fsum's within n 2^-52 sum|terms|, the worst case of ANY summation order; the fit within 1e-9 relative (random reorderings
of the fp64 sums moved s and t by at most 1.1e-12 on a CPU over 200 trials with n <= 4096); the blended map within one fp32 ulp of float32(the
restatement) - the device computes in fp64 and rounds once, one ulp covers a last-bit difference of the fp64 value at a rounding tie. The blend is
judged twice: with the restatement fed the device's own fit (only the blend is judged) and with the restatement's own fit (then the maps may differ
by fit error x the map's range, about 1e-9 x 3, far below an ulp of 1.2e-7 x 3: still one ulp, at ties only)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from muggled_dpt_amd import native, tiling
from muggled_dpt_amd import postprocess as pp
from tests import tile_restate as tr
from tests.mask_restate import resize_f64

pytestmark = pytest.mark.gpu

DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


def _round(x: np.ndarray, dtype) -> np.ndarray:
    """the values as the dtype stores them, as float32"""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dtype).float().numpy()


def _random_boxes(rng, hw, n, lo, hi):
    out = []
    for _ in range(n):
        bw, bh = int(rng.integers(lo, hi + 1)), int(rng.integers(lo, hi + 1))
        x1, y1 = int(rng.integers(0, hw[1] - bw + 1)), int(rng.integers(0, hw[0] - bh + 1))
        out.append((x1, y1, x1 + bw, y1 + bh))
    return out


# name -> (photo (H, W), boxes, the tile maps' sizes in turn, guide size, feather or None for the default)
LAYOUTS = {
    # 2 x 2 grid of 40 x 32 tiles, maps of two sizes in one call; W = 47 is no multiple of the 4 pixels a thread writes
    "grid2x2": ((61, 47), tiling.tile_boxes((61, 47), (40, 32), 5), ((16, 12), (9, 21)), (13, 10), None),
    # 5 x 4 grid of 24 x 24 tiles on 97 x 83: 1, 2 and 4 tiles per pixel, 64 x 16 workgroup blocks straddle tile edges
    "grid5x4": ((97, 83), tiling.tile_boxes((97, 83), 24, 4), ((8, 8), (7, 9)), (13, 10), None),
    # the whole photo, a 1-pixel-wide tile, a 1-pixel-high tile, a box at odd offsets; a fractional feather
    "odd": ((33, 50), [(0, 0, 50, 33), (17, 5, 18, 30), (3, 11, 44, 12), (3, 7, 38, 29), (41, 1, 50, 33)], ((11, 13), (6, 1), (1, 9), (5, 7)), (7, 9), 2.5),
    # 300 random boxes (the cull walks the table in two passes of 256, holes stay NaN) and one map of 50 x 47 > 2048 samples (two fit chunks)
    "many": ((40, 70), [(2, 1, 69, 38)] + _random_boxes(np.random.default_rng(5), (40, 70), 299, 14, 30), ((50, 47), (6, 7), (7, 6), (5, 5)), (13, 10), 3.0),
}
assert len(LAYOUTS["grid5x4"][1]) == 20 and len(LAYOUTS["grid2x2"][1]) == 4


@functools.lru_cache(maxsize=None)
def _case(layout: str, dt: str, seed: int = 0):
    """-> dict(hw, boxes, feather, maps / guide: float32 arrays holding values of the dtype, ref: the restatement's (fit, sums, abs_terms))"""
    hw, boxes, sizes, ghw, feather = LAYOUTS[layout]
    dtype = DTYPES[dt]
    rng = np.random.default_rng(seed)
    guide = _round(0.37 * rng.uniform(1.0, 2.0, ghw) + 2.5, dtype)
    maps = []
    for k, b in enumerate(boxes):
        mh, mw = sizes[k % len(sizes)]
        y = tr.guide_samples(guide, b, (mh, mw), hw)
        maps.append(_round((y - 2.5 - rng.normal(0.0, 0.05, (mh, mw))) / 0.37, dtype))
    feather = float(tiling.smallest_overlap(boxes)) if feather is None else feather
    case = dict(hw=hw, boxes=boxes, feather=feather, maps=maps, guide=guide, dtype=dtype)
    case["ref"] = tr.fit(maps, boxes, guide, hw)
    for v in maps + [guide]:
        v.setflags(write=False)
    return case


def _dev(arrays, dtype):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()[None] for a in arrays]


def _stitch(case, maps=None, guide="case", align="affine", **kw):
    maps = case["maps"] if maps is None else maps
    g = None
    if align == "affine":
        g = _dev([case["guide"] if isinstance(guide, str) else guide], case["dtype"])[0]
    out = pp.stitch_tiles(_dev(maps, case["dtype"]), case["boxes"], case["hw"], guide=g, align=align, feather=case["feather"], return_fit=True, **kw)
    return out[0][0].cpu().numpy(), None if out[1] is None else out[1].cpu().numpy(), None if out[2] is None else out[2].cpu().numpy()


_ulps = tr.ulps


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_fit_and_blend_against_the_restatement(layout, dt):
    case = _case(layout, dt)
    out, fit, sums = _stitch(case)
    ref_fit, ref_sums, abs_terms = case["ref"]
    assert out.shape == case["hw"] and fit.shape == ref_fit.shape and sums.shape == ref_sums.shape
    # sums: the worst-case bound of any summation order
    n = ref_sums[:, :1]
    assert np.array_equal(sums[:, 0], ref_sums[:, 0])
    err, bound = np.abs(sums - ref_sums), n * 2.0 ** -52 * abs_terms
    print(f"{layout} {dt}: sums err / bound max {np.max(err / np.maximum(bound, 1e-300)):.3g}")
    assert np.all(err <= bound)
    rel = np.abs(fit - ref_fit) / np.abs(ref_fit)
    print(f"{layout} {dt}: fit rel err max {rel.max():.3g}, s in [{ref_fit[:, 0].min():.3f}, {ref_fit[:, 0].max():.3f}]")
    assert np.all(ref_fit[:, 0] > 0) and np.all(rel <= 1e-9)
    # the blend alone: the restatement fed the device's fit
    want = tr.blend(case["maps"], case["boxes"], case["hw"], fit, sums[:, 0] == 0, case["feather"]).astype(np.float32)
    d = _ulps(out, want)
    print(f"{layout} {dt}: blend vs restatement (device fit) {d} ulp")
    assert d <= 1
    # ... and end to end, with the restatement's own fit
    want = tr.blend(case["maps"], case["boxes"], case["hw"], ref_fit, ref_sums[:, 0] == 0, case["feather"]).astype(np.float32)
    d = _ulps(out, want)
    print(f"{layout} {dt}: blend vs restatement (own fit) {d} ulp")
    assert d <= 1
    if layout != "many":  # (its random boxes leave holes, which are NaN on both sides)
        assert np.isfinite(out).all() and 2.0 < out.min() and out.max() < 4.0


@pytest.mark.parametrize("dt", list(DTYPES))
def test_one_tile_that_is_the_whole_photo_is_the_cv2_resize(dt):
    rng = np.random.default_rng(1)
    for hw, mhw in (((61, 47), (16, 12)), ((33, 50), (40, 77)), ((5, 3), (5, 3)), ((64, 128), (9, 21))):
        m = _round(rng.uniform(-2.0, 2.0, mhw), DTYPES[dt])
        case = dict(hw=hw, boxes=[(0, 0, hw[1], hw[0])], feather=7.0, maps=[m], dtype=DTYPES[dt])
        out, fit, sums = _stitch(case, align="none")
        assert fit is None and sums is None
        want = resize_f64(m.astype(np.float64), (hw[1], hw[0])).astype(np.float32)  # cv2's rule as the depth masking tests state it
        assert _ulps(out, want) <= 1
        assert np.array_equal(out, tr.resize_tile(m.astype(np.float64), (hw[1], hw[0])).astype(np.float32))
        if hw == mhw:
            assert np.array_equal(out, m)


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_constant_tiles_blend_to_exactly_the_constant(layout):
    case = dict(_case(layout, "fp32"))
    cover = np.zeros(case["hw"], dtype=bool)
    for x1, y1, x2, y2 in case["boxes"]:
        cover[y1:y2, x1:x2] = True
    for c in (1.0, 0.25, -3.25, float(np.float32(0.1)), 1e-30):
        out, _, _ = _stitch(case, maps=[np.full_like(m, c) for m in case["maps"]], align="none")
        assert np.all(out[cover] == np.float32(c)) and np.isnan(out[~cover]).all()


@pytest.mark.parametrize("layout", ["grid2x2", "grid5x4", "odd"])
def test_affine_aligned_output_does_not_depend_on_each_tiles_own_scale_and_shift(layout):
    """m_t -> a_t m_t + b_t with a_t in {0.5, 2, 4} and small integer b_t, exact in fp32 (the maps are multiples of 2^-12 here): the fit absorbs it"""
    case = dict(_case(layout, "fp32"))
    case["maps"] = [np.round(m * 4096.0) / 4096.0 for m in case["maps"]]
    base, fit0, _ = _stitch(case)
    rng = np.random.default_rng(9)
    a = rng.choice([0.5, 2.0, 4.0], len(case["maps"]))
    b = rng.integers(-3, 4, len(case["maps"])).astype(np.float64)
    moved = [(ak * m.astype(np.float64) + bk).astype(np.float32) for m, ak, bk in zip(case["maps"], a, b)]
    assert all(np.array_equal(mv.astype(np.float64), ak * m.astype(np.float64) + bk) for mv, m, ak, bk in zip(moved, case["maps"], a, b))
    out, fit1, _ = _stitch(case, maps=moved)
    assert np.allclose(fit1[:, 0] * a, fit0[:, 0], rtol=1e-9, atol=0)
    assert _ulps(out, base) <= 1


def test_flat_negative_empty_and_holed_tiles():
    case = dict(_case("grid2x2", "fp32"))
    maps = [m.copy() for m in case["maps"]]
    boxes, hw = case["boxes"], case["hw"]
    maps[0][...] = 1.5                                                       # flat: takes the guide's mean over its box
    maps[1] = (-tr.guide_samples(case["guide"], boxes[1], maps[1].shape, hw)).astype(np.float32)  # negatively correlated with the guide: degenerate
    maps[2][...] = np.nan                                                     # all NaN: empty
    maps[3][4, 7] = np.nan                                                    # one NaN sample: skipped by the fit, propagates where its taps reach
    out, fit, sums = _stitch(case, maps=maps)
    ref_fit, ref_sums, abs_terms = tr.fit(maps, boxes, case["guide"], hw)
    assert np.all(np.abs(sums - ref_sums) <= ref_sums[:, :1] * 2.0 ** -52 * abs_terms)
    assert list(sums[:, 0]) == [16 * 12, 9 * 21, 0, 9 * 21 - 1]
    for t in (0, 1):
        assert fit[t, 0] == 0.0 and fit[t, 1] == sums[t, 2] / sums[t, 0] and ref_fit[t, 0] == 0.0
        assert 2.8 < fit[t, 1] < 3.3
    assert fit[2, 0] == 0.0 and fit[2, 1] == 0.0 and np.all(sums[2] == 0.0)
    assert fit[3, 0] > 0 and abs(fit[3, 0] - ref_fit[3, 0]) <= 1e-9 * ref_fit[3, 0]
    want = tr.blend(maps, boxes, hw, fit, sums[:, 0] == 0, case["feather"]).astype(np.float32)
    assert _ulps(out, want) <= 1  # (NaNs at the same pixels)
    x1, y1, x2, y2 = boxes[2]
    alone = np.ones(hw, dtype=bool)
    for k in (0, 1, 3):
        alone[boxes[k][1]:boxes[k][3], boxes[k][0]:boxes[k][2]] = False
    assert alone[y1:y2, x1:x2].any() and np.isnan(out[alone]).all()  # the pixels only the empty tile covers
    holes = np.isnan(out) & ~alone
    bx1, by1, bx2, by2 = boxes[3]
    assert 0 < holes.sum() < (bx2 - bx1) * (by2 - by1) // 4 and not holes[:by1].any() and not holes[:, :bx1].any()
    # a flat tile's pixels that no other tile shares hold the guide's mean over its box
    x1, y1, x2, y2 = boxes[0]
    assert out[y1, x1] == np.float32(fit[0, 1])


def test_two_calls_and_another_stream_give_identical_bits():
    case = _case("grid5x4", "bf16")
    maps, guide = _dev(case["maps"], case["dtype"]), _dev([case["guide"]], case["dtype"])[0]
    first = pp.stitch_tiles(maps, case["boxes"], case["hw"], guide=guide, return_fit=True)
    second = pp.stitch_tiles(maps, case["boxes"], case["hw"], guide=guide, return_fit=True)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        others = [m.clone() for m in maps]  # the same values at other addresses
        third = pp.stitch_tiles(others, case["boxes"], case["hw"], guide=guide.clone(), return_fit=True)
    side.synchronize()
    for a, b, c in zip(first, second, third):
        assert torch.equal(a.view(torch.int32 if a.dtype == torch.float32 else torch.int64), b.view(torch.int32 if b.dtype == torch.float32 else torch.int64))
        assert torch.equal(a.view(torch.int32 if a.dtype == torch.float32 else torch.int64), c.view(torch.int32 if c.dtype == torch.float32 else torch.int64))
    assert first[0].shape == (1, *case["hw"]) and first[0].dtype == torch.float32 and first[1].dtype == torch.float64


def test_default_feather_is_the_smallest_overlap_and_maps_may_be_2d():
    case = _case("grid2x2", "fp16")
    assert case["feather"] == 17.0  # tile_boxes((61, 47), (40, 32), 5): the rows overlap by 19, the columns by 17
    maps, guide = _dev(case["maps"], case["dtype"]), _dev([case["guide"]], case["dtype"])[0]
    a = pp.stitch_tiles(maps, case["boxes"], case["hw"], guide=guide)
    b = pp.stitch_tiles([m[0] for m in maps], case["boxes"], case["hw"], guide=guide[0], feather=case["feather"])
    assert torch.equal(a, b)


def test_bad_arguments_return_errors_and_launch_nothing():
    case = _case("grid2x2", "fp32")
    maps, guide = _dev(case["maps"], case["dtype"]), _dev([case["guide"]], case["dtype"])[0]
    H, W = case["hw"]
    with pytest.raises(ValueError, match="guide"):
        pp.stitch_tiles(maps, case["boxes"], case["hw"])
    with pytest.raises(ValueError, match="outside"):
        pp.stitch_tiles(maps, [(0, 0, W + 1, 40)] + case["boxes"][1:], case["hw"], guide=guide)
    with pytest.raises(RuntimeError, match="one device and one dtype"):
        pp.stitch_tiles([maps[0].half()] + maps[1:], case["boxes"], case["hw"], guide=guide)
    # the C entry points themselves, on real buffers: a box outside the photo is refused and the outputs keep their bytes
    lib = native.load()
    records = np.zeros(len(maps), dtype=pp._TILE_RECORD)
    records["map"] = [m.data_ptr() for m in maps]
    records["h"], records["w"] = [m.shape[1] for m in maps], [m.shape[2] for m in maps]
    for k, name in enumerate(("x1", "y1", "x2", "y2")):
        records[name] = [b[k] for b in case["boxes"]]
    records["x2"][3] = W + 1
    table = torch.from_numpy(records.view(np.uint8).reshape(-1).copy()).cuda()
    out = torch.full((H, W), 7.0, device="cuda")
    fit = torch.full((4, 2), 7.0, device="cuda", dtype=torch.float64)
    sums = torch.full((4, 6), 7.0, device="cuda", dtype=torch.float64)
    scratch = torch.zeros(4 * 6, device="cuda", dtype=torch.float64)
    stream = torch.cuda.current_stream().cuda_stream
    rc = lib.mdpt_post_tile_fit(records.ctypes.data, table.data_ptr(), 4, native.DTYPE_F32, guide.data_ptr(), native.DTYPE_F32, 13, 10, H, W, fit.data_ptr(),
                                sums.data_ptr(), scratch.data_ptr(), scratch.numel() * 8, stream)
    assert rc == -1 and b"outside" in lib.mdpt_last_error()
    rc = lib.mdpt_post_tile_blend(records.ctypes.data, table.data_ptr(), 4, native.DTYPE_F32, H, W, None, None, 3.0, out.data_ptr(), stream)
    assert rc == -1 and b"outside" in lib.mdpt_last_error()
    records["x2"][3] = W
    rc = lib.mdpt_post_tile_fit(records.ctypes.data, table.data_ptr(), 4, native.DTYPE_F32, guide.data_ptr(), native.DTYPE_F32, 13, 10, H, W, fit.data_ptr(),
                                sums.data_ptr(), scratch.data_ptr(), 8, stream)
    assert rc == -1 and b"scratch" in lib.mdpt_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((fit == 7.0).all()) and bool((sums == 7.0).all()) and bool((scratch == 0).all())
