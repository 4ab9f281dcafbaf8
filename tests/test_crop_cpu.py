"""Crop and region inference, the parts that need no GPU: crop_slices_from_norm reproduces the reference's rule on every recorded case
(tests/golden/crop_slices.json, written by tests/golden/gen_crop_slices.py from the reference's own function), is_cropping has its 0.999
boundary, the new C entry points are exported and bound and refuse bad tables on the host, the Python arguments are checked before anything
touches a device, and the region forward plan is image_chunks on the box sizes."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import muggled_dpt_amd
from muggled_dpt_amd import crop_slices_from_norm, is_cropping, native
from muggled_dpt_amd.dpt_model import _check_regions, _crop_box, image_chunks, region_chunks

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "crop_slices.json")
NEW_SYMBOLS = ("mdpt_forward_bgr_regions", "mdpt_forward_bgr_pitched", "mdpt_prepare_image_region")


def test_crop_slices_from_norm_reproduces_every_reference_case():
    cases = json.load(open(GOLDEN))["cases"]
    assert len(cases) >= 200
    kinds = {"reversed": 0, "fallback_x": 0, "clipped": 0, "small": 0}
    for c in cases:
        ys, xs = crop_slices_from_norm(tuple(c["shape"]), c["crop_xy1xy2_norm"], tuple(c["minimum_crop_xy"]))
        assert isinstance(ys, slice) and isinstance(xs, slice)
        assert [ys.start, ys.stop] == c["y"] and [xs.start, xs.stop] == c["x"], c
        assert all(type(v) is int for v in (ys.start, ys.stop, xs.start, xs.stop))
        (x1, _), (x2, _) = c["crop_xy1xy2_norm"]
        kinds["reversed"] += c["x"][0] > c["x"][1]
        kinds["fallback_x"] += c["x"] == [0, c["shape"][1]] and 0 < abs(x2 - x1) < 0.9
        kinds["clipped"] += min(x1, x2) < 0 or max(x1, x2) > 1
        kinds["small"] += c["shape"][0] <= 6
    assert all(v > 0 for v in kinds.values()), kinds  # the fixture holds every kind of case
    # the default minimum is the reference's (5, 5)
    assert crop_slices_from_norm((100, 100), ((0.1, 0.1), (0.14, 0.5))) == (slice(10, 50), slice(0, 100))
    assert crop_slices_from_norm((100, 100), ((0.1, 0.1), (0.15, 0.5))) == (slice(10, 50), slice(10, 15))
    # round half to even on an exact .5 product: 0.125 * 100 = 12.5 -> 12, 0.375 * 100 = 37.5 -> 38
    assert crop_slices_from_norm((100, 100), ((0.125, 0.125), (0.375, 0.375))) == (slice(12, 38), slice(12, 38))


def test_is_cropping_boundary():
    assert not is_cropping(((0.0, 0.0), (1.0, 1.0)))
    assert not is_cropping(((0.0, 0.0), (0.999, 0.999)))
    assert not is_cropping(((0.0005, 0.0), (1.0, 1.0)))
    assert is_cropping(((0.0, 0.0), (0.998, 1.0)))
    assert is_cropping(((0.0, 0.0), (1.0, 0.9989)))
    assert is_cropping(((0.002, 0.0), (1.0, 1.0)))
    assert is_cropping(((0.25, 0.1), (0.75, 0.9)))
    assert is_cropping(((0.8, 0.0), (0.2, 1.0)))  # reversed: the difference is negative
    assert type(is_cropping(((0.0, 0.0), (1.0, 1.0)))) is bool


def test_new_entry_points_are_exported_and_bound():
    lib = native.load()
    for name in NEW_SYMBOLS:
        assert name in native.SYMBOLS, f"{name} is not in native.SYMBOLS"
        assert hasattr(lib, name), f"libmdpt.so does not export {name}"
    assert lib.mdpt_abi_version() == 6 and native.ABI_VERSION == 6  # additive: the ABI version stays
    for name in ("crop_slices_from_norm", "is_cropping"):
        assert name in muggled_dpt_amd.__all__ and callable(getattr(muggled_dpt_amd, name))
    assert hasattr(muggled_dpt_amd.DPTModel, "inference_regions")


def _regions_call(lib, ptrs, hw, pitch, boxes, B, handle=None):
    m3 = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    adr = lambda a: None if a is None else ctypes.addressof(a)  # noqa: E731
    # (the depth pointer, workspace and stream are never reached: every case fails on the host before any launch)
    return lib.mdpt_forward_bgr_regions(handle, adr(ptrs), adr(hw), adr(pitch), adr(boxes), B, 0, 28, 28, m3, m3, 0, 4096, 0, None, 0, None)


@pytest.fixture(scope="module")
def cpu_model():
    from muggled_dpt_amd import make_depthanythingv2_dpt_from_original_state_dict
    from muggled_dpt_amd.synthetic import make_synthetic_original_state_dict
    return make_depthanythingv2_dpt_from_original_state_dict(make_synthetic_original_state_dict("tiny", 0))[1]


def test_forward_bgr_regions_rejects_bad_tables_on_the_host(cpu_model):
    """With a real (unfinalised) handle, so that it is the table that is refused: nothing here touches a device."""
    from muggled_dpt_amd.dpt_model import native_config
    lib = native.load()
    cfg = native_config(cpu_model.config, "v2", native.PREC_BF16)
    handle = ctypes.c_void_p()
    native.check(lib, lib.mdpt_create(ctypes.byref(cfg), ctypes.byref(handle)))
    try:
        ptrs = (ctypes.c_void_p * 2)(4096, 8192)  # never dereferenced
        hw = (ctypes.c_int32 * 4)(20, 30, 41, 17)
        pitch = (ctypes.c_int64 * 2)(90, 64)
        good = [0, 0, 30, 20, 3, 5, 17, 41]
        bad_tables = {
            "null table": (None, hw, pitch, (ctypes.c_int32 * 8)(*good), 2),
            "null sizes": (ptrs, None, pitch, (ctypes.c_int32 * 8)(*good), 2),
            "null boxes": (ptrs, hw, pitch, None, 2),
            "null image": ((ctypes.c_void_p * 2)(4096, None), hw, pitch, (ctypes.c_int32 * 8)(*good), 2),
            "empty box": (ptrs, hw, pitch, (ctypes.c_int32 * 8)(0, 0, 30, 20, 5, 5, 5, 41), 2),
            "reversed box": (ptrs, hw, pitch, (ctypes.c_int32 * 8)(0, 0, 30, 20, 9, 5, 3, 41), 2),
            "negative corner": (ptrs, hw, pitch, (ctypes.c_int32 * 8)(-1, 0, 30, 20, 3, 5, 17, 41), 2),
            "box past the image (x)": (ptrs, hw, pitch, (ctypes.c_int32 * 8)(0, 0, 31, 20, 3, 5, 17, 41), 2),
            "box past the image (y)": (ptrs, hw, pitch, (ctypes.c_int32 * 8)(0, 0, 30, 20, 3, 5, 17, 42), 2),
            "pitch < 3w": (ptrs, hw, (ctypes.c_int64 * 2)(90, 50), (ctypes.c_int32 * 8)(*good), 2),
            "B = 0": (ptrs, hw, pitch, (ctypes.c_int32 * 8)(*good), 0),
            "B < 0": (ptrs, hw, pitch, (ctypes.c_int32 * 8)(*good), -2),
            "B > 65535": (ptrs, hw, pitch, (ctypes.c_int32 * 8)(*good), 65536),
        }
        for what, (a, b, c, d, n) in bad_tables.items():
            assert _regions_call(lib, a, b, c, d, n, handle) == -1, what
            assert lib.mdpt_last_error(), what
        # a null handle is refused too, and so are the sibling entry points' bad arguments
        assert _regions_call(lib, ptrs, hw, pitch, (ctypes.c_int32 * 8)(*good), 2, None) == -1
        m3 = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
        assert lib.mdpt_forward_bgr_pitched(handle, 4096, 2, 20, 30, 89, 4000, 0, 28, 28, m3, m3, 0, 4096, 0, None, 0, None) == -1  # pitch < 3w
        assert lib.mdpt_forward_bgr_pitched(handle, 4096, 2, 20, 30, 90, 0, 0, 28, 28, m3, m3, 0, 4096, 0, None, 0, None) == -1  # no frame stride
        assert lib.mdpt_forward_bgr_pitched(handle, None, 2, 20, 30, 90, 4000, 0, 28, 28, m3, m3, 0, 4096, 0, None, 0, None) == -1
        box = (ctypes.c_int32 * 4)(0, 0, 31, 20)
        assert lib.mdpt_prepare_image_region(4096, 20, 30, 0, box, 4096, 0, 28, 28, m3, m3, 0, None) == -1  # box past the image
        box = (ctypes.c_int32 * 4)(4, 4, 4, 20)
        assert lib.mdpt_prepare_image_region(4096, 20, 30, 0, box, 4096, 0, 28, 28, m3, m3, 0, None) == -1  # empty box
        box = (ctypes.c_int32 * 4)(0, 0, 30, 20)
        assert lib.mdpt_prepare_image_region(4096, 20, 30, 89, box, 4096, 0, 28, 28, m3, m3, 0, None) == -1  # pitch < 3w
        assert lib.mdpt_prepare_image_region(4096, 20, 30, 0, None, 4096, 0, 28, 28, m3, m3, 0, None) == -1
    finally:
        lib.mdpt_destroy(handle)


def test_crop_box_follows_numpy_slicing_and_the_reference_rule():
    img = np.arange(40 * 60 * 3, dtype=np.uint32).reshape(40, 60, 3)
    for crop in ((slice(3, 17), slice(5, 44)), (slice(None), slice(None)), (slice(-10, None), slice(None, -7)), (slice(0, 1000), slice(59, 60)),
                 ((0.25, 0.1), (0.75, 0.9)), ((0.0, 0.0), (1.0, 1.0)), ((0.5, 0.5), (0.51, 0.52)), [[0.1, 0.2], [0.9, 0.8]]):
        x1, y1, x2, y2 = _crop_box(img.shape[:2], crop)
        ys, xs = crop if isinstance(crop[0], slice) else crop_slices_from_norm(img.shape, crop)
        assert np.array_equal(img[y1:y2, x1:x2], img[ys, xs]) and x2 > x1 and y2 > y1
    assert _crop_box((40, 60), None) == (0, 0, 60, 40)


def test_argument_errors_come_before_any_device_work(cpu_model):
    f = np.zeros((20, 30, 3), np.uint8)
    g = np.zeros((41, 17, 3), np.uint8)
    box = ((0.1, 0.1), (0.9, 0.9))
    # bad crop shapes
    for bad in ((0.1, 0.1, 0.9, 0.9), ((0.1, 0.1), (0.9,)), "crop", 3, (slice(0, 5),), (slice(0, 5), (0.1, 0.2)), ((0.1, "a"), (0.2, 0.3)),
                ((0.1, 0.1), (0.9, 0.9), (1.0, 1.0))):
        with pytest.raises(TypeError):
            cpu_model.inference(f, crop=bad)
        with pytest.raises(TypeError):
            cpu_model.inference_batch([f, f], crop=bad)
        with pytest.raises(TypeError):
            cpu_model.prepare_image_bgr(f, crop=bad)
        with pytest.raises(TypeError):
            cpu_model.patch_embed.prepare_image(f, crop=bad)
        with pytest.raises(TypeError):
            cpu_model.inference_images([f, g], crops=bad)
    # empty crops (a reversed box is an empty slice in the reference too) and strided slices
    for bad in (((0.9, 0.1), (0.1, 0.9)), (slice(5, 5), slice(0, 10)), (slice(0, 10), slice(25, 3)), (slice(0, 10, 2), slice(0, 10))):
        with pytest.raises(ValueError):
            cpu_model.inference(f, crop=bad)
        with pytest.raises(ValueError):
            cpu_model.inference_batch(np.stack([f, f]), crop=bad)
        with pytest.raises(ValueError):
            cpu_model.inference_images([f, g], crops=[None, bad])
    with pytest.raises(ValueError):
        cpu_model.inference_images([f, g], crops=[box])  # one crop per image, or one for all
    with pytest.raises(TypeError):
        cpu_model.inference_images([f, g], crops=[box, "x"])
    # crop arguments are keyword-only
    with pytest.raises(TypeError):
        cpu_model.inference(f, None, True, box)
    with pytest.raises(TypeError):
        cpu_model.inference_images([f], None, True, 32, box)
    # regions: shape of the list, index range, boxes inside their image
    for bad in (None, "regions", 5, [(0, 0, 0, 10)], [(0, 0, 0, 10, 10, 3)], [(0, 0.0, 0, 10, 10)], [(True, 0, 0, 10, 10)], [7]):
        with pytest.raises(TypeError):
            cpu_model.inference_regions([f, g], bad)
    with pytest.raises(ValueError):
        cpu_model.inference_regions([f, g], [])
    for bad in ([(2, 0, 0, 5, 5)], [(-1, 0, 0, 5, 5)], [(0, 0, 0, 5, 5), (5, 0, 0, 5, 5)]):
        with pytest.raises(IndexError):
            cpu_model.inference_regions([f, g], bad)
    for bad in ([(0, 0, 0, 31, 20)], [(0, 0, 0, 30, 21)], [(1, 0, 0, 30, 20)], [(0, 5, 5, 5, 10)], [(0, 9, 5, 3, 10)], [(0, -1, 0, 5, 5)], [(0, 0, 0, 5, 5), (1, 0, 40, 17, 42)]):
        with pytest.raises(ValueError):
            cpu_model.inference_regions([f, g], bad)
    # host and device images mixed (the tensor item is checked on the host, it never needs a device here)
    with pytest.raises(TypeError, match="mix"):
        cpu_model.inference_regions([f, torch.zeros((20, 30, 3), dtype=torch.uint8)], [(0, 0, 0, 5, 5)])
    with pytest.raises(ValueError):
        cpu_model.inference_regions([f, g], [(0, 0, 0, 5, 5)], batch_size=0)
    # well-formed arguments on a CPU model: the RuntimeError of every inference entry point
    with pytest.raises(RuntimeError, match="GPU only"):
        cpu_model.inference_regions([f, g], [(0, 0, 0, 5, 5), (1, 3, 5, 17, 41), (0, 2, 2, 30, 20)])
    with pytest.raises(RuntimeError, match="GPU only"):
        cpu_model.inference_regions((f, g), np.asarray([(0, 0, 0, 5, 5), (1, 3, 5, 17, 41)]))
    with pytest.raises(RuntimeError, match="GPU only"):
        cpu_model.inference(f, crop=box)
    with pytest.raises(RuntimeError, match="GPU only"):
        cpu_model.inference_batch([f, f], crop=(slice(2, 9), slice(1, 20)))
    with pytest.raises(RuntimeError, match="GPU only"):
        cpu_model.inference_images([f, g], crops=[box, None])
    with pytest.raises(RuntimeError, match="GPU only"):
        cpu_model.prepare_image_bgr(f, crop=box)
    assert _check_regions([(1, 3, 5, 17, 41)], [f.shape, g.shape]) == [(1, 3, 5, 17, 41)]


def test_region_chunk_plan_is_image_chunks_on_the_box_sizes(cpu_model):
    pe = cpu_model.patch_embed
    rng = np.random.default_rng(5)
    shapes = [(3024, 4032), (333, 217), (720, 1280)]
    regions = []
    for _ in range(40):
        i = int(rng.integers(0, 3))
        h, w = shapes[i]
        x1, y1 = int(rng.integers(0, w)), int(rng.integers(0, h))
        regions.append((i, x1, y1, int(rng.integers(x1 + 1, w + 1)), int(rng.integers(y1 + 1, h + 1))))
    for square in (True, False):
        rule = lambda h, w: pe._scaled_hw(h, w, 252, square)  # noqa: E731
        for bs in (1, 3, 32):
            plan = region_chunks(regions, rule, bs)
            assert plan == image_chunks([(r[4] - r[2], r[3] - r[1]) for r in regions], rule, bs)
            assert sorted(k for _, idx in plan for k in idx) == list(range(len(regions)))
            for hw, idx in plan:
                assert all(tuple(rule(regions[k][4] - regions[k][2], regions[k][3] - regions[k][1])) == hw for k in idx)  # the BOX's size decides
    assert len(region_chunks(regions, lambda h, w: pe._scaled_hw(h, w, 252, True), 64)) == 1
    assert len(region_chunks(regions, lambda h, w: pe._scaled_hw(h, w, 252, False), 64)) > 1
