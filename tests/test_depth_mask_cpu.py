"""Depth masking, the parts that need no GPU: the checker and cv2.resize restatements of tests/mask_restate.py equal the reference's CheckerPattern and
the cv2 stub of tests/golden/gen_depth_mask.py (tests/golden/depth_mask.npz), the new functions check their arguments before anything touches a device,
and the new C entry points are exported, bound and validate on the host."""
import os

import numpy as np
import pytest
import torch

from muggled_dpt_amd import native
from muggled_dpt_amd import postprocess as pp
from tests import mask_restate as mr

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "depth_mask.npz")
NEW_SYMBOLS = ("mdpt_post_mask_display", "mdpt_post_mask_cutout_images")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def test_checker_equals_the_reference_checker_pattern(gold):
    keys = [k for k in gold.files if k.startswith("checker_")]
    assert len(keys) >= 10
    sizes = set()
    for key in keys:
        h, w = (int(v) for v in key[len("checker_"):].split("x"))
        sizes.add((h, w))
        assert np.array_equal(mr.checker(h, w), gold[key]), key
    assert any(h < 64 and w < 64 for h, w in sizes) and (64, 64) in sizes and any(h > 64 and w > 64 for h, w in sizes)
    assert any(h % 2 and w % 2 for h, w in sizes)


def test_resize_restatement_equals_the_fixture(gold):
    keys = [k for k in gold.files if k.startswith("resize_u8_")]
    assert len(keys) >= 6
    for key in keys:
        tag = key[len("resize_u8_"):]
        oh, ow = (int(v) for v in tag.split("_")[1].split("x"))
        got = mr.resize_u8(gold["resize_in_u8_" + tag], (ow, oh))
        assert got.dtype == np.uint8 and np.array_equal(got, gold[key]), key
        got = mr.resize_f64(gold["resize_in_f64_" + tag], (ow, oh))
        assert got.dtype == np.float64 and np.array_equal(got, gold["resize_f64_" + tag]), key


def test_resize_restatement_rules():
    s0, s1, a = mr.linear_taps(8, 4)  # enlargement by 2: (d + 0.5) / 2 - 0.5
    assert list(s0) == [0, 0, 0, 1, 1, 2, 2, 3] and a[0] == 0 and a[-1] == 0 and a[1] == np.float32(0.25) and s1[1] == 1
    x = np.arange(12, dtype=np.float64).reshape(3, 4)
    assert np.array_equal(mr.resize_f64(x, (4, 3)), x)  # same size: a copy
    img = np.arange(36, dtype=np.uint8).reshape(3, 4, 3)
    assert np.array_equal(mr.resize_u8(img, (4, 3)), img)


def test_new_functions_check_arguments_before_the_device():
    host = torch.rand(2, 16, 16)
    photos = torch.zeros(2, 20, 30, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="CUDA"):
        pp.depth_mask_display(host, photos, (30, 20))
    with pytest.raises(RuntimeError, match="CUDA"):
        pp.depth_mask_images(host, [np.zeros((20, 30, 3), np.uint8)] * 2)
    for bad in ((0.6, 0.4), (-0.1, 0.5), (0.2, 1.5)):
        with pytest.raises(ValueError, match="threshold"):
            pp.depth_mask_display(host, photos, (30, 20), threshold=bad)
        with pytest.raises(ValueError, match="threshold"):
            pp.depth_mask_images(host, [np.zeros((20, 30, 3), np.uint8)] * 2, threshold=bad)
    with pytest.raises(ValueError, match="2 predictions but 3 images"):
        pp.depth_mask_images(host, [np.zeros((20, 30, 3), np.uint8)] * 3)
    with pytest.raises(ValueError, match="2 predictions but 1 images"):
        pp.depth_mask_images([host[0], host[1]], [np.zeros((20, 30, 3), np.uint8)])
    for bad in ([np.zeros((20, 30, 3), np.float32)] * 2, [np.zeros((20, 30), np.uint8)] * 2, [np.zeros((20, 30, 4), np.uint8)] * 2,
                [np.zeros((20, 30, 3), np.uint8), torch.zeros(20, 30, 3, dtype=torch.uint8)]):
        with pytest.raises(TypeError):
            pp.depth_mask_images(host, bad)
    with pytest.raises(ValueError, match="empty"):
        pp.depth_mask_images(host, [np.zeros((0, 30, 3), np.uint8)] * 2)
    with pytest.raises(TypeError):
        pp.depth_mask_images(host.numpy(), [np.zeros((20, 30, 3), np.uint8)] * 2)


def test_new_entry_points_are_exported_and_validate_on_the_host():
    lib = native.load()
    for name in NEW_SYMBOLS:
        assert name in native.SYMBOLS, f"{name} is not in native.SYMBOLS"
        assert hasattr(lib, name), f"libmdpt.so does not export {name}"
    assert lib.mdpt_abi_version() == 6  # additive: the ABI version stays
    fake = 16  # never dereferenced: every call below fails its checks before a launch
    assert lib.mdpt_post_mask_display(fake, 0, 1, 4, 4, fake, fake, 0.0, fake, 0.6, 0.2, 0, fake, 4, 4, fake, fake, None) == -1
    assert b"threshold" in lib.mdpt_last_error()
    assert lib.mdpt_post_mask_display(fake, 0, 1, 4, 4, fake, fake, 0.0, fake, 0.0, 1.0, 0, fake, 0, 4, fake, fake, None) == -1
    assert lib.mdpt_post_mask_display(fake, 7, 1, 4, 4, fake, fake, 0.0, fake, 0.0, 1.0, 0, fake, 4, 4, fake, fake, None) == -1
    ptrs = np.full(2, fake, dtype=np.uint64)
    hw = np.array([4, 4, 4, 4], dtype=np.int32)
    offs = np.array([0, 16], dtype=np.int64)
    args = lambda **kw: [kw.get(k, v) for k, v in (("maps", ptrs.ctypes.data), ("map_hw", hw.ctypes.data), ("dt", 0), ("parts", ptrs.ctypes.data),  # noqa: E731
                                                   ("coef", ptrs.ctypes.data), ("vparts", ptrs.ctypes.data), ("f", 0.0), ("images", ptrs.ctypes.data),
                                                   ("image_hw", hw.ctypes.data), ("offs", offs.ctypes.data), ("B", 2), ("tmin", 0.0), ("tmax", 1.0),
                                                   ("invert", 0), ("bgra", fake), ("mask", fake), ("stream", None))]
    assert lib.mdpt_post_mask_cutout_images(*args(tmin=0.5, tmax=0.25)) == -1
    assert b"threshold" in lib.mdpt_last_error()
    assert lib.mdpt_post_mask_cutout_images(*args(bgra=fake + 1)) == -1
    assert b"aligned" in lib.mdpt_last_error()
    bad_hw = np.array([4, 4, 0, 4], dtype=np.int32)
    assert lib.mdpt_post_mask_cutout_images(*args(image_hw=bad_hw.ctypes.data)) == -1
    bad_offs = np.array([0, -4], dtype=np.int64)
    assert lib.mdpt_post_mask_cutout_images(*args(offs=bad_offs.ctypes.data)) == -1
    assert lib.mdpt_post_mask_cutout_images(*args(B=0)) == -1
    assert lib.mdpt_post_mask_cutout_images(*args(maps=None)) == -1
