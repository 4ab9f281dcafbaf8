"""The still-image display tail and the 3D viewer's edge alpha, the parts that need no GPU: plane_sample_points draws the reference's own
points (tests/golden/display_still.npz, written by gen_display_still.py from the reference's plane_fit.get_xyz_samples), the new functions
check their arguments before anything touches a device, and the new C entry points are exported, bound and validate on the host."""
import os

import numpy as np
import pytest
import torch

from muggled_dpt_amd import native
from muggled_dpt_amd import postprocess as pp

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "display_still.npz")
NEW_SYMBOLS = ("mdpt_post_display_prep", "mdpt_post_plane_fit", "mdpt_post_plane_eval", "mdpt_post_plane_minmax", "mdpt_post_threshold",
               "mdpt_post_edge_mag", "mdpt_post_edge_mask", "mdpt_post_pack_u24_alpha")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def test_sample_points_equal_the_reference_for_every_seed_and_size(gold):
    keys = [k for k in gold.files if k.startswith("points_")]
    assert len(keys) >= 20
    for key in keys:
        hw, seed = key[len("points_"):].split("_seed")
        h, w = (int(v) for v in hw.split("x"))
        np.random.seed(int(seed))
        got = pp.plane_sample_points((h, w))
        want = gold[key]
        assert got.dtype == np.int32 and got.shape == want.shape == (min(16, h) * min(16, w), 2), key
        assert np.array_equal(got, want), key


def test_sample_points_stay_inside_and_follow_the_rng():
    rs = np.random.RandomState(3)
    a = pp.plane_sample_points((37, 5), samples_per_side=8, jitter_scale=1.0, rng=rs)
    assert a.shape == (8 * 5, 2)
    assert a[:, 0].min() >= 0 and a[:, 0].max() <= 4 and a[:, 1].min() >= 0 and a[:, 1].max() <= 36
    b = pp.plane_sample_points((37, 5), samples_per_side=8, jitter_scale=1.0, rng=np.random.RandomState(3))
    assert np.array_equal(a, b)
    g = pp.plane_sample_points((20, 30), rng=np.random.default_rng(0))  # a Generator (standard_normal) works too
    assert g.shape == (256, 2)
    grid = pp.plane_sample_points((100, 100), jitter_scale=0.0)  # no jitter: the cell centres
    assert np.array_equal(np.unique(grid[:, 0]), np.int32(np.round((0.5 + np.arange(16, dtype=np.float32)) / 16 * np.float32(99))))
    with pytest.raises(ValueError):
        pp.plane_sample_points((0, 5))
    with pytest.raises(ValueError):
        pp.plane_sample_points((5, 5), samples_per_side=0)


def test_new_functions_check_arguments_before_the_device():
    host = torch.rand(2, 16, 16)
    for fn in (pp.plane_of_best_fit, pp.depth_to_display, pp.depth_for_saving, pp.depth_edge_mask, pp.pack_depth_u24_frames):
        with pytest.raises(RuntimeError, match="CUDA"):
            fn(host)
        with pytest.raises(RuntimeError, match="CUDA"):
            fn(host.numpy())
    for bad in ((0.6, 0.4), (-0.1, 0.5), (0.2, 1.5)):
        with pytest.raises(ValueError, match="threshold"):
            pp.depth_to_display(host, threshold=bad)
        with pytest.raises(ValueError, match="threshold"):
            pp.depth_for_saving(host, threshold=bad)
    with pytest.raises(ValueError, match="alpha"):
        pp.pack_depth_u24_frames(host, alpha="mask")
    # reflect padding needs every side above the pad: 2 px for k = 3 (the Sobel), 3 for k = 5, 4 for k = 7
    for shape, k in (((2, 2), 5), ((3, 9), 7), ((1, 8), 3), ((9, 1), 1), ((2, 3, 3), 7)):
        with pytest.raises(RuntimeError, match="too small"):
            pp.depth_edge_mask(torch.rand(*shape), blur_kernel_size=k)
        with pytest.raises(RuntimeError, match="too small"):
            pp.pack_depth_u24_frames(torch.rand(*shape), blur_kernel_size=k)
    for k, bw in ((17, 1.0), (-1, 1.0), (5, 0.0)):
        with pytest.raises(ValueError):
            pp.depth_edge_mask(torch.rand(8, 8), blur_kernel_size=k, blur_weight=bw)


def test_blur_weights_are_the_viewers_gaussian():
    w = pp._blur_weights(5, 1.0)
    i = np.arange(-2, 3, dtype=np.float64)
    want = np.exp(-(i[:, None] ** 2 + i[None, :] ** 2) * 0.01)
    assert w.shape == (5, 5) and w.dtype == np.float32 and w[2, 2] == 1.0
    assert np.allclose(w, want / want.max(), rtol=1e-6)
    assert pp._blur_weights(4, 2.0).shape == (5, 5) and pp._blur_weights(1, 1.0).shape == (1, 1)  # 1 + 2 (k // 2)


def test_new_entry_points_are_exported_and_validate_on_the_host():
    lib = native.load()
    for name in NEW_SYMBOLS:
        assert name in native.SYMBOLS, f"{name} is not in native.SYMBOLS"
        assert hasattr(lib, name), f"libmdpt.so does not export {name}"
    assert lib.mdpt_abi_version() == 6  # additive: the ABI version stays
    fake = 16  # never dereferenced: every call below fails its checks before a launch
    assert lib.mdpt_post_threshold(fake, 0, 1, 4, 4, fake, fake, 0.0, fake, 0.0, 1.0, native.POST_U8, 1, fake, None, None) == -1
    assert b"reverse" in lib.mdpt_last_error()
    assert lib.mdpt_post_threshold(fake, 0, 1, 4, 4, fake, fake, 0.0, fake, 0.7, 0.2, native.POST_F32, 0, fake, None, None) == -1
    assert lib.mdpt_post_edge_mag(fake, 1, 2, 9, None, (native.ctypes.c_float * 25)(), 5, fake, fake, None) == -1
    assert b"too small" in lib.mdpt_last_error()
    assert lib.mdpt_post_edge_mag(fake, 1, 9, 9, None, (native.ctypes.c_float * 16)(), 4, fake, fake, None) == -1
    assert lib.mdpt_post_plane_fit(fake, 0, 1, 4, 4, None, fake, 0, 0, fake, None) == -1
    assert lib.mdpt_post_pack_u24_alpha(fake, 1, 16, None, 0, fake, fake, fake, 0, fake, None) == -1
    assert lib.mdpt_post_display_prep(None, 0, 1, 4, 4, fake, 4, 4, fake, None, None) == -1
