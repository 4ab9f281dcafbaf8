"""Batched frame inference and the device display tail, the parts that need no GPU: the new C entry points are exported and bound,
DPTModel.inference_batch checks its arguments before anything touches a device, and the value -> bin table the thresholded histogram
equalization hands to its LUT kernel reproduces np.histogram."""
import numpy as np
import pytest
import torch

from muggled_dpt_amd import native
from muggled_dpt_amd import postprocess as pp

NEW_SYMBOLS = ("mdpt_forward_bgr_batch", "mdpt_post_minmax_seg", "mdpt_post_u8_hist_seg", "mdpt_post_histogram", "mdpt_post_equalize_lut",
               "mdpt_post_colorize")


def test_new_entry_points_are_exported_and_bound():
    lib = native.load()
    for name in NEW_SYMBOLS:
        assert name in native.SYMBOLS, f"{name} is not in native.SYMBOLS"
        assert hasattr(lib, name), f"libmdpt.so does not export {name}"
    assert lib.mdpt_abi_version() == 6  # additive: the ABI version stays
    assert native.POST_SEG_PARTS == 64


def test_forward_bgr_batch_rejects_null_arguments_on_the_host():
    lib = native.load()
    m3 = (native.ctypes.c_float * 3)(0.5, 0.5, 0.5)
    # a null handle / source fails before any device work
    assert lib.mdpt_forward_bgr_batch(None, None, 2, 8, 8, 0, 28, 28, m3, m3, 0, None, 0, None, 0, None) == -1
    assert lib.mdpt_post_colorize(None, 1, 16, None, None, 3, None, None) == -1
    assert lib.mdpt_post_equalize_lut(None, 1, None, 0, 255, None, None) == -1


@pytest.fixture(scope="module")
def cpu_model():
    from muggled_dpt_amd import make_depthanythingv2_dpt_from_original_state_dict
    from muggled_dpt_amd.synthetic import make_synthetic_original_state_dict
    return make_depthanythingv2_dpt_from_original_state_dict(make_synthetic_original_state_dict("tiny", 0))[1]


def test_inference_batch_argument_errors_come_before_any_device_work(cpu_model):
    f = np.zeros((20, 30, 3), np.uint8)
    for bad in ([], (), np.zeros((0, 20, 30, 3), np.uint8), torch.zeros((0, 20, 30, 3), dtype=torch.uint8)):
        with pytest.raises(ValueError):
            cpu_model.inference_batch(bad)
    with pytest.raises(ValueError):
        cpu_model.inference_batch([f, np.zeros((21, 30, 3), np.uint8)])
    with pytest.raises(ValueError):
        cpu_model.inference_batch((f, f, np.zeros((20, 31, 3), np.uint8)))
    for bad in ([f.astype(np.float32)], [f[..., :2]], [f[..., 0]], np.zeros((2, 20, 30, 3), np.float32), np.zeros((2, 20, 30), np.uint8),
                torch.zeros((2, 20, 30, 3), dtype=torch.float32), f, "frames", [f, "frame"]):
        with pytest.raises(TypeError):
            cpu_model.inference_batch(bad)
    # well-formed frames on a CPU model: the same RuntimeError prepare_image raises
    for good in ([f, f], np.stack([f, f]), torch.zeros((2, 20, 30, 3), dtype=torch.uint8)):
        with pytest.raises(RuntimeError, match="GPU only"):
            cpu_model.inference_batch(good)
    with pytest.raises(RuntimeError, match="GPU only"):
        cpu_model.prepare_image_bgr(f)


@pytest.mark.parametrize("pcts", [(0.1, 0.9), (0.5, 0.5), (0.0, 0.5), (0.3, 1.0), (0.25, 0.75), (0.9, 0.1), (0.0, 0.99)])
def test_threshold_bin_table_matches_np_histogram(pcts):
    vmin, vmax = pp.equalization_range(*pcts)
    assert 0 <= vmin < vmax <= 255 and (vmin, vmax) != (0, 255)
    table = pp.threshold_bin_table(vmin, vmax)
    assert table.shape == (256,) and table.dtype == np.int32
    nbins = 1 + vmax - vmin
    rng = np.random.default_rng(7)
    for x in (rng.integers(0, 256, (37, 53), dtype=np.uint8), np.arange(256, dtype=np.uint8), np.full((5, 5), vmin, np.uint8),
              np.full((5, 5), vmax, np.uint8), rng.integers(vmin, vmax + 1, (64, 64), dtype=np.uint8)):
        want, _ = np.histogram(x, nbins, range=(vmin, vmax))
        bins = table[x.ravel()]
        got = np.bincount(bins[bins >= 0], minlength=nbins)
        assert np.array_equal(got, want), pcts


def test_equalization_range_follows_the_reference():
    assert pp.equalization_range() == (0, 255)
    assert pp.equalization_range(0.1, 0.9) == (26, 230)  # round(25.5) = 26: Python's round, as the reference uses
    assert pp.equalization_range(0.5, 0.5) == (128, 129)  # max is pushed one above min
    with pytest.raises(ValueError):
        pp.equalization_range(1.0, 1.0)  # (the reference's np.full(-1) fails there too)
