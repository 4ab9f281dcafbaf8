"""The per-image display tail on the device: histogram_equalization (the reference's demo_helpers/postprocess.py:107-145, both branches),
apply_colormap (toadui/colormaps.py:237-259) and depth_to_color, the per-frame loop of run_video.py:348-361 over a batch. cv2 is not a
dependency, so cv2.equalizeHist is restated here in numpy from its definition."""
import numpy as np
import pytest
import torch

from muggled_dpt_amd import postprocess as pp

pytestmark = pytest.mark.gpu


def np_equalize_hist(x: np.ndarray) -> np.ndarray:
    """cv2.equalizeHist: first non-empty bin i; a single-valued image stays i; else lut[i] = 0 and lut[j] = saturate_cast<uchar>(float(cumsum of
    bins i+1..j) * (255.f / (total - hist[i]))), rounded half to even, in fp32."""
    hist = np.bincount(x.ravel(), minlength=256)
    i = int(np.flatnonzero(hist)[0])
    if hist[i] == x.size:
        return np.full_like(x, i)
    scale = np.float32(255.0) / np.float32(x.size - hist[i])
    lut = np.zeros(256, np.uint8)
    s = 0
    for j in range(i + 1, 256):
        s += int(hist[j])
        lut[j] = np.clip(np.rint(np.float32(s) * scale), 0, 255)
    return lut[x]


def np_equalize_thresholded(depth_uint8: np.ndarray, min_pct: float, max_pct: float) -> np.ndarray:
    """The reference's np.histogram branch, restated."""
    min_value, max_value = [int(round(255 * value)) for value in sorted((min_pct, max_pct))]
    max_value = max(max_value, min_value + 1)
    num_bins = 1 + max_value - min_value
    bin_counts, _ = np.histogram(depth_uint8, num_bins, range=(min_value, max_value))
    cdf = bin_counts.cumsum()
    cdf_min, cdf_max = cdf.min(), cdf.max()
    cdf_norm = (cdf - cdf_min) / float(max(cdf_max - cdf_min, 1))
    cdf_uint8 = np.uint8(255 * cdf_norm)
    lut = np.concatenate((np.zeros(min_value, dtype=np.uint8), cdf_uint8, np.full(255 - max_value, 255, dtype=np.uint8)))
    return lut[depth_uint8]


def _maps():
    rng = np.random.default_rng(0)
    skewed = np.clip(rng.normal(60, 20, (97, 131)), 0, 255).astype(np.uint8)
    two = np.where(rng.random((40, 50)) < 0.3, 17, 200).astype(np.uint8)
    return [rng.integers(0, 256, (64, 80), dtype=np.uint8), skewed, np.full((33, 17), 91, np.uint8), two, np.array([[123]], np.uint8),
            rng.integers(100, 140, (512, 518), dtype=np.uint8)]


def test_histogram_equalization_full_range_equals_equalize_hist():
    for x in _maps():
        got = pp.histogram_equalization(torch.from_numpy(x).cuda()).cpu().numpy()
        assert got.shape == x.shape and got.dtype == np.uint8
        assert np.array_equal(got, np_equalize_hist(x)), x.shape


@pytest.mark.parametrize("pcts", [(0.1, 0.9), (0.5, 0.5), (0.0, 0.5), (0.3, 1.0), (0.2, 0.6)])
def test_histogram_equalization_thresholded_equals_the_reference_branch(pcts):
    for x in _maps():
        got = pp.histogram_equalization(torch.from_numpy(x).cuda(), *pcts).cpu().numpy()
        assert np.array_equal(got, np_equalize_thresholded(x, *pcts)), (pcts, x.shape)


def test_histogram_equalization_of_a_batch_is_per_image():
    rng = np.random.default_rng(1)
    xs = np.stack([rng.integers(0, 256, (48, 40), dtype=np.uint8), np.full((48, 40), 5, np.uint8),
                   np.clip(rng.normal(200, 10, (48, 40)), 0, 255).astype(np.uint8)])
    for pcts in ((0.0, 1.0), (0.1, 0.9)):
        got = pp.histogram_equalization(torch.from_numpy(xs).cuda(), *pcts).cpu().numpy()
        for i in range(len(xs)):
            want = np_equalize_hist(xs[i]) if pcts == (0.0, 1.0) else np_equalize_thresholded(xs[i], *pcts)
            assert np.array_equal(got[i], want), (pcts, i)


def test_apply_colormap_equals_fancy_indexing():
    rng = np.random.default_rng(2)
    lut = rng.integers(0, 256, (1, 256, 3), dtype=np.uint8)
    for x in (rng.integers(0, 256, (3, 45, 61), dtype=np.uint8), rng.integers(0, 256, (70, 33), dtype=np.uint8)):
        xd = torch.from_numpy(x).cuda()
        got = pp.apply_colormap(xd, lut).cpu().numpy()
        assert got.shape == (*x.shape, 3)
        assert np.array_equal(got, lut[0][x])
        assert np.array_equal(pp.apply_colormap(xd, torch.from_numpy(lut)).cpu().numpy(), lut[0][x])
        assert np.array_equal(pp.apply_colormap(xd, None).cpu().numpy(), np.repeat(x[..., None], 3, axis=-1))
    with pytest.raises(TypeError):
        pp.apply_colormap(xd, lut.astype(np.float32))


def _per_frame(pred, target_wh, reverse, high_contrast, lut):
    """The per-frame loop of run_video.py:348-361, image by image, through the existing functions."""
    frames = []
    for b in range(pred.shape[0]):
        p = pred[b:b + 1]
        if target_wh is not None:
            p = pp.scale_prediction(p, target_wh)
        u8 = pp.convert_to_uint8(p)
        if reverse:
            u8 = 255 - u8
        if high_contrast:
            u8 = pp.histogram_equalization(u8)
        frames.append(pp.apply_colormap(u8, lut))
    return torch.cat(frames)


def _batch(dtype, seed=3):
    g = torch.Generator().manual_seed(seed)
    pred = torch.rand((5, 37, 52), generator=g) * 4.0 + 1.0
    pred[1] = 2.5  # all constant
    pred[3] *= 1e6 if dtype != torch.float16 else 1e3
    pred[4] = torch.linspace(-3, 7, 37 * 52).reshape(37, 52) ** 2  # smooth, with a flat-ish minimum
    return pred.to("cuda", dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_depth_to_color_equals_the_per_frame_composition(dtype):
    rng = np.random.default_rng(4)
    cmap = rng.integers(0, 256, (1, 256, 3), dtype=np.uint8)
    pred = _batch(dtype)
    for target_wh in (None, (80, 60), (52, 37), (23, 17)):
        for reverse, high_contrast, lut in ((False, False, None), (True, False, cmap), (False, True, cmap), (True, True, None), (True, True, cmap)):
            got = pp.depth_to_color(pred, target_wh, reverse, high_contrast, lut)
            want = _per_frame(pred, target_wh, reverse, high_contrast, lut)
            assert got.shape == want.shape and got.dtype == torch.uint8
            for b in range(pred.shape[0]):
                assert torch.equal(got[b], want[b]), (dtype, target_wh, reverse, high_contrast, lut is None, b)


def test_depth_to_color_images_do_not_see_each_other():
    cmap = np.random.default_rng(5).integers(0, 256, (1, 256, 3), dtype=np.uint8)
    pred = _batch(torch.float32)
    base = pp.depth_to_color(pred, (64, 48), True, True, cmap)
    changed = pred.clone()
    changed[2] = changed[2] * -7.0 + 1e4
    after = pp.depth_to_color(changed, (64, 48), True, True, cmap)
    assert not torch.equal(after[2], base[2])
    for b in (0, 1, 3, 4):
        assert torch.equal(after[b], base[b]), b
    # a NaN map: that image follows MDPT_POST_U8 (all 0 before the reverse), the others are untouched
    nan = pred.clone()
    nan[1, 5, 7] = float("nan")
    got = pp.depth_to_color(nan, (64, 48), True, True, cmap)
    assert torch.equal(got[1], _per_frame(nan[1:2], (64, 48), True, True, cmap)[0])
    assert torch.equal(got[1], torch.from_numpy(np.broadcast_to(cmap[0][255], (48, 64, 3)).copy()).cuda())
    for b in (0, 2, 3, 4):
        assert torch.equal(got[b], base[b]), b


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_segmented_resize_equals_scale_prediction_bit_for_bit(dtype):
    """mdpt_post_minmax_seg's resize is scale_prediction's, value for value (the uint8 step would hide a last-bit difference)."""
    from muggled_dpt_amd import native
    lib = native.load()
    pred = _batch(dtype)
    b, h, w = pred.shape
    for oh, ow in ((60, 80), (37, 52), (17, 23), (491, 517)):
        out = torch.empty((b, oh, ow), device="cuda", dtype=torch.float32)
        parts = torch.empty((b, native.POST_SEG_PARTS, 2), device="cuda", dtype=torch.int32)
        native.check(lib, lib.mdpt_post_minmax_seg(pred.data_ptr(), native.dtype_code(dtype), b, h, w, out.data_ptr(), oh, ow, parts.data_ptr(), None,
                                                   torch.cuda.current_stream().cuda_stream))
        want = pp.scale_prediction(pred, (ow, oh)).float()
        assert torch.equal(out, want), (dtype, oh, ow, int((out != want).sum()))
