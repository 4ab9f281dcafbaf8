"""The display tail for images of different sizes: postprocess.scale_prediction_images and depth_to_color_images, the seg_* and colorize kernels
taking a per-image table. Element i has to equal scale_prediction / depth_to_color of prediction i alone, bit for bit, for upscaling and
downscaling targets, reverse, both high_contrast branches, a LUT and grey output, bf16 / fp16 / fp32 maps of different sizes in one call, and
more images than one table holds (40 > 32)."""
import numpy as np
import pytest
import torch

from muggled_dpt_amd import postprocess as pp

pytestmark = pytest.mark.gpu

# (h, w) of the maps and (w, h) targets: up and down, both orientations, tiny and photo sized
MAP_HW = [(28, 28), (56, 84), (112, 70), (7, 5), (1, 1), (504, 504), (42, 98), (84, 56)]
TARGET_WH = [(640, 480), (13, 9), (70, 112), (1, 1), (33, 47), (4032, 3024), (98, 42), (300, 1000)]


def _bits(t):
    return t.view(torch.int16) if t.dtype in (torch.bfloat16, torch.float16) else t


def _maps(hws, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for k, (h, w) in enumerate(hws):
        m = torch.rand((1, h, w), generator=g) * (3.0 + k) - 1.0
        if k == 3:
            m[0, 0, 0] = 5.0  # one outlier
        out.append(m.to("cuda", dtype))
    return out


def _lut(seed):
    return np.random.default_rng(seed).integers(0, 256, (1, 256, 3), dtype=np.uint8)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_scale_prediction_images_equal_scale_prediction_per_image(dtype):
    maps = _maps(MAP_HW, dtype, 1)
    got = pp.scale_prediction_images(maps, TARGET_WH)
    assert len(got) == len(maps)
    for i, (m, wh) in enumerate(zip(maps, TARGET_WH)):
        want = pp.scale_prediction(m, wh)
        assert got[i].shape == want.shape == (1, wh[1], wh[0]) and got[i].dtype == want.dtype == dtype
        assert torch.equal(_bits(got[i]), _bits(want)), f"{dtype}: image {i} {tuple(m.shape)} -> {wh}"
    # outputs are views into one allocation
    assert len({t.untyped_storage().data_ptr() for t in got}) == 1
    # [h,w] maps and a [B,h,w] tensor give the same
    got2 = pp.scale_prediction_images([m[0] for m in maps], TARGET_WH)
    for a, b in zip(got, got2):
        assert torch.equal(_bits(a), _bits(b))
    batch = torch.cat(_maps([(56, 84)] * 3, dtype, 2))
    got3 = pp.scale_prediction_images(batch, TARGET_WH[:3])
    for i in range(3):
        assert torch.equal(_bits(got3[i]), _bits(pp.scale_prediction(batch[i:i + 1], TARGET_WH[i])))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("reverse,high_contrast,lut_seed", [(False, False, None), (True, False, 3), (False, True, 4), (True, True, None)])
def test_depth_to_color_images_equal_depth_to_color_per_image(dtype, reverse, high_contrast, lut_seed):
    maps = _maps(MAP_HW, dtype, 5)
    lut = None if lut_seed is None else _lut(lut_seed)
    for targets in (TARGET_WH, None):
        got = pp.depth_to_color_images(maps, targets, reverse, high_contrast, lut)
        assert len(got) == len(maps)
        assert len({t.untyped_storage().data_ptr() for t in got}) == 1
        for i, m in enumerate(maps):
            wh = None if targets is None else targets[i]
            want = pp.depth_to_color(m, wh, reverse, high_contrast, lut)
            assert got[i].shape == want.shape and got[i].dtype == torch.uint8
            assert torch.equal(got[i], want), f"{dtype} reverse={reverse} high_contrast={high_contrast} lut={lut_seed}: image {i} -> {wh}"
        if lut is None:
            assert all(torch.equal(t[..., 0], t[..., 1]) and torch.equal(t[..., 0], t[..., 2]) for t in got)  # grey


def test_depth_to_color_images_both_equalization_branches_and_flat_maps():
    """high_contrast hits cv2.equalizeHist's ordinary branch on varied maps and its single-valued branch on a constant one; a constant map
    (max == min) and a NaN map give what depth_to_color gives them and touch no other image."""
    maps = _maps([(30, 40), (64, 64), (17, 23)], torch.float32, 6)
    maps.append(torch.full((1, 20, 20), 0.25, device="cuda"))
    nan = torch.rand((1, 9, 11), device="cuda")
    nan[0, 4, 5] = float("nan")
    maps.append(nan)
    maps.append(torch.rand((1, 33, 31), device="cuda"))
    targets = [(40, 30), (32, 32), (100, 70), (7, 7), (22, 18), (31, 33)]
    for high_contrast in (True, False):
        for tw in (targets, None):
            got = pp.depth_to_color_images(maps, tw, False, high_contrast, _lut(7))
            for i, m in enumerate(maps):
                assert torch.equal(got[i], pp.depth_to_color(m, None if tw is None else tw[i], False, high_contrast, _lut(7))), (high_contrast, i)


def test_display_images_more_than_one_table_and_input_forms():
    """40 maps of different sizes (two tables: 32 + 8), as [1,h,w] tensors, [h,w] tensors and a LUT tensor."""
    rng = np.random.default_rng(8)
    hws = [(int(rng.integers(1, 90)), int(rng.integers(1, 90))) for _ in range(40)]
    whs = [(int(rng.integers(1, 200)), int(rng.integers(1, 200))) for _ in range(40)]
    maps = _maps(hws, torch.bfloat16, 9)
    lut = torch.from_numpy(_lut(10)).cuda()
    got = pp.depth_to_color_images(maps, whs, True, True, lut)
    got_hw = pp.depth_to_color_images([m[0] for m in maps], whs, True, True, lut)
    scaled = pp.scale_prediction_images(maps, whs)
    for i, (m, wh) in enumerate(zip(maps, whs)):
        want = pp.depth_to_color(m, wh, True, True, lut)
        assert torch.equal(got[i], want) and torch.equal(got_hw[i], want), f"image {i} {hws[i]} -> {wh}"
        assert torch.equal(_bits(scaled[i]), _bits(pp.scale_prediction(m, wh)))


def test_inference_images_to_display_at_each_images_own_size():
    """The whole path: images of different sizes -> inference_images -> depth_to_color_images back to each image's own size."""
    from tests.test_gpu_c_host import _family_model
    model, unit = _family_model("v2")
    model = model.to("cuda", torch.bfloat16)
    rng = np.random.default_rng(11)
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in [(120, 160), (333, 217), (64, 64), (480, 640), (37, 300)]]
    whs = [(f.shape[1], f.shape[0]) for f in images]
    for square in (True, False):
        preds = model.inference_images(images, 4 * unit, square, 3)
        frames = pp.depth_to_color_images(preds, whs, high_contrast=True, lut=_lut(12))
        for i, f in enumerate(images):
            assert frames[i].shape == (1, f.shape[0], f.shape[1], 3)
            assert torch.equal(frames[i], pp.depth_to_color(model.inference(f, 4 * unit, square), whs[i], False, True, _lut(12)))


def test_display_images_argument_errors():
    maps = _maps([(8, 8), (9, 7)], torch.float32, 13)
    with pytest.raises(ValueError):
        pp.scale_prediction_images(maps, [(4, 4)])  # one target per image
    with pytest.raises(ValueError):
        pp.depth_to_color_images(maps, [(4, 4), (0, 3)])
    with pytest.raises(RuntimeError):
        pp.depth_to_color_images([maps[0], maps[1].half()])  # one dtype
    with pytest.raises(RuntimeError):
        pp.depth_to_color_images([maps[0], maps[1].cpu()])  # one device
