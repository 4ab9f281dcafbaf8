"""Crop and region inference: a box of an image is a frame the fused resize + normalise + im2col kernel reads where the image lies (base pointer,
row pitch, box), batched like any frame. Every comparison is torch.equal on the bits against the same call on PACKED COPIES of the boxes
(np.ascontiguousarray(image[y1:y2, x1:x2])): DPTModel.inference_regions / mdpt_forward_bgr_regions from device and from host images, crop= on
inference / inference_batch / inference_images / prepare_image_bgr, sliced device views passed without a crop (read in place, one launch), the
pitch-and-box form of prepare, and the stage-by-stage route that listening hooks select. The antialias taps have to stop at the box's edges:
overwriting every pixel outside a box must not change a bit of its map."""
import ctypes

import numpy as np
import pytest
import torch

from muggled_dpt_amd import crop_slices_from_norm, native
from muggled_dpt_amd.dpt_model import _check_frames, _check_images, region_chunks
from tests.test_gpu_c_host import _family_model

pytestmark = pytest.mark.gpu

CASES = [("v2", torch.float32, None), ("v2", torch.bfloat16, None), ("v2", torch.float32, "mixed"), ("v1", torch.float16, None),
         ("beit", torch.bfloat16, None), ("beit", torch.float32, "bf16x3"), ("swinv2", torch.float32, "mixed"), ("swinv2", torch.bfloat16, None)]

# (h, w): the small image is 333 rows of 217 pixels (row pitch 651 bytes, not a multiple of 4), the large one a 12 MP photo
SMALL_HW, LARGE_HW = (333, 217), (4032, 3024)
# (image, x1, y1, x2, y2)
BOXES = [
    (0, 0, 0, 217, 333),        # the full image
    (0, 0, 40, 100, 200),       # touches the left edge
    (0, 31, 0, 150, 90),        # ... the top edge
    (0, 57, 20, 217, 300),      # ... the right edge
    (0, 20, 100, 180, 333),     # ... the bottom edge
    (0, 33, 41, 160, 230),      # interior, odd x1: first byte at 41 * 651 + 99
    (0, 101, 77, 102, 78),      # 1 x 1
    (0, 216, 10, 217, 310),     # 1 wide, N high (the last column)
    (0, 5, 332, 211, 333),      # N wide, 1 high (the last row)
    (0, 90, 150, 103, 161),     # smaller than the tensor: upscales
    (1, 0, 0, 3024, 4032),      # the full 12 MP image: downscales, antialias taps span many rows
    (1, 1001, 777, 3001, 2778), # interior, odd x1, much larger than the tensor
    (1, 0, 1500, 900, 2500),    # left edge
    (1, 2100, 3000, 3024, 4032),# bottom right corner
    (1, 3023, 4031, 3024, 4032),# the last pixel of the allocation
    (1, 1517, 9, 1540, 40),     # small box of the large image: upscales
]


def _bits(t):
    return t.view(torch.int16) if t.dtype != torch.float32 else t


def _model(family, dtype, precision, latency=False):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    model, unit = _family_model(family)
    model = model.to("cuda", dtype)
    if precision:
        model.set_precision(precision)
    if latency:
        model.set_latency_mode(True)
    side = 4 * unit if family != "swinv2" else 128
    return model, side


_CACHE = {}


def _image(hw, seed):
    key = (hw, seed)
    if key not in _CACHE:
        _CACHE[key] = np.random.default_rng(seed).integers(0, 256, (*hw, 3), dtype=np.uint8)
    return _CACHE[key]


def _device(images):
    key = ("dev",) + tuple(id(f) for f in images)
    if key not in _CACHE:
        _CACHE[key] = (images, [torch.from_numpy(f).cuda() for f in images])  # (the host arrays are kept alive with their ids)
    return _CACHE[key][1]


def _two_images():
    return [_image(SMALL_HW, 11), _image(LARGE_HW, 12)]


def _packed(images, regions):
    return [np.ascontiguousarray(images[i][y1:y2, x1:x2]) for i, x1, y1, x2, y2 in regions]


def _check_equal(got, want, what):
    assert len(got) == len(want)
    for r, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dim() == 3 and g.shape[0] == 1 and g.dtype == w.dtype, f"{what}: region {r} {g.shape} {w.shape}"
        assert torch.equal(_bits(g), _bits(w)), f"{what}: region {r} differs from the packed copy of its box"


@pytest.mark.parametrize("family,dtype,precision,latency", [c + (False,) for c in CASES] + [("v2", torch.bfloat16, None, True)])
def test_regions_equal_inference_images_on_packed_copies_bit_for_bit(family, dtype, precision, latency):
    model, side = _model(family, dtype, precision, latency)
    images = _two_images()
    want = model.inference_images(_packed(images, BOXES), side)  # the route without the feature: a packed copy of every box (16: split 8 / 8)
    what = f"{family} {dtype} {precision} latency={latency}"
    _check_equal(model.inference_regions(_device(images), BOXES, side), want, what + " device")
    _check_equal(model.inference_regions(images, BOXES, side), want, what + " host")
    assert all(float(t.float().abs().max()) > 0 for t in want)
    assert not torch.equal(want[0], want[5]) and not torch.equal(want[10], want[11])
    if not latency:  # the default modes are batch-invariant: every region is inference() of its packed copy, and of its crop
        for r in (5, 9, 11):
            i, x1, y1, x2, y2 = BOXES[r]
            single = model.inference(_packed(images, [BOXES[r]])[0], side)
            assert torch.equal(_bits(want[r]), _bits(single))
            assert torch.equal(_bits(model.inference(images[i], side, crop=(slice(y1, y2), slice(x1, x2)))), _bits(single))


def test_taps_stay_inside_the_box():
    """Every pixel outside the box replaced by other random values: the region's map must not change by a bit (the antialias taps clip at the
    box's edges, as the reference's resize of the cropped array does) - for boxes that downscale (wide filters) and that upscale."""
    model, side = _model("v2", torch.bfloat16, None)
    images = _two_images()
    for region in (BOXES[5], BOXES[9], BOXES[11], BOXES[15], BOXES[1], BOXES[3]):
        i, x1, y1, x2, y2 = region
        other = np.random.default_rng(99).integers(0, 256, images[i].shape, dtype=np.uint8)
        other[y1:y2, x1:x2] = images[i][y1:y2, x1:x2]
        assert not np.array_equal(other, images[i])
        a = model.inference_regions([torch.from_numpy(images[i]).cuda()], [(0, x1, y1, x2, y2)], side)[0]
        b = model.inference_regions([torch.from_numpy(other).cuda()], [(0, x1, y1, x2, y2)], side)[0]
        c = model.inference_batch(torch.from_numpy(other).cuda()[None], side, crop=(slice(y1, y2), slice(x1, x2)))
        assert torch.equal(_bits(a), _bits(b)) and torch.equal(_bits(a), _bits(c)), region
        bicubic = [model.prepare_image_bgr(f, side, interpolation_mode="bicubic", crop=(slice(y1, y2), slice(x1, x2))) for f in (images[i], other)]
        assert torch.equal(_bits(bicubic[0]), _bits(bicubic[1]))


def _random_regions(shapes, n, rng, max_side):
    out = []
    for _ in range(n):
        i = int(rng.integers(0, len(shapes)))
        h, w = shapes[i]
        bw, bh = int(rng.integers(1, min(w, max_side) + 1)), int(rng.integers(1, min(h, max_side) + 1))
        x1, y1 = int(rng.integers(0, w - bw + 1)), int(rng.integers(0, h - bh + 1))
        out.append((i, x1, y1, x1 + bw, y1 + bh))
    return out


def test_batching_nine_regions_split_and_seventy_regions_in_two_tables():
    """9 regions (split 4 / 5: the second half starts at table entry 4) and 70 regions of mixed sizes from 3 images in one chunk: split 35 / 35,
    then unsplit, where the boxes go to the im2col kernel as two tables (64 + 6). Regions of one image overlap."""
    model, side = _model("v2", torch.bfloat16, None)
    images = [_image(SMALL_HW, 11), _image((240, 400), 13), _image((95, 64), 14)]
    shapes = [f.shape[:2] for f in images]
    rng = np.random.default_rng(7)
    nine = _random_regions(shapes, 9, rng, 300)
    want = model.inference_images(_packed(images, nine), side)
    _check_equal(model.inference_regions(_device(images), nine, side), want, "9 regions, device")
    _check_equal(model.inference_regions(images, nine, side), want, "9 regions, host")
    seventy = _random_regions(shapes, 66, rng, 200) + [(0, 10, 10, 110, 110), (0, 60, 60, 160, 160), (0, 10, 10, 110, 110), (0, 0, 0, 217, 333)]
    want = model.inference_images(_packed(images, seventy), side, True, 70)
    _check_equal(model.inference_regions(_device(images), seventy, side, True, 70), want, "70 regions, device")
    _check_equal(model.inference_regions(images, seventy, side, True, 70), want, "70 regions, host")
    assert torch.equal(_bits(want[66]), _bits(want[68])) and not torch.equal(_bits(want[66]), _bits(want[67]))
    eng = model._get_engine()
    native.check(eng.lib, eng.lib.mdpt_set_batch_split(eng.handle, 0))  # unsplit: all 70 boxes in one plan, 64 + 6 per im2col launch
    want = model.inference_images(_packed(images, seventy), side, True, 70)
    _check_equal(model.inference_regions(_device(images), seventy, side, True, 70), want, "70 regions, device, unsplit")
    _check_equal(model.inference_regions(images, seventy, side, True, 70), want, "70 regions, host, unsplit")


def test_aspect_sizing_gives_several_groups_and_one_call_per_chunk(monkeypatch):
    model, side = _model("v2", torch.float32, None)
    images = [_image(SMALL_HW, 11), _image((240, 400), 13)]
    regions = [(0, 0, 0, 217, 333), (1, 0, 0, 400, 240), (0, 10, 20, 110, 70), (1, 100, 40, 200, 90), (0, 33, 41, 160, 230), (1, 5, 5, 105, 205),
               (0, 3, 3, 103, 203), (1, 1, 1, 201, 101), (0, 50, 50, 150, 150)]
    eng = model._get_engine()
    calls = []
    real = eng.call_checked
    monkeypatch.setattr(eng, "call_checked", lambda fn_name, *a, **kw: (calls.append((fn_name, kw.get("batch"))), real(fn_name, *a, **kw))[1])
    pe = model.patch_embed
    for bs in (32, 2):
        plan = region_chunks(regions, lambda h, w: pe._scaled_hw(h, w, side, False), bs)
        assert len({hw for hw, _ in plan}) > 2
        for src in (images, _device(images)):
            calls.clear()
            got = model.inference_regions(src, regions, side, False, bs)
            assert calls == [("mdpt_forward_bgr_regions", len(idx)) for _, idx in plan]
            _check_equal(got, model.inference_images(_packed(images, regions), side, False, bs), f"aspect bs={bs}")
        assert len({tuple(t.shape) for t in got}) > 2


def test_crop_arguments_equal_the_packed_copies():
    model, side = _model("v2", torch.bfloat16, None)
    frames = np.random.default_rng(21).integers(0, 256, (5, 120, 200, 3), dtype=np.uint8)
    norm = ((0.1625, 0.2), (0.83, 0.95))  # 0.1625 * 200 = 32.5 -> x1 = 32
    ys, xs = crop_slices_from_norm(frames.shape[1:], norm)
    assert (xs.start, xs.stop, ys.start, ys.stop) == (32, 166, 24, 114)
    want = model.inference_batch(np.ascontiguousarray(frames[:, ys, xs]), side)
    for crop in (norm, (ys, xs)):
        for src in (frames, list(frames), tuple(frames), torch.from_numpy(frames).cuda(), torch.from_numpy(frames)):
            assert torch.equal(_bits(model.inference_batch(src, side, crop=crop)), _bits(want))
    want_aspect = model.inference_batch(np.ascontiguousarray(frames[:, ys, xs]), side, False)
    assert want_aspect.shape != want.shape
    assert torch.equal(_bits(model.inference_batch(torch.from_numpy(frames).cuda(), side, False, crop=norm)), _bits(want_aspect))
    # a crop that falls back to the full frame by the reference's rule, and crop=None, are today's call
    full = model.inference_batch(frames, side)
    assert torch.equal(_bits(model.inference_batch(frames, side, crop=((0.5, 0.5), (0.51, 0.52)))), _bits(full))
    assert torch.equal(_bits(model.inference_batch(frames, side, crop=None)), _bits(full))
    # inference_images: one crop per image (or None), and one for all
    images = [_image(SMALL_HW, 11), _image((240, 400), 13), _image((95, 64), 14), _image(LARGE_HW, 12)]
    crops = [((0.1, 0.2), (0.7, 0.9)), None, (slice(3, 90), slice(1, 64)), (slice(-1000, None), slice(1001, -23))]
    packed = [np.ascontiguousarray(images[0][crop_slices_from_norm(images[0].shape, crops[0])]), images[1], np.ascontiguousarray(images[2][crops[2]]),
              np.ascontiguousarray(images[3][crops[3]])]
    for square in (True, False):
        want = model.inference_images(packed, side, square, 3)
        _check_equal(model.inference_images(images, side, square, 3, crops=crops), want, "crops per image, host")
        _check_equal(model.inference_images(_device(images), side, square, 3, crops=crops), want, "crops per image, device")
    want = model.inference_images([np.ascontiguousarray(f[crop_slices_from_norm(f.shape, norm)]) for f in images], side)
    _check_equal(model.inference_images(images, side, crops=norm), want, "one crop for all, host")
    _check_equal(model.inference_images(_device(images), side, crops=norm), want, "one crop for all, device")
    # inference(crop=...)
    for f, c, pk in zip(images, crops, packed):
        assert torch.equal(_bits(model.inference(f, side, crop=c)), _bits(model.inference(pk, side)))
        assert torch.equal(_bits(model.inference(f, side, False, crop=c)), _bits(model.inference(pk, side, False)))


def test_sliced_device_views_are_read_in_place(monkeypatch):
    model, side = _model("v2", torch.float32, None)
    t = torch.from_numpy(np.random.default_rng(31).integers(0, 256, (6, 120, 200, 3), dtype=np.uint8)).cuda()
    eng = model._get_engine()
    calls = []
    real = eng.call_checked
    monkeypatch.setattr(eng, "call_checked", lambda fn_name, *a, **kw: (calls.append((fn_name, kw.get("batch"))), real(fn_name, *a, **kw))[1])
    for view in (t[:, 24:114, 33:166], t[1:, :, 33:], t[:, 7:, :], t[::2, 3:50, 1:2], t[:, ::2], t[:, 119:, 199:]):
        assert not view.is_contiguous()
        kept = _check_frames(view)[0]
        assert kept.data_ptr() == view.data_ptr() and kept.stride() == view.stride()  # no copy: the kernel gets the view's own pointer
        calls.clear()
        got = model.inference_batch(view, side)
        assert calls == [("mdpt_forward_bgr_pitched", view.shape[0])]  # one run, one call
        assert torch.equal(got, model.inference_batch(view.contiguous(), side))
        assert torch.equal(got, model.inference_batch(view.cpu().numpy(), side))
    # layouts the kernel cannot read are still copied: columns strided, rows and columns swapped
    for view in (t[:, :, ::2], t.transpose(1, 2)):
        kept = _check_frames(view)[0]
        assert kept.is_contiguous() and kept.data_ptr() != view.data_ptr()
        assert torch.equal(model.inference_batch(view, side), model.inference_batch(view.contiguous(), side))
    calls.clear()
    model.inference_batch(t, side)
    assert calls == [("mdpt_forward_bgr_batch", 6)]  # a packed tensor goes the way it went
    # the image list of inference_images / inference_regions
    views = [t[0, 24:114, 33:166], t[1, :, 5:], t[2], t[3, 100:101, :]]
    kept, on_device = _check_images(views, 32)
    assert on_device and all(k.data_ptr() == v.data_ptr() for k, v in zip(kept, views))
    got = model.inference_images(views, side)
    want = model.inference_images([v.contiguous() for v in views], side)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    got = model.inference_regions(views, [(0, 1, 2, 100, 80), (1, 0, 0, 195, 120), (3, 7, 0, 150, 1)], side)
    want = model.inference_regions([v.contiguous() for v in views], [(0, 1, 2, 100, 80), (1, 0, 0, 195, 120), (3, 7, 0, 150, 1)], side)
    for a, b in zip(got, want):
        assert torch.equal(a, b)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_standalone_prepare_on_a_box_equals_prepare_on_the_packed_copy(dtype):
    model, side = _model("v2", dtype, None)
    images = _two_images()
    pe = model.patch_embed
    lib = native.load()
    for region in (BOXES[5], BOXES[3], BOXES[6], BOXES[9], BOXES[11], BOXES[14], BOXES[15]):
        i, x1, y1, x2, y2 = region
        packed = _packed(images, [region])[0]
        crop = (slice(y1, y2), slice(x1, x2))
        for mode, interp in (("bilinear", native.INTERP_BILINEAR), ("bicubic", native.INTERP_BICUBIC)):
            for square in (True, False):
                want = model.prepare_image_bgr(packed, side, square, mode)
                assert torch.equal(_bits(model.prepare_image_bgr(images[i], side, square, mode, crop=crop)), _bits(want)), (region, mode)
                assert torch.equal(_bits(pe.prepare_image(images[i], side, square, mode, crop=crop)), _bits(want)), (region, mode)
            # the pitch-and-box form of the C entry point on the image where it lies on the device
            dev = _device(images)[i]
            out = torch.empty_like(want)
            mean3, std3 = pe._norm_constants()
            box = (ctypes.c_int32 * 4)(x1, y1, x2, y2)
            for pitch in (0, 3 * dev.shape[1]):
                out.zero_()
                native.check(lib, lib.mdpt_prepare_image_region(dev.data_ptr(), dev.shape[0], dev.shape[1], pitch, box, out.data_ptr(), native.dtype_code(dtype),
                                                                want.shape[2], want.shape[3], mean3, std3, interp, torch.cuda.current_stream().cuda_stream))
                assert torch.equal(_bits(out), _bits(want)), (region, mode, pitch)
    norm = ((0.1, 0.2), (0.7, 0.9))
    want = model.prepare_image_bgr(np.ascontiguousarray(images[0][crop_slices_from_norm(images[0].shape, norm)]), side)
    assert torch.equal(_bits(model.prepare_image_bgr(images[0], side, crop=norm)), _bits(want))


def test_listening_block_hook_takes_the_stage_route_on_the_cropped_tensor():
    from muggled_dpt_amd.dpt_model import TransformerBlock
    model, side = _model("v2", torch.float32, None)
    images = [_image(SMALL_HW, 11), _image((240, 400), 13)]
    regions = [(0, 33, 41, 160, 230), (1, 100, 40, 200, 90), (0, 0, 0, 217, 333), (1, 399, 239, 400, 240), (0, 10, 20, 110, 70)]
    frames = torch.from_numpy(np.random.default_rng(41).integers(0, 256, (3, 120, 200, 3), dtype=np.uint8)).cuda()
    crop = (slice(24, 114), slice(33, 166))
    want = model.inference_regions(_device(images), regions, side, True, 3)
    want_batch = model.inference_batch(frames, side, crop=crop)
    block = [m for m in model.modules() if isinstance(m, TransformerBlock)][1]
    seen = []
    handle = block.register_forward_hook(lambda m, a, out: seen.append(tuple(out.shape)))
    try:
        got_dev = model.inference_regions(_device(images), regions, side, True, 3)
        got_host = model.inference_regions(images, regions, side, True, 3)
        got_batch = model.inference_batch(frames, side, crop=crop)
        got_batch_host = model.inference_batch(frames.cpu().numpy(), side, crop=crop)
        got_images = model.inference_images(_device(images), side, crops=[(slice(41, 230), slice(33, 160)), None])
        got_one = model.inference(images[0], side, crop=(slice(41, 230), slice(33, 160)))
    finally:
        handle.remove()
    assert [s[0] for s in seen] == [3, 2, 3, 2, 3, 3, 2, 1]  # the hook fired once per chunk: the stage-by-stage route ran
    _check_equal(got_dev, want, "hooked, device")
    _check_equal(got_host, want, "hooked, host")
    assert torch.equal(got_batch, want_batch) and torch.equal(got_batch_host, want_batch)
    assert torch.equal(got_images[0], want[0]) and torch.equal(got_one, want[0])
