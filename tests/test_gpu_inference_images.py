"""DPTModel.inference_images / mdpt_forward_bgr_frames: a list of uint8 images of ANY sizes in, a list of [1,H_i,W_i] maps out, one batched forward
per chunk of images that share a model tensor size, the fused resize + normalise + im2col kernel reading every frame from its own place with
its own size. Element i has to equal model(torch.cat([prepare_image_bgr(f) for f in its chunk]))[its row] bit for bit in every family, dtype and
arithmetic mode (latency mode included), for square sizing (one group for any mix of sizes) and aspect sizing (a few groups), for sources from
1x1 to 3024x4032, for chunks the forward splits across two streams (9 and 11 images) and for a chunk larger than one frame table (70 > 64)."""
import numpy as np
import pytest
import torch

from muggled_dpt_amd.dpt_model import image_chunks
from tests.test_gpu_c_host import _family_model

pytestmark = pytest.mark.gpu

CASES = [("v2", torch.float32, None), ("v2", torch.bfloat16, None), ("v2", torch.float32, "mixed"), ("v1", torch.float16, None),
         ("beit", torch.bfloat16, None), ("beit", torch.float32, "bf16x3"), ("swinv2", torch.float32, "mixed"), ("swinv2", torch.bfloat16, None)]

# (h, w) of the sources: 11 images, tiny to a 12 MP photo in both orientations
SIZES = [(61, 90), (1, 1), (4032, 3024), (333, 217), (95, 64), (120, 200), (720, 1280), (3, 7), (480, 640), (3024, 4032), (217, 333)]
# aspect sizing on the Swin V2 model: sources whose tensor sizes its windows take (the sizes test_gpu_inference_batch.py runs), in two groups
SWIN_ASPECT_SIZES = [(333, 217), (120, 200), (4032, 3024), (660, 434), (240, 400), (999, 651), (60, 100), (333, 217), (120, 200)]


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


_IMAGE_CACHE = {}


def _images(sizes, seed):
    out = []
    for k, hw in enumerate(sizes):
        key = (hw, seed + k)
        if key not in _IMAGE_CACHE:
            _IMAGE_CACHE[key] = np.random.default_rng(seed + k).integers(0, 256, (*hw, 3), dtype=np.uint8)
        out.append(_IMAGE_CACHE[key])
    return out


def _two_step_chunks(model, images, side, square, batch_size):
    """element i from model(torch.cat([prepare_image_bgr(f) for f in its chunk])), chunks as inference_images plans them"""
    pe = model.patch_embed
    out = [None] * len(images)
    with torch.inference_mode():
        for _, idx in image_chunks([f.shape[:2] for f in images], lambda h, w: pe._scaled_hw(h, w, side, square), batch_size):
            y = model(torch.cat([model.prepare_image_bgr(images[i], side, square) for i in idx]))
            for k, i in enumerate(idx):
                out[i] = y[k:k + 1]
    return out


def _check_equal(got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dim() == 3 and g.shape[0] == 1 and g.dtype == w.dtype, f"{what}: image {i} {g.shape} {w.shape}"
        assert torch.equal(_bits(g), _bits(w)), f"{what}: image {i} differs from prepare + cat + forward"


@pytest.mark.parametrize("family,dtype,precision,latency", [c + (False,) for c in CASES] + [("v2", torch.bfloat16, None, True)])
def test_inference_images_equals_prepare_cat_forward_per_chunk_bit_for_bit(family, dtype, precision, latency):
    model, side = _model(family, dtype, precision, latency)
    images = _images(SIZES, seed=100)
    # square sizing: one group; 11 images in one chunk (split 5 / 6 across two streams), and chunks of 4, 4, 3
    for bs in (32, 4):
        y = model.inference_images(images, side, True, bs)
        _check_equal(y, _two_step_chunks(model, images, side, True, bs), f"{family} {dtype} {precision} latency={latency} square bs={bs}")
        assert len({tuple(t.shape) for t in y}) == 1
        assert all(float(t.float().abs().max()) > 0 for t in y)
        assert not torch.equal(y[0], y[3])  # different images, different maps (every frame reaches the kernel from its own place)
    # aspect sizing: several groups, each cut into chunks
    aspect = _images(SWIN_ASPECT_SIZES, seed=200) if family == "swinv2" else images
    for bs in (32, 2):
        y = model.inference_images(aspect, side, False, bs)
        _check_equal(y, _two_step_chunks(model, aspect, side, False, bs), f"{family} {dtype} {precision} latency={latency} aspect bs={bs}")
        assert len({tuple(t.shape) for t in y}) > 1


def test_inference_images_group_of_nine_splits_and_more_images_than_one_frame_table():
    """A square-sized chunk of 9 (split 4 / 5: the second half starts at table entry 4) and one of 70 mixed sizes: split 35 / 35, then
    unsplit, where its frames go to the im2col kernel as two frame tables (64 + 6)."""
    model, side = _model("v2", torch.bfloat16, None)
    rng = np.random.default_rng(9)
    sizes9 = [(int(rng.integers(1, 300)), int(rng.integers(1, 300))) for _ in range(9)]
    images9 = _images(sizes9, seed=300)
    _check_equal(model.inference_images(images9, side), _two_step_chunks(model, images9, side, True, 32), "square, 9 images")
    sizes70 = [(int(rng.integers(1, 200)), int(rng.integers(1, 200))) for _ in range(70)]
    images70 = _images(sizes70, seed=400)
    y = model.inference_images(images70, side, True, 70)
    _check_equal(y, _two_step_chunks(model, images70, side, True, 70), "square, 70 images in one chunk")
    from muggled_dpt_amd import native
    eng = model._get_engine()
    native.check(eng.lib, eng.lib.mdpt_set_batch_split(eng.handle, 0))  # unsplit: all 70 frames in one plan, 64 + 6 frames per im2col launch
    y1 = model.inference_images(images70, side, True, 70)
    _check_equal(y1, _two_step_chunks(model, images70, side, True, 70), "square, 70 images, unsplit")


@pytest.mark.parametrize("family,dtype,precision", CASES)
def test_inference_images_equal_per_image_inference(family, dtype, precision):
    """The default modes are batch-invariant: every element equals inference() of that image alone."""
    model, side = _model(family, dtype, precision)
    images = _images(SIZES, seed=500)
    y = model.inference_images(images, side)
    for i, f in enumerate(images):
        assert torch.equal(_bits(y[i]), _bits(model.inference(f, side))), f"{family} {dtype} {precision}: image {i} differs from inference()"
    aspect = _images(SWIN_ASPECT_SIZES, seed=600) if family == "swinv2" else images
    y = model.inference_images(aspect, side, False, 3)
    for i, f in enumerate(aspect):
        assert torch.equal(_bits(y[i]), _bits(model.inference(f, side, False))), f"{family} {dtype} {precision}: aspect image {i} differs"


def test_device_tensor_input_equals_host_input():
    model, side = _model("v2", torch.bfloat16, None)
    images = _images(SIZES, seed=700)
    for square in (True, False):
        y_host = model.inference_images(images, side, square, 5)
        y_tuple = model.inference_images(tuple(images), side, square, 5)
        y_dev = model.inference_images([torch.from_numpy(f).cuda() for f in images], side, square, 5)
        for a, b, c in zip(y_host, y_tuple, y_dev):
            assert torch.equal(_bits(a), _bits(b)) and torch.equal(_bits(a), _bits(c))
    # non-contiguous views are staged (host) or made contiguous (device) like contiguous images
    wide = [np.concatenate([f, f], axis=1) for f in images[:4]]
    views = [w[:, : f.shape[1]] for w, f in zip(wide, images[:4])]
    want = model.inference_images(images[:4], side)
    for got in (model.inference_images(views, side), model.inference_images([torch.from_numpy(w).cuda()[:, : f.shape[1]] for w, f in zip(wide, images)], side)):
        for a, b in zip(got, want):
            assert torch.equal(_bits(a), _bits(b))


def test_inference_images_with_listening_hooks_takes_the_stage_route():
    from torch import nn
    from muggled_dpt_amd import make_depthanythingv2_dpt_from_original_state_dict
    from muggled_dpt_amd.synthetic import make_synthetic_original_state_dict
    _, model = make_depthanythingv2_dpt_from_original_state_dict(make_synthetic_original_state_dict("tiny", 0), enable_optimizations=False)
    model = model.to("cuda", torch.float32)
    images = _images(SIZES[:5], seed=800)
    y = model.inference_images(images, 112, True, 3)
    softmaxes = [m for m in model.modules() if isinstance(m, nn.Softmax)]
    assert softmaxes
    seen = {i: [] for i in range(len(softmaxes))}
    handles = [m.register_forward_hook(lambda m, a, out, i=i: seen[i].append(tuple(out.shape))) for i, m in enumerate(softmaxes)]
    try:
        y_hooked = model.inference_images(images, 112, True, 3)
        y_dev = model.inference_images([torch.from_numpy(f).cuda() for f in images], 112, True, 3)
    finally:
        for hd in handles:
            hd.remove()
    assert all(len(v) == 4 for v in seen.values()), "every block's hook fires once per chunk (3 + 2 images, two calls)"
    assert all([s[0] for s in v] == [3, 2, 3, 2] for v in seen.values())
    for a, b, c in zip(y, y_hooked, y_dev):
        assert torch.equal(a, b) and torch.equal(a, c)


def test_one_forward_call_per_chunk(monkeypatch):
    model, side = _model("v2", torch.float32, None)
    eng = model._get_engine()
    calls = []
    real = eng.call_checked

    def counting(fn_name, *args, **kw):
        calls.append((fn_name, kw.get("batch")))
        return real(fn_name, *args, **kw)

    monkeypatch.setattr(eng, "call_checked", counting)
    images = _images(SIZES, seed=900)
    model.inference_images(images, side)  # square: 11 mixed sizes, one tensor size
    assert calls == [("mdpt_forward_bgr_frames", 11)]
    calls.clear()
    pe = model.patch_embed
    for bs in (32, 2):
        model.inference_images(images, side, False, bs)
        plan = image_chunks([f.shape[:2] for f in images], lambda h, w: pe._scaled_hw(h, w, side, False), bs)
        assert len(plan) > 2
        assert calls == [("mdpt_forward_bgr_frames", len(idx)) for _, idx in plan]
        calls.clear()


def test_inference_images_full_size_vitl_bf16():
    """The bench's model at its default size (518 -> 504 square), on photo-sized sources: every element equals inference() of its image."""
    from muggled_dpt_amd import make_depthanythingv2_dpt_from_original_state_dict
    from muggled_dpt_amd.synthetic import make_synthetic_original_state_dict
    _, model = make_depthanythingv2_dpt_from_original_state_dict(make_synthetic_original_state_dict("vitl", 0))
    model = model.to("cuda", torch.bfloat16)
    images = _images([(480, 640), (720, 1280), (1080, 1920), (1920, 1080), (4032, 3024), (800, 800), (480, 640), (1080, 1920), (800, 800)], seed=1000)
    y = model.inference_images(images)
    for i, f in enumerate(images):
        assert y[i].shape == (1, 504, 504)
        assert torch.equal(_bits(y[i]), _bits(model.inference(f)))
    y = model.inference_images(images, use_square_sizing=False)
    for i, f in enumerate(images):
        assert torch.equal(_bits(y[i]), _bits(model.inference(f, use_square_sizing=False)))
