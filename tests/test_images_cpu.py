"""Inference and display for images of different sizes, the parts that need no GPU: the new C entry points are exported and bound and refuse
null arguments on the host, DPTModel.inference_images checks its arguments before anything touches a device, and the forward plan
(image_chunks) groups images by the reference's size rule, keeps their order and cuts groups into chunks."""
import ctypes

import numpy as np
import pytest
import torch

from muggled_dpt_amd import native
from muggled_dpt_amd import postprocess as pp
from muggled_dpt_amd.dpt_model import image_chunks

NEW_SYMBOLS = ("mdpt_forward_bgr_frames", "mdpt_post_minmax_images", "mdpt_post_u8_hist_images", "mdpt_post_colorize_images")


def test_new_entry_points_are_exported_and_bound():
    lib = native.load()
    for name in NEW_SYMBOLS:
        assert name in native.SYMBOLS, f"{name} is not in native.SYMBOLS"
        assert hasattr(lib, name), f"libmdpt.so does not export {name}"
    assert lib.mdpt_abi_version() == 6  # additive: the ABI version stays
    assert native.BGR_RUNS == 64 and native.POST_RUNS == 32


def test_forward_bgr_frames_rejects_bad_arguments_on_the_host():
    lib = native.load()
    m3 = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    hw = (ctypes.c_int32 * 4)(8, 8, 9, 7)
    ptrs = (ctypes.c_void_p * 2)(None, None)
    # a null handle / table fails before any device work, with mdpt_forward_bgr_batch's code
    assert lib.mdpt_forward_bgr_frames(None, None, None, 2, 0, 28, 28, m3, m3, 0, None, 0, None, 0, None) == -1
    assert lib.mdpt_forward_bgr_frames(None, ctypes.addressof(ptrs), ctypes.addressof(hw), 2, 0, 28, 28, m3, m3, 0, None, 0, None, 0, None) == -1
    assert lib.mdpt_forward_bgr_batch(None, None, 2, 8, 8, 0, 28, 28, m3, m3, 0, None, 0, None, 0, None) == -1
    assert lib.mdpt_post_minmax_images(None, None, 0, 1, None, None, None, None, None) == -1
    assert lib.mdpt_post_u8_hist_images(None, None, 0, 1, None, 0, None, None, None) == -1
    assert lib.mdpt_post_colorize_images(None, None, 1, None, None, 3, None, None) == -1


@pytest.fixture(scope="module")
def cpu_model():
    from muggled_dpt_amd import make_depthanythingv2_dpt_from_original_state_dict
    from muggled_dpt_amd.synthetic import make_synthetic_original_state_dict
    return make_depthanythingv2_dpt_from_original_state_dict(make_synthetic_original_state_dict("tiny", 0))[1]


def test_inference_images_argument_errors_come_before_any_device_work(cpu_model):
    f = np.zeros((20, 30, 3), np.uint8)
    g = np.zeros((41, 17, 3), np.uint8)
    for bad in ([], ()):
        with pytest.raises(ValueError):
            cpu_model.inference_images(bad)
    with pytest.raises(ValueError):
        cpu_model.inference_images([f, np.zeros((0, 30, 3), np.uint8)])
    for bs in (0, -3):
        with pytest.raises(ValueError):
            cpu_model.inference_images([f, g], batch_size=bs)
    with pytest.raises(TypeError):
        cpu_model.inference_images([f, g], batch_size=2.0)
    for bad in ([f.astype(np.float32)], [f[..., :2]], [f[..., 0]], [f, "image"], f, np.stack([f, f]), torch.zeros((2, 20, 30, 3), dtype=torch.uint8),
                [torch.zeros((20, 30, 3), dtype=torch.uint8)], "images"):
        with pytest.raises(TypeError):
            cpu_model.inference_images(bad)
    # host arrays and device tensors do not mix (the tensor item is checked on the host, it never needs a device here)
    with pytest.raises(TypeError, match="mix"):
        cpu_model.inference_images([f, torch.zeros((20, 30, 3), dtype=torch.uint8)])
    # a well-formed list of different sizes on a CPU model: the same RuntimeError prepare_image raises
    for good in ([f, g], (g, f, f)):
        with pytest.raises(RuntimeError, match="GPU only"):
            cpu_model.inference_images(good)
    # inference_batch still refuses mixed sizes
    with pytest.raises(ValueError):
        cpu_model.inference_batch([f, g])


SIZES = [(480, 640), (720, 1280), (1080, 1920), (1920, 1080), (4032, 3024), (800, 800), (1, 1), (61, 90), (90, 61), (333, 217), (3, 5000)]


def test_square_sizing_gives_one_group_for_any_mix_of_sizes(cpu_model):
    pe = cpu_model.patch_embed
    rule = lambda h, w: pe._scaled_hw(h, w, 252, True)  # noqa: E731
    chunks = image_chunks(SIZES, rule, 32)
    assert len(chunks) == 1
    (hw, idx), = chunks
    assert hw == tuple(rule(7, 9)) and hw[0] == hw[1] and idx == list(range(len(SIZES)))
    # cut into chunks of batch_size, order kept
    chunks = image_chunks(SIZES, rule, 4)
    assert [idx for _, idx in chunks] == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10]]
    assert {hw for hw, _ in chunks} == {hw}
    assert [idx for _, idx in image_chunks(SIZES, rule, 1)] == [[i] for i in range(len(SIZES))]


def test_aspect_sizing_groups_by_the_size_rule_in_order_of_first_appearance(cpu_model):
    pe = cpu_model.patch_embed
    rule = lambda h, w: tuple(pe._scaled_hw(h, w, 252, False))  # noqa: E731
    sizes = SIZES + [(480, 640), (1080, 1920), (481, 641), (640, 480), (720, 1280)] * 2
    for bs in (1, 2, 3, 32):
        chunks = image_chunks(sizes, rule, bs)
        assert sorted(i for _, idx in chunks for i in idx) == list(range(len(sizes)))  # every image exactly once
        seen = []
        for hw, idx in chunks:
            assert 1 <= len(idx) <= bs and idx == sorted(idx)
            assert all(rule(*sizes[i]) == hw for i in idx)  # one tensor size per chunk
            if hw not in seen:
                seen.append(hw)
            else:
                assert seen[-1] == hw  # a group's chunks are consecutive
        # groups in order of first appearance, each holding every image of its tensor size
        first = []
        for s in sizes:
            if rule(*s) not in first:
                first.append(rule(*s))
        assert seen == first
        for hw in first:
            assert [i for h, idx in chunks if h == hw for i in idx] == [i for i, s in enumerate(sizes) if rule(*s) == hw]
    assert len(image_chunks(sizes, rule, 32)) == len(first) > 1


def test_display_images_refuse_host_tensors():
    x = torch.zeros((1, 8, 8))
    with pytest.raises(RuntimeError):
        pp.scale_prediction_images([x], [(4, 4)])
    with pytest.raises(RuntimeError):
        pp.depth_to_color_images([x, torch.zeros((5, 7))])
    with pytest.raises(ValueError):
        pp.depth_to_color_images([])
    with pytest.raises(TypeError):
        pp.depth_to_color_images([np.zeros((4, 4), np.float32)])
