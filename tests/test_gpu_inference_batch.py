"""DPTModel.inference_batch / mdpt_forward_bgr_batch: B uint8 frames of one size in, [B,H,W] depth out, the fused resize + normalise + im2col
kernel taking the frame index. Row b has to equal model(torch.cat([prepare_image_bgr(frame) for frame in frames]))[b] bit for bit in every
family, dtype and arithmetic mode (latency mode included), for an unsplit batch (3) and one the forward splits across two streams (9 = 4 + 5:
the second half's frames start 4 frames into the source)."""
import numpy as np
import pytest
import torch

from tests.test_gpu_c_host import _family_model

pytestmark = pytest.mark.gpu

CASES = [("v2", torch.float32, None), ("v2", torch.bfloat16, None), ("v2", torch.float32, "mixed"), ("v1", torch.float16, None),
         ("beit", torch.bfloat16, None), ("beit", torch.float32, "bf16x3"), ("swinv2", torch.float32, "mixed"), ("swinv2", torch.bfloat16, None)]


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


def _frames(b, hw, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (*hw, 3), dtype=np.uint8) for _ in range(b)]


def _two_step(model, frames, max_side, square):
    with torch.inference_mode():
        return model(torch.cat([model.prepare_image_bgr(f, max_side, square) for f in frames]))


@pytest.mark.parametrize("family,dtype,precision,latency", [c + (False,) for c in CASES] + [("v2", torch.bfloat16, None, True)])
def test_inference_batch_equals_prepare_cat_forward_bit_for_bit(family, dtype, precision, latency):
    model, side = _model(family, dtype, precision, latency)
    for b, (ih, iw), square in ((3, (61, 90), True), (3, (333, 217), False), (9, (95, 64), True), (9, (120, 200), False)):
        frames = _frames(b, (ih, iw), seed=b * 1000 + ih)
        y = model.inference_batch(frames, side, square)
        y2 = _two_step(model, frames, side, square)
        assert y.shape == y2.shape and y.shape[0] == b and y.dtype == y2.dtype == dtype
        assert torch.equal(_bits(y), _bits(y2)), f"{family} {dtype} {precision} latency={latency} B={b} {ih}x{iw}: batched and two-step routes differ"
        assert all(float(y[i].float().abs().max()) > 0 for i in range(b))
        assert not torch.equal(y[0], y[1])  # different frames, different maps (the frame index reaches the kernel)


@pytest.mark.parametrize("family,dtype,precision", CASES)
def test_inference_batch_rows_equal_per_frame_inference(family, dtype, precision):
    """The default mode is batch-invariant: every row of a batch equals inference() of that frame alone."""
    model, side = _model(family, dtype, precision)
    for b, square in ((3, True), (9, False)):
        frames = _frames(b, (70, 101), seed=b)
        y = model.inference_batch(frames, side, square)
        for i, f in enumerate(frames):
            yi = model.inference(f, side, square)
            assert torch.equal(_bits(y[i:i + 1]), _bits(yi)), f"{family} {dtype} {precision} B={b}: row {i} differs from inference()"


def test_inference_batch_input_forms_agree():
    model, side = _model("v2", torch.bfloat16, None)
    frames = _frames(9, (77, 64), seed=5)
    y_list = model.inference_batch(frames, side)
    y_tuple = model.inference_batch(tuple(frames), side)
    y_np = model.inference_batch(np.stack(frames), side)
    dev = torch.from_numpy(np.stack(frames)).to("cuda")
    y_dev = model.inference_batch(dev, side)
    y_cpu_tensor = model.inference_batch(torch.from_numpy(np.stack(frames)), side)
    for y in (y_tuple, y_np, y_dev, y_cpu_tensor):
        assert torch.equal(_bits(y), _bits(y_list))
    # a non-contiguous view of host frames is staged like a contiguous one
    big = np.stack([np.concatenate([f, f], axis=1) for f in frames])
    assert torch.equal(_bits(model.inference_batch(big[:, :, :64], side)), _bits(y_list))


def test_inference_batch_with_listening_hooks_takes_the_stage_route():
    from torch import nn
    from muggled_dpt_amd import make_depthanythingv2_dpt_from_original_state_dict
    from muggled_dpt_amd.synthetic import make_synthetic_original_state_dict
    _, model = make_depthanythingv2_dpt_from_original_state_dict(make_synthetic_original_state_dict("tiny", 0), enable_optimizations=False)
    model = model.to("cuda", torch.float32)
    frames = _frames(3, (100, 140), seed=4)
    y = model.inference_batch(frames, 112)
    softmaxes = [m for m in model.modules() if isinstance(m, nn.Softmax)]
    assert softmaxes
    seen = {i: [] for i in range(len(softmaxes))}
    handles = [m.register_forward_hook(lambda m, a, out, i=i: seen[i].append(tuple(out.shape))) for i, m in enumerate(softmaxes)]
    try:
        y_hooked = model.inference_batch(frames, 112)
        y_dev = model.inference_batch(torch.from_numpy(np.stack(frames)).cuda(), 112)
    finally:
        for hd in handles:
            hd.remove()
    assert all(len(v) == 2 for v in seen.values()), "every block's hook fires once per call"
    assert all(v[0][0] == 3 for v in seen.values())
    assert torch.equal(y, y_hooked) and torch.equal(y, y_dev)


def test_inference_batch_full_size_vitl_bf16():
    """The bench's model and batch from uint8 frames: ViT-L bf16, 32 frames of 518 x 518 (split 16 / 16)."""
    from muggled_dpt_amd import make_depthanythingv2_dpt_from_original_state_dict
    from muggled_dpt_amd.synthetic import make_synthetic_original_state_dict
    _, model = make_depthanythingv2_dpt_from_original_state_dict(make_synthetic_original_state_dict("vitl", 0))
    model = model.to("cuda", torch.bfloat16)
    frames = _frames(32, (518, 518), seed=11)
    y = model.inference_batch(frames)
    y2 = _two_step(model, frames, None, True)
    assert y.shape == y2.shape and y.shape[0] == 32
    assert torch.equal(_bits(y), _bits(y2))
    for i in (0, 13, 31):
        assert torch.equal(_bits(y[i:i + 1]), _bits(model.inference(frames[i])))


def test_forward_bgr_batch_rejects_bad_arguments():
    import ctypes
    from muggled_dpt_amd import native
    model, unit = _family_model("v2")
    model = model.to("cuda", torch.float32)
    eng = model._get_engine()
    lib = native.load()
    img = torch.zeros((2, 32, 32, 3), dtype=torch.uint8, device="cuda")
    out = torch.empty((2, 2 * unit, 2 * unit), device="cuda")
    m3, s3 = (ctypes.c_float * 3)(0.5, 0.5, 0.5), (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    ws_ptr, ws_bytes = eng.workspace(2, (2 * unit, 2 * unit))
    args = lambda **kw: [eng.handle, img.data_ptr(), kw.get("b", 2), 32, 32, native.dtype_code(torch.float32), 2 * unit, 2 * unit, m3, s3,
                         kw.get("interp", native.INTERP_BILINEAR), out.data_ptr(), native.dtype_code(torch.float32), ws_ptr, ws_bytes, None]
    assert lib.mdpt_forward_bgr_batch(*args()) == 0
    assert lib.mdpt_forward_bgr_batch(*args(b=0)) == -1
    assert lib.mdpt_forward_bgr_batch(*args(interp=5)) == -6
    torch.cuda.synchronize()
