"""Photo-guided upsampling on the device (postprocess.guided_upsample_images -> mdpt_post_guided_upsample, csrc/postprocess.hip guided_* kernels)
against the fp64 restatement tests/guided_restate.py, which is written from the definition (window slices, np.linalg.solve) and not from the kernels'
row / column sums and Cholesky solve.

Bounds. Output: |q_dev - q_restated| <= 2^-23 max|p|, one fp32 ulp at the map's maximum - the single rounding to fp32 costs half an ulp, and the fp64
noise amplified by Sigma's condition number <= (0.75 + eps) / eps stays far below the other half: on the shapes and data of CASES the restatement
differs from its own np.longdouble run by at most 3.3e-6 of that ulp before the rounding (measured on a CPU; worst at 5 x 7 radius 1, eps 1e-4; after
the rounding the two agree exactly on six cases, and on the 451 x 485 pixels of the radius 0 case differ where a value sits on a rounding boundary).
Coefficients: the restatement differs from its np.longdouble run by at most COEF_NOISE = 3.19e-11 on these shapes and data (measured on a CPU:
3.19e-11 at 5 x 7 radius 1, 8.5e-12 at 37 x 29 radius 4, 2.7e-12 at 24 x 24 radius 8, below 4e-13 on the rest); the device, with another equally valid
summation order and solve, must stay within 16 x that, 5.1e-10. No test here uses an eps below 1e-4 under these bounds."""
import functools

import numpy as np
import pytest
import torch

from muggled_dpt_amd import postprocess as pp
from tests import guided_restate as gr

pytestmark = pytest.mark.gpu

# (map h x w, photo H x W, radius, eps)
CASES = [((5, 7), (13, 17), 1, 1e-4), ((5, 7), (13, 17), 3, 1e-4), ((5, 7), (13, 17), 9, 1e-4), ((16, 16), (16, 16), 2, 1e-2),
         ((37, 29), (300, 211), 4, 1e-4), ((24, 24), (100, 90), 8, 1e-4), ((64, 80), (64 * 7 + 3, 80 * 6 + 5), 0, 1e-4)]
COEF_NOISE = 3.19e-11


def make_case(case, dtype=np.float32):
    """-> (map fp32 holding values of `dtype`'s grid scaled to 0 .. 50, photo uint8): seeded by the shapes, so every test sees the same data"""
    (h, w), (H, W), radius, _ = case
    rng = np.random.default_rng(1000 * h + 10 * W + radius)
    p = torch.from_numpy(rng.uniform(0.0, 50.0, (h, w)).astype(np.float32))
    if dtype is not np.float32:
        p = p.to(dtype).to(torch.float32)
    return p.numpy(), rng.integers(0, 256, (H, W, 3), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def restated(index: int, dtype=np.float32):
    """the restatement of CASES[index], computed once and shared (read only)"""
    p, photo = make_case(CASES[index], dtype)
    q, mean, _ = gr.guided_upsample(p, photo, CASES[index][2], CASES[index][3])
    for a in (p, photo, q, mean):
        a.setflags(write=False)
    return p, photo, q, mean


def _run(p, photo, radius, eps, dtype=torch.float32, device_photo=True, coefficients=True):
    maps = [torch.from_numpy(np.array(p)).to("cuda", dtype)[None]]
    photos = [torch.from_numpy(np.array(photo)).cuda() if device_photo else photo]
    return pp.guided_upsample_images(maps, photos, radius, eps, return_coefficients=coefficients)


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32 if t.dtype == torch.float32 else np.uint64)


@pytest.mark.parametrize("index", range(len(CASES)))
def test_output_and_coefficients_match_the_restatement(index):
    (h, w), (H, W), radius, eps = CASES[index]
    p, photo, q, mean = restated(index)
    out, coef = _run(p, photo, radius, eps)
    assert out[0].shape == (1, H, W) and out[0].dtype == torch.float32 and coef[0].shape == (h, w, 4) and coef[0].dtype == torch.float64
    got, got_c = out[0][0].cpu().numpy(), coef[0].cpu().numpy()
    ulp = 2.0 ** -23 * float(np.abs(p).max())
    dq, dc = float(np.abs(got.astype(np.float64) - q.astype(np.float64)).max()), float(np.abs(got_c - mean).max())
    print(f"guided {h}x{w} -> {H}x{W} r{radius} eps {eps:g}: |q - restated| = {dq / ulp:.3f} ulp, |coef - restated| = {dc:.3e}")
    assert np.isfinite(got).all()
    assert dq <= ulp
    assert dc <= 16 * COEF_NOISE
    if radius == 0:  # a = 0 exactly, and the map comes back as its bilinear resize
        assert not got_c[..., :3].any() and np.array_equal(got_c[..., 3], p.astype(np.float64))
        assert np.array_equal(got, gr.bilinear_resize(p, H, W).astype(np.float32))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("index", [1, 4])
def test_16_bit_maps_are_read_as_they_are(index, dtype):
    _, _, radius, eps = CASES[index]
    p, photo, q, mean = restated(index, dtype)
    out, coef = _run(p, photo, radius, eps, dtype)
    ulp = 2.0 ** -23 * float(np.abs(p).max())
    assert out[0].dtype == torch.float32
    assert float(np.abs(out[0][0].cpu().numpy().astype(np.float64) - q.astype(np.float64)).max()) <= ulp
    assert float(np.abs(coef[0].cpu().numpy() - mean).max()) <= 16 * COEF_NOISE


def test_pairs_of_different_sizes_share_one_call_and_a_second_call_repeats_it():
    picks = [4, 1, 5]  # 37x29 -> 300x211, 5x7 -> 13x17, 24x24 -> 100x90, all at radius 3
    data = [restated(k)[:2] for k in picks]
    maps = [torch.from_numpy(p.copy()).cuda()[None] for p, _ in data]
    photos = [torch.from_numpy(f.copy()).cuda() for _, f in data]
    out, coef = pp.guided_upsample_images(maps, photos, 3, 1e-4, return_coefficients=True)
    again, coef2 = pp.guided_upsample_images(maps, photos, 3, 1e-4, return_coefficients=True)
    for k in range(3):
        alone, alone_c = pp.guided_upsample_images(maps[k:k + 1], photos[k:k + 1], 3, 1e-4, return_coefficients=True)
        assert out[k].shape == (1, *data[k][1].shape[:2])
        assert np.array_equal(_bits(out[k]), _bits(alone[0])) and np.array_equal(_bits(coef[k]), _bits(alone_c[0]))
        assert np.array_equal(_bits(out[k]), _bits(again[k])) and np.array_equal(_bits(coef[k]), _bits(coef2[k]))
    plain = pp.guided_upsample_images(torch.cat(maps[1:2] * 2), photos[1:2] * 2, 3, 1e-4)  # a [B,h,w] tensor, no coefficients
    assert len(plain) == 2 and all(np.array_equal(_bits(m), _bits(out[1])) for m in plain)


def test_a_host_photo_equals_the_same_photo_on_the_device():
    p, photo, _, _ = restated(4)
    on_dev, _ = _run(p, photo, 4, 1e-4)
    on_host, _ = _run(p, photo, 4, 1e-4, device_photo=False)
    strided = np.zeros((300, 211 + 5, 3), np.uint8)  # a host view that is not contiguous
    strided[:, 2:213] = photo
    on_view = pp.guided_upsample_images([torch.from_numpy(p.copy()).cuda()], [strided[:, 2:213]], 4, 1e-4)
    assert np.array_equal(_bits(on_dev[0]), _bits(on_host[0])) and np.array_equal(_bits(on_dev[0]), _bits(on_view[0]))


def test_a_sliced_device_view_is_read_through_its_pitch():
    p, photo, _, _ = restated(4)
    big = torch.from_numpy(np.random.default_rng(9).integers(0, 256, (320, 240, 3), dtype=np.uint8)).cuda()
    y1, x1 = 11, 7  # odd x1: the view starts at an odd byte address and its pitch is no multiple of 4 either way
    big[y1:y1 + 300, x1:x1 + 211] = torch.from_numpy(photo.copy()).cuda()
    view = big[y1:y1 + 300, x1:x1 + 211]
    assert not view.is_contiguous() and view.data_ptr() % 2 == 1
    m = [torch.from_numpy(p.copy()).cuda()]
    assert np.array_equal(_bits(pp.guided_upsample_images(m, [view], 4, 1e-4)[0]), _bits(pp.guided_upsample_images(m, [view.contiguous()], 4, 1e-4)[0]))
    assert np.array_equal(_bits(pp.guided_upsample_images(m, [view], 4, 1e-4)[0]), _bits(_run(p, photo, 4, 1e-4)[0][0]))
    flipped = big[y1:y1 + 300, x1:x1 + 2 * 211:2]  # every other pixel: not readable through a row pitch, taken as its packed copy
    assert np.array_equal(_bits(pp.guided_upsample_images(m, [flipped], 4, 1e-4)[0]), _bits(pp.guided_upsample_images(m, [flipped.contiguous()], 4, 1e-4)[0]))


def test_a_depth_edge_follows_the_photos_edge():
    """A 63 x 63 photo, 51 left of column 31 and 204 from it on, and a 12 x 12 map equal to alpha (cell mean / 255) + 1 with alpha = 2: the ideal result is
    alpha I / 255 + 1, a step of 1.2 at column 31, which falls inside cell column 5 (columns 27 .. 31). On a CPU the restatement's worst error against
    the ideal is 0.0747 = 0.037 alpha, at the straddling cell, and the bilinear resize's is 0.537: it ramps over the neighbouring cells. The device
    must at least halve the bilinear's worst error, measured here with scale_prediction_images."""
    photo = np.full((63, 63, 3), 51, dtype=np.uint8)
    photo[:, 31:] = 204
    p = (2.0 * gr.low_res_guide(photo, 12, 12)[..., 0] + 1.0).astype(np.float32)
    ideal = 2.0 * photo[..., 0].astype(np.float64) / 255.0 + 1.0
    out, _ = _run(p, photo, 2, 1e-4)
    bilinear = pp.scale_prediction_images([torch.from_numpy(p).cuda()[None]], [(63, 63)])[0][0].cpu().numpy().astype(np.float64)
    err_guided = float(np.abs(out[0][0].cpu().numpy().astype(np.float64) - ideal).max())
    err_bilinear = float(np.abs(bilinear - ideal).max())
    print(f"edge: worst error guided {err_guided:.4f}, bilinear {err_bilinear:.4f} (alpha 2, step 1.2)")
    assert err_bilinear > 0.1  # (the bilinear ramp is there to be beaten)
    assert err_guided <= 0.5 * err_bilinear


def test_inference_guided_is_inference_images_then_guided_upsample_images():
    from muggled_dpt_amd import make_depthanythingv2_dpt_from_original_state_dict as make
    from muggled_dpt_amd.synthetic import make_synthetic_original_state_dict
    rng = np.random.default_rng(6)
    photos = [rng.integers(0, 256, (150, 130, 3), dtype=np.uint8), rng.integers(0, 256, (120, 200, 3), dtype=np.uint8)]
    model = make(make_synthetic_original_state_dict("tiny", 0))[1].to("cuda", torch.bfloat16)
    got = model.inference_guided(photos, 3, 1e-3, 112)
    preds = model.inference_images(photos, 112, True, 32)
    want = pp.guided_upsample_images(preds, photos, 3, 1e-3)
    assert [tuple(g.shape) for g in got] == [(1, 150, 130), (1, 120, 200)]
    for g, w in zip(got, want):
        assert g.dtype == torch.float32 and np.array_equal(_bits(g), _bits(w)) and torch.isfinite(g).all()
