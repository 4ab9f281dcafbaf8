"""Synthetic depth of field on the device (refocus.refocus_images / defocus_planes -> mdpt_post_refocus, csrc/post_refocus.inc) against the fp64 numpy
restatement tests/refocus_restate.py, which is written from the definition (a loop over the taps of the whole photo) and knows nothing of tiles, halos or the
per-tile window. The arithmetic is IEEE fp64 with nothing contracted on both sides, so the comparison is exact: rq equal on every pixel, e32 bit for bit,
the output equal on every byte.

Shapes: 1 x 1; 17 x 9 (smaller than the halo at radius 32); 37 x 53 and 65 x 67 (no tile multiples: taps cross tile corners, 65 x 67 has 3 x 3 tiles); 70 x 33;
maps of 12 x 9 and 5 x 7 and a map at photo size; max_radius 0, 1, 5, 32 and both sides of the thresholds between the three LDS sizes of the gather
(8 | 9, 16 | 17)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from muggled_dpt_amd import mesh_io, refocus
from tests import refocus_restate as rr

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (map h x w, photo H x W, map dtype, keywords of the call)
CASES = [
    ((1, 1), (1, 1), "float32", dict(max_radius=5)),
    ((5, 7), (17, 9), "float32", dict(max_radius=32, aperture=64.0, focus=0.2)),
    ((12, 9), (37, 53), "bfloat16", dict(max_radius=5, aperture=12.0, focus_xy=(0.4, 0.6))),
    ((12, 9), (65, 67), "float16", dict(max_radius=32, aperture=90.0, focus=0.3, focus_range=0.2)),
    ((65, 67), (65, 67), "float32", dict(max_radius=5, aperture=9.0, focus=2.0, space="depth")),
    ((5, 7), (70, 33), "float32", dict(max_radius=1, aperture=40.0, focus_xy=(1.0, 1.0), space="depth")),
    ((12, 9), (70, 33), "float32", dict(max_radius=0, aperture=50.0)),
    ((12, 9), (37, 53), "float32", dict(max_radius=8, aperture=30.0, focus=0.7)),
    ((12, 9), (37, 53), "float32", dict(max_radius=9, aperture=30.0, focus=0.7)),
    ((5, 7), (37, 53), "bfloat16", dict(max_radius=16, aperture=40.0, focus_xy=(0.0, 0.0))),
    ((12, 9), (37, 53), "float16", dict(max_radius=17, aperture=40.0, focus=1.0, focus_range=0.1)),
    ((5, 7), (37, 53), "float32", dict(max_radius=5, aperture=20.0, focus=1.5, space="depth")),
    ((12, 9), (5, 4), "float32", dict(max_radius=5, aperture=20.0, focus=0.5)),
]
TORCH = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16}


def make_case(index: int):
    """-> (map fp32 holding values of the case's dtype, photo uint8): seeded by the index, so every test sees the same data. Depth-space maps hold zeros,
    negatives, +inf and NaN."""
    (h, w), (H, W), dtype, kw = CASES[index]
    rng = np.random.default_rng(500 + index)
    if kw.get("space") == "depth":
        p = rng.uniform(0.3, 12.0, (h, w)).astype(np.float32)
        if p.size > 8:
            flat = p.reshape(-1)
            flat[rng.choice(p.size, 4, replace=False)] = (0.0, -2.5, np.inf, np.nan)
    else:
        p = (rng.uniform(-4.0, 9.0, (h, w)) + 3.0 * np.sin(np.arange(w) / 2.0)[None, :]).astype(np.float32)
    p = torch.from_numpy(p).to(TORCH[dtype]).to(torch.float32).numpy()
    return p, rng.integers(0, 256, (H, W, 3), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def restated(index: int):
    """the restatement of CASES[index], computed once and shared (read only)"""
    p, photo = make_case(index)
    out, rq, e32 = rr.refocus(p, photo, **CASES[index][3])
    for a in (p, photo, out, rq, e32):
        a.setflags(write=False)
    return p, photo, out, rq, e32


def _dev_map(index: int, p):
    return torch.from_numpy(np.array(p)).to("cuda", TORCH[CASES[index][2]])[None]


@pytest.mark.parametrize("index", range(len(CASES)))
def test_planes_and_output_equal_the_restatement(index):
    (h, w), (H, W), dtype, kw = CASES[index]
    p, photo, out, rq, e32 = restated(index)
    got, planes = refocus.refocus_images([_dev_map(index, p)], [torch.from_numpy(np.array(photo)).cuda()], return_radius=True, **kw)
    assert got[0].shape == (H, W, 3) and got[0].dtype == torch.uint8 and planes[0][0].shape == (H, W) and planes[0][0].dtype == torch.uint8
    assert planes[0][1].shape == (H, W) and planes[0][1].dtype == torch.float32
    g_out, g_rq, g_e = got[0].cpu().numpy(), planes[0][0].cpu().numpy(), planes[0][1].cpu().numpy()
    bad_rq, bad_e, bad_out = int((g_rq != rq).sum()), int((g_e.view(np.uint32) != e32.view(np.uint32)).sum()), int((g_out != out).sum())
    print(f"refocus {h}x{w} {dtype} -> {H}x{W} {kw}: rq max {int(rq.max())}, differing rq {bad_rq}, e32 {bad_e}, bytes {bad_out}, "
          f"changed bytes {int((out != photo).sum())} of {out.size}")
    assert bad_rq == 0
    assert bad_e == 0
    assert bad_out == 0
    alone = refocus.defocus_planes([_dev_map(index, p)], [np.array(photo)], **kw)  # the preparation alone, from a host photo
    assert torch.equal(alone[0][0], planes[0][0]) and torch.equal(alone[0][1].view(torch.int32), planes[0][1].view(torch.int32))


def test_the_cases_blur_and_the_large_radius_is_reached():
    """what the comparison above stands on: the cases are not trivially sharp, and radius 32 is really reached"""
    assert int(restated(1)[3].max()) == 128 and int(restated(3)[3].max()) == 128
    for index in (1, 2, 3, 4, 5, 7, 8, 9, 10, 11):
        p, photo, out, rq, e32 = restated(index)
        assert (out != photo).mean() > 0.2, index
    for index in (0, 6):
        assert np.array_equal(restated(index)[2], restated(index)[1])
    assert not np.isfinite(restated(4)[0]).all() and (restated(4)[0] <= 0).any()


def test_pairs_of_different_sizes_share_one_call_and_a_second_call_repeats_it():
    picks, kw = [7, 0, 12, 2], dict(max_radius=8, aperture=30.0, focus=0.7)  # 37x53, 1x1, 5x4 (a photo smaller than its map), 37x53 from a bf16-valued map
    data = [restated(k)[:2] for k in picks]
    maps = [torch.from_numpy(p.copy()).cuda()[None] for p, _ in data]
    photos = [torch.from_numpy(f.copy()).cuda() for _, f in data]
    out, planes = refocus.refocus_images(maps, photos, return_radius=True, **kw)
    again, planes2 = refocus.refocus_images(maps, photos, return_radius=True, **kw)
    assert out[0].untyped_storage().data_ptr() == out[3].untyped_storage().data_ptr()  # views into one allocation
    for k in range(4):
        alone, alone_p = refocus.refocus_images(maps[k:k + 1], photos[k:k + 1], return_radius=True, **kw)
        assert out[k].shape == data[k][1].shape
        for a, b in ((out[k], alone[0]), (planes[k][0], alone_p[0][0]), (planes[k][1].view(torch.int32), alone_p[0][1].view(torch.int32)), (out[k], again[k]),
                     (planes[k][0], planes2[k][0]), (planes[k][1].view(torch.int32), planes2[k][1].view(torch.int32))):
            assert torch.equal(a, b), k
    assert np.array_equal(out[0].cpu().numpy(), restated(7)[2])
    same = refocus.refocus_images(torch.cat(maps[:1] * 2), photos[:1] * 2, **kw)  # a [B,h,w] tensor
    assert len(same) == 2 and all(torch.equal(m, out[0]) for m in same)


def test_host_photos_and_pitched_device_views_are_the_same_photo():
    index = 3
    (h, w), (H, W), dtype, kw = CASES[index]
    p, photo, out, _, _ = restated(index)
    m = [_dev_map(index, p)]
    on_host = refocus.refocus_images(m, [np.array(photo)], **kw)
    strided = np.zeros((H, W + 5, 3), np.uint8)  # a host view that is not contiguous
    strided[:, 2:2 + W] = photo
    on_view = refocus.refocus_images(m, [strided[:, 2:2 + W]], **kw)
    big = torch.from_numpy(np.random.default_rng(9).integers(0, 256, (H + 20, W + 30, 3), dtype=np.uint8)).cuda()
    y1, x1 = 11, 8  # 3 (11 * 97 + 8) is odd: the view starts at an odd byte address, and its pitch of 291 bytes is odd too
    big[y1:y1 + H, x1:x1 + W] = torch.from_numpy(np.array(photo)).cuda()
    view = big[y1:y1 + H, x1:x1 + W]
    assert not view.is_contiguous() and view.data_ptr() % 2 == 1
    pitched = refocus.refocus_images(m, [view], **kw)
    every_other = big[y1:y1 + H, x1:x1 + 2 * W:2]  # not readable through a row pitch: taken as its packed copy
    for got in (on_host[0], on_view[0], pitched[0]):
        assert np.array_equal(got.cpu().numpy(), out)
    assert torch.equal(refocus.refocus_images(m, [every_other], **kw)[0], refocus.refocus_images(m, [every_other.contiguous()], **kw)[0])


def _model():
    from muggled_dpt_amd import make_depthanythingv2_dpt_from_original_state_dict as make
    from muggled_dpt_amd.synthetic import make_synthetic_original_state_dict
    return make(make_synthetic_original_state_dict("tiny", 0))[1].to("cuda", torch.bfloat16)


def _photos():
    rng = np.random.default_rng(6)
    return {"a": rng.integers(0, 256, (150, 130, 3), dtype=np.uint8), "b": rng.integers(0, 256, (120, 200, 3), dtype=np.uint8)}


def test_inference_refocus_is_inference_images_then_refocus_images():
    from muggled_dpt_amd import postprocess as pp
    model, photos = _model(), list(_photos().values())
    preds = model.inference_images(photos, 112, True, 32)
    got = model.inference_refocus(photos, focus_xy=(0.5, 0.5), aperture=40.0, max_radius=6, max_side_length=112)
    want = refocus.refocus_images(preds, photos, focus_xy=(0.5, 0.5), aperture=40.0, max_radius=6)
    assert [tuple(g.shape) for g in got] == [(150, 130, 3), (120, 200, 3)]
    assert all(g.dtype == torch.uint8 and torch.equal(g, w) for g, w in zip(got, want))
    assert any(not np.array_equal(g.cpu().numpy(), f) for g, f in zip(got, photos))
    got = model.inference_refocus(photos, 0.8, None, 40.0, 6, 0.05, guided=(3, 1e-3), max_side_length=112)
    want = refocus.refocus_images(pp.guided_upsample_images(preds, photos, 3, 1e-3), photos, 0.8, None, 40.0, 6, 0.05)
    assert all(torch.equal(g, w) for g, w in zip(got, want))


def test_refocus_flags_write_a_png_per_photo(tmp_path):
    from muggled_dpt_amd import postprocess as pp
    photos = _photos()
    for k in photos:
        np.save(tmp_path / f"{k}.npy", photos[k])
    cmd = [sys.executable, os.path.join(REPO, "tools", "mdpt_run_image.py"), "--synthetic", "tiny", "-s", "112", "-i", str(tmp_path / "a.npy"), "-i",
           str(tmp_path / "b.npy"), "--refocus", "0.5", "40", "--refocus_at", "0.25", "0.75", "--refocus_radius", "6", "--refocus_guided", "3", "1e-3"]
    r = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=REPO), cwd=tmp_path, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    frames = list(photos.values())
    guided = pp.guided_upsample_images(_model().inference_images(frames, 112, True, 32), frames, 3, 1e-3)
    want = refocus.refocus_images(guided, frames, 0.5, (0.25, 0.75), 40.0, 6)
    for k, name in enumerate(photos):
        with open(tmp_path / f"{name}_refocus.png", "rb") as fh:
            assert fh.read() == mesh_io.encode_png(np.ascontiguousarray(want[k].cpu().numpy()[:, :, ::-1]))
