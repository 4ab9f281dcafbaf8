"""Surface normals and relighting on the device (relight.depth_normals / relight_images -> mdpt_post_normals, csrc/post_normals.inc) against the fp64 numpy
restatement tests/normals_restate.py, which is written from the definition (whole-photo arrays shifted by the step) and knows nothing of tiles, halos or LDS.
Every operation of the definition is a correctly rounded IEEE operation in a fixed order on both sides, nothing contracted, so the comparison is exact:
every bit of the fp32 normals, every encoded byte, every relit byte.

Shapes: 5 x 7 from 3 x 4 (smaller than one tile); 33 x 65 from 9 x 12 (2 x 3 tiles, the halo crosses tile borders) at steps 1, 3, 16 and the default (5);
40 x 40 from 40 x 40 (the direct read); 9 x 6 from 12 x 16 (a map larger than its photo); 5 x 7 at step 16 (no usable neighbour: everything invalid, the photo
comes back)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from muggled_dpt_amd import mesh_io, relight
from tests import normals_restate as nr

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (map h x w, photo H x W, map dtype, what the map holds, camera keywords)
CASES = [
    ((3, 4), (5, 7), "float32", "plain", dict()),
    ((9, 12), (33, 65), "bfloat16", "plain", dict(step=1)),
    ((9, 12), (33, 65), "float16", "plain", dict(step=3, edge_ratio=1.0, fov_deg=70.0)),
    ((9, 12), (33, 65), "float32", "plain", dict(step=16, edge_ratio=float("inf"))),
    ((40, 40), (40, 40), "float32", "holes", dict(space="depth", step=1)),
    ((12, 16), (9, 6), "float32", "plain", dict(min_depth=2.0, max_depth=9.0)),
    ((3, 4), (5, 7), "float32", "plain", dict(step=16)),
    ((9, 12), (33, 65), "float32", "holes", dict(space="depth", step=3, edge_ratio=1.0)),
    ((9, 12), (33, 65), "float32", "flat", dict(step=3)),
    ((9, 12), (33, 65), "bfloat16", "holes", dict(edge_ratio=float("inf"))),
    ((40, 40), (40, 40), "float16", "plain", dict(step=2)),
]
# (lights, shading keywords): three lights with one facing away and a tight highlight; one light, no highlight; the widest highlight
SHADINGS = [
    ([(-1.0, 1.0, 1.0), (0.0, 0.0, -1.0), (0.3, -0.2, 0.5)], dict(ambient=0.3, diffuse=0.8, specular=0.6, shininess_log2=5)),
    ((0.5, 0.5, 1.0), dict()),
    ([(1.0, 0.0, 0.4)], dict(ambient=0.2, diffuse=1.4, specular=0.9, shininess_log2=0)),
]
TORCH = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16}


def make_case(index: int):
    """-> (map fp32 holding values of the case's dtype, photo uint8): seeded by the index, so every test sees the same data. "holes": NaN and +inf and, in
    depth space, zeros and negatives. The maps are smooth with a step across them, so both the central and the one-sided differences occur."""
    (h, w), (H, W), dtype, holds, kw = CASES[index]
    rng = np.random.default_rng(700 + index)
    yy, xx = np.mgrid[0:h, 0:w]
    p = 2.0 + 0.08 * xx + 0.05 * yy + 0.02 * rng.standard_normal((h, w)) + 1.5 * (xx > w * 0.55)
    if holds == "flat":
        p = np.full((h, w), 3.25)
    p = p.astype(np.float32)
    if holds == "holes":
        flat = p.reshape(-1)
        picks = rng.choice(p.size, 6, replace=False)
        flat[picks[:2]] = (np.nan, np.inf)
        if kw.get("space") == "depth":
            flat[picks[2:]] = (0.0, -2.5, np.nan, 0.0)
    p = torch.from_numpy(p).to(TORCH[dtype]).to(torch.float32).numpy()
    return p, rng.integers(0, 256, (H, W, 3), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def restated(index: int):
    """the restatement of CASES[index], computed once and shared (read only) -> (map, photo, n32, encoded, [frames per shading], valid)"""
    p, photo = make_case(index)
    kw = CASES[index][4]
    n, valid, P = nr.normals(p, photo.shape[0], photo.shape[1], **kw)
    frames = [nr.shade(photo, n, valid, P, lights, **sh) for lights, sh in SHADINGS]
    out = (p, photo, n.astype(np.float32), nr.encode(n), frames, valid)
    for a in (p, photo, out[2], out[3], valid, *frames):
        a.setflags(write=False)
    return out


def _dev_map(index: int, p):
    return torch.from_numpy(np.array(p)).to("cuda", TORCH[CASES[index][2]])[None]


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("index", range(len(CASES)))
def test_normals_encoding_and_frames_equal_the_restatement(index):
    (h, w), (H, W), dtype, holds, kw = CASES[index]
    p, photo, n32, enc, frames, valid = restated(index)
    m, dev_photo = [_dev_map(index, p)], [torch.from_numpy(np.array(photo)).cuda()]
    got_n, got_e = relight.depth_normals(m, [(H, W)], encode=True, **kw)
    assert got_n[0].shape == (H, W, 3) and got_n[0].dtype == torch.float32 and got_e[0].shape == (H, W, 3) and got_e[0].dtype == torch.uint8
    bad_n = int((got_n[0].cpu().numpy().view(np.uint32) != n32.view(np.uint32)).sum())
    bad_e = int((got_e[0].cpu().numpy() != enc).sum())
    print(f"normals {h}x{w} {dtype} {holds} -> {H}x{W} {kw}: valid {int(valid.sum())} of {valid.size}, differing normal words {bad_n}, encoded bytes {bad_e}")
    assert bad_n == 0
    assert bad_e == 0
    for (lights, sh), want in zip(SHADINGS, frames):
        got, again_n = relight.relight_images(m, dev_photo, lights, return_normals=True, **sh, **kw)
        bad = int((got[0].cpu().numpy() != want).sum())
        print(f"  relit {sh}: frames {tuple(got[0].shape)}, differing bytes {bad}, changed bytes {int((want != photo[None]).sum())} of {want.size}")
        assert got[0].shape == want.shape and got[0].dtype == torch.uint8
        assert bad == 0
        assert torch.equal(_bits(again_n[0]), _bits(got_n[0]))  # return_normals / encode variants share the plain call's outputs
        assert torch.equal(relight.relight_images(m, dev_photo, lights, **sh, **kw)[0], got[0])
    assert torch.equal(_bits(relight.depth_normals(m, None, dev_photo, **kw)[0]), _bits(got_n[0]))  # the size from the photo


def test_the_cases_cover_what_they_claim():
    """what the comparison above stands on: both kinds of difference occur, invalid pixels exist where holes were put, step 16 on 5 x 7 leaves nothing valid"""
    assert not restated(6)[5].any() and all(np.array_equal(f, np.broadcast_to(restated(6)[1], f.shape)) for f in restated(6)[4])
    assert (restated(6)[3] == 128).all() and not restated(6)[2].any()
    for index in (4, 7, 9):
        valid = restated(index)[5]
        assert 0 < (~valid).sum() < valid.size / 2, index
    assert (restated(8)[2] == np.array([0, 0, 1], np.float32)).all()  # a flat map faces the camera
    for index in (1, 2, 3, 5, 10):
        p, photo, n32, enc, frames, valid = restated(index)
        assert valid.all() and len(np.unique(enc.reshape(-1, 3), axis=0)) > 8 and (frames[0] != photo[None]).mean() > 0.5, index
    p, photo = make_case(1)
    edge = nr.normals(p, 33, 65, step=1)[0]
    central = nr.normals(p, 33, 65, step=1, edge_ratio=float("inf"))[0]
    assert 0.02 < (np.abs(edge - central).max(axis=-1) > 1e-6).mean() < 0.9  # the edge rule is in force on some pixels, the central difference on the others
    assert not np.array_equal(restated(1)[4][2], restated(1)[4][0][:1])


def test_pairs_of_different_sizes_share_one_call_and_a_second_call_repeats_it():
    picks, kw = [1, 0, 5, 10], dict(step=2, edge_ratio=2.0)
    lights, sh = SHADINGS[0]
    data = [restated(k)[:2] for k in picks]
    maps = [torch.from_numpy(p.copy()).cuda()[None] for p, _ in data]
    photos = [torch.from_numpy(f.copy()).cuda() for _, f in data]
    out, normals = relight.relight_images(maps, photos, lights, return_normals=True, **sh, **kw)
    again, normals2 = relight.relight_images(maps, photos, lights, return_normals=True, **sh, **kw)
    assert out[0].untyped_storage().data_ptr() == out[3].untyped_storage().data_ptr()  # views into one allocation
    for k in range(4):
        alone, alone_n = relight.relight_images(maps[k:k + 1], photos[k:k + 1], lights, return_normals=True, **sh, **kw)
        assert out[k].shape == (3, *data[k][1].shape)
        for a, b in ((out[k], alone[0]), (_bits(normals[k]), _bits(alone_n[0])), (out[k], again[k]), (_bits(normals[k]), _bits(normals2[k]))):
            assert torch.equal(a, b), k
    p, photo = data[0]
    n, valid, P = nr.normals(p, 33, 65, **kw)
    assert np.array_equal(out[0].cpu().numpy(), nr.shade(photo, n, valid, P, lights, **sh))
    same = relight.depth_normals(torch.cat(maps[:1] * 2), [(33, 65)] * 2, **kw)  # a [B,h,w] tensor
    assert len(same) == 2 and all(torch.equal(_bits(m), _bits(normals[0])) for m in same)


def test_host_photos_pitched_device_views_and_white_clay():
    index = 2
    (h, w), (H, W), dtype, holds, kw = CASES[index]
    p, photo, _, _, frames, _ = restated(index)
    lights, sh = SHADINGS[0]
    m = [_dev_map(index, p)]
    on_host = relight.relight_images(m, [np.array(photo)], lights, **sh, **kw)
    big = torch.from_numpy(np.random.default_rng(9).integers(0, 256, (H + 3, W + 5, 3), dtype=np.uint8)).cuda()
    big[2:-1, 3:-2] = torch.from_numpy(np.array(photo)).cuda()
    view = big[2:-1, 3:-2]  # a pitched slice, read in place
    assert not view.is_contiguous() and tuple(view.shape) == (H, W, 3)
    pitched = relight.relight_images(m, [view], lights, **sh, **kw)
    every_other = big[2:-1, 3:3 + 2 * (W // 2):2]  # not readable through a row pitch: taken as its packed copy
    for got in (on_host[0], pitched[0]):
        assert np.array_equal(got.cpu().numpy(), frames[0])
    assert torch.equal(relight.relight_images(m, [every_other], lights, **sh, **kw)[0], relight.relight_images(m, [every_other.contiguous()], lights, **sh, **kw)[0])
    clay = relight.relight_images(m, None, lights, target_hws=[(H, W)], **sh, **kw)
    white = np.full((H, W, 3), 255, np.uint8)
    n, valid, P = nr.normals(p, H, W, **kw)
    assert np.array_equal(clay[0].cpu().numpy(), nr.shade(white, n, valid, P, lights, **sh))
    own_size = relight.relight_images(m, None, (0.0, 0.0, 1.0))  # neither photos nor sizes: the map's own size
    assert tuple(own_size[0].shape) == (1, h, w, 3)


def _model():
    from muggled_dpt_amd import make_depthanythingv2_dpt_from_original_state_dict as make
    from muggled_dpt_amd.synthetic import make_synthetic_original_state_dict
    return make(make_synthetic_original_state_dict("tiny", 0))[1].to("cuda", torch.bfloat16)


def _photos():
    rng = np.random.default_rng(6)
    return {"a": rng.integers(0, 256, (150, 130, 3), dtype=np.uint8), "b": rng.integers(0, 256, (120, 200, 3), dtype=np.uint8)}


def test_model_methods_are_the_composition_they_document():
    from muggled_dpt_amd import postprocess as pp
    model, photos = _model(), list(_photos().values())
    lights = relight.light_sweep(3, 40.0)
    preds = model.inference_images(photos, 112, True, 32)
    got = model.inference_relight(photos, lights, specular=0.3, max_side_length=112, fov_deg=60.0)
    want = relight.relight_images(preds, photos, lights, specular=0.3, fov_deg=60.0)
    assert [tuple(g.shape) for g in got] == [(3, 150, 130, 3), (3, 120, 200, 3)]
    assert all(g.dtype == torch.uint8 and torch.equal(g, w) for g, w in zip(got, want))
    assert any(not np.array_equal(g[0].cpu().numpy(), f) for g, f in zip(got, photos))
    got_n, got_e = model.inference_normals(photos, encode=True, max_side_length=112)
    want_n, want_e = relight.depth_normals(preds, None, photos, encode=True)
    assert all(torch.equal(_bits(g), _bits(w)) for g, w in zip(got_n, want_n)) and all(torch.equal(g, w) for g, w in zip(got_e, want_e))
    guided = pp.guided_upsample_images(preds, photos, 3, 1e-3)
    got = model.inference_relight(photos, (0.0, 1.0, 1.0), guided=(3, 1e-3), max_side_length=112, step=1)
    assert all(torch.equal(g, w) for g, w in zip(got, relight.relight_images(guided, photos, (0.0, 1.0, 1.0), step=1)))
    got_n = model.inference_normals(photos, guided=(3, 1e-3), max_side_length=112, step=1)
    assert all(torch.equal(_bits(g), _bits(w)) for g, w in zip(got_n, relight.depth_normals(guided, None, photos, step=1)))
    metric = _model()  # a metric config picks depth space
    metric.config["is_metric"] = True
    preds = metric.inference_images(photos, 112, True, 32)
    got_n = metric.inference_normals(photos, max_side_length=112)
    assert all(torch.equal(_bits(g), _bits(w)) for g, w in zip(got_n, relight.depth_normals(preds, None, photos, space="depth")))
    got = metric.inference_relight(photos, (0.0, 1.0, 1.0), max_side_length=112)
    assert all(torch.equal(g, w) for g, w in zip(got, relight.relight_images(preds, photos, (0.0, 1.0, 1.0), space="depth")))


def test_normals_and_relight_flags_write_pngs(tmp_path):
    photos = _photos()
    for k in photos:
        np.save(tmp_path / f"{k}.npy", photos[k])
    cmd = [sys.executable, os.path.join(REPO, "tools", "mdpt_run_image.py"), "--synthetic", "tiny", "-s", "112", "-i", str(tmp_path / "a.npy"), "-i",
           str(tmp_path / "b.npy"), "--normals", "--relight", "-1", "1", "1", "--relight_sweep", "2"]
    r = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=REPO), cwd=tmp_path, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    frames = list(photos.values())
    preds = _model().inference_images(frames, 112, True, 32)
    enc = relight.depth_normals(preds, None, frames, encode=True)[1]
    for k, name in enumerate(photos):
        with open(tmp_path / f"{name}_normals.png", "rb") as fh:
            assert fh.read() == mesh_io.encode_png(np.ascontiguousarray(enc[k].cpu().numpy()[:, :, ::-1]))
        assert os.path.exists(tmp_path / f"{name}_relit000.png") and os.path.exists(tmp_path / f"{name}_relit001.png")
