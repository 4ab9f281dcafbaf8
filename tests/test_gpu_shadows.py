"""Cast shadows and ambient occlusion on the device (relight.light_occlusion / shade_images -> mdpt_post_shadows, csrc/post_shadows.inc) against the fp64 numpy
restatement tests/shadows_restate.py, which is written from the definition (whole-grid arrays, one gather per march step) and knows nothing of tiles, halos
or LDS. Every operation of the definition is a correctly rounded IEEE operation in a fixed order on both sides, nothing contracted, so the comparison is
exact: every bit of the ao planes, every vis value, every shaded byte. The scenes and what they cover: tests/shadows_cases.py (whose coverage condition
tests/test_shadows_cpu.py asserts on the CPU)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from muggled_dpt_amd import mesh_io, relight
from tests import shadows_cases as sc

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev_map(index: int, p):
    return torch.from_numpy(np.array(p)).to("cuda", sc.TORCH[sc.CASES[index]["dtype"]])[None]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _occlusion_kw(kw):
    return {k: v for k, v in kw.items() if k not in sc.SHADING and k != "step"}


@pytest.mark.parametrize("index", range(len(sc.CASES)))
def test_planes_and_frames_equal_the_restatement(index):
    c = sc.CASES[index]
    p, photo, frames, ao, vis, valid = sc.restated(index)
    (H, W), V = c["HW"], len(c["lights"])
    m, dev_photo = [_dev_map(index, p)], [torch.from_numpy(np.array(photo)).cuda()]
    got, got_ao, got_vis = relight.shade_images(m, dev_photo, c["lights"], grid_hw=c["grid"], return_planes=True, **c["kw"])
    assert got[0].shape == (V, H, W, 3) and got[0].dtype == torch.uint8 and got_ao[0].shape == ao.shape and got_ao[0].dtype == torch.float32
    assert got_vis[0].shape == vis.shape and got_vis[0].dtype == torch.float32
    bad_ao = int((got_ao[0].cpu().numpy().view(np.uint32) != ao.view(np.uint32)).sum())
    bad_vis = int((got_vis[0].cpu().numpy() != vis).sum())
    bad = int((got[0].cpu().numpy() != frames).sum())
    print(f"shadows {c['hw']} {c['dtype']} {c['holds']} grid {c['grid']} -> {H}x{W} {c['kw']}: valid nodes {int(valid.sum())} of {valid.size}, in shadow "
          f"{[int((v == 0).sum()) for v in vis]}, ao < 1 on {int((ao < 1).sum())}; differing ao words {bad_ao}, vis values {bad_vis}, bytes {bad} of {frames.size}")
    assert bad_ao == 0
    assert bad_vis == 0
    assert bad == 0
    assert torch.equal(relight.shade_images(m, dev_photo, c["lights"], grid_hw=c["grid"], **c["kw"])[0], got[0])  # without return_planes
    planes_ao, planes_vis = relight.light_occlusion(m, c["lights"], grid_hw=c["grid"], target_hws=[(H, W)], **_occlusion_kw(c["kw"]))
    assert torch.equal(_bits(planes_ao[0]), _bits(got_ao[0])) and torch.equal(_bits(planes_vis[0]), _bits(got_vis[0]))
    only_ao, none = relight.light_occlusion(m, None, grid_hw=c["grid"], target_hws=[(H, W)], **_occlusion_kw(c["kw"]))
    assert none is None and torch.equal(_bits(only_ao[0]), _bits(got_ao[0]))
    one = relight.shade_images(m, dev_photo, c["lights"][-1], grid_hw=c["grid"], **c["kw"])  # V = 1: the last light alone
    assert one[0].shape == (1, H, W, 3) and torch.equal(one[0][0], got[0][-1])


@pytest.mark.parametrize("index", [2, 3, 4, 6])
def test_with_the_features_off_the_frames_are_relight_images(index):
    c = sc.CASES[index]
    p, photo = sc.restated(index)[:2]
    m, dev_photo = [_dev_map(index, p)], [torch.from_numpy(np.array(photo)).cuda()]
    plain = {k: v for k, v in c["kw"].items() if k in sc.SHADING or k in ("space", "fov_deg", "min_depth", "max_depth", "edge_ratio", "step")}
    want = relight.relight_images(m, dev_photo, c["lights"], **plain)
    for off in (dict(shadow_reach=0, ao_strength=0.0), dict(shadow_reach=0, ao_reach=0)):
        got = relight.shade_images(m, dev_photo, c["lights"], grid_hw=c["grid"], **{**c["kw"], **off})
        assert torch.equal(got[0], want[0]), off
    half, ao, vis = relight.shade_images(m, dev_photo, c["lights"], grid_hw=c["grid"], return_planes=True, **{**c["kw"], "shadow_reach": 0})
    assert (vis[0] == 1.0).all() and not torch.equal(half[0], want[0])  # the occlusion alone; the planes asked for come back constant


def test_pairs_of_different_sizes_share_one_call_and_a_second_call_repeats_it():
    picks, kw, lights = [3, 0, 5, 4], dict(ao_radius=0.6, shadow_thickness=0.4, **sc.SHADING), sc.CASES[3]["lights"]
    data = [sc.restated(k)[:2] for k in picks]
    grids = [sc.CASES[k]["grid"] for k in picks]
    maps = [torch.from_numpy(p.copy()).cuda()[None] for p, _ in data]
    photos = [torch.from_numpy(f.copy()).cuda() for _, f in data]
    out, ao, vis = relight.shade_images(maps, photos, lights, grid_hw=grids, return_planes=True, **kw)
    again, ao2, vis2 = relight.shade_images(maps, photos, lights, grid_hw=grids, return_planes=True, **kw)
    assert out[0].untyped_storage().data_ptr() == out[3].untyped_storage().data_ptr()  # views into one allocation
    for k in range(4):
        alone, alone_ao, alone_vis = relight.shade_images(maps[k:k + 1], photos[k:k + 1], lights, grid_hw=grids[k:k + 1], return_planes=True, **kw)
        assert out[k].shape == (3, *data[k][1].shape)
        for a, b in ((out[k], alone[0]), (_bits(ao[k]), _bits(alone_ao[0])), (_bits(vis[k]), _bits(alone_vis[0])), (out[k], again[k]), (_bits(ao[k]), _bits(ao2[k])),
                     (_bits(vis[k]), _bits(vis2[k]))):
            assert torch.equal(a, b), k
    want = sc.sr.shade_images(data[0][0], data[0][1], lights, **kw)
    assert np.array_equal(out[0].cpu().numpy(), want[0]) and np.array_equal(ao[0].cpu().numpy(), want[1]) and np.array_equal(vis[0].cpu().numpy(), want[2])
    same = relight.light_occlusion(torch.cat(maps[:1] * 2), lights, target_hws=[(33, 65)] * 2, ao_radius=0.6, shadow_thickness=0.4)  # a [B,h,w] tensor
    assert len(same[0]) == 2 and all(torch.equal(_bits(a), _bits(ao[0])) for a in same[0]) and all(torch.equal(_bits(v), _bits(vis[0])) for v in same[1])


def test_host_photos_pitched_device_views_and_white_clay():
    index = 3
    c = sc.CASES[index]
    (H, W), lights, kw = c["HW"], c["lights"], c["kw"]
    p, photo, frames = sc.restated(index)[:3]
    m = [_dev_map(index, p)]
    on_host = relight.shade_images(m, [np.array(photo)], lights, **kw)
    big = torch.from_numpy(np.random.default_rng(9).integers(0, 256, (H + 3, W + 5, 3), dtype=np.uint8)).cuda()
    big[2:-1, 3:-2] = torch.from_numpy(np.array(photo)).cuda()
    view = big[2:-1, 3:-2]  # a pitched slice, read in place
    assert not view.is_contiguous() and tuple(view.shape) == (H, W, 3)
    pitched = relight.shade_images(m, [view], lights, **kw)
    for got in (on_host[0], pitched[0]):
        assert np.array_equal(got.cpu().numpy(), frames)
    clay = relight.shade_images(m, None, lights, target_hws=[(H, W)], **kw)
    assert np.array_equal(clay[0].cpu().numpy(), sc.sr.shade_images(p, np.full((H, W, 3), 255, np.uint8), lights, **kw)[0])
    own_size = relight.shade_images(m, None, (0.0, 0.0, 1.0))  # neither photos nor sizes: the map's own size
    assert tuple(own_size[0].shape) == (1, *c["hw"], 3)


def _model():
    from muggled_dpt_amd import make_depthanythingv2_dpt_from_original_state_dict as make
    from muggled_dpt_amd.synthetic import make_synthetic_original_state_dict
    return make(make_synthetic_original_state_dict("tiny", 0))[1].to("cuda", torch.bfloat16)


def _photos():
    rng = np.random.default_rng(6)
    return {"a": rng.integers(0, 256, (150, 130, 3), dtype=np.uint8), "b": rng.integers(0, 256, (120, 200, 3), dtype=np.uint8)}


def test_inference_shade_is_the_composition_it_documents():
    from muggled_dpt_amd import postprocess as pp
    model, photos = _model(), list(_photos().values())
    lights = relight.light_sweep(3, 40.0)
    preds = model.inference_images(photos, 112, True, 32)
    got = model.inference_shade(photos, lights, specular=0.3, max_side_length=112, fov_deg=60.0, shadow_reach=12, ao_radius=0.5)
    want = relight.shade_images(preds, photos, lights, specular=0.3, fov_deg=60.0, shadow_reach=12, ao_radius=0.5)
    assert [tuple(g.shape) for g in got] == [(3, 150, 130, 3), (3, 120, 200, 3)]
    assert all(g.dtype == torch.uint8 and torch.equal(g, w) for g, w in zip(got, want))
    assert any(not torch.equal(g, r) for g, r in zip(got, relight.relight_images(preds, photos, lights, specular=0.3, fov_deg=60.0)))
    guided = pp.guided_upsample_images(preds, photos, 3, 1e-3)
    got = model.inference_shade(photos, (0.0, 1.0, 1.0), guided=(3, 1e-3), max_side_length=112, step=1, grid_hw=(40, 40))
    assert all(torch.equal(g, w) for g, w in zip(got, relight.shade_images(guided, photos, (0.0, 1.0, 1.0), step=1, grid_hw=(40, 40))))
    metric = _model()  # a metric config picks depth space
    metric.config["is_metric"] = True
    preds = metric.inference_images(photos, 112, True, 32)
    got = metric.inference_shade(photos, (0.0, 1.0, 1.0), max_side_length=112)
    assert all(torch.equal(g, w) for g, w in zip(got, relight.shade_images(preds, photos, (0.0, 1.0, 1.0), space="depth")))


def test_the_shade_flag_writes_pngs(tmp_path):
    photos = _photos()
    for k in photos:
        np.save(tmp_path / f"{k}.npy", photos[k])
    cmd = [sys.executable, os.path.join(REPO, "tools", "mdpt_run_image.py"), "--synthetic", "tiny", "-s", "112", "-i", str(tmp_path / "a.npy"), "-i",
           str(tmp_path / "b.npy"), "--shade", "-1", "1", "1", "--shade_sweep", "2", "--shade_reach", "12", "--shade_ao", "0.7"]
    r = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=REPO), cwd=tmp_path, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    frames = list(photos.values())
    preds = _model().inference_images(frames, 112, True, 32)
    ring = relight.light_sweep(2, math.degrees(math.atan2(1.0, math.hypot(-1.0, 1.0))))  # the tool's ring: the light's elevation, starting at its azimuth
    turn = math.atan2(1.0, -1.0)
    lights = [(math.cos(turn) * lx - math.sin(turn) * ly, math.sin(turn) * lx + math.cos(turn) * ly, lz) for lx, ly, lz in ring.tolist()]
    want = relight.shade_images(preds, frames, lights, shadow_reach=12, ao_strength=0.7)
    for k, name in enumerate(photos):
        for v in range(2):
            with open(tmp_path / f"{name}_shaded{v:03d}.png", "rb") as fh:
                assert fh.read() == mesh_io.encode_png(np.ascontiguousarray(want[k][v].cpu().numpy()[:, :, ::-1])), (name, v)
