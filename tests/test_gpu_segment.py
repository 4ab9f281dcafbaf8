"""The depth segmentation on the device against its numpy restatement (tests/segment_restate.py): every output equal, element for element and bit for bit -
labels, counts, every statistic, vmin / vmax / mean, masks and cutouts. The shapes are the smallest at which each stage can go wrong with 32 x 32 tiles: a
single tile, ragged tiles on both axes, chains through every tile (serpentine, comb), every slab row used (checkerboard), K = 0, hi == lo.
tests/test_segment_cpu.py holds that the scenes have the properties relied on here."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from muggled_dpt_amd import segment
from tests import segment_restate as sr
from tests import segment_scenes as sc

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _as32(v, dtype):
    """the scene as the device holds it (rounded to dtype), back as fp32 for the restatement"""
    t = torch.from_numpy(np.ascontiguousarray(v)).to(dtype)
    return t, t.to(torch.float32).numpy()


def check(seg, index, v32, print_as=None, **kw):
    """image `index` of a device result against the restatement of its map; -> the restated result"""
    res = sr.segment(v32, **kw)
    rows = seg.region_views()[index]
    K = res["count"]
    if print_as:
        print(f"{print_as}: K = {K} (device {rows['count']}), dropped or invalid nodes {int((res['labels'] < 0).sum())}")
    assert rows["count"] == K == int(seg.counts[index]) and K <= seg.capacities[index]
    assert np.array_equal(seg.labels[index].cpu().numpy(), res["labels"]) and seg.labels[index].dtype == torch.int32
    for name in ("area", "bbox", "first", "sum_q"):
        assert np.array_equal(rows[name].cpu().numpy(), res[name]), name
    for name, dt in (("vmin", np.uint32), ("vmax", np.uint32), ("mean", np.uint64)):
        assert np.array_equal(rows[name].cpu().numpy().view(dt), res[name].view(dt)), name  # bit-equal
    assert float(seg.lo[index]) == res["lo"] and float(seg.hi[index]) == res["hi"]
    return res


@functools.lru_cache(maxsize=None)
def scene(name):
    if name.startswith("size"):
        h, w = sc.SIZES[int(name[4:])]
        return sc.piecewise(11 + int(name[4:]), h, w, 0.004) if h * w > 40 else np.linspace(0.0, 1.0, h * w, dtype=np.float32).reshape(h, w)
    return {"serpentine": sc.serpentine, "comb": sc.comb, "plate": sc.plate_before_wall, "flat": lambda: np.full((33, 65), 2.5, np.float32),
            "nan": lambda: np.full((40, 37), np.nan, np.float32), "checker": lambda: sc.checkerboard(37, 41), "diagonal": lambda: sc.diagonal(70)}[name]()


@pytest.mark.parametrize("name,kw", [(f"size{k}", dict(min_area=m)) for k in range(len(sc.SIZES)) for m in (1, 16)] + [
    ("serpentine", dict(min_area=1)), ("serpentine", dict(min_area=16, connectivity=8)), ("comb", dict(min_area=1)), ("comb", dict(min_area=80)),
    ("checker", dict(min_area=1, connectivity=4)), ("checker", dict(min_area=1, connectivity=8)), ("checker", dict(min_area=2)),
    ("diagonal", dict(min_area=1, connectivity=8)), ("diagonal", dict(min_area=1, connectivity=4)), ("nan", dict(min_area=1)), ("flat", dict(min_area=16, step=0.0)),
    ("flat", dict(space="depth")), ("plate", dict()), ("plate", dict(min_area=100000))])
def test_every_output_equals_the_restatement(name, kw):
    v = scene(name)
    seg = segment.segment_depth([torch.from_numpy(v).cuda()], **kw)
    res = check(seg, 0, v, print_as=f"{name} {kw}", **kw)
    h, w = v.shape
    if name == "checker" and kw.get("connectivity") == 4 and kw["min_area"] == 1:
        assert res["count"] == h * w == seg.capacities[0]  # every slab row used
    if name == "checker" and kw.get("connectivity") == 8:
        assert res["count"] == 2
    if name in ("serpentine", "comb") and kw["min_area"] == 1:
        assert res["area"][0] == int((v == 1.0).sum()) and res["bbox"][0].tolist() == [0, 0, w - 1, h - 1]  # one component through every tile
    if name == "nan" or kw.get("min_area", 16) > h * w:
        assert res["count"] == 0 and (res["labels"] == -1).all()
    if name == "flat":
        assert res["count"] == 1 and res["lo"] == res["hi"] == 2.5 and res["sum_q"].tolist() == [0]


@pytest.mark.parametrize("space", ["inverse", "depth"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("which", range(len(sc.RANDOM_SCENES)))
def test_random_piecewise_maps_in_every_dtype_and_space(which, dtype, space):
    seed, h, w, noise = sc.RANDOM_SCENES[which]
    t, v32 = _as32(sc.piecewise(seed, h, w, noise, positive=space == "depth"), dtype)
    for kw in (dict(step=0.02 if space == "inverse" else 0.012, min_area=16), dict(step=0.02, min_area=1, connectivity=8)):
        seg = segment.segment_depth([t.cuda()], space=space, **kw)
        res = check(seg, 0, v32, print_as=f"scene {which} {dtype} {space} {kw}", space=space, **kw)
        assert res["count"] >= 2
        if dtype == torch.float32 and kw["min_area"] == 16:
            props = sc.region_properties(res, sr.valid_nodes(v32, space))
            assert props["dropped"] and props["multi_tile"] and (props["edges"] or noise > 0.02)


def _four():
    maps = [sc.piecewise(21, 70, 45, 0.004), sc.serpentine(65, 40), sc.checkerboard(9, 33), sc.piecewise(22, 33, 65, 0.05)]
    return [torch.from_numpy(m).cuda() for m in maps], maps


def _columns(seg, i):
    rows = seg.region_views()[i]
    return [seg.labels[i]] + [rows[n] for n in ("area", "bbox", "first", "vmin", "vmax", "sum_q", "mean")] + [seg.lo[i], seg.hi[i], seg.counts[i]]


def test_four_maps_in_one_call_equal_the_single_calls_in_any_order_and_a_second_call_repeats_it():
    dev, maps = _four()
    kw = dict(step=0.02, min_area=4, connectivity=8)
    together, again = segment.segment_depth(dev, **kw), segment.segment_depth(dev, **kw)
    order = [2, 0, 3, 1]
    shuffled = segment.segment_depth([dev[k] for k in order], **kw)
    for i in range(4):
        check(together, i, maps[i], **kw)
        alone = segment.segment_depth([dev[i]], **kw)
        for a, b, c, d in zip(_columns(together, i), _columns(alone, 0), _columns(again, i), _columns(shuffled, order.index(i))):
            assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, d)
    stacked = torch.stack([dev[0], dev[0].flip(0)])  # a [B,h,w] tensor
    seg = segment.segment_depth(stacked, **kw)
    check(seg, 1, np.ascontiguousarray(maps[0][::-1]), **kw)


def _cutout_case(H, W, seed=5):
    v = sc.piecewise(21, 70, 45, 0.004)
    seg = segment.segment_depth([torch.from_numpy(v).cuda()], min_area=16)
    res = sr.segment(v, min_area=16)
    photo = np.random.default_rng(seed).integers(1, 256, (H, W, 3), dtype=np.uint8)
    return v, seg, res, photo


def _dropped_point(res):
    ys, xs = np.nonzero(res["labels"] < 0)
    h, w = res["labels"].shape
    return ((xs[0] + 0.5) / w, (ys[0] + 0.5) / h)


@pytest.mark.parametrize("H,W", [(150, 131), (31, 22), (70, 45)])  # a photo larger than its map, smaller, of its size
def test_cutouts_equal_the_restatement(H, W):
    v, seg, res, photo = _cutout_case(H, W)
    big = int(np.argmax(res["area"]))
    y, x = divmod(int(res["first"][big]), 45)
    inside = ((x + 0.5) / 45, (y + 0.5) / 70)
    cases = [[inside], [inside, inside], [(0.0, 0.0), (1.0, 1.0), (0.5, 0.5)], [_dropped_point(res)], []]
    for points in cases:
        chosen = sr.picked(res["labels"], points)
        for invert in (False, True):
            want_bgra, want_mask = sr.cutout(res["labels"], photo, chosen, invert)
            for kw in (dict(points=[points]), dict(labels=[sorted(chosen)])):
                (bgra, mask), = segment.region_cutouts(seg, [photo], invert=invert, **kw)
                assert tuple(bgra.shape) == (H, W, 4) and tuple(mask.shape) == (H, W) and bgra.dtype == mask.dtype == torch.uint8
                assert np.array_equal(mask.cpu().numpy(), want_mask) and np.array_equal(bgra.cpu().numpy(), want_bgra), (points, invert, list(kw))
    assert sr.picked(res["labels"], cases[3]) == set() and len(sr.picked(res["labels"], cases[1])) == 1 and 0 < want_mask.mean() <= 255
    (_, none), = segment.region_cutouts(seg, [photo])
    assert not none.any()


def test_host_photos_and_pitched_device_views_are_the_same_photo_and_an_empty_result_cuts_nothing():
    H, W = 97, 61
    v, seg, res, photo = _cutout_case(H, W)
    points = [(0.5, 0.5), (0.1, 0.9)]
    want_bgra, want_mask = sr.cutout(res["labels"], photo, sr.picked(res["labels"], points))
    strided = np.zeros((H, W + 5, 3), np.uint8)
    strided[:, 2:2 + W] = photo
    big = torch.from_numpy(np.random.default_rng(9).integers(0, 256, (H + 20, W + 36, 3), dtype=np.uint8)).cuda()
    big[11:11 + H, 8:8 + W] = torch.from_numpy(photo).cuda()
    view = big[11:11 + H, 8:8 + W]
    assert not view.is_contiguous()
    for given in (photo, strided[:, 2:2 + W], view, torch.from_numpy(photo).cuda()):
        (bgra, mask), = segment.region_cutouts(seg, [given], points=[points])
        assert np.array_equal(mask.cpu().numpy(), want_mask) and np.array_equal(bgra.cpu().numpy(), want_bgra)
    empty = segment.segment_depth([torch.full((40, 37), float("nan")).cuda()], min_area=1)
    (bgra, mask), = segment.region_cutouts(empty, [photo], points=[points])
    assert int(empty.counts[0]) == 0 and not mask.any() and not bgra.any()
    (bgra, mask), = segment.region_cutouts(empty, [photo], points=[points], invert=True)
    assert (mask == 255).all() and np.array_equal(bgra[..., :3].cpu().numpy(), photo)


def test_several_photos_share_one_cutout_call_and_the_colors_are_the_hash():
    dev, maps = _four()
    kw = dict(step=0.02, min_area=4, connectivity=8)
    seg = segment.segment_depth(dev, **kw)
    rng = np.random.default_rng(3)
    photos = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in ((90, 50), (65, 40), (30, 70), (20, 130))]
    points = [[(0.3, 0.3)], [(0.0, 0.0), (0.99, 0.5)], [(0.5, 0.5)], []]
    got = segment.region_cutouts(seg, photos, points=points)
    for i in range(4):
        lab = sr.segment(maps[i], **kw)["labels"]
        bgra, mask = sr.cutout(lab, photos[i], sr.picked(lab, points[i]))
        assert np.array_equal(got[i][0].cpu().numpy(), bgra) and np.array_equal(got[i][1].cpu().numpy(), mask), i
        assert np.array_equal(segment.label_colors(seg)[i].cpu().numpy(), sr.colors(lab)), i


def _model(metric=False):
    from muggled_dpt_amd import make_depthanythingv2_dpt_from_original_state_dict as make
    from muggled_dpt_amd.synthetic import make_synthetic_original_state_dict
    model = make(make_synthetic_original_state_dict("tiny", 0))[1].to("cuda", torch.bfloat16)
    if metric:
        model.config["is_metric"] = True
    return model


def _photos():
    rng = np.random.default_rng(6)
    return {"a": rng.integers(0, 256, (150, 130, 3), dtype=np.uint8), "b": rng.integers(0, 256, (120, 200, 3), dtype=np.uint8)}


@pytest.mark.parametrize("metric", [False, True])
def test_inference_segments_is_inference_images_then_segment_depth(metric):
    model, photos = _model(metric), list(_photos().values())
    preds = model.inference_images(photos, 112, True, 32)
    got = model.inference_segments(photos, step=0.05, min_area=4, max_side_length=112)
    want = segment.segment_depth(preds, space="depth" if metric else "inverse", step=0.05, min_area=4)
    for i in range(2):
        assert all(torch.equal(a, b) for a, b in zip(_columns(got, i), _columns(want, i)))
        check(got, i, preds[i].reshape(preds[i].shape[-2:]).to(torch.float32).cpu().numpy(), space="depth" if metric else "inverse", step=0.05, min_area=4)


def test_segment_flags_write_the_labels_the_regions_and_the_picked_cutouts(tmp_path):
    photos = _photos()
    for k in photos:
        np.save(tmp_path / f"{k}.npy", photos[k])
    cmd = [sys.executable, os.path.join(REPO, "tools", "mdpt_run_image.py"), "--synthetic", "tiny", "-s", "112", "-i", str(tmp_path / "a.npy"), "-i",
           str(tmp_path / "b.npy"), "--segments", "0.05", "--segments_min_area", "4", "--segments_conn", "8", "--pick", "0.25", "0.75", "--pick", "0.5", "0.5"]
    r = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=REPO), cwd=tmp_path, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    frames = list(photos.values())
    seg = segment.segment_depth(_model().inference_images(frames, 112, True, 32), step=0.05, min_area=4, connectivity=8)
    cuts = segment.region_cutouts(seg, frames, points=[[(0.25, 0.75), (0.5, 0.5)]] * 2)
    for k, (name, rows) in enumerate(zip(photos, seg.region_views())):
        assert np.array_equal(np.load(tmp_path / f"{name}_labels.npy"), seg.labels[k].cpu().numpy())
        table = json.load(open(tmp_path / f"{name}_regions.json"))
        assert table["count"] == rows["count"] and table["area"] == rows["area"].tolist() and table["bbox"] == rows["bbox"].tolist()
        assert table["first"] == rows["first"].tolist() and table["mean"] == rows["mean"].tolist() and table["vmin"] == rows["vmin"].tolist()
        assert np.array_equal(np.load(tmp_path / f"{name}_pick_mask.npy"), cuts[k][1].cpu().numpy())
        assert np.array_equal(np.load(tmp_path / f"{name}_pick_cutout.npy"), cuts[k][0].cpu().numpy())
