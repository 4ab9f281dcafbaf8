"""Depth masking on the device (postprocess.depth_mask_display / depth_mask_images) against the reference's outputs (tests/golden/depth_mask.npz,
written by gen_depth_mask.py from the reference's plane fit, postprocess helpers and CheckerPattern) and the fp64 numpy restatements of
tests/mask_restate.py.

A mask byte may differ from the reference only where the fp64 value it thresholds is within 1e-5 of the threshold's min or max (the device's Jacobi
plane normal and numpy's SVD normal differ in the last bits). Where the masks agree, cutout bytes and checker bytes are exact and composite image
bytes are within 1 (cv2's uint8 resize is specified by its scalar fixed-point formula)."""
import os

import numpy as np
import pytest
import torch

from muggled_dpt_amd import postprocess as pp
from tests import mask_restate as mr

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "depth_mask.npz")
TIE = 1e-5


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def seeded_points(hw, seed):
    np.random.seed(seed)
    return pp.plane_sample_points(hw)


def near(v, tmin, tmax):
    with np.errstate(invalid="ignore"):
        return (np.abs(v - tmin) < TIE) | (np.abs(v - tmax) < TIE)


def check_mask(got, want, value, tmin, tmax, what):
    assert got.shape == want.shape and got.dtype == np.uint8, what
    differ = got != want
    bad = differ & ~near(value, tmin, tmax)
    assert not bad.any(), f"{what}: {int(bad.sum())} mask bytes differ away from the threshold (of {got.size})"
    return ~differ


def check_display(mask, comp, want_mask, want_comp, value, tmin, tmax, what):
    agree = check_mask(mask, want_mask, value, tmin, tmax, what)
    on = agree & (want_mask == 255)
    off = agree & (want_mask == 0)
    assert np.array_equal(comp[off], want_comp[off]), f"{what}: checker bytes differ"
    assert np.abs(comp[on].astype(np.int32) - want_comp[on].astype(np.int32)).max(initial=0) <= 1, f"{what}: image bytes differ by more than 1"


def check_cutout(cut, mask, want_cut, want_mask, value, tmin, tmax, what):
    agree = check_mask(mask, want_mask, value, tmin, tmax, what)
    assert cut.shape == want_cut.shape and cut.dtype == np.uint8, what
    assert np.array_equal(cut[agree], want_cut[agree]), f"{what}: cutout bytes differ where the masks agree"
    assert np.array_equal(cut[:, :, 3], mask), f"{what}: alpha is not the mask"


def test_display_and_save_equal_the_reference(gold):
    settings = gold["settings"]
    flips = 0
    for i in range(3):
        d, img = gold[f"map{i}"], gold[f"photo{i}"]
        wh = tuple(int(v) for v in gold[f"display_wh{i}"])
        pred = torch.from_numpy(d).cuda()[None]
        img_dev = torch.from_numpy(img).cuda()
        for j, (f, tmin, tmax, inv) in enumerate(settings):
            inv = bool(inv)
            what = f"map{i} setting{j}"
            seed = int(gold[f"case{i}_{j}_display_seed"])
            pts = seeded_points((wh[1], wh[0]), seed)
            mask, comp = pp.depth_mask_display(pred, img_dev, wh, f, (tmin, tmax), inv, sample_xy=pts)
            assert mask.shape == (1, wh[1], wh[0]) and comp.shape == (1, wh[1], wh[0], 3)
            _, _, n = mr.display(pred[0], img, wh, pts, f, tmin, tmax, inv)
            want_mask = gold[f"case{i}_{j}_display_mask"]
            check_display(mask[0].cpu().numpy(), comp[0].cpu().numpy(), want_mask, gold[f"case{i}_{j}_display_composite"], n, tmin, tmax, what + " display")
            flips += int((mask[0].cpu().numpy() != want_mask).sum())

            seed = int(gold[f"case{i}_{j}_save_seed"])
            pts = seeded_points(d.shape, seed)
            [(cut, sm)] = pp.depth_mask_images([pred], [img], f, (tmin, tmax), inv, sample_xy=[pts])
            assert cut.shape == img.shape[:2] + (4,) and sm.shape == img.shape[:2]
            _, _, s = mr.save(pred[0], img, pts, f, tmin, tmax, inv)
            check_cutout(cut.cpu().numpy(), sm.cpu().numpy(), gold[f"case{i}_{j}_save_cutout"], gold[f"case{i}_{j}_save_mask"], s, tmin, tmax, what + " save")
    assert flips <= 8, flips  # ties are rare: the bulk of every mask is exact


def _map(h, w, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    y, x = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    z = 1.0 + 0.02 * x - 0.03 * y + 0.5 * torch.sin(x / 5.0) * torch.cos(y / 7.0) + 0.05 * torch.randn(h, w, generator=g)
    return z.to(dtype).cuda()


def _photo(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_sizes_against_the_restatement(dtype):
    m = _map(37, 50, 3, dtype)
    for k, (ih, iw) in enumerate(((1, 1), (1, 77), (77, 1), (20, 31), (37, 50), (101, 63), (3024, 4032) if dtype == torch.float32 else (301, 403))):
        img = _photo(ih, iw, k)
        pts = seeded_points((37, 50), k)
        for f, (tmin, tmax), inv in ((0.5, (0.3, 0.8), False), (-0.5, (0.0, 0.45), True)):
            [(cut, mask)] = pp.depth_mask_images([m], [img], f, (tmin, tmax), inv, sample_xy=[pts])
            want_cut, want_mask, s = mr.save(m, img, pts, f, tmin, tmax, inv)
            check_cutout(cut.cpu().numpy(), mask.cpu().numpy(), want_cut, want_mask, s, tmin, tmax, f"{dtype} {ih}x{iw}")
    for k, (ih, iw, wh) in enumerate(((45, 61, (7, 5)), (480, 640, (211, 157)), (9, 5, (3, 9)), (37, 50, (50, 37)))):
        img = _photo(ih, iw, 10 + k)
        pts = seeded_points((wh[1], wh[0]), k)
        mask, comp = pp.depth_mask_display(m, torch.from_numpy(img).cuda(), wh, 0.75, (0.2, 0.9), bool(k % 2), sample_xy=pts)
        want_mask, want_comp, n = mr.display(m, img, wh, pts, 0.75, 0.2, 0.9, bool(k % 2))
        check_display(mask[0].cpu().numpy(), comp[0].cpu().numpy(), want_mask, want_comp, n, 0.2, 0.9, f"display {dtype} {ih}x{iw} -> {wh}")


def test_lists_equal_single_calls_bit_for_bit():
    sizes = [(37, 50), (50, 37), (37, 50), (64, 64), (50, 37)] * 8  # 40 maps: more than one table of photos
    maps = [_map(h, w, k) for k, (h, w) in enumerate(sizes)]
    rng = np.random.default_rng(0)
    photos = [_photo(int(rng.integers(1, 90)), int(rng.integers(1, 90)), k) for k in range(len(sizes))]
    photos[3] = _photo(3024, 4032, 99)
    pts = [seeded_points(hw, 50 + k) for k, hw in enumerate(sizes)]
    for f, thr, inv in ((0.0, (0.0, 1.0), False), (1.0, (0.5, 1.0), True)):
        many = pp.depth_mask_images(maps, photos, f, thr, inv, sample_xy=pts)
        dev = pp.depth_mask_images(maps, [torch.from_numpy(p).cuda() for p in photos], f, thr, inv, sample_xy=pts)
        assert len(many) == len(dev) == len(sizes)
        for k in range(len(sizes)):
            [(cut, mask)] = pp.depth_mask_images([maps[k]], [photos[k]], f, thr, inv, sample_xy=[pts[k]])
            assert torch.equal(many[k][0], cut) and torch.equal(many[k][1], mask), k
            assert torch.equal(dev[k][0], cut) and torch.equal(dev[k][1], mask), k
    # a [B,h,w] tensor (one size group read in place) equals its list
    batch = torch.stack([_map(37, 50, 200 + k) for k in range(3)])
    small = [_photo(30 + k, 41 - k, k) for k in range(3)]
    p3 = [seeded_points((37, 50), k) for k in range(3)]
    a = pp.depth_mask_images(batch, small, 0.5, (0.2, 0.8), sample_xy=p3)
    b = pp.depth_mask_images(list(batch.unbind(0)), small, 0.5, (0.2, 0.8), sample_xy=p3)
    for (ca, ma), (cb, mb) in zip(a, b):
        assert torch.equal(ca, cb) and torch.equal(ma, mb)
    # a display batch row equals the call on that row
    photos_dev = torch.from_numpy(np.stack([_photo(60, 80, k) for k in range(3)])).cuda()
    p3d = np.stack([seeded_points((45, 70), k) for k in range(3)])
    mask, comp = pp.depth_mask_display(batch, photos_dev, (70, 45), 0.5, (0.3, 0.9), sample_xy=p3d)
    for k in range(3):
        m1, c1 = pp.depth_mask_display(batch[k:k + 1], photos_dev[k], (70, 45), 0.5, (0.3, 0.9), sample_xy=p3d[k])
        assert torch.equal(mask[k], m1[0]) and torch.equal(comp[k], c1[0]), k


def test_bad_maps_stay_in_their_image():
    good = [_map(37, 50, 1), _map(37, 50, 2)]
    const = torch.full((37, 50), 3.0, device="cuda")
    nan = torch.full((37, 50), float("nan"), device="cuda")  # what non-finite propagation writes for an image
    maps = [good[0], const, nan, good[1]]
    photos = [_photo(40 + k, 55 + k, k) for k in range(4)]
    pts = [seeded_points((37, 50), k) for k in range(4)]
    for inv in (False, True):
        out = pp.depth_mask_images(maps, photos, 0.5, (0.2, 0.8), inv, sample_xy=pts)
        for k in (1, 2):
            cut, mask = out[k]
            assert bool((mask == (255 if inv else 0)).all()), (k, inv)
            want = np.concatenate((photos[k], np.full(photos[k].shape[:2] + (1,), 255, np.uint8)), axis=2) if inv else np.zeros(photos[k].shape[:2] + (4,), np.uint8)
            assert np.array_equal(cut.cpu().numpy(), want), (k, inv)
        for k in (0, 3):
            [(cut, mask)] = pp.depth_mask_images([maps[k]], [photos[k]], 0.5, (0.2, 0.8), inv, sample_xy=[pts[k]])
            assert torch.equal(out[k][0], cut) and torch.equal(out[k][1], mask), (k, inv)
        batch = torch.stack(maps)
        dev_photos = torch.from_numpy(np.stack([_photo(30, 40, k) for k in range(4)])).cuda()
        p4 = np.stack([seeded_points((25, 33), k) for k in range(4)])
        mask, comp = pp.depth_mask_display(batch, dev_photos, (33, 25), 0.5, (0.2, 0.8), inv, sample_xy=p4)
        for k in (1, 2):
            assert bool((mask[k] == (255 if inv else 0)).all()), (k, inv)
            if not inv:
                assert np.array_equal(comp[k].cpu().numpy(), np.repeat(mr.checker(25, 33)[:, :, None], 3, axis=2))
        for k in (0, 3):
            m1, c1 = pp.depth_mask_display(batch[k:k + 1], dev_photos[k], (33, 25), 0.5, (0.2, 0.8), inv, sample_xy=p4[k])
            assert torch.equal(mask[k], m1[0]) and torch.equal(comp[k], c1[0]), (k, inv)


def test_end_to_end_from_inference_images():
    from muggled_dpt_amd import make_depthanythingv2_dpt_from_original_state_dict
    from muggled_dpt_amd.synthetic import make_synthetic_original_state_dict
    _, model = make_depthanythingv2_dpt_from_original_state_dict(make_synthetic_original_state_dict("tiny", 0))
    model = model.to("cuda", torch.float32)
    photos = [_photo(h, w, k) for k, (h, w) in enumerate(((120, 90), (64, 200), (33, 47), (90, 120)))]
    depths = model.inference_images(photos, 56, use_square_sizing=False)
    pts = [seeded_points(tuple(d.shape[1:]), 7 + k) for k, d in enumerate(depths)]
    out = pp.depth_mask_images(depths, photos, 0.5, (0.25, 0.85), False, sample_xy=pts)
    for k, (d, img) in enumerate(zip(depths, photos)):
        want_cut, want_mask, s = mr.save(d[0], img, pts[k], 0.5, 0.25, 0.85, False)
        check_cutout(out[k][0].cpu().numpy(), out[k][1].cpu().numpy(), want_cut, want_mask, s, 0.25, 0.85, f"image {k}")
