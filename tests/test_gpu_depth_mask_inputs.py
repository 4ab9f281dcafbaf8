"""depth_mask_images on inputs the allocator lays out in ways a caller does not control: separately allocated maps of one size (small blocks that
usually sit back to back in one segment) and device photos that are views at an odd byte offset (the cutout kernel's byte-wise BGR path). Every
element equals the call on its map and photo alone, bit for bit."""
import numpy as np
import pytest
import torch

from muggled_dpt_amd import postprocess as pp

pytestmark = pytest.mark.gpu


def _points(hw, seed):
    np.random.seed(seed)
    return pp.plane_sample_points(hw)


def _photo(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _equal_to_single_calls(maps, photos, pts):
    many = pp.depth_mask_images(maps, photos, 0.5, (0.25, 0.8), sample_xy=pts)
    for k in range(len(maps)):
        [(cut, mask)] = pp.depth_mask_images([maps[k]], [photos[k]], 0.5, (0.25, 0.8), sample_xy=[pts[k]])
        assert torch.equal(many[k][0], cut) and torch.equal(many[k][1], mask), k
        assert bool((cut[:, :, 3] == mask).all()), k
    masks = torch.cat([m.reshape(-1) for _, m in many])
    assert bool((masks == 0).any()) and bool((masks == 255).any())  # both sides of the threshold occur


def test_separately_allocated_maps_of_one_size():
    g = torch.Generator(device="cuda").manual_seed(0)
    for h, w in ((64, 64), (512, 512)):
        maps = [torch.rand(h, w, device="cuda", generator=g) for _ in range(8)]
        photos = [_photo(40 + 3 * k, 70 - 2 * k, k) for k in range(8)]
        _equal_to_single_calls(maps, photos, [_points((h, w), k) for k in range(8)])


def test_device_photos_at_odd_offsets():
    g = torch.Generator(device="cuda").manual_seed(1)
    maps = [torch.rand(37, 50, device="cuda", generator=g) for _ in range(4)]
    big = torch.from_numpy(_photo(101, 63, 5)).cuda()
    photos = [big[1:], big[3:60], big[2:], big[5:6]]  # row views of an odd-width photo: data at byte offsets 189, 567, 378, 945
    assert [p.data_ptr() % 4 for p in photos] == [1, 3, 2, 1]
    pts = [_points((37, 50), k) for k in range(4)]
    _equal_to_single_calls(maps, photos, pts)
    host = pp.depth_mask_images(maps, [p.cpu().numpy() for p in photos], 0.5, (0.25, 0.8), sample_xy=pts)
    dev = pp.depth_mask_images(maps, photos, 0.5, (0.25, 0.8), sample_xy=pts)
    for (ch, mh), (cd, md) in zip(host, dev):
        assert torch.equal(ch, cd) and torch.equal(mh, md)
