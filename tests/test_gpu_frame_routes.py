"""Every uint8 route is a list of views: DPTModel.inference_regions on device images hands the library what DPTModel.inference_images gets for
the device views img[y1:y2, x1:x2] - the view's own pointer and row pitch with a full box - so the two routes have to agree on every bit,
whatever the chunking. Pins the identity base pointer + box == view pointer for the boxes where it could break: the image's last pixel, one
row, the whole image."""
import pytest
import torch

from tests.test_gpu_regions import SMALL_HW, _bits, _device, _image, _model

pytestmark = pytest.mark.gpu

# (image, x1, y1, x2, y2) on a 333-row image of 217 pixels (row pitch 651 bytes) and a 240-row image of 400
REGIONS = [
    (0, 216, 332, 217, 333),  # 1 x 1 at the last pixel of the allocation
    (1, 399, 239, 400, 240),
    (0, 5, 332, 211, 333),    # one row (the last)
    (1, 0, 100, 400, 101),    # one full row: a packed view
    (0, 0, 0, 217, 333),      # the full image: a packed view
    (1, 0, 0, 400, 240),
    (0, 33, 41, 160, 230),    # interior, odd x1
    (1, 100, 40, 200, 90),
]


def test_device_regions_equal_inference_images_on_the_device_views_bit_for_bit():
    model, side = _model("v2", torch.float32, None)
    images = _device([_image(SMALL_HW, 11), _image((240, 400), 13)])
    views = [images[i][y1:y2, x1:x2] for i, x1, y1, x2, y2 in REGIONS]
    assert [v.is_contiguous() for v in views] == [True, True, True, True, True, True, False, False]  # (single rows count as packed)
    for square in (True, False):
        for batch_size in (3, 32):  # below the region count (several chunks per group) and above it
            got = model.inference_regions(images, REGIONS, side, square, batch_size)
            want = model.inference_images(views, side, square, batch_size)
            assert len(got) == len(want) == len(REGIONS)
            for r, (g, w) in enumerate(zip(got, want)):
                assert g.shape == w.shape and g.dtype == w.dtype, (square, batch_size, r)
                assert torch.equal(_bits(g), _bits(w)), f"square={square} batch_size={batch_size}: region {r} differs from its view"
            assert all(float(t.abs().max()) > 0 for t in want)
            assert not torch.equal(want[4], want[6]) and not torch.equal(want[5], want[7])
        if not square:
            assert len({tuple(t.shape) for t in want}) > 2  # aspect sizing: several tensor sizes, so several groups
