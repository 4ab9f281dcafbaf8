"""DPTModel.inference_tiled: one inference_regions call (the whole image as region 0, the guide, then the tiles) and one postprocess.stitch_tiles
call. Bit for bit the same as those two calls made by hand, from host and from device images; region 0 is inference(image) in the default
(batch-invariant) modes; a 1 x 1 grid without alignment is cv2's resize of inference(image) (the restatement's); the command line writes a map of
the photo's size. Tiny synthetic models: output quality on photographs is not what is tested here."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from muggled_dpt_amd import postprocess as pp
from muggled_dpt_amd import tiling
from tests.test_gpu_c_host import _family_model
from tests.tile_restate import resize_tile, ulps

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HW = (150, 120)


def _bits(t):
    return t.view(torch.int16) if t.dtype != torch.float32 else t


def _model(family, dtype, precision):
    """a tiny synthetic model of the family on the GPU and a model tensor side that suits it"""
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    model, unit = _family_model(family)
    model = model.to("cuda", dtype)
    if precision:
        model.set_precision(precision)
    return model, (4 * unit if family != "swinv2" else 128)


def _photo():
    # smooth structure plus noise, so that tiles and guide correlate as depth maps of one scene do
    yy, xx = np.mgrid[:HW[0], :HW[1]]
    base = 128 + 90 * np.sin(yy / 23.0) * np.cos(xx / 17.0)
    rng = np.random.default_rng(5)
    return np.clip(base[:, :, None] + rng.normal(0, 12, (*HW, 3)), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("family,dtype,precision", [("v2", torch.bfloat16, None), ("v2", torch.float32, None), ("swinv2", torch.bfloat16, None)])
def test_inference_tiled_is_regions_plus_stitch_bit_for_bit(family, dtype, precision):
    model, side = _model(family, dtype, precision)
    img = _photo()
    boxes = tiling.tile_grid_boxes(HW, (2, 2), 0.25)
    regions = [(0, 0, 0, HW[1], HW[0])] + [(0, *b) for b in boxes]
    maps = model.inference_regions([img], regions, side)
    want, want_fit, want_sums = pp.stitch_tiles(maps[1:], boxes, HW, guide=maps[0], return_fit=True)
    dev_img = torch.from_numpy(img).cuda()
    for src in (img, dev_img):
        got, parts = model.inference_tiled(src, tiles=(2, 2), max_side_length=side, return_parts=True)
        assert got.shape == (1, *HW) and got.dtype == torch.float32
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
        assert torch.equal(parts["fit"], want_fit) and torch.equal(parts["sums"], want_sums) and parts["boxes"] == boxes
        assert len(parts["regions"]) == 5 and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(parts["regions"], maps))
        # region 0, the guide, is the plain inference of the image
        assert torch.equal(_bits(parts["regions"][0]), _bits(model.inference(img, side)))
        assert torch.equal(model.inference_tiled(src, tiles=(2, 2), max_side_length=side), got)
    assert bool(torch.isfinite(got).all()) and float(got.max() - got.min()) > 0
    # tile_hw: tiles of a given size with a fractional overlap are tile_boxes' layout
    th_boxes = tiling.tile_boxes(HW, (90, 70), (22, 18))
    got, parts = model.inference_tiled(img, tile_hw=(90, 70), overlap=0.25, max_side_length=side, return_parts=True)
    assert parts["boxes"] == th_boxes and len(th_boxes) == 4
    maps = model.inference_regions([img], [(0, 0, 0, HW[1], HW[0])] + [(0, *b) for b in th_boxes], side)
    assert torch.equal(got, pp.stitch_tiles(maps[1:], th_boxes, HW, guide=maps[0]))


def test_one_by_one_grid_without_alignment_is_the_resize_of_inference():
    model, side = _model("v2", torch.bfloat16, None)
    img = _photo()
    got, parts = model.inference_tiled(img, tiles=(1, 1), align="none", max_side_length=side, return_parts=True)
    assert parts["fit"] is None and parts["sums"] is None and parts["boxes"] == [(0, 0, HW[1], HW[0])]
    depth = model.inference(img, side)
    want = resize_tile(depth[0].float().cpu().numpy().astype(np.float64), (HW[1], HW[0])).astype(np.float32)
    assert ulps(got[0].cpu().numpy(), want) <= 1
    with pytest.raises(ValueError, match="either"):
        model.inference_tiled(img)
    with pytest.raises(ValueError, match="either"):
        model.inference_tiled(img, tiles=(2, 2), tile_hw=64)
    with pytest.raises(TypeError, match="one uint8"):
        model.inference_tiled([img], tiles=(2, 2))


def test_command_line_writes_a_map_of_the_photos_size(tmp_path):
    np.save(tmp_path / "photo.npy", _photo())
    env = dict(os.environ, PYTHONPATH=REPO)
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "mdpt_run_image.py"), "--synthetic", "tiny", "-i", str(tmp_path / "photo.npy"), "-s", "112",
                        "--tiles", "2", "2", "--tile_overlap", "0.3"], capture_output=True, text=True, env=env, cwd=tmp_path, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = np.load(tmp_path / "photo_tiled.npy")
    assert out.shape == HW and out.dtype == np.float32 and np.isfinite(out).all() and out.std() > 0
