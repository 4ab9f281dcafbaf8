"""render_mesh / DPTModel.render_views / tools/mdpt_run_image.py --render with hole filling: the fill_holes argument is render_mesh followed by
postprocess.fill_holes, bit for bit, face ids untouched; None is the call as it was."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from muggled_dpt_amd import orbit_camera as oc
from muggled_dpt_amd import postprocess as pp
from tests import render_restate as rr
from tests.test_gpu_render_tool import _decode_png

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WH = (64, 48)


def tri_mesh():
    c, frames, table, textures = rr.case_mesh_inputs("tri")
    out = pp.depth_frames_to_mesh(torch.from_numpy(frames.copy()).cuda(), rr.IMAGE_WH, edge_threshold=c["thr"], vertex_xy=table, mode=c["mode"],
                                  grid_xy=c["grid"], **rr.MESH_CAMERA)
    return out[:4], textures, rr.case_views("tri", WH)


def test_render_with_fill_is_render_then_fill():
    slabs, textures, views = tri_mesh()
    plain = pp.render_mesh(*slabs, textures, views, WH, "back", 1.0, return_depth=True, return_face_ids=True)
    color, depth, ids = pp.render_mesh(*slabs, textures, views, WH, "back", 1.0, return_depth=True, return_face_ids=True, fill_holes=0.1)
    want_c, want_d = pp.fill_holes(plain[0], plain[1], 0.1, return_depth=True)
    assert torch.equal(color, want_c) and torch.equal(depth.view(torch.int32), want_d.view(torch.int32)) and torch.equal(ids, plain[2])
    holes = plain[0][..., 3] == 0
    assert holes.any() and (ids[holes] == -1).all()
    covered = (plain[0][..., 3] != 0).flatten(2).any(dim=2)  # [B,V]
    assert covered.any() and (color[covered][..., 3] == 255).all() and torch.isfinite(depth[covered]).all()
    assert (color[~covered] == 0).all()
    assert torch.equal(color[~holes], plain[0][~holes])
    # the colour alone, and chunked over views and images by the scratch cap
    assert torch.equal(pp.render_mesh(*slabs, textures, views, WH, "back", 1.0, fill_holes=0.1), color)
    assert torch.equal(pp.render_mesh(*slabs, textures, views, WH, "back", 1.0, max_scratch_bytes=1, fill_holes=0.1), color)
    only_ids = pp.render_mesh(*slabs, textures, views, WH, "back", 1.0, return_face_ids=True, fill_holes=0.1)
    assert len(only_ids) == 2 and torch.equal(only_ids[0], color) and torch.equal(only_ids[1], plain[2])


def test_fill_holes_none_is_the_call_as_it_was():
    slabs, textures, views = tri_mesh()
    a = pp.render_mesh(*slabs, textures, views, WH, "none", 1.0, return_depth=True, return_face_ids=True)
    b = pp.render_mesh(*slabs, textures, views, WH, "none", 1.0, return_depth=True, return_face_ids=True, fill_holes=None)
    assert all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(a, b))
    assert (a[0][..., 3] == 0).any()
    with pytest.raises(ValueError, match=r"fill_holes must be in \[0, 1\]"):
        pp.render_mesh(*slabs, textures, views, WH, fill_holes=2.0)
    with pytest.raises(TypeError, match="fill_holes must be a number"):
        pp.render_mesh(*slabs, textures, views, WH, fill_holes=True)


def test_render_views_fills_every_view():
    from muggled_dpt_amd import make_depthanythingv2_dpt_from_original_state_dict as make
    from tests.helpers import synthetic_model
    model = make(synthetic_model("tiny")[0])[1].to("cuda", torch.bfloat16)
    image = np.random.default_rng(5).integers(0, 256, size=(60, 84, 3)).astype(np.uint8)
    views = oc.swing_views(3, 9.0, 4.0, aspect=48 / 36)
    plain = model.render_views(image, views, (48, 36), max_side_length=112, target_num_faces=700, return_depth=True)
    color, depth = model.render_views(image, views, (48, 36), max_side_length=112, target_num_faces=700, return_depth=True, fill_holes=0.1)
    assert color.shape == (1, 3, 36, 48, 4) and depth.shape == (1, 3, 36, 48)
    assert (plain[0][..., 3] == 0).any() and (color[..., 3] == 255).all() and torch.isfinite(depth).all()
    want = pp.fill_holes(plain[0], plain[1], 0.1, return_depth=True)
    assert torch.equal(color, want[0]) and torch.equal(depth, want[1])


def test_tool_render_fill_writes_opaque_pngs(tmp_path):
    img = np.random.default_rng(2).integers(0, 256, (90, 120, 3), dtype=np.uint8)
    np.save(tmp_path / "photo.npy", img)
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "mdpt_run_image.py"), "--synthetic", "tiny", "-i", str(tmp_path / "photo.npy"), "-s", "112",
                        "--render", str(tmp_path / "out"), "--render_views", "3", "--render_swing", "10", "5", "--render_wh", "96", "54", "--mesh_faces", "2000",
                        "--render_fill"],
                       capture_output=True, text=True, cwd=REPO, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    names = sorted(os.listdir(tmp_path / "out"))
    assert names == ["photo_view000.png", "photo_view001.png", "photo_view002.png"]
    views = [_decode_png((tmp_path / "out" / n).read_bytes()) for n in names]
    assert all(v.shape == (54, 96, 4) and (v[..., 3] == 255).all() for v in views) and not np.array_equal(views[0], views[1])
