"""postprocess.render_mesh / DPTModel.render_views (mdpt_post_render) against the numpy restatement of tests/render_restate.py, on the meshes
depth_frames_to_mesh makes on the device: on the restatement's safe pixels face ids, coverage and background are identical, colour is identical
(+-1 where its value before rounding lies within 1e-6 of a half), view depth within one fp32 ulp. tests/test_render_cpu.py holds every case to at
most 2 % unsafe pixels per image, with the mesh restatement's vertices; the share is asserted here again for the device's own vertices (which may
differ from those by one ulp)."""
import functools

import numpy as np
import pytest
import torch

from muggled_dpt_amd import orbit_camera as oc
from muggled_dpt_amd import postprocess as pp
from tests import render_restate as rr

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def device_mesh(name: str):
    """the case's slabs on the device, and the kept entries of every image on the host for the restatement"""
    c, frames, table, textures = rr.case_mesh_inputs(name)
    out = pp.depth_frames_to_mesh(torch.from_numpy(frames.copy()).cuda(), rr.IMAGE_WH, edge_threshold=c["thr"], vertex_xy=table, mode=c["mode"],
                                  grid_xy=c["grid"], **rr.MESH_CAMERA)
    kept = [(x.cpu().numpy(), u.cpu().numpy(), f.cpu().numpy().astype(np.int64)) for x, u, f, _ in pp.mesh_views(*out)]
    return out, kept, textures


@functools.lru_cache(maxsize=None)
def reference(name: str, wh, cull: str, point_size: float):
    _, kept, textures = device_mesh(name)
    return rr.render_case(kept, textures, rr.case_views(name, wh), wh, cull, point_size)


def compare(color, depth, ids, refs, tag):
    color, depth, ids = color.cpu().numpy(), depth.cpu().numpy(), ids.cpu().numpy()
    clean = 0
    for i, row in enumerate(refs):
        for v, r in enumerate(row):
            safe, where = r["safe"], (tag, i, v)
            share = float((~safe).mean())
            clean += share == 0.0
            assert share <= 0.02, where
            np.testing.assert_array_equal(ids[i, v][safe], r["ids"][safe], err_msg=str(where))
            np.testing.assert_array_equal(color[i, v][..., 3][safe], r["color"][..., 3][safe], err_msg=str(where))  # coverage
            diff = np.abs(color[i, v].astype(np.int64) - r["color"].astype(np.int64)).max(axis=-1)
            assert (diff[safe & ~r["soft"]] == 0).all() and (diff[safe] <= 1).all(), where
            d = rr.ulps(depth[i, v], r["depth"])
            print(f"{where}: covered {(r['ids'] >= 0).mean():.3f} unsafe {share:.4f} dropped {r['dropped']} boxes {r['small_boxes']}+{r['big_boxes']} "
                  f"depth ulps {d[safe].max()} colour diff {diff[safe].max()}")
            assert d[safe].max() <= 1, where
            bg = safe & (r["ids"] < 0)
            assert (color[i, v][bg] == 0).all() and (ids[i, v][bg] == -1).all() and np.isposinf(depth[i, v][bg]).all(), where
    assert clean >= 1, tag


def run(name, wh, cull="back", point_size=1.0, **kw):
    (xyz, uv, faces, counts, _), _, textures = device_mesh(name)
    return pp.render_mesh(xyz, uv, faces, counts, textures, rr.case_views(name, wh), wh, cull, point_size, **kw)


RUNS = [(n, wh, cull, ps) for n, c in rr.CASES.items() for wh in c["out_whs"] for cull in c["culls"] for ps in c["point_sizes"]]


@pytest.mark.parametrize("name, wh, cull, point_size", RUNS, ids=[f"{n}-{wh[0]}x{wh[1]}-{cull}-{ps}" for n, wh, cull, ps in RUNS])
def test_render_matches_restatement(name, wh, cull, point_size):
    """tri: B = 2 with different kept counts, three views (the third with part of the mesh behind the camera), two sizes, both cull modes;
    coop: faces above and below the small-box threshold; points: sizes 1 and 3; ties: vertices on pixel centres, the fill rule on the device"""
    color, depth, ids = run(name, wh, cull, point_size, return_depth=True, return_face_ids=True)
    refs = reference(name, wh, cull, point_size)
    b, v = len(refs), len(refs[0])
    assert color.shape == (b, v, wh[1], wh[0], 4) and depth.shape == ids.shape == (b, v, wh[1], wh[0])
    assert (color.dtype, depth.dtype, ids.dtype) == (torch.uint8, torch.float32, torch.int32)
    compare(color, depth, ids, refs, (name, wh, cull, point_size))


def test_ties_are_decided_by_the_fill_rule():
    color, ids = run("ties", rr.TIES_OUT_WH, "none", return_face_ids=True)
    want = np.zeros(rr.TIES_OUT_WH[::-1], dtype=bool)
    want[6:42, 8:56] = True  # the full grid spans columns 8.5 .. 56.5, rows 6.5 .. 42.5: left / top edges belong, right / bottom do not
    np.testing.assert_array_equal((ids[0, 0] >= 0).cpu().numpy(), want)
    np.testing.assert_array_equal(ids[0, 0].cpu().numpy(), reference("ties", rr.TIES_OUT_WH, "none", 1.0)[0][0]["ids"])


def test_empty_mesh_is_background():
    (xyz, uv, faces, counts, _), _, textures = device_mesh("tri")
    empty = torch.zeros_like(counts)
    # the slabs' tails are unspecified: poison them, nothing of them may be read into the result
    color, depth, ids = pp.render_mesh(torch.full_like(xyz, float("nan")), uv, torch.full_like(faces, 2 ** 30), empty, textures,
                                       rr.case_views("tri", (64, 48)), (64, 48), "none", return_depth=True, return_face_ids=True)
    assert (color == 0).all() and (ids == -1).all() and torch.isposinf(depth).all()
    # one empty, one not: the other image is what it is alone
    half = counts.clone()
    half[0] = 0
    color2 = pp.render_mesh(xyz, uv, faces, half, textures, rr.case_views("tri", (64, 48)), (64, 48))
    assert (color2[0] == 0).all() and torch.equal(color2[1], run("tri", (64, 48))[1])


def test_deterministic_and_views_independent():
    a = run("tri", (64, 48), "none", return_depth=True, return_face_ids=True)
    b = run("tri", (64, 48), "none", return_depth=True, return_face_ids=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    (xyz, uv, faces, counts, _), _, textures = device_mesh("tri")
    views = rr.case_views("tri", (64, 48))
    for v in range(views.shape[0]):
        one = pp.render_mesh(xyz, uv, faces, counts, textures, views[v:v + 1], (64, 48), "none", return_depth=True, return_face_ids=True)
        assert all(torch.equal(x[:, 0], y[:, v]) for x, y in zip(one, a)), v
    # chunked over views by the scratch cap: the same bytes; per-mesh matrices [B,V,16]: the same again
    small = pp.render_mesh(xyz, uv, faces, counts, textures, views, (64, 48), "none", return_depth=True, return_face_ids=True, max_scratch_bytes=1)
    assert all(torch.equal(x, y) for x, y in zip(small, a))
    per_mesh = pp.render_mesh(xyz, uv, faces, counts, textures, torch.from_numpy(np.stack([views, views])).cuda(), (64, 48), "none")
    assert torch.equal(per_mesh, a[0])


def test_slabs_are_read_in_place_and_texture_views_are_accepted():
    (xyz, uv, faces, counts, _), _, textures = device_mesh("tri")
    before = [(t.data_ptr(), t.clone()) for t in (xyz, uv, faces, counts)]
    want = run("tri", (37, 29))
    wide = [torch.from_numpy(np.concatenate([t, t], axis=1)).cuda() for t in textures]
    got = pp.render_mesh(xyz, uv, faces, counts, [w[:, :t.shape[1]] for w, t in zip(wide, textures)], rr.case_views("tri", (37, 29)), (37, 29))
    assert torch.equal(got, want)
    # (bit for bit: the slabs' tails are unspecified and may hold NaN left by whichever test owned the memory before, which compares unequal to itself)
    assert all(t.data_ptr() == p and torch.equal(t.view(torch.int32), c.view(torch.int32)) for t, (p, c) in zip((xyz, uv, faces, counts), before))


def test_render_views_is_the_four_step_composition():
    from muggled_dpt_amd import make_depthanythingv2_dpt_from_original_state_dict as make
    from tests.helpers import synthetic_model
    model = make(synthetic_model("tiny")[0])[1].to("cuda", torch.bfloat16)
    image = np.random.default_rng(5).integers(0, 256, size=(60, 84, 3)).astype(np.uint8)
    views = oc.swing_views(3, 9.0, 4.0, aspect=48 / 36)
    color, depth = model.render_views(image, views, (48, 36), max_side_length=112, target_num_faces=700, return_depth=True)
    assert color.shape == (1, 3, 36, 48, 4) and depth.shape == (1, 3, 36, 48) and (color[..., 3] == 255).any()
    frames = pp.pack_depth_u24_frames(model.inference(image, 112), is_metric=False)
    xyz, uv, faces, counts, _ = pp.depth_frames_to_mesh(frames, (84, 60), target_num_faces=700)
    want = pp.render_mesh(xyz, uv, faces, counts, [image], views, (48, 36), "back", 2.0, return_depth=True)
    assert torch.equal(color, want[0]) and torch.equal(depth, want[1])
    default = model.render_views(image, None, (48, 36), max_side_length=112, target_num_faces=700)
    assert default.shape == (1, 1, 36, 48, 4) and torch.equal(default[:, 0], model.render_views(image, oc.viewer_view_proj(aspect=48 / 36)[None], (48, 36),
                                                                                              max_side_length=112, target_num_faces=700)[:, 0])
