"""What the renderer's tests can check without a GPU: the restatement itself (tests/render_restate.py) is watertight and obeys the fill rule, the
orbit camera (muggled_dpt_amd/orbit_camera.py) against hand-evaluated matrices, the input condition of every case tests/test_gpu_render.py renders
(the unsafe share of the safe mask), and render_mesh's host-side argument checks."""
import functools
import math

import numpy as np
import pytest
import torch

from muggled_dpt_amd import orbit_camera as oc
from muggled_dpt_amd import postprocess as pp
from tests import mesh_restate as ms
from tests import render_restate as rr


@functools.lru_cache(maxsize=None)
def restated_meshes(name: str):
    """the kept (xyz fp32, uv fp32, faces) of every image of a case by the mesh restatement, and the textures"""
    c, frames, table, textures = rr.case_mesh_inputs(name)
    out = []
    for i in range(frames.shape[0]):
        m = ms.mesh_of_frame(frames[i], rr.IMAGE_WH, *c["grid"], edge_threshold=c["thr"], vertex_xy=table, mode=c["mode"], **rr.MESH_CAMERA)
        out.append((m["xyz"].astype(np.float32), m["uv"].astype(np.float32), m["faces"]))
    return out, textures


def case_runs(name: str):
    c = rr.CASES[name]
    return [(wh, cull, ps) for wh in c["out_whs"] for cull in c["culls"] for ps in c["point_sizes"]]


# ---- the input condition of the GPU cases

@pytest.mark.parametrize("name", list(rr.CASES))
def test_unsafe_share_of_every_gpu_case(name):
    meshes, textures = restated_meshes(name)
    for wh, cull, ps in case_runs(name):
        res = rr.render_case(meshes, textures, rr.case_views(name, wh), wh, cull, ps)
        shares = [float((~r["safe"]).mean()) for row in res for r in row]
        print(name, wh, cull, ps, "unsafe shares", shares, "covered", [float((r["ids"] >= 0).mean()) for row in res for r in row])
        assert max(shares) <= 0.02, (name, wh, cull, ps, shares)
        assert min(shares) == 0.0, (name, wh, cull, ps, shares)
        assert any((r["ids"] >= 0).any() for row in res for r in row)


def test_cases_exercise_what_they_claim():
    meshes, textures = restated_meshes("tri")
    assert len(meshes[0][2]) != len(meshes[1][2]) and all(len(m[2]) < 2 * 12 * 9 for m in meshes)  # kept counts differ, both drop faces
    res = rr.render_case(meshes, textures, rr.case_views("tri", (64, 48)), (64, 48), "none", 1.0)
    assert all(row[2]["dropped"] > 0 and (row[2]["ids"] >= 0).any() for row in res)  # the third pose: part of the mesh behind the camera
    assert all(row[0]["dropped"] == 0 for row in res)
    coop_meshes, coop_tex = restated_meshes("coop")
    (coop,), = rr.render_case(coop_meshes, coop_tex, rr.case_views("coop", (160, 120)), (160, 120), "back", 1.0)
    assert coop["small_boxes"] > 50 and coop["big_boxes"] > 50  # both raster paths
    # the ties case: vertices on pixel centres, so pixel centres ON edges (columns, rows and diagonals of the grid)
    tm, _ = restated_meshes("ties")
    X, Y, _, _, near = rr.vertex_stage(tm[0][0], rr.case_views("ties", rr.TIES_OUT_WH)[0], *rr.TIES_OUT_WH)
    assert not near.any() and ((X - 128) % 256 == 0).all() and ((Y - 128) % 256 == 0).all() and (np.diff(np.unique(X)) == 256 * rr.TIES_STEP).all()


# ---- watertightness and the fill rule of the restatement

def _full_mesh(nx=9, ny=7, seed=2):
    frames = rr.case_frames(24, 18, ("all255",), seed, True)
    table = ms.jitter_xy(nx, ny, 1.0, np.random.RandomState(seed))
    m = ms.mesh_of_frame(frames[0], rr.IMAGE_WH, nx, ny, edge_threshold=0.0, vertex_xy=table, **rr.MESH_CAMERA)
    return m["xyz"].astype(np.float32), m["uv"].astype(np.float32), m["faces"]


def _silhouette(X, Y, faces, W, H):
    """pixel centres strictly inside the union of the faces, by a floating-point test independent of the fill rule: inside some face with all three
    barycentrics above a margin, or within the margin of an edge that two faces share (interior edges)"""
    py, px = np.mgrid[:H, :W]
    P = np.stack([px * 256 + 128, py * 256 + 128], axis=-1).astype(np.float64)
    inside = np.zeros((H, W), dtype=bool)
    for f in faces:
        a, b, c = (np.array([X[i], Y[i]], dtype=np.float64) for i in f)
        den = (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])
        l1 = ((P[..., 0] - a[0]) * (c[1] - a[1]) - (P[..., 1] - a[1]) * (c[0] - a[0])) / den
        l2 = ((b[0] - a[0]) * (P[..., 1] - a[1]) - (b[1] - a[1]) * (P[..., 0] - a[0])) / den
        inside |= (l1 > 1e-9) & (l2 > 1e-9) & (1 - l1 - l2 > 1e-9)
    return inside


@pytest.mark.parametrize("pose", [dict(distance=2.3), dict(yaw_deg=31.0, pitch_deg=7.0, distance=2.6)], ids=["head_on", "oblique"])
def test_restatement_is_watertight(pose):
    xyz, uv, faces = _full_mesh()
    W, H = 71, 53
    M = oc.viewer_view_proj(rr.pose(**pose), min_depth=0.5, max_depth=20.0, view_fov_deg=31.0, aspect=W / H)
    tex = rr.case_texture(11, 9, 1)
    r = rr.render(xyz, uv, faces, tex, M, (W, H), cull="none")
    X, Y, *_ = rr.vertex_stage(xyz, M, W, H)
    interior = _silhouette(X, Y, faces, W, H)
    assert interior.sum() > 200
    assert (r["cover"][interior] >= 1).all()          # no crack: every pixel inside some face is covered
    assert (r["color"][..., 3][r["ids"] >= 0] == 255).all() and (r["color"][r["ids"] < 0] == 0).all()


def test_shared_edges_belong_to_exactly_one_face():
    """the regular grid through the orthographic camera (the ties case): no face overlaps another, the grid's lines pass through pixel centres, and
    every covered pixel is covered exactly once - for both windings"""
    meshes, textures = restated_meshes("ties")
    M = rr.case_views("ties", rr.TIES_OUT_WH)[0]
    for cull in ("back", "none"):
        r = rr.render(*meshes[0], textures[0], M, rr.TIES_OUT_WH, cull)
        cover = r["cover"]
        # the full grid spans columns 8.5 .. 56.5 and rows 6.5 .. 42.5: left / top edges belong, right / bottom edges do not
        want = np.zeros_like(cover)
        want[6:42, 8:56] = 1
        np.testing.assert_array_equal(cover, want)
        assert r["safe"].all()
    # the mirrored mesh (x negated, windings flipped) seen with cull "none" covers the same pixels once each
    xyz, uv, faces = meshes[0]
    flipped = rr.render(xyz * np.array([-1, 1, 1], np.float32), uv, faces, textures[0], M, rr.TIES_OUT_WH, "none")
    assert flipped["cover"].max() == 1 and flipped["cover"].sum() == 36 * 48
    assert rr.render(xyz * np.array([-1, 1, 1], np.float32), uv, faces, textures[0], M, rr.TIES_OUT_WH, "back")["cover"].sum() == 0


def test_points_and_texture_rule():
    M = oc.orthographic(-1, 1, -1, 1, -10, 10).reshape(16)
    xyz = np.array([[0.0, 0.0, -1.0]], np.float32)  # the middle of an 8 x 8 output: pixel corner (4, 4)
    uv = np.array([[0.25, 1.0]], np.float32)
    tex = np.zeros((2, 2, 3), np.uint8)
    tex[0, 0], tex[0, 1] = (10, 20, 30), (110, 120, 130)
    r = rr.render(xyz, uv, np.array([[0]]), tex, M, (8, 8), point_size=2.0)
    assert sorted(zip(*np.nonzero(r["ids"] >= 0))) == [(3, 3), (3, 4), (4, 3), (4, 4)]
    # u = 0.25 is the centre of texel 0 of 2; v = 1 the top edge of the first row (clamped)
    assert r["color"][3, 3].tolist() == [10, 20, 30, 255]
    r = rr.render(xyz, np.array([[0.5, 1.0]], np.float32), np.array([[0]]), tex, M, (8, 8), point_size=1.0)
    # a 1-pixel square on pixel corner (4, 4) spans [3.5, 4.5): half-open, it holds the centre at 3.5 alone; u = 0.5 is midway between the texels
    assert r["color"][3, 3].tolist() == [60, 70, 80, 255] and (r["ids"] >= 0).sum() == 1


# ---- the camera

def test_reset_pose_is_a_translation():
    cam = oc.OrbitCamera(50)
    want = np.eye(4)
    want[3, 2] = -50.0
    np.testing.assert_allclose(cam.world_to_view(), want, atol=1e-12)
    np.testing.assert_array_equal(cam.position_norm, [0, 0, 1])


def test_quarter_turn_puts_the_camera_on_the_x_axis():
    cam = oc.OrbitCamera(50)
    cam.rotate(-(math.pi / 2) / oc.ORBIT_SENSITIVITY, 0.0)  # rotate negates the drag: dx < 0 turns by +pi/2 about the world's up axis
    np.testing.assert_allclose(cam.position_norm, [1, 0, 0], atol=1e-12)
    np.testing.assert_allclose(cam.right, [0, 0, -1], atol=1e-12)
    np.testing.assert_allclose(cam.up, [0, 1, 0], atol=1e-12)
    snapped = oc.OrbitCamera(50)
    snapped.snap_to_axis(snap_x=True)
    np.testing.assert_allclose(cam.world_to_view(), snapped.world_to_view(), atol=1e-12)
    cam = oc.OrbitCamera(50)
    cam.rotate((math.pi / 2) / oc.ORBIT_SENSITIVITY, 0.0)
    np.testing.assert_allclose(cam.position_norm, [-1, 0, 0], atol=1e-12)
    np.testing.assert_allclose(cam.right, [0, 0, 1], atol=1e-12)


def test_camera_invariants():
    rng = np.random.RandomState(4)
    cam = oc.OrbitCamera(7.0)
    for dx, dy in rng.uniform(-300, 300, size=(1000, 2)):
        cam.rotate(dx, dy)
    forward = -cam.position_norm
    for a in (cam.up, cam.right, forward):
        assert abs(np.linalg.norm(a) - 1.0) < 1e-12
    assert abs(cam.up @ cam.right) < 1e-9 and abs(cam.up @ forward) < 1e-9 and abs(cam.right @ forward) < 1e-9
    cam.translate(13.0, -4.0, 2.0)
    real_origin = cam.origin + cam.origin_offset
    la = oc.look_at(cam.position_norm * cam.distance + real_origin, real_origin, cam.up)
    np.testing.assert_allclose(cam.world_to_view() @ la, np.eye(4), atol=1e-12)


def test_zoom_translate_offset():
    cam = oc.OrbitCamera(50)
    cam.zoom(1)
    assert cam.distance == 50 * 0.95
    cam.zoom(-1)
    cam.zoom(-1)
    assert abs(cam.distance - 50 / 0.95) < 1e-12
    for _ in range(200):
        cam.zoom(-1)
    assert cam.distance == 500.0
    cam.translate(100.0, 40.0, 0.0)
    np.testing.assert_allclose(cam.origin, [-0.5, 0.2, 0.0], atol=1e-15)
    cam.set_origin_offset(10.0, math.radians(30.0))
    np.testing.assert_allclose(cam.origin_offset, [0.0, -5.0, -10.0 * math.cos(math.radians(30.0))], atol=1e-12)


def test_projection_entries():
    fov, aspect = math.radians(60.0), 16 / 9
    p = oc.OrbitCamera().view_to_clip(fov, aspect)
    near, far = 0.0125, 1000.0
    f = math.tan(0.5 * (math.pi - fov))  # = 1 / tan(30 deg) = sqrt(3)
    assert abs(f - math.sqrt(3.0)) < 1e-12
    want = np.zeros((4, 4))
    want[0, 0], want[1, 1], want[2, 2], want[2, 3], want[3, 2] = f / aspect, f, (near + far) / (near - far), -1.0, 2 * near * far / (near - far)
    np.testing.assert_allclose(p, want, rtol=1e-15, atol=0)
    cam = oc.OrbitCamera(50)
    cam.set_origin_offset(50.0, 0.0)
    o = cam.view_to_clip(fov, 2.0, True)
    zoom = (50.0 - 25.0) * 0.5
    np.testing.assert_allclose(np.diag(o), [1 / (2 * zoom), 1 / zoom, 2 / (-2000.0), 1.0], rtol=1e-15)
    assert o[3, 2] == 0.0


def test_viewer_view_proj_and_views():
    cam = oc.OrbitCamera()
    m = oc.viewer_view_proj(cam, tilt_deg=10.0, view_offset=0.5, min_depth=50.0, max_depth=100.0, aspect=1.5).reshape(4, 4)
    np.testing.assert_allclose(cam.origin_offset, [0, -50 * math.sin(math.radians(10)), -50 * math.cos(math.radians(10))], atol=1e-12)
    want = oc.rotate_x(-math.radians(10.0)) @ (cam.world_to_view() @ oc.perspective(math.radians(60.0), 1.5))
    np.testing.assert_allclose(m, want, atol=1e-13)
    far = oc.OrbitCamera()
    oc.viewer_view_proj(far, view_offset=0.75)  # min + (max - min) (2 x 0.75 - 1)
    assert far.origin_offset[2] == -75.0
    # the mesh's middle (0, 0, -75) lands in the middle of the screen, in front of the camera
    clip = np.array([0.0, 0.0, -50.0, 1.0]) @ oc.viewer_view_proj().reshape(4, 4)
    assert abs(clip[0]) < 1e-9 and abs(clip[1]) < 1e-9 and abs(clip[3] - 50.0) < 1e-9
    swing = oc.swing_views(8, 10.0, 5.0, aspect=1.5)
    assert swing.shape == (8, 16) and len({s.tobytes() for s in swing}) == 8
    np.testing.assert_allclose(oc.swing_views(4, 0.0, 0.0)[2], oc.viewer_view_proj(), atol=1e-12)
    left, right = oc.stereo_views(2.0).reshape(2, 4, 4)
    p = np.array([0.0, 0.0, -50.0, 1.0])
    assert (p @ left)[0] > 0 > (p @ right)[0]  # seen from the left eye, the point lies to the right
    np.testing.assert_allclose((p @ left)[0], -(p @ right)[0], rtol=1e-12)


# ---- render_mesh's host-side checks

def _slabs(b=2, nv=6, nf=4, per=3):
    return (torch.zeros((b, nv, 3)), torch.zeros((b, nv, 2)), torch.zeros((b, nf, per), dtype=torch.int32), torch.zeros((b, 2), dtype=torch.int32))


@pytest.mark.parametrize("change, match", [
    (dict(xyz=torch.zeros((2, 6, 2))), "render_mesh: xyz must be float32"),
    (dict(uv=torch.zeros((2, 5, 2))), "render_mesh: uv must be float32"),
    (dict(faces=torch.zeros((2, 4, 3), dtype=torch.int64)), "render_mesh: faces must be int32"),
    (dict(faces=torch.zeros((2, 4, 1), dtype=torch.int32)), "render_mesh: a point list holds one face per vertex"),
    (dict(counts=torch.zeros((2, 3), dtype=torch.int32)), "render_mesh: counts must be int32"),
    (dict(cull="front"), "render_mesh: cull must be"),
    (dict(point_size=0.0), "render_mesh: point_size must be"),
    (dict(out_wh=(0, 4)), "render_mesh: out_wh must be"),
    (dict(view_proj=np.zeros((3, 15))), "render_mesh: view_proj must be"),
    (dict(view_proj=np.zeros((3, 2, 16))), "render_mesh: view_proj must be"),
    (dict(view_proj=np.full((1, 16), np.nan)), "render_mesh: view_proj holds values"),
    (dict(max_scratch_bytes=0), "render_mesh: max_scratch_bytes must be"),
])
def test_render_mesh_argument_checks(change, match):
    xyz, uv, faces, counts = _slabs()
    args = dict(xyz=xyz, uv=uv, faces=faces, counts=counts, textures_bgr=[np.zeros((2, 2, 3), np.uint8)] * 2, view_proj=np.zeros((1, 16)), out_wh=(8, 8))
    args.update(change)
    with pytest.raises(ValueError, match=match):
        pp.render_mesh(**args)


def test_render_mesh_texture_and_device_checks():
    xyz, uv, faces, counts = _slabs()
    with pytest.raises(ValueError, match="render_mesh: 2 predictions but 1 images"):
        pp.render_mesh(xyz, uv, faces, counts, [np.zeros((2, 2, 3), np.uint8)], np.zeros((1, 16)), (8, 8))
    with pytest.raises(TypeError, match="render_mesh expects OpenCV-style uint8"):
        pp.render_mesh(xyz, uv, faces, counts, [np.zeros((2, 2), np.uint8)] * 2, np.zeros((1, 16)), (8, 8))
    with pytest.raises(TypeError, match="render_mesh: xyz must be a tensor"):
        pp.render_mesh(xyz.numpy(), uv, faces, counts, [np.zeros((2, 2, 3), np.uint8)] * 2, np.zeros((1, 16)), (8, 8))
    with pytest.raises(RuntimeError, match="render_mesh: expected a CUDA tensor"):  # host slabs: there is no CPU renderer in the package
        pp.render_mesh(xyz, uv, faces, counts, [np.zeros((2, 2, 3), np.uint8)] * 2, np.zeros((1, 16)), (8, 8))
