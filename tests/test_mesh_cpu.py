"""The host side of the depth-to-mesh export, no GPU: the grid rule of mdpt_post_mesh_grid against tests/mesh_restate.py, the jitter helper, the
.glb / .obj / PNG writers of muggled_dpt_amd/mesh_io.py parsed back with struct, json and zlib, and argument checks that raise before any
device call."""
import ctypes
import json
import struct
import zlib

import numpy as np
import pytest
import torch

from muggled_dpt_amd import mesh_io, native
from muggled_dpt_amd import postprocess as pp
from tests import mesh_restate as ms


@pytest.fixture(scope="module")
def lib():
    return native.load()


# (w, h, target faces): targets below 2, a very wide and a very tall photo, rx on .5 (tv = 25, w / h = 1 / 4 -> rx = 2.5 -> 3), ry on .5
# (w / h = 4), the viewer's default target and its maximum, a fractional target
GRID_CASES = [(640, 480, 0), (640, 480, 1.5), (640, 480, 2), (518, 518, 312500), (1920, 1080, 250000), (10000, 10, 5000), (10, 10000, 5000),
              (1, 4, 38), (4, 1, 38), (3, 2, 2000000), (7, 5, 100), (1024, 768, 5000000), (800, 600, 19531.25)]


@pytest.mark.parametrize("w,h,target", GRID_CASES)
def test_grid_rule(lib, w, h, target):
    nx, ny = ctypes.c_int32(), ctypes.c_int32()
    assert lib.mdpt_post_mesh_grid(w, h, float(target), ctypes.byref(nx), ctypes.byref(ny)) == 0
    assert (nx.value, ny.value) == ms.plane_grid(w, h, target)
    assert pp.mesh_plane_grid((w, h), target)[:2] == (nx.value, ny.value)
    assert nx.value >= 2 and ny.value >= 2


def test_grid_half_cases_round_up():
    assert ms.plane_grid(1, 4, 38) == (3, 10)  # rx = sqrt(25 / 4) = 2.5 exactly
    assert ms.plane_grid(4, 1, 38) == (10, 3)  # ry = 10 / 4 = 2.5 exactly
    assert ms.js_round(2.5) == 3 and ms.js_round(-2.5) == -2 and ms.js_round(2.4999) == 2


def test_grid_rejects(lib):
    nx, ny = ctypes.c_int32(), ctypes.c_int32()
    assert lib.mdpt_post_mesh_grid(0, 4, 10.0, ctypes.byref(nx), ctypes.byref(ny)) == -1
    assert lib.mdpt_post_mesh_grid(4, 4, float("nan"), ctypes.byref(nx), ctypes.byref(ny)) == -1
    assert lib.mdpt_post_mesh_grid(4, 4, 1e10, ctypes.byref(nx), ctypes.byref(ny)) == -1  # 2^31 vertices or more
    assert b"2^31" in lib.mdpt_last_error()
    assert lib.mdpt_post_mesh_grid(4, 4, 10.0, None, ctypes.byref(ny)) == -1


def test_entry_point_rejects_before_launching(lib):
    fake = ctypes.c_void_p(4096)
    need = ctypes.c_size_t()
    assert lib.mdpt_post_mesh_scratch_bytes(2, 3, 2, ctypes.byref(need)) == 0
    assert need.value == 4 * 2 * (6 + 1 + 1 + 6)

    def call(B=2, H=5, W=7, nx=3, ny=2, mode=0, thr=0.0, frames=fake, scratch_bytes=need.value):
        return lib.mdpt_post_mesh(frames, B, H, W, nx, ny, None, 0.01, 0.01, 0.5, 1.0, 1.0, thr, 0, mode, fake, fake, fake, fake, fake, fake, scratch_bytes,
                                  None)

    assert call(nx=1) == -1 and b"at least 2" in lib.mdpt_last_error()
    assert call(ny=1) == -1
    assert call(nx=65536, ny=32768) == -1 and b"2^31" in lib.mdpt_last_error()
    assert call(B=0) == -1 and call(H=0) == -1 and call(W=0) == -1
    assert call(mode=2) == -1
    assert call(thr=float("nan")) == -1
    assert call(frames=None) == -1
    assert call(frames=ctypes.c_void_p(4097)) == -1
    assert call(scratch_bytes=need.value - 4) == -1 and b"scratch" in lib.mdpt_last_error()
    assert lib.mdpt_post_mesh_scratch_bytes(2, 1, 2, ctypes.byref(need)) == -1


def test_python_rejects_before_the_device():
    frames = torch.zeros((1, 5, 7, 4), dtype=torch.uint8)
    ok = dict(image_wh=(7, 5), fov_deg=50.0, min_depth=1.0, max_depth=2.0)
    for bad, exc in ((dict(mode="lines"), ValueError), (dict(fov_deg=180.0), ValueError), (dict(fov_deg=0.0), ValueError),
                     (dict(min_depth=0.0), ValueError), (dict(min_depth=3.0), ValueError), (dict(edge_threshold=1.5), ValueError),
                     (dict(edge_threshold=float("nan")), ValueError), (dict(image_wh=(0, 5)), ValueError), (dict(grid_xy=(1, 2)), ValueError),
                     (dict(target_num_faces=float("inf")), ValueError), (dict(grid_xy=(3, 2), vertex_xy=np.zeros((5, 2))), ValueError),
                     (dict(grid_xy=(3, 2), vertex_xy=np.zeros((6, 2), dtype=np.int32)), ValueError),
                     (dict(grid_xy=(3, 2), vertex_xy=np.full((6, 2), np.nan)), ValueError)):
        with pytest.raises(exc):
            pp.depth_frames_to_mesh(frames, **{**ok, **bad})
    with pytest.raises(TypeError):
        pp.depth_frames_to_mesh(frames.float(), **ok)
    with pytest.raises(TypeError):
        pp.depth_frames_to_mesh(frames[..., :3], **ok)
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # a host tensor: there is no CPU implementation
        pp.depth_frames_to_mesh(frames, **ok)
    with pytest.raises(ValueError):
        pp.mesh_plane_grid((7, 5), 100, jitter_pct=1.5)


def test_jitter_helper_follows_the_rule():
    nx, ny, none = pp.mesh_plane_grid((64, 48), 400)
    assert none is None and (nx, ny) == ms.plane_grid(64, 48, 400)
    for make in (np.random.RandomState, np.random.default_rng):
        nx2, ny2, xy = pp.mesh_plane_grid((64, 48), 400, jitter_pct=0.7, rng=make(5))
        assert (nx2, ny2) == (nx, ny) and xy.dtype == np.float64 and xy.shape == (nx * ny, 2)
        np.testing.assert_array_equal(xy, ms.jitter_xy(nx, ny, 0.7, make(5)))
        base = ms.grid_xy(nx, ny)
        border = (np.abs(base[:, 0]) == 1) | (np.abs(base[:, 1]) == 1)
        np.testing.assert_array_equal(xy[border], base[border])
        assert (xy[~border] != base[~border]).any(axis=1).all()
        assert np.abs(xy[:, 0] - base[:, 0]).max() <= 0.7 * (2 / (nx - 1)) * 0.45 and np.abs(xy[:, 1] - base[:, 1]).max() <= 0.7 * (2 / (ny - 1)) * 0.45


def _png_pixels(png: bytes) -> np.ndarray:
    assert png[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(png):
        n, kind = struct.unpack(">I4s", png[pos:pos + 8])
        data = png[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", png[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(kind + data) & 0xFFFFFFFF
        chunks.append((kind, data))
        pos += 12 + n
    assert [k for k, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    w, h, depth, ctype, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, comp, filt, lace) == (8, 0, 0, 0)
    ch = {0: 1, 2: 3, 6: 4}[ctype]
    rows = np.frombuffer(zlib.decompress(chunks[1][1]), dtype=np.uint8).reshape(h, 1 + w * ch)
    assert (rows[:, 0] == 0).all()
    return rows[:, 1:].reshape(h, w, ch)


def _mesh(rng, nv, nf, per_face):
    xyz = rng.standard_normal((nv, 3)).astype(np.float32) * np.float32(37.5)
    xyz[0] = (0.0, -0.0, 1e-7)
    uv = rng.random((nv, 2)).astype(np.float32)
    faces = rng.integers(0, nv, size=(nf, per_face)).astype(np.int32)
    return xyz, uv, faces


@pytest.mark.parametrize("per_face,nv,nf,tex_hw", [(3, 11, 7, (5, 3)), (1, 6, 6, (4, 4)), (3, 4, 2, (1, 1))])
def test_write_glb_parses_back(tmp_path, per_face, nv, nf, tex_hw):
    rng = np.random.default_rng(per_face + nv)
    xyz, uv, faces = _mesh(rng, nv, nf, per_face)
    tex = rng.integers(0, 256, size=tex_hw + (3,), dtype=np.uint8)
    bounds = np.stack([xyz.min(axis=0), xyz.max(axis=0)])
    path = tmp_path / "m.glb"
    mesh_io.write_glb(path, torch.from_numpy(xyz), uv, faces, tex, bounds)
    raw = path.read_bytes()
    assert raw == mesh_io.glb_bytes(xyz, uv, faces, tex)  # (bounds computed by the writer are the same)
    magic, version, total = struct.unpack("<III", raw[:12])
    assert (magic, version, total) == (0x46546C67, 2, len(raw)) and total % 4 == 0
    jlen, jkind = struct.unpack("<II", raw[12:20])
    assert jkind == 0x4E4F534A and jlen % 4 == 0
    text = raw[20:20 + jlen]
    doc = json.loads(text)
    assert text.rstrip(b" ") == json.dumps(doc, separators=(",", ":")).encode() and len(text) - len(text.rstrip(b" ")) < 4
    blen, bkind = struct.unpack("<II", raw[20 + jlen:28 + jlen])
    assert bkind == 0x004E4942 and blen % 4 == 0 and 28 + jlen + blen == total
    body = raw[28 + jlen:]
    assert doc["buffers"] == [{"byteLength": blen}]
    views = doc["bufferViews"]
    assert [v["byteOffset"] for v in views] == [0, 12 * nv, 20 * nv, 20 * nv + 4 * nf * per_face]
    assert [v["byteLength"] for v in views[:3]] == [12 * nv, 8 * nv, 4 * nf * per_face]
    assert [v.get("target") for v in views] == [34962, 34962, 34963, None]
    assert views[3]["byteOffset"] + views[3]["byteLength"] <= blen < views[3]["byteOffset"] + views[3]["byteLength"] + 4
    assert body[views[3]["byteOffset"] + views[3]["byteLength"]:] == b"\0" * (blen - views[3]["byteOffset"] - views[3]["byteLength"])
    piece = lambda i: body[views[i]["byteOffset"]:views[i]["byteOffset"] + views[i]["byteLength"]]  # noqa: E731
    assert piece(0) == xyz.tobytes() and piece(1) == uv.tobytes() and piece(2) == faces.astype("<u4").tobytes()
    np.testing.assert_array_equal(_png_pixels(piece(3)), tex[::-1])  # (the photo's rows, last first: test_glb_texture_orientation)
    acc = doc["accessors"]
    assert [(a["bufferView"], a["componentType"], a["count"], a["type"]) for a in acc] == [(0, 5126, nv, "VEC3"), (1, 5126, nv, "VEC2"),
                                                                                           (2, 5125, nf * per_face, "SCALAR")]
    assert np.array_equal(np.float32(acc[0]["min"]), bounds[0]) and np.array_equal(np.float32(acc[0]["max"]), bounds[1])
    prim = doc["meshes"][0]["primitives"][0]
    assert prim == {"attributes": {"POSITION": 0, "TEXCOORD_0": 1}, "indices": 2, "material": 0, "mode": 0 if per_face == 1 else 4}
    assert doc["materials"] == [{"extensions": {"KHR_materials_unlit": {}}, "pbrMetallicRoughness": {"baseColorTexture": {"index": 0}}}]
    assert doc["extensionsUsed"] == ["KHR_materials_unlit"] and doc["images"] == [{"bufferView": 3, "mimeType": "image/png"}]
    assert doc["asset"] == {"version": "2.0"} and doc["nodes"] == [{"mesh": 0, "name": "depth_prediction"}] and doc["scene"] == 0


def test_glb_texture_orientation():
    """The mesh's uv has v = 1 on the photo's top row (shaders.js:185-205 samples the vertically flipped frame), and glTF samples v = 0 from the
    first row of the embedded image: the v = 1 vertices must read the photo's top row, the v = 0 vertices its bottom row. The reference embeds the
    flipped photo for this (index.html:1067-1070 imageOrientation "flipY", read back as stored). Ready-made PNG bytes are embedded untouched."""
    photo = np.array([[[200, 10, 10], [210, 20, 20]], [[10, 10, 200], [20, 20, 210]]], dtype=np.uint8)  # top row red, bottom row blue
    xy = ms.grid_xy(2, 2)
    uv = ((xy + 1) / 2).astype(np.float32)  # the kernel's uv: row 0 of the grid is y = 1 (the top), v = 1
    xyz = np.concatenate([xy, -np.ones((4, 1))], axis=1).astype(np.float32)
    faces = np.array([[0, 2, 3], [0, 3, 1]], dtype=np.int32)

    def embedded(texture):
        raw = mesh_io.glb_bytes(xyz, uv, faces, texture)
        jlen = struct.unpack("<I", raw[12:16])[0]
        view = json.loads(raw[20:20 + jlen])["bufferViews"][3]
        return _png_pixels(raw[28 + jlen + view["byteOffset"]:28 + jlen + view["byteOffset"] + view["byteLength"]])

    image = embedded(photo)
    rows = image.shape[0]
    for i in range(4):  # glTF: texel row of v = v * rows, clamped to the image (nearest, the corner texels)
        row = min(int(uv[i, 1] * rows), rows - 1)
        col = min(int(uv[i, 0] * image.shape[1]), image.shape[1] - 1)
        on_top = xyz[i, 1] > 0
        np.testing.assert_array_equal(image[row, col], photo[0 if on_top else 1, col])
    assert uv[0, 1] == 1 and xyz[0, 1] == 1  # (vertex 0 is the top left corner)
    np.testing.assert_array_equal(embedded(torch.from_numpy(photo)), photo[::-1])
    np.testing.assert_array_equal(embedded(mesh_io.encode_png(photo)), photo)


def test_glb_of_an_empty_mesh_has_the_initial_bounds():
    empty = mesh_io.glb_bytes(np.zeros((0, 3), np.float32), np.zeros((0, 2), np.float32), np.zeros((0, 3), np.int32), np.zeros((2, 2, 3), np.uint8))
    jlen = struct.unpack("<I", empty[12:16])[0]
    acc = json.loads(empty[20:20 + jlen])["accessors"][0]
    assert acc["min"] == [1e6] * 3 and acc["max"] == [-1e6] * 3 and acc["count"] == 0


@pytest.mark.parametrize("shape", [(3, 5), (3, 5, 3), (2, 7, 4)])
def test_png_inflates_back(shape):
    img = np.random.default_rng(1).integers(0, 256, size=shape, dtype=np.uint8)
    np.testing.assert_array_equal(_png_pixels(mesh_io.encode_png(img)), img.reshape(shape[0], shape[1], -1))
    with pytest.raises(ValueError):
        mesh_io.encode_png(img.astype(np.float32))


@pytest.mark.parametrize("per_face", [3, 1])
def test_write_obj_parses_back(tmp_path, per_face):
    xyz, uv, faces = _mesh(np.random.default_rng(9), 13, 8, per_face)
    path = tmp_path / "m.obj"
    mesh_io.write_obj(path, xyz, uv, faces)
    lines = path.read_text().split("\n")
    assert lines[0].startswith("# Made with MuggledDPT") and lines[1] == f"# 13 vertices  |  8 faces  |  {per_face} verts per face"
    assert lines[2] == "o depth_prediction" and len(lines) == 3 + 13 + 13 + 8
    v = np.array([[np.float32(t) for t in ln.split()[1:]] for ln in lines[3:16]], dtype=np.float32)
    vt = np.array([[np.float32(t) for t in ln.split()[1:]] for ln in lines[16:29]], dtype=np.float32)
    assert all(ln.startswith("v ") for ln in lines[3:16]) and all(ln.startswith("vt ") for ln in lines[16:29])
    assert v.tobytes() == xyz.tobytes() and vt.tobytes() == uv.tobytes()  # (the same float32, -0.0 included)
    assert not any("e" in ln for ln in lines[3:29])
    f = []
    for ln in lines[29:]:
        head, *items = ln.split()
        assert head == "f" and len(items) == per_face
        pairs = [it.split("/") for it in items]
        assert all(a == b for a, b in pairs)
        f.append([int(a) for a, _ in pairs])
    np.testing.assert_array_equal(np.array(f), faces.astype(np.int64) + 1)


def test_writers_reject_bad_arrays():
    xyz, uv, faces = _mesh(np.random.default_rng(2), 5, 3, 3)
    tex = np.zeros((2, 2, 3), np.uint8)
    with pytest.raises(TypeError):
        mesh_io.glb_bytes(xyz.astype(np.float64), uv, faces, tex)
    with pytest.raises(ValueError):
        mesh_io.glb_bytes(xyz, uv[:4], faces, tex)
    with pytest.raises(ValueError):
        mesh_io.glb_bytes(xyz, uv, faces + 5, tex)
    with pytest.raises(ValueError):
        mesh_io.obj_string(xyz, uv, faces[:, :2])
    with pytest.raises(ValueError):
        mesh_io.obj_string(xyz, uv, -faces - 1)


def test_gpu_cases_meet_the_input_condition():
    """every case of tests/test_gpu_mesh.py passes the restatement's own assertion (no interpolated alpha within 1e-6 of the threshold), checked
    here without a GPU; the jittered tables are the helper's"""
    from tests import test_gpu_mesh as tg
    for name, c in tg.CASES.items():
        refs = tg.reference(name)
        assert len(refs) == tg.B and all(r["xyz"].shape[0] == r["valid"].sum() for r in refs), name
        if c["jitter"]:
            nx, ny = c["grid"]
            np.testing.assert_array_equal(tg.case_inputs(name)[2], ms.jitter_xy(nx, ny, c["jitter"], np.random.default_rng(7)))
    tg.test_patterns_do_what_they_say()
