"""Host-side writers for the meshes postprocess.depth_frames_to_mesh / mesh_views produce: the files the reference's 3D viewer saves
(demo_helpers/3dviewer/save_gltf.js create_glb_binary, save_obj.js create_obj_string) and a minimal PNG encoder for the texture (the viewer's
canvas.toBlob). numpy, json, struct and zlib only. Arrays may be numpy arrays or torch tensors (CUDA tensors are copied to the host here); they go
into the files as they are, no value is recomputed."""

from __future__ import annotations

import json
import struct
import zlib

import numpy as np

GLB_MAGIC, GLB_VERSION, GLB_JSON, GLB_BIN = 0x46546C67, 2, 0x4E4F534A, 0x004E4942  # save_gltf.js:98-101
_F32, _U32, _ARRAY_BUFFER, _ELEMENT_BUFFER = 5126, 5125, 34962, 34963  # save_gltf.js:46-47


def _host(a, dtype, cols, what: str) -> np.ndarray:
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    a = np.asarray(a)
    if a.ndim != 2 or (cols is not None and a.shape[1] != cols):
        raise ValueError(f"{what} must be [n,{cols if cols is not None else '1..3'}], got {a.shape}")
    if np.dtype(dtype).kind == "f" and a.dtype != np.float32:
        raise TypeError(f"{what} must be float32 (the device arrays go into the file as they are), got {a.dtype}")
    if np.dtype(dtype).kind == "u":
        if a.dtype.kind not in "iu":
            raise TypeError(f"{what} must hold integers, got {a.dtype}")
        if a.size and (a.min() < 0 or a.max() > 0xFFFFFFFF):
            raise ValueError(f"{what} holds indices outside uint32")
    return np.ascontiguousarray(a, dtype=np.dtype(dtype).newbyteorder("<"))


def _mesh_arrays(xyz, uv, faces) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    xyz, uv, faces = _host(xyz, np.float32, 3, "xyz"), _host(uv, np.float32, 2, "uv"), _host(faces, np.uint32, None, "faces")
    if faces.shape[1] not in (1, 3):
        raise ValueError(f"faces must have 1 (points) or 3 (triangles) vertices each, got {faces.shape[1]}")
    if uv.shape[0] != xyz.shape[0]:
        raise ValueError(f"{xyz.shape[0]} vertices but {uv.shape[0]} texture coordinates")
    if faces.size and faces.max() >= xyz.shape[0]:
        raise ValueError(f"a face refers to vertex {int(faces.max())} of {xyz.shape[0]}")
    return xyz, uv, faces


def encode_png(image) -> bytes:
    """uint8 [H,W] (grey), [H,W,3] (RGB) or [H,W,4] (RGBA) -> PNG bytes: 8-bit, filter 0 on every row, one zlib stream, no ancillary chunks."""
    if hasattr(image, "detach"):
        image = image.detach().cpu().numpy()
    img = np.asarray(image)
    if img.dtype != np.uint8 or img.ndim not in (2, 3) or img.size == 0 or (img.ndim == 3 and img.shape[2] not in (1, 3, 4)):
        raise ValueError(f"encode_png takes uint8 [H,W], [H,W,3] or [H,W,4], got {img.dtype} {img.shape}")
    h, w = img.shape[:2]
    channels = 1 if img.ndim == 2 else img.shape[2]
    rows = np.zeros((h, 1 + w * channels), dtype=np.uint8)  # (filter byte 0 = None)
    rows[:, 1:] = img.reshape(h, w * channels)

    def chunk(kind: bytes, data: bytes) -> bytes:
        return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)

    ihdr = struct.pack(">IIBBBBB", w, h, 8, {1: 0, 3: 2, 4: 6}[channels], 0, 0, 0)
    return b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", ihdr) + chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) + chunk(b"IEND", b"")


def _pad4(n: int) -> int:
    return (n + 3) // 4 * 4


def glb_bytes(xyz, uv, faces, texture_rgb, bounds=None) -> bytes:
    """create_glb_binary's file (save_gltf.js:2-146): the 12-byte header, the JSON chunk padded with spaces to a multiple of 4, the BIN chunk with
    xyz, uv, the uint32 indices and the PNG texture in that order, zero-padded to a multiple of 4; the same bufferViews, accessors and
    KHR_materials_unlit material; primitive mode 4 for triangles, 0 for points. bounds = [2,3] {min xyz, max xyz} for the POSITION accessor
    (depth_frames_to_mesh's; None: computed here as save_gltf.js:16-25 does, without its +-1e6 clamp of real values).
    texture_rgb: the photo as uint8 [H,W,3] (or anything encode_png takes), top row first. Orientation: the mesh's uv has v = 1 on the photo's top
    row, and glTF puts v = 0 on the first row of an image, so the photo is embedded upside down - as the reference embeds it, whose texture was
    uploaded with imageOrientation "flipY" (index.html:1067-1070) and read back as it lies in the GPU (TEXTUREDATA.read_current_texture_data).
    PNG bytes are embedded as they are: they must hold the photo already flipped. (.obj's v = 0 is the bottom row: its image is not flipped.)"""
    xyz, uv, faces = _mesh_arrays(xyz, uv, faces)
    if isinstance(texture_rgb, (bytes, bytearray, memoryview)):
        png = bytes(texture_rgb)
    else:
        if hasattr(texture_rgb, "detach"):
            texture_rgb = texture_rgb.detach().cpu().numpy()
        png = encode_png(np.asarray(texture_rgb)[::-1])
    if bounds is None:
        lo = xyz.min(axis=0) if xyz.shape[0] else np.full(3, 1e6, np.float32)
        hi = xyz.max(axis=0) if xyz.shape[0] else np.full(3, -1e6, np.float32)
    else:
        if hasattr(bounds, "detach"):
            bounds = bounds.detach().cpu().numpy()
        lo, hi = np.asarray(bounds, dtype=np.float32).reshape(2, 3)
    parts = [xyz.tobytes(), uv.tobytes(), faces.tobytes(), png]
    offsets = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).tolist()
    bin_length = _pad4(offsets[-1])
    doc = {
        "asset": {"version": "2.0"},
        "buffers": [{"byteLength": bin_length}],
        "bufferViews": [
            {"buffer": 0, "byteOffset": offsets[0], "byteLength": len(parts[0]), "target": _ARRAY_BUFFER},
            {"buffer": 0, "byteOffset": offsets[1], "byteLength": len(parts[1]), "target": _ARRAY_BUFFER},
            {"buffer": 0, "byteOffset": offsets[2], "byteLength": len(parts[2]), "target": _ELEMENT_BUFFER},
            {"buffer": 0, "byteOffset": offsets[3], "byteLength": len(parts[3])},
        ],
        "accessors": [
            {"bufferView": 0, "componentType": _F32, "count": int(xyz.shape[0]), "type": "VEC3", "max": [float(v) for v in hi],
             "min": [float(v) for v in lo]},
            {"bufferView": 1, "componentType": _F32, "count": int(uv.shape[0]), "type": "VEC2"},
            {"bufferView": 2, "componentType": _U32, "count": int(faces.size), "type": "SCALAR"},
        ],
        "images": [{"bufferView": 3, "mimeType": "image/png"}],
        "textures": [{"source": 0}],
        "materials": [{"extensions": {"KHR_materials_unlit": {}}, "pbrMetallicRoughness": {"baseColorTexture": {"index": 0}}}],
        "extensionsUsed": ["KHR_materials_unlit"],
        "meshes": [{"primitives": [{"attributes": {"POSITION": 0, "TEXCOORD_0": 1}, "indices": 2, "material": 0,
                                    "mode": 0 if faces.shape[1] == 1 else 4}]}],
        "nodes": [{"mesh": 0, "name": "depth_prediction"}],
        "scenes": [{"nodes": [0]}],
        "scene": 0,
    }
    text = json.dumps(doc, separators=(",", ":")).encode("utf-8")  # (JSON.stringify's compact form)
    text += b" " * (_pad4(len(text)) - len(text))
    body = b"".join(parts)
    body += b"\0" * (bin_length - len(body))
    total = 12 + 8 + len(text) + 8 + bin_length
    return b"".join([struct.pack("<III", GLB_MAGIC, GLB_VERSION, total), struct.pack("<II", len(text), GLB_JSON), text,
                     struct.pack("<II", bin_length, GLB_BIN), body])


def write_glb(path, xyz, uv, faces, texture_rgb, bounds=None) -> None:
    """glb_bytes(...) -> the file `path` (texture_rgb = the photo, top row first: glb_bytes embeds it flipped, as glTF's v axis needs)"""
    data = glb_bytes(xyz, uv, faces, texture_rgb, bounds)
    with open(path, "wb") as fh:
        fh.write(data)


def obj_string(xyz, uv, faces) -> str:
    """create_obj_string's records (save_obj.js:2-35): the three header lines, `v x y z` per vertex, `vt u v` per vertex, `f i/i ...` per face with
    1-based indices, joined by newlines. Numbers are written as the shortest text that parses back to the same float32 (JavaScript prints the
    double's shortest text: the same values, possibly other digits)."""
    xyz, uv, faces = _mesh_arrays(xyz, uv, faces)
    lines = ["# Made with MuggledDPT: https://github.com/heyoeyo/muggled_dpt",
             f"# {xyz.shape[0]} vertices  |  {faces.shape[0]} faces  |  {faces.shape[1]} verts per face",
             "o depth_prediction"]
    num = lambda v: np.format_float_positional(v, unique=True, trim="-") if np.isfinite(v) else str(v)  # noqa: E731  (no exponents in .obj)
    lines += ["v " + " ".join(num(v) for v in row) for row in xyz]
    lines += ["vt " + " ".join(num(v) for v in row) for row in uv]
    lines += ["f " + " ".join(f"{i}/{i}" for i in row) for row in (faces.astype(np.int64) + 1).tolist()]
    return "\n".join(lines)


def write_obj(path, xyz, uv, faces) -> None:
    """obj_string(...) -> the file `path`"""
    text = obj_string(xyz, uv, faces)
    with open(path, "w", encoding="utf-8", newline="\n") as fh:
        fh.write(text)
