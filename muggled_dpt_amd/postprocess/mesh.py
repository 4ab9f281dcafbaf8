"""The 3D viewer's mesh export, the client half of the reference's viewer and its "Save 3D Model" (depth_frames_to_mesh / mesh_views:
demo_helpers/3dviewer/*.js, JavaScript on the CPU there; files through mesh_io). Kernels: csrc/post_mesh.inc."""

from __future__ import annotations

import ctypes
import math

import numpy as np
import torch
from torch import Tensor

from .. import native
from ._common import _launch, _need_cuda, ptr, scratch_bytes

MESH_MODES = {"triangles": native.MESH_TRIANGLES, "points": native.MESH_POINTS}
# the viewer's controls as it starts (3dviewer/index.html): FOV 50 (:507), edge threshold 0 (:515), max depth 1.0 x depth_limit 100 (:464, :503),
# min depth 0.5 x max (:502), mesh density 0.5 -> 0.5^4 x max_faces 5e6 target faces (:465, :513, :985)
MESH_FOV_DEG, MESH_MIN_DEPTH, MESH_MAX_DEPTH, MESH_EDGE_THRESHOLD, MESH_TARGET_FACES = 50.0, 50.0, 100.0, 0.0, 312500


def _mesh_grid(image_wh, target_num_faces, what: str) -> tuple[int, int, int, int]:
    """(w, h, nx, ny): the photo size and the plane grid mdpt_post_mesh_grid gives for it (host arithmetic: no device call)"""
    w, h = int(image_wh[0]), int(image_wh[1])
    t = float(target_num_faces)
    if w <= 0 or h <= 0 or not np.isfinite(t):
        raise ValueError(f"{what}: bad photo size {tuple(image_wh)} or face target {target_num_faces}")
    lib = native.load()
    nx, ny = ctypes.c_int32(), ctypes.c_int32()
    native.check(lib, lib.mdpt_post_mesh_grid(w, h, t, ctypes.byref(nx), ctypes.byref(ny)))
    return w, h, nx.value, ny.value


def mesh_plane_grid(image_wh, target_num_faces=MESH_TARGET_FACES, jitter_pct: float = 0.0, rng=np.random):
    """-> (nx, ny, vertex_xy | None): the viewer's plane grid for a photo of image_wh = (w, h) (3dviewer/mesh.js:184-200, through mdpt_post_mesh_grid) and, with
    jitter_pct > 0, its jittered float64 [nx ny, 2] vertex table for depth_frames_to_mesh(vertex_xy=...), drawn by apply_mesh_jitter's rule (mesh.js:258-283): every
    vertex off the border (|x| != 1 and |y| != 1), in index order, moves by (cos(angle) offset max_x, sin(angle) offset max_y) with offset = random(), angle = random() 2
    pi (two draws per vertex, in that order) and max = jitter_pct x step x 0.5 x 0.9. rng: anything with random(size) - np.random, a RandomState, a Generator; the
    viewer's own Math.random cannot be reproduced. The viewer starts with jitter 1 (index.html:514)."""
    _, _, nx, ny = _mesh_grid(image_wh, target_num_faces, "mesh_plane_grid")
    jitter_pct = float(jitter_pct)
    if not 0.0 <= jitter_pct <= 1.0:
        raise ValueError(f"mesh_plane_grid: jitter_pct must be in [0, 1], got {jitter_pct}")
    if jitter_pct == 0.0:
        return nx, ny, None
    x_step, y_step = 2.0 / (nx - 1), 2.0 / (ny - 1)
    xs = np.arange(nx, dtype=np.float64) * x_step - 1.0
    ys = 1.0 - np.arange(ny, dtype=np.float64) * y_step
    xy = np.stack(np.meshgrid(xs, ys), axis=-1).reshape(-1, 2)
    inner = np.flatnonzero((np.abs(xy[:, 0]) != 1) & (np.abs(xy[:, 1]) != 1))
    draws = np.asarray(rng.random((inner.size, 2)), dtype=np.float64)
    offset, angle = draws[:, 0], draws[:, 1] * (np.pi * 2.0)
    xy[inner, 0] += np.cos(angle) * offset * (jitter_pct * x_step * 0.5 * 0.9)
    xy[inner, 1] += np.sin(angle) * offset * (jitter_pct * y_step * 0.5 * 0.9)
    return nx, ny, xy


def _mesh_vertex_table(vertex_xy, what: str):
    """a caller's vertex table as float64 [n, 2] (host array or CUDA tensor), checked where it can be without a device read"""
    if isinstance(vertex_xy, torch.Tensor) and vertex_xy.device.type == "cuda":
        if vertex_xy.dim() != 2 or vertex_xy.shape[1] != 2 or not vertex_xy.dtype.is_floating_point:
            raise ValueError(f"{what}: vertex_xy must be a floating-point [n,2] table, got {vertex_xy.dtype} {tuple(vertex_xy.shape)}")
        return vertex_xy.detach()
    arr = np.asarray(vertex_xy.numpy() if isinstance(vertex_xy, torch.Tensor) else vertex_xy)
    if arr.ndim != 2 or arr.shape[1] != 2 or arr.dtype.kind != "f":
        raise ValueError(f"{what}: vertex_xy must be a floating-point [n,2] table, got {arr.dtype} {arr.shape}")
    if not np.isfinite(arr).all():
        raise ValueError(f"{what}: vertex_xy holds values that are not finite")
    return np.ascontiguousarray(arr, dtype=np.float64)


def depth_frames_to_mesh(frames_bgra: Tensor, image_wh, fov_deg: float = MESH_FOV_DEG, min_depth: float = MESH_MIN_DEPTH,
                         max_depth: float = MESH_MAX_DEPTH, is_metric: bool = False, edge_threshold: float = MESH_EDGE_THRESHOLD,
                         target_num_faces=MESH_TARGET_FACES, vertex_xy=None, mode: str = "triangles", grid_xy=None):
    """uint8 [B,H,W,4] (or [H,W,4]) frames as pack_depth_u24_frames returns them -> the textured mesh the reference's 3D viewer saves, for every
    frame at once and on the device: run_vertex_shader_cpu (3dviewer/shaders.js:163-264), _make_plane_mesh and filter_mesh_vertices
    (mesh.js:170-254, 330-371) with the camera of index.html:1163-1188. image_wh = the photo's (w, h): it sets the grid (mesh_plane_grid; grid_xy =
    (nx, ny) overrides it) and the aspect scaling. Defaults are the viewer's controls as it starts (MESH_* above). vertex_xy: a float [nx ny, 2]
    table (host or device) that replaces the grid's coordinates - mesh_plane_grid's jittered table - shared by the frames. mode: "triangles" or
    "points" (one face [i] per vertex). -> (xyz, uv, faces, counts, bounds), CUDA tensors, nothing read back, no synchronisation:
      xyz    fp32 [B,nv,3], uv fp32 [B,nv,2], faces int32 [B,nf,3] with nf = 2 (nx-1)(ny-1) (points: [B,nv,1]): full-capacity slabs, every
             image's kept entries packed at the front in the reference's order, the rest unspecified
      counts int32 [B,2]: kept vertices and kept faces;  bounds fp32 [B,2,3]: min / max of the kept xyz (none kept: +1e6 / -1e6)
    A vertex is kept if its interpolated alpha reaches edge_threshold x 255; a face if all its vertices are. Computed in fp64, rounded once.
    Deviations from the JavaScript: the 24-bit depth value is interpolated (it interpolates the bytes separately and truncates each: garbage across
    a byte carry), and real bounds are not clamped to +-1e6. mesh_views slices the slabs; mesh_io writes .glb / .obj."""
    what = "depth_frames_to_mesh"
    if mode not in MESH_MODES:
        raise ValueError(f"{what}: mode must be 'triangles' or 'points', got {mode!r}")
    fov_deg, min_depth, max_depth, edge_threshold = float(fov_deg), float(min_depth), float(max_depth), float(edge_threshold)
    if not 0.0 < fov_deg < 180.0:
        raise ValueError(f"{what}: fov_deg must be in (0, 180), got {fov_deg}")
    if not (0.0 < min_depth < max_depth and np.isfinite(max_depth)) and not (is_metric and 0.0 <= min_depth <= max_depth and np.isfinite(max_depth)):
        raise ValueError(f"{what}: need 0 < min_depth < max_depth (metric: 0 <= min_depth <= max_depth), got {min_depth}, {max_depth}")
    if not 0.0 <= edge_threshold <= 1.0:
        raise ValueError(f"{what}: edge_threshold must be in [0, 1], got {edge_threshold}")
    if grid_xy is None:
        w, h, nx, ny = _mesh_grid(image_wh, target_num_faces, what)
    else:
        w, h, nx, ny = int(image_wh[0]), int(image_wh[1]), int(grid_xy[0]), int(grid_xy[1])
        if w <= 0 or h <= 0:
            raise ValueError(f"{what}: bad photo size {tuple(image_wh)}")
        i32 = 2 ** 31 - 1
        try:  # the library's own limits and words (host arithmetic: no device call)
            scratch_bytes("mdpt_post_mesh_scratch_bytes", 1, max(-i32, min(nx, i32)), max(-i32, min(ny, i32)))
        except native.MdptError as e:
            raise ValueError(f"{what}: {e}") from None
    nv, nf = nx * ny, 2 * (nx - 1) * (ny - 1)
    table = None
    if vertex_xy is not None:
        table = _mesh_vertex_table(vertex_xy, what)
        if table.shape[0] != nv:
            raise ValueError(f"{what}: vertex_xy has {table.shape[0]} rows for a {nx}x{ny} grid of {nv} vertices")
    if not isinstance(frames_bgra, torch.Tensor) or frames_bgra.dtype != torch.uint8 or frames_bgra.dim() not in (3, 4) or frames_bgra.shape[-1] != 4 \
            or frames_bgra.numel() == 0:
        raise TypeError(f"{what}: frames must be uint8 [B,H,W,4] (pack_depth_u24_frames), got {getattr(frames_bgra, 'dtype', type(frames_bgra))} "
                        f"{tuple(getattr(frames_bgra, 'shape', ()))}")
    _need_cuda([frames_bgra], what)
    frames = frames_bgra.detach()
    frames = (frames[None] if frames.dim() == 3 else frames).contiguous()
    b, fh, fw, _ = frames.shape
    dev = frames.device
    if table is not None:
        table = (table if isinstance(table, torch.Tensor) else torch.from_numpy(table)).to(dev, torch.float64).contiguous()
    if is_metric:  # index.html:1179-1188
        pa, pb = min_depth, max_depth - min_depth
    else:
        pa, pb = 1.0 / max_depth, (1.0 / min_depth) - (1.0 / max_depth)
    x_scale, y_scale = (1.0, h / w) if w > h else (w / h, 1.0)  # index.html:1163-1165
    need = scratch_bytes("mdpt_post_mesh_scratch_bytes", b, nx, ny)
    scratch = torch.empty(need // 4, device=dev, dtype=torch.int32)
    xyz = torch.empty((b, nv, 3), device=dev, dtype=torch.float32)
    uv = torch.empty((b, nv, 2), device=dev, dtype=torch.float32)
    faces = torch.empty((b, nv, 1) if mode == "points" else (b, nf, 3), device=dev, dtype=torch.int32)
    counts = torch.empty((b, 2), device=dev, dtype=torch.int32)
    bounds = torch.empty((b, 2, 3), device=dev, dtype=torch.float32)
    _launch(dev, "mdpt_post_mesh", frames.data_ptr(), b, fh, fw, nx, ny, ptr(table), pa, pb,
            math.tan(fov_deg * 0.5 * (math.pi / 180.0)), x_scale, y_scale, edge_threshold, int(bool(is_metric)), MESH_MODES[mode], xyz.data_ptr(),
            uv.data_ptr(), faces.data_ptr(), counts.data_ptr(), bounds.data_ptr(), scratch.data_ptr(), need)
    return xyz, uv, faces, counts, bounds


def mesh_views(xyz: Tensor, uv: Tensor, faces: Tensor, counts: Tensor, bounds: Tensor) -> list[tuple[Tensor, Tensor, Tensor, Tensor]]:
    """depth_frames_to_mesh's slabs -> per image (xyz [kv,3], uv [kv,2], faces [kf,3 or 1], bounds [2,3]): views of the kept entries. Reads counts
    once (the only synchronisation of the mesh path)."""
    if counts.dim() != 2 or counts.shape[1] != 2 or not (xyz.shape[0] == uv.shape[0] == faces.shape[0] == bounds.shape[0] == counts.shape[0]):
        raise ValueError("mesh_views: expected the five tensors depth_frames_to_mesh returns")
    kept = counts.cpu().tolist()
    return [(xyz[i, :kv], uv[i, :kv], faces[i, :kf], bounds[i]) for i, (kv, kf) in enumerate(kept)]
