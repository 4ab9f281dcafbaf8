"""fp64 numpy restatement of the reference's 3D viewer "Save 3D Model" path (demo_helpers/3dviewer, JavaScript there) for tests/test_mesh_cpu.py and
tests/test_gpu_mesh.py: the plane grid (mesh.js:184-229 _make_plane_mesh), its jitter (mesh.js:258-283 apply_mesh_jitter), the vertex shader on the
CPU (shaders.js:163-264 run_vertex_shader_cpu with _uv_sample_texture / _get_bilinear_xys, in the viewer's vertically flipped frame,
index.html:1067-1070, with the camera of index.html:1163-1188), the pruning (mesh.js:330-371 filter_mesh_vertices) and the bounds of
save_gltf.js:16-25. JavaScript numbers are doubles, so every step is float64 in the order the JavaScript evaluates it.

Two deliberate deviations, shared with the device code: the 24-bit depth VALUE is interpolated (the JavaScript interpolates the three bytes
separately and truncates each with <<, which is garbage across a byte carry), and real bounds are not clamped to +-1e6."""
from __future__ import annotations

import math

import numpy as np

ALPHA_MARGIN = 1e-6  # no vertex's interpolated alpha may lie this close to edge_threshold * 255: a condition on the test inputs, not a tolerance


def js_round(v: float) -> float:
    """Math.round: halves go toward +inf"""
    f = math.floor(v)
    return f + 1.0 if v - f >= 0.5 else float(f)


def plane_grid(w: int, h: int, target_faces: float) -> tuple[int, int]:
    """mesh.js:184-193 -> (nx, ny)"""
    t = max(float(target_faces), 2.0)
    tv = js_round(0.5 * t + math.sqrt(t))
    aspect = w / h
    rx = math.sqrt(tv * aspect)
    ry = rx / aspect
    return int(max(js_round(rx), 2)), int(max(js_round(ry), 2))


def grid_xy(nx: int, ny: int) -> np.ndarray:
    """mesh.js:198-215 -> float64 [nx ny, 2], vertex (row r, col c) at index c + r nx"""
    xs = np.arange(nx, dtype=np.float64) * (2.0 / (nx - 1)) - 1.0
    ys = 1.0 - np.arange(ny, dtype=np.float64) * (2.0 / (ny - 1))
    return np.stack(np.meshgrid(xs, ys), axis=-1).reshape(-1, 2)


def jitter_xy(nx: int, ny: int, jitter_pct: float, rng) -> np.ndarray:
    """mesh.js:258-283 one vertex at a time, two draws each (offset, then angle), with rng.random() in place of Math.random"""
    xy = grid_xy(nx, ny)
    max_x = jitter_pct * (2.0 / (nx - 1)) * 0.5 * 0.9
    max_y = jitter_pct * (2.0 / (ny - 1)) * 0.5 * 0.9
    for i in range(xy.shape[0]):
        if abs(xy[i, 0]) != 1 and abs(xy[i, 1]) != 1:
            offset = float(rng.random())
            angle = float(rng.random()) * (math.pi * 2.0)
            xy[i, 0] += math.cos(angle) * offset * max_x
            xy[i, 1] += math.sin(angle) * offset * max_y
    return xy


def plane_faces(nx: int, ny: int, mode: str = "triangles") -> np.ndarray:
    """mesh.js:207-229 (and :287-300 for points) -> int64 [nf, 3] or [nv, 1]"""
    if mode == "points":
        return np.arange(nx * ny, dtype=np.int64)[:, None]
    r, c = np.meshgrid(np.arange(ny - 1), np.arange(nx - 1), indexing="ij")
    v = (c + r * nx).reshape(-1)
    first = np.stack([v, v + nx, v + nx + 1], axis=1)
    second = np.stack([v, v + nx + 1, v + 1], axis=1)
    return np.stack([first, second], axis=1).reshape(-1, 3)


def camera(image_wh, fov_deg: float, min_depth: float, max_depth: float, is_metric: bool):
    """index.html:1163-1188 -> (a, b, tan_half_fov, x_scale, y_scale)"""
    w, h = image_wh
    x_scale, y_scale = (1.0, h / w) if w > h else (w / h, 1.0)
    tan_half_fov = math.tan(fov_deg * 0.5 * (math.pi / 180.0))
    if is_metric:
        return min_depth, max_depth - min_depth, tan_half_fov, x_scale, y_scale
    return 1.0 / max_depth, (1.0 / min_depth) - (1.0 / max_depth), tan_half_fov, x_scale, y_scale


def sample_frame(frame: np.ndarray, uv: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """shaders.js:212-252 on the flipped frame (flipped row j = frame row H - 1 - j) -> (depth in [0, 1), alpha in [0, 255]) per vertex, float64.
    Depth taps are u24 / 2^24 (the value, not its bytes: the deviation above)."""
    H, W = frame.shape[:2]
    f = frame.astype(np.int64)
    planes = (((f[..., 2] << 16) + (f[..., 1] << 8) + f[..., 0]).astype(np.float64) / float(2 ** 24), f[..., 3].astype(np.float64))
    xr = np.clip(uv[:, 0], 0.0, 1.0) * (W - 1)
    yr = np.clip(uv[:, 1], 0.0, 1.0) * (H - 1)
    x1 = np.floor(xr).astype(np.int64)
    y1 = np.floor(yr).astype(np.int64)
    x2 = np.minimum(x1 + 1, W - 1)
    y2 = np.minimum(y1 + 1, H - 1)
    tx, ty = xr - x1, yr - y1
    out = []
    for p in planes:
        tl, tr, bl, br = p[H - 1 - y1, x1], p[H - 1 - y1, x2], p[H - 1 - y2, x1], p[H - 1 - y2, x2]
        left = (1.0 - ty) * tl + ty * bl
        right = (1.0 - ty) * tr + ty * br
        out.append((1.0 - tx) * left + tx * right)
    return out[0], out[1]


def mesh_of_frame(frame: np.ndarray, image_wh, nx: int, ny: int, fov_deg: float, min_depth: float, max_depth: float, is_metric: bool = False,
                  edge_threshold: float = 0.0, vertex_xy=None, mode: str = "triangles") -> dict:
    """One uint8 [H,W,4] frame -> dict(valid bool [nv], xyz / uv float64 [kept, 3 / 2], faces int64 [kept faces, 3 or 1], bounds float64 [2,3]).
    Asserts the input condition: no interpolated alpha within ALPHA_MARGIN of the threshold."""
    xy = grid_xy(nx, ny) if vertex_xy is None else np.asarray(vertex_xy, dtype=np.float64)
    assert xy.shape == (nx * ny, 2)
    a, b, tan_half_fov, x_scale, y_scale = camera(image_wh, fov_deg, min_depth, max_depth, is_metric)
    uv = (xy + 1.0) * 0.5  # shaders.js:188
    d, alpha = sample_frame(frame, uv)
    limit = edge_threshold * 255.0  # shaders.js:175
    gap = np.abs(alpha - limit).min()
    assert gap > ALPHA_MARGIN, f"an interpolated alpha lies within {gap:g} of the threshold {limit}: choose another threshold / seed"
    valid = alpha >= limit  # shaders.js:198
    depth = (a + b * d) if is_metric else 1.0 / (a + b * d)  # shaders.js:178-180
    xyz = np.stack([depth * xy[:, 0] * x_scale * tan_half_fov, depth * xy[:, 1] * y_scale * tan_half_fov, -depth], axis=1)  # shaders.js:201-204
    # mesh.js:346-368
    new_index = np.cumsum(valid) - 1
    faces = plane_faces(nx, ny, mode)
    faces = new_index[faces[valid[faces].all(axis=1)]]
    kept = xyz[valid]
    if kept.shape[0]:
        bounds = np.stack([kept.min(axis=0), kept.max(axis=0)])
    else:
        bounds = np.array([[1e6] * 3, [-1e6] * 3])  # save_gltf.js:16-17
    return dict(valid=valid, xyz=kept, uv=uv[valid], faces=faces, bounds=bounds)
