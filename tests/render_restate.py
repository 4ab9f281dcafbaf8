"""Numpy restatement of mdpt_post_render (include/mdpt.h) for small cases, operation by operation: the vertex stage in fp64, int64 coverage with the
top-left rule, the minimum of the (fp32 z01 bits, face) keys, and the resolve. Slow by design: a Python loop over the faces.

It also returns the per-pixel `safe` mask. A pixel is UNSAFE where another, equally valid evaluation order may decide differently:
  snapping ... a face whose bounding box, grown by one pixel, holds the pixel has a vertex whose pre-snap coordinate (in 1/256 pixel) lies within
               SNAP_MARGIN of a rounding boundary of the grid;
  depths ..... the two smallest z01 among the faces covering the pixel differ by fewer than CLOSE_ULPS fp32 steps;
  planes ..... the winning z01 lies within PLANE_MARGIN of 0 or 1.
`soft` marks the pixels whose colour, before rounding, lies within COLOUR_MARGIN of k + 0.5 in some channel: +-1 is allowed there.
Exact integer ties - an edge through a pixel centre, shared edges - are NOT unsafe: the fill rule decides them.

The shared cases of tests/test_render_cpu.py and tests/test_gpu_render.py live here too (CASES, case_frames, case_views)."""
from __future__ import annotations

import functools
import math

import numpy as np

from muggled_dpt_amd import orbit_camera as oc
from tests import mesh_restate as ms

SNAP_MARGIN, CLOSE_ULPS, PLANE_MARGIN, COLOUR_MARGIN = 1e-6, 4, 1e-9, 1e-6
UNUSABLE = -2 ** 31
SMALL_BOX = 64  # RENDER_SMALL_BOX of csrc/mdpt_kernels.h: boxes up to this many pixels are walked by one lane, larger ones by the workgroup


def vertex_stage(xyz: np.ndarray, M: np.ndarray, W: int, H: int):
    """xyz [n,3] (any float type), M [16] -> (X, Y int64 [n] with UNUSABLE in X, invw, z01 fp64 [n], near_boundary bool [n])"""
    p = np.asarray(xyz, dtype=np.float64)
    M = np.asarray(M, dtype=np.float64).reshape(16)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        c = [x * M[j] + y * M[4 + j] + z * M[8 + j] + M[12 + j] for j in range(4)]
        w = c[3]
        tx = (c[0] / w + 1.0) * 0.5 * float(W) * 256.0
        ty = (1.0 - c[1] / w) * 0.5 * float(H) * 256.0
        sx, sy = np.rint(tx), np.rint(ty)
        ok = (w > 0.0) & (np.abs(sx) < 2.0 ** 30) & (np.abs(sy) < 2.0 ** 30)
        X = np.where(ok, sx, UNUSABLE).astype(np.int64)
        Y = np.where(ok, sy, 0).astype(np.int64)
        near = ok & ((np.abs(np.abs(tx - np.floor(tx)) - 0.5) < SNAP_MARGIN) | (np.abs(np.abs(ty - np.floor(ty)) - 0.5) < SNAP_MARGIN))
        # a w within rounding of 0 could make the vertex usable one way and not the other
        near |= np.abs(w) < 1e-12
        invw = np.where(ok, 1.0 / w, 0.0)
        z01 = np.where(ok, (c[2] / w + 1.0) * 0.5, 0.0)
    return X, Y, invw, z01, near


def _edge(ax, ay, bx, by, px, py):
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax)


def _edge_in(e, a, b):
    return (e > 0) | ((e == 0) & ((a > 0) | ((a == 0) & (b > 0))))


def _f32_key(z: np.ndarray) -> np.ndarray:
    return (z.astype(np.float32) + np.float32(0)).view(np.uint32).astype(np.int64)


def sample_texture(tex: np.ndarray, u: np.ndarray, v: np.ndarray):
    """-> (uint8 [n,3], the values before rounding fp64 [n,3])"""
    th, tw = tex.shape[:2]
    tx = np.minimum(np.maximum(u * float(tw) - 0.5, -1.0), float(tw))
    ty = np.minimum(np.maximum((1.0 - v) * float(th) - 0.5, -1.0), float(th))
    fx0, fy0 = np.floor(tx), np.floor(ty)
    wx, wy = (tx - fx0)[:, None], (ty - fy0)[:, None]
    x0, x1 = np.clip(fx0.astype(np.int64), 0, tw - 1), np.clip(fx0.astype(np.int64) + 1, 0, tw - 1)
    y0, y1 = np.clip(fy0.astype(np.int64), 0, th - 1), np.clip(fy0.astype(np.int64) + 1, 0, th - 1)
    t = tex.astype(np.float64)
    a = (1.0 - wx) * t[y0, x0] + wx * t[y0, x1]
    d = (1.0 - wx) * t[y1, x0] + wx * t[y1, x1]
    raw = (1.0 - wy) * a + wy * d
    return np.clip(np.floor(raw + 0.5), 0, 255).astype(np.uint8), raw


def render(xyz, uv, faces, tex, M, out_wh, cull: str = "back", point_size: float = 1.0) -> dict:
    """One mesh's KEPT entries (xyz [kv,3], uv [kv,2], faces [kf,3] or [kf,1]), its uint8 [h,w,3] texture and one matrix -> dict(color uint8
    [H,W,4], depth fp32 [H,W], ids int32 [H,W], cover int [H,W] = the faces covering each pixel with z01 in [0,1], safe / soft bool [H,W],
    dropped = the faces dropped for an unusable vertex, tested = fragments tested, small_boxes / big_boxes = the faces walked by either path)."""
    W, H = int(out_wh[0]), int(out_wh[1])
    faces = np.asarray(faces, dtype=np.int64)
    uv = np.asarray(uv, dtype=np.float64)
    kv, points = np.asarray(xyz).shape[0], faces.shape[1] == 1
    X, Y, invw, z01, near = vertex_stage(xyz, M, W, H)
    half = int(np.rint(point_size * 128.0))
    big = np.iinfo(np.int64).max
    best = np.full((H, W), big, dtype=np.int64)   # the winning key
    zmin1 = np.full((H, W), np.inf)               # the two smallest fp32 z01 keys among the covering faces (as integers)
    zmin2 = np.full((H, W), np.inf)
    cover = np.zeros((H, W), dtype=np.int64)
    snap = np.zeros((H, W), dtype=bool)
    dropped = tested = small_boxes = big_boxes = 0
    for f in range(faces.shape[0]):
        idx = faces[f]
        if (idx < 0).any() or (idx >= kv).any():
            continue
        if (X[idx] == UNUSABLE).any():
            dropped += 1
            if not near[idx].any():
                continue
            # usable one way and not the other: everything the face could touch is unsafe - the whole image, since a box is not known
            snap[:] = True
            continue
        xs, ys = X[idx], Y[idx]
        if points:
            s, minx, maxx, miny, maxy = 1, xs[0] - half, xs[0] + half - 1, ys[0] - half, ys[0] + half - 1
        else:
            area = int(_edge(xs[0], ys[0], xs[1], ys[1], xs[2], ys[2]))
            minx, maxx, miny, maxy = xs.min(), xs.max(), ys.min(), ys.max()
        x0, x1 = max(0, int((minx + 127) >> 8)), min(W - 1, int((maxx - 128) >> 8))
        y0, y1 = max(0, int((miny + 127) >> 8)), min(H - 1, int((maxy - 128) >> 8))
        if near[idx].any():  # (before any culling: the other rounding may flip the winding of a sliver)
            snap[max(0, y0 - 1):min(H, y1 + 2), max(0, x0 - 1):min(W, x1 + 2)] = True
        if not points:
            if area == 0 or (area > 0 and cull == "back"):
                continue
            s = -1 if area < 0 else 1
        if x0 > x1 or y0 > y1:
            continue
        py, px = np.mgrid[y0:y1 + 1, x0:x1 + 1]
        PX, PY = px * 256 + 128, py * 256 + 128
        tested += PX.size
        small_boxes, big_boxes = small_boxes + (PX.size <= SMALL_BOX), big_boxes + (PX.size > SMALL_BOX)
        if points:
            inside = np.ones(PX.shape, dtype=bool)
            z = np.full(PX.shape, z01[idx[0]])
        else:
            e, inside = [], np.ones(PX.shape, dtype=bool)
            for k in range(3):
                p, q = idx[(k + 1) % 3], idx[(k + 2) % 3]
                ek = s * _edge(X[p], Y[p], X[q], Y[q], PX, PY)
                inside &= _edge_in(ek, -s * (Y[q] - Y[p]), s * (X[q] - X[p]))
                e.append(ek)
            E = float(s * area)
            z = (e[0].astype(np.float64) * z01[idx[0]] + e[1].astype(np.float64) * z01[idx[1]] + e[2].astype(np.float64) * z01[idx[2]]) / E
        inside &= (z >= 0.0) & (z <= 1.0)
        if not inside.any():
            continue
        zk = _f32_key(z)
        key = np.where(inside, (zk << 32) | f, big)
        sub = (slice(y0, y1 + 1), slice(x0, x1 + 1))
        best[sub] = np.minimum(best[sub], key)
        cover[sub] += inside
        zf = np.where(inside, zk.astype(np.float64), np.inf)
        lo, hi = np.minimum(zmin1[sub], zf), np.maximum(zmin1[sub], zf)
        zmin2[sub] = np.minimum(zmin2[sub], hi)
        zmin1[sub] = lo
    hit = best != big
    ids = np.where(hit, best & 0xFFFFFFFF, -1).astype(np.int32)
    color = np.zeros((H, W, 4), dtype=np.uint8)
    depth = np.full((H, W), np.inf, dtype=np.float32)
    soft = np.zeros((H, W), dtype=bool)
    planes = np.zeros((H, W), dtype=bool)
    yy, xx = np.nonzero(hit)
    if yy.size:
        fi = faces[ids[yy, xx]]
        if points:
            i0 = fi[:, 0]
            u, v, w = uv[i0, 0], uv[i0, 1], 1.0 / invw[i0]
            zwin = z01[i0]
        else:
            PX, PY = xx * 256 + 128, yy * 256 + 128
            area = _edge(X[fi[:, 0]], Y[fi[:, 0]], X[fi[:, 1]], Y[fi[:, 1]], X[fi[:, 2]], Y[fi[:, 2]])
            s = np.where(area < 0, -1, 1)
            e = [s * _edge(X[fi[:, (k + 1) % 3]], Y[fi[:, (k + 1) % 3]], X[fi[:, (k + 2) % 3]], Y[fi[:, (k + 2) % 3]], PX, PY) for k in range(3)]
            sk = [e[k].astype(np.float64) * invw[fi[:, k]] for k in range(3)]
            S = sk[0] + sk[1] + sk[2]
            bk = [sk[k] / S for k in range(3)]
            u = bk[0] * uv[fi[:, 0], 0] + bk[1] * uv[fi[:, 1], 0] + bk[2] * uv[fi[:, 2], 0]
            v = bk[0] * uv[fi[:, 0], 1] + bk[1] * uv[fi[:, 1], 1] + bk[2] * uv[fi[:, 2], 1]
            E = (s * area).astype(np.float64)
            w = E / S
            zwin = (e[0].astype(np.float64) * z01[fi[:, 0]] + e[1].astype(np.float64) * z01[fi[:, 1]] + e[2].astype(np.float64) * z01[fi[:, 2]]) / E
        bgr, raw = sample_texture(np.asarray(tex), u, v)
        color[yy, xx, :3], color[yy, xx, 3] = bgr, 255
        depth[yy, xx] = w.astype(np.float32)
        soft[yy, xx] = (np.abs(raw - np.floor(raw) - 0.5) < COLOUR_MARGIN).any(axis=1)
        planes[yy, xx] = (zwin < PLANE_MARGIN) | (zwin > 1.0 - PLANE_MARGIN)
    with np.errstate(invalid="ignore"):
        close = np.isfinite(zmin2) & (zmin2 - zmin1 < CLOSE_ULPS)
    return dict(color=color, depth=depth, ids=ids, cover=cover, safe=~(snap | close | planes), soft=soft, dropped=dropped, tested=tested, small_boxes=small_boxes,
                big_boxes=big_boxes)


def ulps(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """distance in fp32 steps; equal infinities are 0 apart"""
    ia, ib = (np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64) for x in (a, b))
    return np.abs(ia - ib)


# ---- the cases the GPU tests render and the CPU test checks the safe-mask cap for

MESH_CAMERA = dict(fov_deg=50.0, min_depth=0.5, max_depth=20.0)  # of depth_frames_to_mesh, as tests/test_gpu_mesh.py
ALPHAS = ("checker_blocks", "hole")  # one per image: the kept counts differ and both drop faces


def _alpha(kind: str, h: int, w: int) -> np.ndarray:
    yy, xx = np.mgrid[:h, :w]
    if kind == "all255":
        return np.full((h, w), 255, np.uint8)
    if kind == "checker_blocks":
        return np.where(((yy // 7) + (xx // 9)) % 4 == 3, 0, 255).astype(np.uint8)
    if kind == "hole":
        return np.where((yy - h // 2) ** 2 + (xx - w // 3) ** 2 < (h // 4) ** 2, 0, 255).astype(np.uint8)
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def case_frames(w: int, h: int, alphas: tuple, seed: int, smooth: bool) -> np.ndarray:
    """uint8 [B,h,w,4] frames as tests/test_gpu_mesh.py builds them: random 24-bit depth (smooth: a random low-order surface instead, so that a
    dense grid makes a surface and not spikes) and a structured alpha per image"""
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 256, size=(len(alphas), h, w, 4)).astype(np.uint8)
    if smooth is True:
        yy, xx = np.mgrid[:h, :w] / float(max(h, w))
        for i in range(len(alphas)):
            a = rng.uniform(-1, 1, size=6)
            d = 0.5 + 0.2 * (a[0] * np.sin(5 * xx + a[1]) + a[2] * np.cos(4 * yy + a[3]) + a[4] * np.sin(7 * xx * yy + a[5]))
            u24 = np.clip(d * 2 ** 24, 0, 2 ** 24 - 1).astype(np.int64)
            f[i, ..., 0], f[i, ..., 1], f[i, ..., 2] = u24 & 255, (u24 >> 8) & 255, u24 >> 16
    if smooth == "constant":
        f[..., 0], f[..., 1], f[..., 2] = TIES_U24 & 255, (TIES_U24 >> 8) & 255, TIES_U24 >> 16
    for i, kind in enumerate(alphas):
        f[i, ..., 3] = _alpha(kind, h, w)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def case_texture(w: int, h: int, seed: int) -> np.ndarray:
    t = np.random.default_rng(seed).integers(0, 256, size=(h, w, 3)).astype(np.uint8)
    t.setflags(write=False)
    return t


def pose(yaw_deg=0.0, pitch_deg=0.0, distance=None, zooms=0, translate=(0.0, 0.0, 0.0)) -> oc.OrbitCamera:
    cam = oc.OrbitCamera() if distance is None else oc.OrbitCamera(distance)
    cam.rotate(math.radians(yaw_deg) / oc.ORBIT_SENSITIVITY, math.radians(pitch_deg) / oc.ORBIT_SENSITIVITY)
    for _ in range(zooms):
        cam.zoom(1)
    cam.translate(*translate)
    return cam


def _views(poses, wh, view_fov_deg=57.3, orthographic=False) -> np.ndarray:
    return np.stack([oc.viewer_view_proj(pose(**p), min_depth=MESH_CAMERA["min_depth"], max_depth=MESH_CAMERA["max_depth"], view_fov_deg=view_fov_deg,
                                         aspect=wh[0] / wh[1], orthographic=orthographic) for p in poses])


# near head-on, 35 degrees oblique, and a camera inside the depth range: part of the mesh lies behind it (dropped faces, near discard)
TRI_POSES = (dict(yaw_deg=1.7, pitch_deg=-0.9, distance=2.3), dict(yaw_deg=35.0, pitch_deg=6.1, distance=2.9),
             dict(yaw_deg=-21.3, pitch_deg=3.3, distance=0.8, translate=(0.0, 0.0, 300.0)))
IMAGE_WH = (640, 480)  # the photo the meshes stand for (aspect scaling of depth_frames_to_mesh)
TIES_OUT_WH, TIES_STEP = (65, 49), 4  # odd sides: the middle of the output is a pixel centre; grid columns / rows TIES_STEP pixels apart


def _ties_pose() -> dict:
    """the orthographic camera, head-on, at the distance that puts the 13 x 10 regular grid of the constant-depth frame on pixel centres: ortho zoom
    = (distance + origin_z / 2) / 2 (orbitcam.js:192-194) with origin_z = -min_depth at view offset 0.5; a grid column moves depth tan(fov / 2) 2 /
    (nx - 1) in the world, which must be TIES_STEP pixels = TIES_STEP 2 zoom / H in the world"""
    a, b, tan_half, _, _ = ms.camera(IMAGE_WH, is_metric=False, **MESH_CAMERA)
    depth = 1.0 / (a + b * (TIES_U24 / float(2 ** 24)))
    zoom = depth * tan_half * 2.0 / 12.0 * TIES_OUT_WH[1] / (2.0 * TIES_STEP)
    return dict(distance=2.0 * zoom + 0.5 * MESH_CAMERA["min_depth"])


TIES_U24 = 0x604080
CASES = {
    # name: frame (w, h), grid, alphas, threshold, jitter seed (None: the regular grid), smooth, photo / texture (w, h), poses, fov, orthographic, mode
    "tri": dict(frame_wh=(40, 30), grid=(13, 10), alphas=ALPHAS, thr=0.503, jitter_seed=11, smooth=False, tex_wh=(23, 17), poses=TRI_POSES, fov=27.3,
                ortho=False, mode="triangles", out_whs=((64, 48), (37, 29)), culls=("back", "none"), point_sizes=(1.0,)),
    "coop": dict(frame_wh=(64, 48), grid=(64, 48), alphas=("all255",), thr=0.0, jitter_seed=5, smooth=True, tex_wh=(31, 22),
                 poses=(dict(yaw_deg=12.1, pitch_deg=-4.3, distance=0.3),), fov=13.7, ortho=False, mode="triangles", out_whs=((160, 120),), culls=("back",),
                 point_sizes=(1.0,)),
    "points": dict(frame_wh=(40, 30), grid=(13, 10), alphas=ALPHAS, thr=0.503, jitter_seed=11, smooth=False, tex_wh=(23, 17), poses=TRI_POSES[:2], fov=27.3,
                   ortho=False, mode="points", out_whs=((64, 48),), culls=("back",), point_sizes=(1.0, 3.0)),
    # a regular grid of constant depth, head-on through the orthographic camera: vertex columns, rows and the cells' diagonals pass through pixel
    # centres, so the fill rule alone decides those pixels
    "ties": dict(frame_wh=(40, 30), grid=(13, 10), alphas=("all255", "hole"), thr=0.503, jitter_seed=None, smooth="constant", tex_wh=(23, 17),
                 poses=(_ties_pose(),), fov=57.3, ortho=True, mode="triangles", out_whs=(TIES_OUT_WH,), culls=("back", "none"), point_sizes=(1.0,)),
}


def case_mesh_inputs(name: str):
    """-> (case, frames uint8 [B,h,w,4], vertex table or None, textures list): what depth_frames_to_mesh / mesh_restate.mesh_of_frame take"""
    c = CASES[name]
    # (the viewer's jitter rule on the case's own grid, seed pinned: mesh_plane_grid's rule, whose grid follows from a face target instead)
    table = None if c["jitter_seed"] is None else ms.jitter_xy(*c["grid"], 1.0, np.random.RandomState(c["jitter_seed"]))
    frames = case_frames(*c["frame_wh"], c["alphas"], 3, c["smooth"])
    return c, frames, table, [case_texture(*c["tex_wh"], 20 + i) for i in range(len(c["alphas"]))]


def case_views(name: str, out_wh) -> np.ndarray:
    c = CASES[name]
    return _views(c["poses"], out_wh, c["fov"], c["ortho"])


def render_case(meshes, textures, views, out_wh, cull, point_size) -> list:
    """meshes = per image (xyz, uv, faces) kept entries -> [image][view] dicts of render()"""
    return [[render(x, u, f, t, M, out_wh, cull, point_size) for M in views] for (x, u, f), t in zip(meshes, textures)]
