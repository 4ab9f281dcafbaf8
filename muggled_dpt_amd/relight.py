"""Surface normals and relighting from depth maps (not in the reference): the surface normal of every photo pixel under the camera of the mesh export
(postprocess.depth_frames_to_mesh: x right, y up, the camera looks along -z), so the normals are by construction those of the mesh this project exports and
renders. depth_normals returns them as fp32 unit vectors and, asked, as encoded uint8 normal maps; relight_images shades the photo once per light ("portrait
lighting", the sibling of refocus's "portrait mode"), or a white surface where no photo is given (a hillshade, which shows the facets, ringing and seams of a
depth map that a colormap hides); DPTModel.inference_normals / inference_relight start from the photos. The differences are edge-aware: across a depth
discontinuity the one-sided difference is taken, never the central one, which would smear every depth edge into a band of grazing normals.
shade_images is relight_images with cast shadows and ambient occlusion: screen-space shadow marches and horizon occlusion on a small working grid, resized
to the photo and folded into the shading; light_occlusion returns the two kinds of plane alone; DPTModel.inference_shade starts from the photos.
Kernels: csrc/post_normals.inc (mdpt_post_normals), csrc/post_shadows.inc (mdpt_post_shadows); the arithmetic is written out in include/mdpt.h.

Known limits: the normals of a relative-depth model depend on the assumed fov_deg, min_depth and max_depth, which are the viewer's controls, not measurements.
Shading multiplies a photo that already carries its own lighting and is done on the gamma-encoded bytes, not in linear light. relight_images has no cast
shadows and no ambient occlusion; shade_images' are screen space only - a depth map knows the first surface along every ray of one camera, so what lies
outside the frame or hidden behind that surface casts nothing, and how thick an occluder is (shadow_thickness) is assumed, not known; a shadow march and an
occlusion direction reach at most 32 nodes of the working grid; the only penumbra is the bilinear resize of the 0 / 1 shadow plane to the photo. Output
quality on real photographs is unverified - no checkpoint can be loaded where this was written; the tests hold the arithmetic and synthetic scenes only."""

from __future__ import annotations

import math

import numpy as np
import torch

from . import native
from .postprocess._common import (NORMALS_RECORD, SHADOWS_RECORD, _launch, _photo_list, _photo_pointers, _prediction_list, _upload_records, _views,
                                  packed_offsets, prediction_count, record_table, scratch_bytes)
from .postprocess.mesh import MESH_FOV_DEG, MESH_MAX_DEPTH, MESH_MIN_DEPTH

__all__ = ["NORMALS_SPACES", "depth_normals", "relight_images", "light_sweep", "default_step", "light_occlusion", "shade_images"]

NORMALS_SPACES = {"inverse": native.ALIGN_INVERSE, "depth": native.ALIGN_DEPTH}
# (NORMALS_RECORD and SHADOWS_RECORD, mdpt_normals_pair and mdpt_shadows_pair of include/mdpt.h, stand with the other record tables in
# postprocess/_common.py; csrc/mdpt_post_photo.cpp static_asserts the layouts)


def light_sweep(n: int, elevation_deg: float = 35.0) -> np.ndarray:
    """A closed ring of n unit light directions around the camera axis -> float64 [n,3]: direction k points towards the light at azimuth 2 pi k / n in the
    image plane (0: from the right, counter-clockwise seen from the camera) and elevation_deg above it, towards the camera (90: straight from the camera).
    The lights of relight_images for a sweep around a portrait, as orbit_camera.swing_views is the cameras' of a swing. Plain host math."""
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1:
        raise ValueError(f"light_sweep: n must be an int >= 1, got {n!r}")
    el = float(elevation_deg)
    if not -90.0 <= el <= 90.0:
        raise ValueError(f"light_sweep: elevation_deg must be in [-90, 90], got {elevation_deg}")
    az = np.arange(int(n), dtype=np.float64) * (2.0 * math.pi / int(n))
    d = np.stack([math.cos(math.radians(el)) * np.cos(az), math.cos(math.radians(el)) * np.sin(az), np.full(int(n), math.sin(math.radians(el)))], axis=1)
    return d / np.sqrt((d * d).sum(axis=1, keepdims=True))


def default_step(W: int, w: int) -> int:
    """the difference step for a map w wide shown on a photo W wide: about one map cell, min(16, max(1, floor(W / w + 0.5))) photo pixels"""
    return min(native.NORMALS_MAX_STEP, max(1, int(math.floor(W / w + 0.5))))


def _unit_lights(light_dirs, what: str) -> np.ndarray:
    """a single (x, y, z) or [V,3] directions towards the lights -> float64 [V,3], each normalised in fp64"""
    d = np.asarray(light_dirs.detach().cpu().numpy() if isinstance(light_dirs, torch.Tensor) else light_dirs, dtype=np.float64)
    if d.ndim == 1:
        d = d[None]
    if d.ndim != 2 or d.shape[1] != 3 or not 1 <= d.shape[0] <= native.NORMALS_MAX_LIGHTS:
        raise ValueError(f"{what}: light_dirs must be (x, y, z) or [V,3] with 1 <= V <= {native.NORMALS_MAX_LIGHTS}, got shape {d.shape}")
    with np.errstate(all="ignore"):
        length = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    if not (np.isfinite(d).all() and np.isfinite(length).all() and (length > 0.0).all()):
        raise ValueError(f"{what}: every light direction must be finite and not zero, got {d.tolist()}")
    return np.ascontiguousarray(d / length[:, None])


def _normals_checked(predictions, target_hws, images_bgr, space, fov_deg, min_depth, max_depth, step, edge_ratio, what: str):
    """everything the calls can refuse from shapes and values alone, before any tensor has to be on the device -> the checked scalars"""
    if space not in NORMALS_SPACES:
        raise ValueError(f"{what}: space must be one of {sorted(NORMALS_SPACES)}, got {space!r}")
    fov_deg, min_depth, max_depth, edge_ratio = float(fov_deg), float(min_depth), float(max_depth), float(edge_ratio)
    if not 0.0 < fov_deg < 180.0:
        raise ValueError(f"{what}: fov_deg must be in (0, 180), got {fov_deg}")
    if space == "inverse" and not (0.0 < min_depth < max_depth < float("inf")):
        raise ValueError(f"{what}: need 0 < min_depth < max_depth, finite, got {min_depth}, {max_depth}")
    if step is not None and (isinstance(step, bool) or not isinstance(step, (int, np.integer)) or not 1 <= int(step) <= native.NORMALS_MAX_STEP):
        raise ValueError(f"{what}: step must be None (about one map cell) or an int in 1 .. {native.NORMALS_MAX_STEP} (photo pixels), got {step!r}")
    if not edge_ratio >= 1.0:
        raise ValueError(f"{what}: edge_ratio must be >= 1 (inf: always the central difference), got {edge_ratio}")
    n = prediction_count(predictions)
    if n >= 0 and isinstance(images_bgr, (list, tuple)):
        if len(images_bgr) != n:
            raise ValueError(f"{what}: {n} predictions but {len(images_bgr)} images")
        for k, f in enumerate(images_bgr):
            if isinstance(f, (np.ndarray, torch.Tensor)) and (f.dtype != (torch.uint8 if isinstance(f, torch.Tensor) else np.uint8) or f.ndim != 3 or f.shape[2] != 3):
                raise ValueError(f"{what}: image {k} is not a uint8 HxWx3 BGR photo (shape {tuple(f.shape)}, dtype {f.dtype})")
    if target_hws is not None:
        if images_bgr is not None:
            raise ValueError(f"{what}: give target_hws or images_bgr, not both (the output has the photo's size)")
        target_hws = [(int(hw[0]), int(hw[1])) for hw in target_hws]
        if n >= 0 and len(target_hws) != n:
            raise ValueError(f"{what}: {n} predictions but {len(target_hws)} target sizes")
        if any(h <= 0 or w <= 0 or h * w >= 2 ** 31 for h, w in target_hws):
            raise ValueError(f"{what}: target sizes must be positive (H, W) of fewer than 2^31 pixels, got {target_hws}")
    return target_hws, fov_deg, min_depth, max_depth, None if step is None else int(step), edge_ratio


def _shading_checked(ambient, diffuse, specular, shininess_log2, what: str):
    ambient, diffuse, specular = float(ambient), float(diffuse), float(specular)
    for name, v in (("ambient", ambient), ("diffuse", diffuse), ("specular", specular)):
        if not 0.0 <= v < float("inf"):
            raise ValueError(f"{what}: {name} must be finite and >= 0, got {v}")
    if isinstance(shininess_log2, bool) or not isinstance(shininess_log2, (int, np.integer)) or not 0 <= int(shininess_log2) <= 10:
        raise ValueError(f"{what}: shininess_log2 must be an int in 0 .. 10 (the exponent is 2^shininess_log2), got {shininess_log2!r}")
    return ambient, diffuse, specular, int(shininess_log2)


def _pair_table(record, symbol: str, predictions, images_bgr, checked, what: str, grid_hws=None):
    """what both entry points' tables share -> (maps, dev, what must stay alive until the launch, the photo sizes, the records with map / photo / camera /
    step / tile_off / scratch_off (and, for a record that has one, the working grid: grid_hws[i] or the map's own size, and gtile_off) filled, the scratch
    bytes): the photos taken as refocus_images takes them, the camera of depth_frames_to_mesh"""
    target_hws, fov_deg, min_depth, max_depth, step, edge_ratio = checked
    n = prediction_count(predictions)
    photos = None
    if images_bgr is not None:
        photos, on_device = _photo_list(images_bgr, n, what) if n >= 0 else (None, False)
    maps = _prediction_list(predictions, what)
    dev = maps[0].device
    if photos is not None:
        keep, img_ptrs, pitches = _photo_pointers(images_bgr, photos, on_device, dev, what)
        hws = [(int(f.shape[0]), int(f.shape[1])) for f in photos]
    else:
        keep, img_ptrs, pitches = None, [0] * len(maps), [0] * len(maps)
        hws = target_hws if target_hws is not None else [(int(m.shape[0]), int(m.shape[1])) for m in maps]
        if len(hws) != len(maps):
            raise ValueError(f"{what}: {len(maps)} predictions but {len(hws)} target sizes")
    if any(h * w >= 2 ** 31 for h, w in hws):
        raise ValueError(f"{what}: a photo of 2^31 pixels or more is not supported")
    tan_half = math.tan(fov_deg * 0.5 * (math.pi / 180.0))
    scales = [(1.0, h / w) if w > h else (w / h, 1.0) for h, w in hws]  # (x_scale, y_scale): depth_frames_to_mesh's aspect rule
    records = record_table(record, maps, photo=img_ptrs, pitch=pitches, H=[h for h, _ in hws], W=[w for _, w in hws],
                           kx=[sx * tan_half for sx, _ in scales], ky=[sy * tan_half for _, sy in scales],
                           step=[default_step(w, int(m.shape[1])) if step is None else step for (_, w), m in zip(hws, maps)])
    tile = native.NORMALS_TILE
    records["tile_off"], _ = packed_offsets([((h + tile - 1) // tile) * ((w + tile - 1) // tile) for h, w in hws])
    if "gh" in record.names:
        if grid_hws is not None and len(grid_hws) != len(maps):
            raise ValueError(f"{what}: {len(maps)} predictions but {len(grid_hws)} grid sizes")
        grids = [(int(m.shape[0]), int(m.shape[1])) if g is None else g for m, g in zip(maps, grid_hws or [None] * len(maps))]
        records["gh"], records["gw"] = [g[0] for g in grids], [g[1] for g in grids]
        records["gtile_off"], _ = packed_offsets([((gh + tile - 1) // tile) * ((gw + tile - 1) // tile) for gh, gw in grids])
    records["scratch_off"], at = packed_offsets([scratch_bytes(symbol, records[k:k + 1].ctypes.data, 1) for k in range(len(maps))])
    return maps, dev, keep, hws, records, at


def _run(predictions, images_bgr, checked, space, what: str, lights, shading, want_normals: bool, want_encoded: bool):
    _, _, min_depth, max_depth, _, edge_ratio = checked
    maps, dev, keep, hws, records, at = _pair_table(NORMALS_RECORD, "mdpt_post_normals_scratch_bytes", predictions, images_bgr, checked, what)
    offs, total = packed_offsets([h * w for h, w in hws])
    normals = encoded = relit = table_l = None
    V = 0 if lights is None else int(lights.shape[0])
    if want_normals:
        normals = torch.empty(3 * total, device=dev, dtype=torch.float32)
        records["normals"] = [normals.data_ptr() + 12 * o for o in offs]
    if want_encoded:
        encoded = torch.empty(3 * total, device=dev, dtype=torch.uint8)
        records["encoded"] = [encoded.data_ptr() + 3 * o for o in offs]
    if V:
        relit = torch.empty(3 * V * total, device=dev, dtype=torch.uint8)
        records["relit"] = [relit.data_ptr() + 3 * V * o for o in offs]
        table_l = _upload_records(lights, dev)
    scratch = torch.empty(at // 8, device=dev, dtype=torch.float64)
    table = _upload_records(records, dev)
    ambient, diffuse, specular, shininess_log2 = shading
    _launch(dev, "mdpt_post_normals", records.ctypes.data, table.data_ptr(), len(maps), native.dtype_code(maps[0].dtype), NORMALS_SPACES[space], min_depth,
            max_depth, edge_ratio, None if table_l is None else table_l.data_ptr(), V, ambient, diffuse, specular, shininess_log2, scratch.data_ptr(), at)
    del table, table_l, keep, scratch  # (the caching allocator reuses them in stream order only)
    frames = [relit[3 * V * o:3 * V * (o + h * w)].view(V, h, w, 3) for o, (h, w) in zip(offs, hws)] if V else None
    return ([v[0] for v in _views(normals, hws, (3,))] if want_normals else None, [v[0] for v in _views(encoded, hws, (3,))] if want_encoded else None, frames)


def depth_normals(predictions, target_hws=None, images_bgr=None, *, space: str = "inverse", fov_deg: float = MESH_FOV_DEG, min_depth: float = MESH_MIN_DEPTH,
                  max_depth: float = MESH_MAX_DEPTH, step=None, edge_ratio: float = 2.0, encode: bool = False):
    """Depth maps -> one fp32 [H_i,W_i,3] unit surface normal (x, y, z) per map, in order, on the device (views into one allocation), in the camera frame of
    depth_frames_to_mesh: x right, y up, the camera looks along -z, so a surface that faces the camera has n = (0, 0, 1). The output size is the photo's if
    images_bgr is given (only its size is used), else target_hws[i] = (H, W), else the map's own. encode=True: -> (normals, uint8 [H_i,W_i,3] BGR normal maps,
    byte = floor((c + 1) / 2 * 255 + 0.5), B, G, R = z, y, x, the usual bluish tangent-space look).
    Per output pixel: s = the map at the pixel's centre (bilinear; a map of the output's size is read directly); space="inverse" (relative models):
    z = 1 / (a + b v) with v = the map in its own range of finite values, a = 1 / max_depth, b = 1 / min_depth - 1 / max_depth - the viewer's depth, as
    depth_frames_to_mesh(is_metric=False); space="depth" (metric maps): z = s, valid where s > 0. The pixel is unprojected with fov_deg and the aspect rule of
    the mesh; per axis the tangent is the difference of the neighbours `step` pixels away: central where the depth differences to both are within edge_ratio
    of each other, else one-sided towards the nearer one in depth (so no normal is taken across a depth edge; edge_ratio=inf: always central), one-sided next
    to an invalid (NaN, inf; depth space: <= 0) neighbour or the border. n = Tx x Ty, normalised; a pixel without a usable neighbour on an axis is (0, 0, 0)
    and encodes to 128, 128, 128. step: an int in 1 .. 16 photo pixels; None: about one map cell, min(16, max(1, floor(W / w + 0.5))), because a
    bilinearly enlarged map is piecewise bilinear and a 1-pixel difference shows its cell grid as facets; for a guided-upsampled map of the photo's own size
    step=1 is right. The defaults (step, edge_ratio 2, the viewer's fov 50 and depths 50 .. 100) are user-facing choices, not measured optima.
    predictions / images_bgr as refocus_images takes them - a [B,h,w] tensor or a list of [1,h,w] / [h,w] CUDA maps of one dtype (fp32 / bf16 / fp16) whose
    sizes may differ. fp64 arithmetic, bit-deterministic, every pair independent of the others, at most three launches for the whole call, nothing read back,
    no synchronisation. Limits: see this module's docstring."""
    what = "depth_normals"
    checked = _normals_checked(predictions, target_hws, images_bgr, space, fov_deg, min_depth, max_depth, step, edge_ratio, what)
    if images_bgr is not None:  # only the sizes are used: no photo is uploaded or read
        checked = ([(int(f.shape[0]), int(f.shape[1])) for f in _photo_list(images_bgr, prediction_count(predictions), what)[0]],) + checked[1:]
    normals, encoded, _ = _run(predictions, None, checked, space, what, None, (0.0, 0.0, 0.0, 0), True, bool(encode))
    return (normals, encoded) if encode else normals


def relight_images(predictions, images_bgr, light_dirs, ambient: float = 0.35, diffuse: float = 0.9, specular: float = 0.0, shininess_log2: int = 4, *,
                   target_hws=None, space: str = "inverse", fov_deg: float = MESH_FOV_DEG, min_depth: float = MESH_MIN_DEPTH, max_depth: float = MESH_MAX_DEPTH,
                   step=None, edge_ratio: float = 2.0, return_normals: bool = False):
    """Depth maps and the photos they came from -> one uint8 [V,H_i,W_i,3] BGR tensor per pair, in order, on the device (views into one allocation): the photo
    shaded by its surface normals, one frame per row of light_dirs [V,3] (a single (x, y, z): V = 1; at most 64; directions TOWARDS the light in the camera frame
    of depth_normals, normalised here in fp64; light_sweep gives a ring of them). The normals are depth_normals' (same space / fov_deg / min_depth / max_depth /
    step / edge_ratio), formed once per pixel for all V lights. Per light: shade = ambient + diffuse max(0, n.l); with specular > 0 a Blinn-Phong highlight
    255 specular max(0, n.h)^(2^shininess_log2), h the half vector of the light and the view direction, the power by repeated squaring (no pow, whose last bit
    differs between libraries); out = min(255, floor(photo shade + highlight + 0.5)) per byte. A pixel without a normal keeps the photo's bytes.
    images_bgr=None with target_hws: a white-clay hillshade (every photo byte is 255). return_normals: -> (frames, fp32 [H_i,W_i,3] normals). The defaults
    (ambient 0.35, diffuse 0.9, no highlight) are user-facing choices, not measured optima. predictions / images_bgr as refocus_images takes them: host photos
    go through pinned staging, CUDA photos and pitched slices are read in place byte by byte, a photo may have any size relative to its map. fp64 arithmetic,
    bit-deterministic, at most three launches whatever the number of pairs and lights, nothing read back. Limits (gamma-space mix of a photo that carries its
    own lighting, no cast shadows, no ambient occlusion): see this module's docstring."""
    what = "relight_images"
    checked = _normals_checked(predictions, target_hws, images_bgr, space, fov_deg, min_depth, max_depth, step, edge_ratio, what)
    shading = _shading_checked(ambient, diffuse, specular, shininess_log2, what)
    lights = _unit_lights(light_dirs, what)
    normals, _, frames = _run(predictions, images_bgr, checked, space, what, lights, shading, bool(return_normals), False)
    return (frames, normals) if return_normals else frames


def _occlusion_checked(n: int, grid_hw, shadow_reach, shadow_bias, shadow_thickness, ao_reach, ao_radius, ao_bias, ao_strength, what: str):
    """the occlusion controls and the working grid, refused from values alone -> (per-pair grid sizes or None, the checked controls in the entry point's order)"""
    for name, v in (("shadow_reach", shadow_reach), ("ao_reach", ao_reach)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= native.SHADOWS_MAX_REACH:
            raise ValueError(f"{what}: {name} must be an int in 0 .. {native.SHADOWS_MAX_REACH} (grid nodes), got {v!r}")
    shadow_bias, shadow_thickness, ao_radius, ao_bias, ao_strength = float(shadow_bias), float(shadow_thickness), float(ao_radius), float(ao_bias), float(ao_strength)
    if not 0.0 <= shadow_bias < 1.0:
        raise ValueError(f"{what}: shadow_bias must be in [0, 1), got {shadow_bias}")
    if not shadow_thickness >= 0.0:
        raise ValueError(f"{what}: shadow_thickness must be >= 0 (inf: an occluder of any thickness), got {shadow_thickness}")
    if not 0.0 < ao_radius < float("inf"):
        raise ValueError(f"{what}: ao_radius must be finite and > 0, got {ao_radius}")
    for name, v in (("ao_bias", ao_bias), ("ao_strength", ao_strength)):
        if not 0.0 <= v < float("inf"):
            raise ValueError(f"{what}: {name} must be finite and >= 0, got {v}")
    grids = None
    if grid_hw is not None:
        try:
            one = len(grid_hw) == 2 and all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in grid_hw)
            grids = [grid_hw] * max(n, 1) if one else list(grid_hw)
            grids = [None if g is None else (int(g[0]), int(g[1])) for g in grids]
            if any(g is not None and (len(g) != 2) for g in grids):
                raise TypeError
        except TypeError:
            raise ValueError(f"{what}: grid_hw must be None (each map's own size), one (gh, gw) or one (gh, gw) / None per pair, got {grid_hw!r}") from None
        if n >= 0 and len(grids) != n:
            raise ValueError(f"{what}: {n} predictions but {len(grids)} grid sizes")
        if any(g is not None and (g[0] <= 0 or g[1] <= 0 or g[0] * g[1] >= 2 ** 31) for g in grids):
            raise ValueError(f"{what}: grid sizes must be positive (gh, gw) of fewer than 2^31 nodes, got {grid_hw!r}")
    return grids, (int(shadow_reach), shadow_bias, shadow_thickness, int(ao_reach), ao_radius, ao_bias, ao_strength)


def _run_shadows(predictions, images_bgr, checked, space, what: str, lights, shading, grids, occlusion, want_frames: bool, want_planes: bool):
    """one mdpt_post_shadows call -> (frames or None, ao planes or None, vis planes or None)"""
    _, _, min_depth, max_depth, _, edge_ratio = checked
    maps, dev, keep, hws, records, at = _pair_table(SHADOWS_RECORD, "mdpt_post_shadows_scratch_bytes", predictions, images_bgr, checked, what, grids)
    ghws = [(int(r["gh"]), int(r["gw"])) for r in records]
    shadow_reach, _, _, ao_reach, _, _, ao_strength = occlusion
    V = 0 if lights is None else int(lights.shape[0])
    ao = vis = relit = table_l = None
    goffs, gtotal = packed_offsets([gh * gw for gh, gw in ghws])
    if want_planes or (want_frames and ao_reach > 0 and ao_strength > 0.0):
        ao = torch.empty(gtotal, device=dev, dtype=torch.float32)
        records["ao"] = [ao.data_ptr() + 4 * o for o in goffs]
    if V and (want_planes or (want_frames and shadow_reach > 0)):
        vis = torch.empty(V * gtotal, device=dev, dtype=torch.float32)
        records["vis"] = [vis.data_ptr() + 4 * V * o for o in goffs]
    offs, total = packed_offsets([h * w for h, w in hws])
    if want_frames:
        relit = torch.empty(3 * V * total, device=dev, dtype=torch.uint8)
        records["relit"] = [relit.data_ptr() + 3 * V * o for o in offs]
    if V:
        table_l = _upload_records(lights, dev)
    scratch = torch.empty(at // 8, device=dev, dtype=torch.float64)
    table = _upload_records(records, dev)
    ambient, diffuse, specular, shininess_log2 = shading
    _launch(dev, "mdpt_post_shadows", records.ctypes.data, table.data_ptr(), len(maps), native.dtype_code(maps[0].dtype), NORMALS_SPACES[space], min_depth,
            max_depth, edge_ratio, None if table_l is None else table_l.data_ptr(), V, ambient, diffuse, specular, shininess_log2, *occlusion, scratch.data_ptr(), at)
    del table, table_l, keep, scratch  # (the caching allocator reuses them in stream order only)
    frames = [relit[3 * V * o:3 * V * (o + h * w)].view(V, h, w, 3) for o, (h, w) in zip(offs, hws)] if want_frames else None
    ao_planes = [ao[o:o + gh * gw].view(gh, gw) for o, (gh, gw) in zip(goffs, ghws)] if ao is not None and want_planes else None
    vis_planes = [vis[V * o:V * (o + gh * gw)].view(V, gh, gw) for o, (gh, gw) in zip(goffs, ghws)] if vis is not None and want_planes else None
    return frames, ao_planes, vis_planes


def light_occlusion(predictions, light_dirs=None, *, grid_hw=None, target_hws=None, space: str = "inverse", fov_deg: float = MESH_FOV_DEG,
                    min_depth: float = MESH_MIN_DEPTH, max_depth: float = MESH_MAX_DEPTH, edge_ratio: float = 2.0, shadow_reach: int = 32,
                    shadow_bias: float = 0.02, shadow_thickness: float = float("inf"), ao_reach: int = 8, ao_radius: float = 0.25, ao_bias: float = 0.05,
                    ao_strength: float = 1.0):
    """Depth maps -> (ao, vis): per map the ambient-occlusion plane, fp32 [gh,gw] in [0, 1] (1: open), and the cast-shadow planes, fp32 [V,gh,gw] of 0.0
    (in shadow) / 1.0 (lit), one per row of light_dirs (None: vis is None) - the planes shade_images folds into its shading, alone, for callers who composite
    themselves; on the device, views into one allocation each. grid_hw: the working grid, None = each map's own (h, w) (read directly), or one (gh, gw) for
    every pair, or one (gh, gw) / None per pair: node (i, j) is pixel (i, j) of a gh x gw image over the photo's field of view, the depth there by
    depth_normals' rule (space / min_depth / max_depth), its normal by depth_normals' at a step of one node (edge_ratio). target_hws: the photos' sizes
    (H, W), which set the camera's aspect (None: the map's own). Shadow: from every node the ray towards the light is marched shadow_reach nodes (0 .. 32)
    along its projection; a nearer surface whose depth is less than the ray's by more than shadow_bias (relative) and by at most shadow_thickness (relative;
    inf: any) shadows the node. Occlusion: along the eight lattice directions, ao_reach nodes (0 .. 32), the highest rise of the surface above the node's
    tangent plane beyond ao_bias, faded to nothing at the distance ao_radius times the node's depth; ao = 1 - ao_strength times their mean. Screen space:
    what is outside the frame or hidden behind the first surface casts nothing. The defaults are user-facing choices, not measured optima. fp64
    arithmetic written out in include/mdpt.h (mdpt_post_shadows), bit-deterministic, at most three launches, nothing read back."""
    what = "light_occlusion"
    checked = _normals_checked(predictions, target_hws, None, space, fov_deg, min_depth, max_depth, None, edge_ratio, what)
    grids, occlusion = _occlusion_checked(prediction_count(predictions), grid_hw, shadow_reach, shadow_bias, shadow_thickness, ao_reach, ao_radius, ao_bias,
                                          ao_strength, what)
    lights = None if light_dirs is None else _unit_lights(light_dirs, what)
    _, ao, vis = _run_shadows(predictions, None, checked, space, what, lights, (0.0, 0.0, 0.0, 0), grids, occlusion, False, True)
    return ao, vis


def shade_images(predictions, images_bgr, light_dirs, ambient: float = 0.35, diffuse: float = 0.9, specular: float = 0.0, shininess_log2: int = 4, *,
                 shadow_reach: int = 32, shadow_bias: float = 0.02, shadow_thickness: float = float("inf"), ao_reach: int = 8, ao_radius: float = 0.25,
                 ao_bias: float = 0.05, ao_strength: float = 1.0, grid_hw=None, target_hws=None, space: str = "inverse", fov_deg: float = MESH_FOV_DEG,
                 min_depth: float = MESH_MIN_DEPTH, max_depth: float = MESH_MAX_DEPTH, step=None, edge_ratio: float = 2.0, return_planes: bool = False):
    """relight_images with cast shadows and ambient occlusion -> one uint8 [V,H_i,W_i,3] BGR tensor per pair, in order, on the device: the planes of
    light_occlusion (same controls, same working grid) are formed once, resized to the photo (bilinear at the pixel's centre, the only penumbra) and folded
    into relight_images' shading: shade = ambient ao + diffuse max(0, n.l) vis_v, the highlight times vis_v; everything else - normals, photo bytes, invalid
    pixels, inputs (host photos through pinned staging, pitched CUDA views in place, images_bgr=None with target_hws for white clay) - is relight_images'.
    shadow_reach=0 switches the shadows off, ao_strength=0 (or ao_reach=0) the occlusion; with both off every byte equals relight_images'.
    return_planes: -> (frames, ao planes, vis planes). The defaults (shadow_reach 32, shadow_bias 0.02, shadow_thickness inf, ao_reach 8, ao_radius 0.25,
    ao_bias 0.05, ao_strength 1) are user-facing choices, not measured optima. fp64 arithmetic, bit-deterministic, at most four launches whatever the
    number of pairs and lights, nothing read back. Limits (screen space only, an assumed thickness, a reach of at most 32 grid nodes, a gamma-space mix,
    unverified on real photographs): see this module's docstring."""
    what = "shade_images"
    checked = _normals_checked(predictions, target_hws, images_bgr, space, fov_deg, min_depth, max_depth, step, edge_ratio, what)
    shading = _shading_checked(ambient, diffuse, specular, shininess_log2, what)
    grids, occlusion = _occlusion_checked(prediction_count(predictions), grid_hw, shadow_reach, shadow_bias, shadow_thickness, ao_reach, ao_radius, ao_bias,
                                          ao_strength, what)
    lights = _unit_lights(light_dirs, what)
    frames, ao, vis = _run_shadows(predictions, images_bgr, checked, space, what, lights, shading, grids, occlusion, True, bool(return_planes))
    return (frames, ao, vis) if return_planes else frames
