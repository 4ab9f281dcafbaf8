"""The 3D viewer's WebGL drawing of the mesh from any number of viewpoints, the step that needs a browser there (render_mesh:
3dviewer/index.html:1158-1228; cameras in orbit_camera.py, DPTModel.render_views makes the whole call). Kernels: csrc/post_render.inc."""

from __future__ import annotations

import numpy as np
import torch
from torch import Tensor

from .. import native
from . import fill
from ._common import TEXTURE_RECORD, _launch, _need_cuda, _photo_list, _upload_records, ptr, record_table, scratch_bytes, scratch_chunk, upload

RENDER_CULL = ("back", "none")


def render_mesh(xyz: Tensor, uv: Tensor, faces: Tensor, counts: Tensor, textures_bgr, view_proj, out_wh, cull: str = "back", point_size: float = 1.0,
                return_depth: bool = False, return_face_ids: bool = False, max_scratch_bytes: int = fill.RENDER_MAX_SCRATCH_BYTES, fill_holes=None):
    """The slabs depth_frames_to_mesh returns (its bounds are not needed), read in place with their device-side counts, rendered from V viewpoints each: what the
    reference's 3D viewer draws with WebGL (3dviewer/index.html:1158-1228 render_3d, the mesh shaders of shaders.js) and saves frame by frame through canvas.toDataURL().
    textures_bgr: one uint8 [h,w,3] BGR image per mesh, any sizes - host arrays (staged through pinned memory) or CUDA tensors (read in place; a strided view is copied) -
    the photo, or a depth_to_color image for the viewer's "depth as texture". view_proj: [V,16] (shared by the meshes) or [B,V,16], the reference's layout, clip = [x, y,
    z, 1] M: orbit_camera.viewer_view_proj / swing_views / stereo_views make them. out_wh = (w, h). cull: "back" = the viewer's gl.enable(CULL_FACE), "none" draws both
    windings. The mode follows faces.shape[-1]: 3 triangles, 1 points (squares of point_size pixels). -> color uint8 [B,V,h,w,4] BGRA (covered pixels alpha 255,
    background 0,0,0,0) and, as asked, depth fp32 [B,V,h,w] (the clip-space w: the distance along the view axis for the perspective camera; background +inf) and face ids
    int32 [B,V,h,w] (index in the kept-face order, background -1): a tuple when more than the colour is asked for. Nothing is read back, nothing synchronises; the result
    is bit-deterministic. The arithmetic (include/mdpt.h, mdpt_post_render): vertices in fp64 snapped to 1/256 pixel, int64 edge functions with the top-left fill rule, a
    uint64 z-buffer merged with integer atomic min, perspective-correct fp64 barycentrics, bilinear texture sample, one rounding. Deviations from GL: a face with a vertex
    at w <= 0 is dropped, not clipped against the near plane; mipmapped minification (LINEAR_MIPMAP_LINEAR, textures.js:200) and anti-aliasing are NOT reproduced (level
    0, one sample per pixel). Four launches per chunk of views; the views are chunked so that the scratch (8 bytes per output pixel and 24 per vertex, per mesh and view)
    stays within max_scratch_bytes where one view allows. fill_holes: None, or the band of fill_holes below, applied to every view after the render: the colour and, when
    asked for, the depth are the filled ones (exactly what fill_holes makes of this call's result without it); face ids stay -1 on filled pixels."""
    what = "render_mesh"
    if fill_holes is not None:
        band = fill._fill_band(fill_holes, what, "fill_holes")
        out = render_mesh(xyz, uv, faces, counts, textures_bgr, view_proj, out_wh, cull, point_size, True, return_face_ids, max_scratch_bytes)
        filled = fill.fill_holes(out[0], out[1], band, return_depth, max_scratch_bytes)
        out = ((filled[0], filled[1]) if return_depth else (filled,)) + tuple(out[2:])
        return out[0] if len(out) == 1 else out
    for t, name in ((xyz, "xyz"), (uv, "uv"), (faces, "faces"), (counts, "counts")):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{what}: {name} must be a tensor depth_frames_to_mesh returned, got {type(t)}")
    if xyz.dim() != 3 or xyz.shape[2] != 3 or xyz.dtype != torch.float32 or xyz.shape[0] == 0 or xyz.shape[1] == 0:
        raise ValueError(f"{what}: xyz must be float32 [B,nv,3], got {xyz.dtype} {tuple(xyz.shape)}")
    b, nv = int(xyz.shape[0]), int(xyz.shape[1])
    if uv.dtype != torch.float32 or tuple(uv.shape) != (b, nv, 2):
        raise ValueError(f"{what}: uv must be float32 [{b},{nv},2], got {uv.dtype} {tuple(uv.shape)}")
    if faces.dtype != torch.int32 or faces.dim() != 3 or faces.shape[0] != b or faces.shape[2] not in (1, 3) or faces.shape[1] == 0:
        raise ValueError(f"{what}: faces must be int32 [{b},nf,3] (triangles) or [{b},{nv},1] (points), got {faces.dtype} {tuple(faces.shape)}")
    points = faces.shape[2] == 1
    if points and faces.shape[1] != nv:
        raise ValueError(f"{what}: a point list holds one face per vertex, got {faces.shape[1]} faces for {nv} vertices")
    if counts.dtype != torch.int32 or tuple(counts.shape) != (b, 2):
        raise ValueError(f"{what}: counts must be int32 [{b},2], got {counts.dtype} {tuple(counts.shape)}")
    if cull not in RENDER_CULL:
        raise ValueError(f"{what}: cull must be 'back' or 'none', got {cull!r}")
    point_size = float(point_size)
    if not 0.0 < point_size <= 1024.0:
        raise ValueError(f"{what}: point_size must be in (0, 1024], got {point_size}")
    w, h = int(out_wh[0]), int(out_wh[1])
    if not (0 < w <= 32768 and 0 < h <= 32768):
        raise ValueError(f"{what}: out_wh must be (w, h) with sides of 1 .. 32768, got {tuple(out_wh)}")
    scratch_chunk(1, 1, max_scratch_bytes, what)  # (the budget is checked before the device is)
    on_device = isinstance(view_proj, torch.Tensor) and view_proj.device.type == "cuda"
    views = view_proj.detach() if on_device else np.asarray(view_proj.numpy() if isinstance(view_proj, torch.Tensor) else view_proj, dtype=np.float64)
    if tuple(views.shape[-2:]) == (4, 4):
        views = views.reshape(*views.shape[:-2], 16)
    if views.ndim not in (2, 3) or views.shape[-1] != 16 or views.shape[-2] == 0 or (views.ndim == 3 and views.shape[0] != b):
        raise ValueError(f"{what}: view_proj must be [V,16] or [{b},V,16] (row vector times matrix), got {tuple(views.shape)}")
    if not on_device and not np.isfinite(views).all():
        raise ValueError(f"{what}: view_proj holds values that are not finite")
    if on_device and not views.dtype.is_floating_point:
        raise ValueError(f"{what}: view_proj must be floating point, got {views.dtype}")
    nf, n_views = int(faces.shape[1]), int(views.shape[-2])
    photos, on_device = _photo_list(textures_bgr, b, what)
    _need_cuda([xyz, uv, faces, counts], what)
    dev = xyz.device
    if any(t.device != dev for t in (uv, faces, counts)) or (on_device and photos[0].device != dev):
        raise RuntimeError(f"{what}: the tensors are on different devices")
    xyz, uv, faces, counts = (t.detach().contiguous() for t in (xyz, uv, faces, counts))
    if isinstance(views, np.ndarray):
        views = torch.from_numpy(np.array(np.broadcast_to(views, (b, n_views, 16))))
    views = views.to(dev, torch.float64).expand(b, n_views, 16).contiguous()
    staged, tex_ptrs = (None, [f.data_ptr() for f in photos]) if on_device else upload(photos, dev, 16)
    records = record_table(TEXTURE_RECORD, photos, ("bgr", "h", "w"), tex_ptrs)
    table = _upload_records(records, dev)
    per_view = scratch_bytes("mdpt_post_render_scratch_bytes", b, 1, nv, nf, h, w)
    chunk = scratch_chunk(n_views, per_view, max_scratch_bytes, what, 65535 // b)
    if b > 65535:
        raise ValueError(f"{what}: at most 65535 meshes per call, got {b}")
    color = torch.empty((b, n_views, h, w, 4), device=dev, dtype=torch.uint8)
    depth = torch.empty((b, n_views, h, w), device=dev, dtype=torch.float32) if return_depth else None
    ids = torch.empty((b, n_views, h, w), device=dev, dtype=torch.int32) if return_face_ids else None
    scratch = torch.empty(chunk * per_view // 8, device=dev, dtype=torch.int64)
    mode = native.MESH_POINTS if points else native.MESH_TRIANGLES
    for v0 in range(0, n_views, chunk):
        nvw = min(chunk, n_views - v0)
        whole = nvw == n_views
        # a chunk of views writes its own [B,nvw,...] block, copied into place (one call, no copy, when the scratch allows every view)
        vp = views if whole else views[:, v0:v0 + nvw].contiguous()
        c = color if whole else torch.empty((b, nvw, h, w, 4), device=dev, dtype=torch.uint8)
        d = depth if whole or depth is None else torch.empty((b, nvw, h, w), device=dev, dtype=torch.float32)
        i = ids if whole or ids is None else torch.empty((b, nvw, h, w), device=dev, dtype=torch.int32)
        _launch(dev, "mdpt_post_render", xyz.data_ptr(), uv.data_ptr(), faces.data_ptr(), counts.data_ptr(), b, nv, nf, mode, records.ctypes.data,
                table.data_ptr(), vp.data_ptr(), nvw, h, w, int(cull == "back"), point_size, c.data_ptr(), ptr(d), ptr(i), scratch.data_ptr(), nvw * per_view)
        if not whole:
            color[:, v0:v0 + nvw] = c
            if depth is not None:
                depth[:, v0:v0 + nvw] = d
            if ids is not None:
                ids[:, v0:v0 + nvw] = i
    del staged  # (the caching allocator reuses it in stream order only)
    out = (color,) + ((depth,) if return_depth else ()) + ((ids,) if return_face_ids else ())
    return out[0] if len(out) == 1 else out
