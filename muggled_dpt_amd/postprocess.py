"""Depth post-processing on the GPU: drop-in for the tensor helpers of the reference's muggled_dpt/demo_helpers/postprocess.py
(scale_prediction :22-29, normalize_01 :63-74, convert_to_uint8 :79-91) plus the 24-bit packing step of run_3dviewer.py:576-590, and the
display tail of its video / image demos per image (histogram_equalization :107-145, the colormap LUT of toadui/colormaps.py:237-259, and
depth_to_color, the whole per-frame loop of run_video.py:348-361 over a batch), the still-image demo's display loop and save path
(depth_to_display / depth_for_saving, run_image.py:185-195, 323-358, with the plane fit of demo_helpers/plane_fit.py) and the 3D viewer's
edge alpha (depth_edge_mask / pack_depth_u24_frames, run_3dviewer.py:455-505, 576-593), and the depth masking demo's display and cutouts
(depth_mask_display / depth_mask_images, experiments/depth_masking.py), and the tiles of its block norm viewer (block_norm_display,
experiments/block_norm_visualization.py), and the 3D viewer's mesh export (depth_frames_to_mesh / mesh_views, demo_helpers/3dviewer/*.js; files
through mesh_io), and - not in the reference, which only describes the fit - the stitching of tile maps into one map at a photo's resolution
(stitch_tiles; layouts in tiling.py, DPTModel.inference_tiled makes the whole call), and the alignment of predictions to measured depth maps with
the standard metrics and true depth (fit_true_depth / depth_metrics / true_depth; DPTModel.evaluate_depth makes the whole call), and the 3D viewer's
WebGL drawing of the mesh from any number of viewpoints (render_mesh; cameras in orbit_camera.py, DPTModel.render_views makes the whole call), and
the enlargement of a map to its photo's size with the photo as the guide (guided_upsample_images; DPTModel.inference_guided makes the whole call), and - not in the reference - the filling of the holes a moved camera
uncovers in rendered views (fill_holes; render_mesh and DPTModel.render_views take it as an option).

Every function takes the CUDA tensor the model returned and launches HIP kernels (libmdpt: mdpt_post_*) on the current torch
stream; results stay on the device (the reference's convert_to_uint8 does the same, postprocess.py:85-87). min / max never visit
the host. There is no CPU implementation here: host arrays raise (numpy callers should keep using numpy).
"""

from __future__ import annotations

import functools

import numpy as np
import torch
from torch import Tensor

from . import native


def _need_cuda(tensors, what: str, expected: str = "expected a CUDA tensor") -> None:
    """There is no CPU implementation: anything among `tensors` that is not a CUDA tensor raises."""
    if not all(isinstance(t, torch.Tensor) and t.device.type == "cuda" for t in tensors):
        raise RuntimeError(f"{what}: {expected} (muggled_dpt_amd post-processing runs on the MI355X only, no CPU fallback)")


def _dev_f32(t, what: str) -> Tensor:
    _need_cuda([t], what)
    return t.detach().to(torch.float32).contiguous()


def _launch(dev, fn, *args):
    lib = native.load()
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        native.check(lib, getattr(lib, fn)(*args, stream))


def scale_prediction(prediction_tensor: Tensor, target_wh: tuple[int, int], interpolation: str = "bilinear") -> Tensor:
    """BxHxW -> Bx(target_h)x(target_w), F.interpolate(mode="bilinear", align_corners=False) (postprocess.py:22-29)."""
    if interpolation != "bilinear":
        raise NotImplementedError(f"interpolation '{interpolation}' is not built on the MI355X path (bilinear only)")
    x = _dev_f32(prediction_tensor, "scale_prediction")
    if x.dim() != 3:
        raise RuntimeError(f"scale_prediction expects BxHxW, got {tuple(x.shape)}")
    b, h, w = x.shape
    oh, ow = int(target_wh[1]), int(target_wh[0])
    out = torch.empty((b, oh, ow), device=x.device, dtype=torch.float32)
    _launch(x.device, "mdpt_post_scale_prediction", x.data_ptr(), b, h, w, out.data_ptr(), oh, ow, None, None)
    return out.to(prediction_tensor.dtype)


def _minmax(x: Tensor) -> Tensor:
    mm = torch.empty(2, device=x.device, dtype=torch.float32)
    scratch = torch.empty(2, device=x.device, dtype=torch.int32)
    _launch(x.device, "mdpt_post_minmax", x.data_ptr(), x.numel(), mm.data_ptr(), scratch.data_ptr())
    return mm


def normalize_01(data: Tensor) -> Tensor:
    """(data - min) / (max - min) (postprocess.py:63-74); result in the input dtype."""
    x = _dev_f32(data, "normalize_01")
    out = torch.empty_like(x)
    mm = _minmax(x)
    _launch(x.device, "mdpt_post_normalize", x.data_ptr(), x.numel(), mm.data_ptr(), out.data_ptr(), native.POST_F32, 0)
    return out.to(data.dtype)


def convert_to_uint8(depth_prediction_tensor: Tensor) -> Tensor:
    """(255 * normalize_01(x)).byte(), still on the device (postprocess.py:79-91)."""
    x = _dev_f32(depth_prediction_tensor, "convert_to_uint8")
    out = torch.empty(x.shape, device=x.device, dtype=torch.uint8)
    mm = _minmax(x)
    _launch(x.device, "mdpt_post_normalize", x.data_ptr(), x.numel(), mm.data_ptr(), out.data_ptr(), native.POST_U8, 0)
    return out


def scale_and_convert_to_uint8(prediction_tensor: Tensor, target_wh: tuple[int, int]) -> Tensor:
    """convert_to_uint8(scale_prediction(x, target_wh)) as the video loop does (run_video.py:348-349): the resize pass also
    reduces min / max, so the display-size fp32 map is written once and read once."""
    x = _dev_f32(prediction_tensor, "scale_and_convert_to_uint8")
    b, h, w = x.shape
    oh, ow = int(target_wh[1]), int(target_wh[0])
    scaled = torch.empty((b, oh, ow), device=x.device, dtype=torch.float32)
    mm = torch.empty(2, device=x.device, dtype=torch.float32)
    scratch = torch.empty(2, device=x.device, dtype=torch.int32)
    _launch(x.device, "mdpt_post_scale_prediction", x.data_ptr(), b, h, w, scaled.data_ptr(), oh, ow, mm.data_ptr(), scratch.data_ptr())
    out = torch.empty((b, oh, ow), device=x.device, dtype=torch.uint8)
    _launch(x.device, "mdpt_post_normalize", scaled.data_ptr(), scaled.numel(), mm.data_ptr(), out.data_ptr(), native.POST_U8, 0)
    return out


def pack_depth_u24(depth_prediction: Tensor, is_metric: bool = False, lossy: bool = False) -> Tensor:
    """[1,H,W] (or [H,W]) depth -> uint8 [H,W,4] BGRA carrying round(16777215 * normalize_01(depth)) in B (low), G, R (high);
    alpha is zero for the caller's mask (run_3dviewer.py:576-593). is_metric skips the normalisation, lossy keeps the top byte."""
    x = _dev_f32(depth_prediction, "pack_depth_u24").squeeze()
    if x.dim() != 2:
        raise RuntimeError(f"pack_depth_u24 expects one depth map, got {tuple(depth_prediction.shape)}")
    out = torch.empty((x.shape[0], x.shape[1], 4), device=x.device, dtype=torch.uint8)
    mm = None if is_metric else _minmax(x)
    _launch(x.device, "mdpt_post_normalize", x.data_ptr(), x.numel(), None if mm is None else mm.data_ptr(), out.data_ptr(),
            native.POST_U24, int(bool(lossy)))
    return out


def remove_inf_tensor(data: Tensor, inf_replacement_value: float = 0.0, in_place: bool = True) -> Tensor:
    """postprocess.py:34-40 (plain torch indexing on whatever device the tensor lives on; not a kernel of ours)."""
    data = data if in_place else data.clone()
    data[data.isinf()] = inf_replacement_value
    return data


# ---- per-image display tail


def _dev_u8(t, what: str) -> Tensor:
    _need_cuda([t], what)
    if t.dtype != torch.uint8 or t.dim() not in (2, 3) or t.numel() == 0:
        raise TypeError(f"{what}: expected a uint8 HxW or BxHxW tensor, got {t.dtype} {tuple(t.shape)}")
    return t.detach().contiguous()


def equalization_range(min_pct: float = 0.0, max_pct: float = 1.0) -> tuple[int, int]:
    """The reference's (min_value, max_value) of histogram_equalization (postprocess.py:124-126); (0, 255) is the cv2.equalizeHist branch."""
    min_value, max_value = [int(round(255 * value)) for value in sorted((min_pct, max_pct))]
    max_value = max(max_value, min_value + 1)
    if min_value < 0 or max_value > 255:  # (the reference's np.zeros / np.full fail on these)
        raise ValueError(f"histogram_equalization range {min_pct}, {max_pct} gives values [{min_value}, {max_value}] outside 0..255")
    return min_value, max_value


@functools.lru_cache(maxsize=64)
def threshold_bin_table(min_value: int, max_value: int) -> np.ndarray:
    """value -> bin of np.histogram(x, 1 + max_value - min_value, range=(min_value, max_value)) for the 256 uint8 values (-1: not counted).
    The bins are not unit wide, so the table is taken from numpy itself, one value at a time, and handed to the LUT kernel."""
    nbins = 1 + max_value - min_value
    table = np.full(256, -1, dtype=np.int32)
    for v in range(256):
        counts, _ = np.histogram(np.array([v], dtype=np.uint8), nbins, range=(min_value, max_value))
        hit = np.flatnonzero(counts)
        if hit.size:
            table[v] = hit[0]
    table.setflags(write=False)
    return table


def _equalize_lut(x3: Tensor, min_pct: float, max_pct: float) -> Tensor:
    """[B,256] equalization LUTs of a uint8 [B,H,W] batch, one per image."""
    vmin, vmax = equalization_range(min_pct, max_pct)
    b = x3.shape[0]
    hist = torch.zeros((b, 256), device=x3.device, dtype=torch.int32)
    _launch(x3.device, "mdpt_post_histogram", x3.data_ptr(), b, x3[0].numel(), hist.data_ptr())
    table = None
    if (vmin, vmax) != (0, 255):
        table = torch.from_numpy(threshold_bin_table(vmin, vmax).copy()).to(x3.device)
    lut = torch.empty((b, 256), device=x3.device, dtype=torch.uint8)
    _launch(x3.device, "mdpt_post_equalize_lut", hist.data_ptr(), b, None if table is None else table.data_ptr(), vmin, vmax, lut.data_ptr())
    return lut


def histogram_equalization(depth_uint8: Tensor, min_pct: float = 0.0, max_pct: float = 1.0) -> Tensor:
    """uint8 [H,W] or [B,H,W] on the device -> same shape, every image equalized on its own (postprocess.py:107-145): cv2.equalizeHist for the
    full range, the np.histogram branch otherwise. One histogram pass, one LUT launch, one apply pass; nothing visits the host."""
    x = _dev_u8(depth_uint8, "histogram_equalization")
    x3 = x if x.dim() == 3 else x[None]
    lut = _equalize_lut(x3, min_pct, max_pct)
    out = torch.empty_like(x3)
    _launch(x.device, "mdpt_post_colorize", x3.data_ptr(), x3.shape[0], x3[0].numel(), lut.data_ptr(), None, 1, out.data_ptr())
    return out.view(x.shape)


def _cmap_tensor(lut, device) -> Tensor | None:
    if lut is None:
        return None
    if isinstance(lut, np.ndarray):
        if lut.dtype != np.uint8 or lut.size != 256 * 3:
            raise TypeError(f"colormap LUT must be a uint8 1x256x3 array, got {lut.dtype} {lut.shape}")
        return torch.from_numpy(np.ascontiguousarray(lut).reshape(256, 3)).to(device)
    if isinstance(lut, torch.Tensor):
        if lut.dtype != torch.uint8 or lut.numel() != 256 * 3:
            raise TypeError(f"colormap LUT must be a uint8 1x256x3 tensor, got {lut.dtype} {tuple(lut.shape)}")
        return lut.detach().to(device).contiguous().reshape(256, 3)
    raise TypeError(f"Error applying colormap, unrecognized colormap type: {type(lut)}")


def apply_colormap(depth_uint8: Tensor, lut=None) -> Tensor:
    """uint8 [H,W] or [B,H,W] -> uint8 [...,H,W,3] BGR through a 1x256x3 BGR LUT (ndarray or tensor), or gray when lut is None:
    cv2.LUT(cv2.cvtColor(x, GRAY2BGR), lut) (toadui/colormaps.py:237-259)."""
    x = _dev_u8(depth_uint8, "apply_colormap")
    cmap = _cmap_tensor(lut, x.device)
    x3 = x if x.dim() == 3 else x[None]
    out = torch.empty((*x.shape, 3), device=x.device, dtype=torch.uint8)
    _launch(x.device, "mdpt_post_colorize", x3.data_ptr(), x3.shape[0], x3[0].numel(), None, None if cmap is None else cmap.data_ptr(), 3, out.data_ptr())
    return out


def depth_to_color(prediction: Tensor, target_wh: tuple[int, int] | None = None, reverse: bool = False, high_contrast: bool = False,
                   lut=None) -> Tensor:
    """[B,h,w] depth prediction -> uint8 [B,H,W,3] BGR display frames, the per-frame loop of run_video.py:348-361 for every image at once:
    scale_prediction (target_wh given) -> convert_to_uint8 -> 255 - x (reverse) -> histogram_equalization (high_contrast) -> colormap (lut; gray
    when None). Image b's frame equals that composition on prediction[b:b+1] bit for bit (its own min / max and histogram). Four launches at
    most: resize + per-image min/max (also clears the histogram), uint8 + histogram, LUT, equalize-and-colormap as one lookup."""
    x = _batch_maps(prediction, "depth_to_color")
    dev = x.device
    cmap = _cmap_tensor(lut, dev)
    b, h, w = x.shape
    dt = native.dtype_code(x.dtype)
    scaled = None
    oh, ow = h, w
    if target_wh is not None:
        oh, ow = int(target_wh[1]), int(target_wh[0])
        scaled = torch.empty((b, oh, ow), device=dev, dtype=torch.float32)
    parts = torch.empty((b, native.POST_SEG_PARTS, 2), device=dev, dtype=torch.int32)
    hist = torch.empty((b, 256), device=dev, dtype=torch.int32) if high_contrast else None
    hist_ptr = None if hist is None else hist.data_ptr()
    _launch(dev, "mdpt_post_minmax_seg", x.data_ptr(), dt, b, h, w, None if scaled is None else scaled.data_ptr(), oh, ow, parts.data_ptr(), hist_ptr)
    n = oh * ow
    u8 = torch.empty((b, oh, ow), device=dev, dtype=torch.uint8)
    src, src_dt = (x, dt) if scaled is None else (scaled, native.DTYPE_F32)
    _launch(dev, "mdpt_post_u8_hist_seg", src.data_ptr(), src_dt, b, n, parts.data_ptr(), int(bool(reverse)), u8.data_ptr(), hist_ptr)
    eq = None
    if high_contrast:
        eq = torch.empty((b, 256), device=dev, dtype=torch.uint8)
        _launch(dev, "mdpt_post_equalize_lut", hist.data_ptr(), b, None, 0, 255, eq.data_ptr())
    out = torch.empty((b, oh, ow, 3), device=dev, dtype=torch.uint8)
    _launch(dev, "mdpt_post_colorize", u8.data_ptr(), b, n, None if eq is None else eq.data_ptr(), None if cmap is None else cmap.data_ptr(), 3, out.data_ptr())
    return out


# ---- the same for images of different sizes


def _prediction_list(predictions, what: str) -> list[Tensor]:
    """[1,h,w] / [h,w] tensors (sizes may differ) or a [B,h,w] tensor -> list of contiguous [h,w] maps of one device and one float dtype."""
    if isinstance(predictions, torch.Tensor):
        if predictions.dim() != 3:
            raise RuntimeError(f"{what} expects a list of [1,h,w] / [h,w] maps or a BxHxW tensor, got {tuple(predictions.shape)}")
        maps = list(predictions.detach().unbind(0))
    elif isinstance(predictions, (list, tuple)):
        maps = []
        for p in predictions:
            if not isinstance(p, torch.Tensor):
                raise TypeError(f"{what} expects depth tensors, got {type(p)}")
            p = p.detach()
            if p.dim() == 3 and p.shape[0] == 1:
                p = p[0]
            if p.dim() != 2:
                raise RuntimeError(f"{what} expects [1,h,w] or [h,w] maps, got {tuple(p.shape)}")
            maps.append(p)
    else:
        raise TypeError(f"{what} expects a list of depth tensors or a BxHxW tensor, got {type(predictions)}")
    if not maps:
        raise ValueError(f"{what} got no predictions")
    _need_cuda(maps, what, "expected CUDA tensors")
    if len({m.device for m in maps}) != 1 or len({m.dtype for m in maps}) != 1:
        raise RuntimeError(f"{what}: all predictions must share one device and one dtype")
    if any(m.numel() == 0 for m in maps):
        raise RuntimeError(f"{what}: empty prediction")
    if maps[0].dtype not in (torch.float32, torch.bfloat16, torch.float16):
        maps = [m.to(torch.float32) for m in maps]
    return [m.contiguous() for m in maps]


def _target_hw(target_whs, n: int, what: str) -> list[tuple[int, int]]:
    whs = list(target_whs)
    if len(whs) != n:
        raise ValueError(f"{what}: {n} predictions but {len(whs)} target sizes")
    hw = [(int(wh[1]), int(wh[0])) for wh in whs]
    if any(h <= 0 or w <= 0 for h, w in hw):
        raise ValueError(f"{what}: target sizes must be positive, got {whs}")
    return hw


def _ptrs_hw(ptrs, hws):
    """host arrays of the *_images entry points (they are read during the call only; the caller keeps these alive until then)"""
    return np.asarray(ptrs, dtype=np.uint64), np.asarray(hws, dtype=np.int32).reshape(-1)


def _minmax_images(maps: list[Tensor], out_hw, hist: Tensor | None):
    """mdpt_post_minmax_images: per-image min/max partials, and (out_hw given) every map resized into one packed fp32 buffer -> (parts, scaled)"""
    dev = maps[0].device
    b = len(maps)
    ptrs, in_hw = _ptrs_hw([m.data_ptr() for m in maps], [m.shape for m in maps])
    scaled = None
    o_hw = None
    if out_hw is not None:
        o_hw = np.asarray(out_hw, dtype=np.int32).reshape(-1)
        scaled = torch.empty(int(sum(h * w for h, w in out_hw)), device=dev, dtype=torch.float32)
    parts = torch.empty((b, native.POST_SEG_PARTS, 2), device=dev, dtype=torch.int32)
    _launch(dev, "mdpt_post_minmax_images", ptrs.ctypes.data, in_hw.ctypes.data, native.dtype_code(maps[0].dtype), b,
            None if scaled is None else scaled.data_ptr(), None if o_hw is None else o_hw.ctypes.data, parts.data_ptr(),
            None if hist is None else hist.data_ptr())
    return parts, scaled


def _views(flat: Tensor, hws, tail=()) -> list[Tensor]:
    out, at = [], 0
    for h, w in hws:
        n = h * w * int(np.prod(tail, dtype=np.int64))
        out.append(flat[at:at + n].view(1, h, w, *tail))
        at += n
    return out


def scale_prediction_images(predictions, target_whs) -> list[Tensor]:
    """scale_prediction for images of different sizes: predictions (a list of [1,h,w] / [h,w] maps whose sizes may differ, as
    DPTModel.inference_images returns, or a [B,h,w] tensor) and one (w, h) per image -> a list of [1,H_i,W_i] maps in the predictions' dtype.
    Element i equals scale_prediction(prediction i, target_whs[i]) bit for bit. One launch per 32 images; the outputs are views into one
    allocation."""
    maps = _prediction_list(predictions, "scale_prediction_images")
    hws = _target_hw(target_whs, len(maps), "scale_prediction_images")
    _, scaled = _minmax_images(maps, hws, None)  # (the resize kernel rounds to the input dtype, so the cast below is exact)
    out_dtype = predictions.dtype if isinstance(predictions, torch.Tensor) else predictions[0].dtype
    return _views(scaled.to(out_dtype), hws)


def depth_to_color_images(predictions, target_whs=None, reverse: bool = False, high_contrast: bool = False, lut=None) -> list[Tensor]:
    """depth_to_color for images of different sizes: predictions as for scale_prediction_images, target_whs one (w, h) per image (None: each
    map's own size) -> a list of uint8 [1,H_i,W_i,3] BGR frames, element i equal to depth_to_color(prediction i, target_whs[i], reverse,
    high_contrast, lut) bit for bit (its own min/max and histogram). At most four launches per 32 images: resize + min/max (also clears the
    histograms), uint8 + histogram, LUT, equalize-and-colormap. The outputs are views into one allocation."""
    maps = _prediction_list(predictions, "depth_to_color_images")
    dev = maps[0].device
    cmap = _cmap_tensor(lut, dev)
    b = len(maps)
    in_hw = [tuple(m.shape) for m in maps]
    out_hw = None if target_whs is None else _target_hw(target_whs, b, "depth_to_color_images")
    hws = in_hw if out_hw is None else out_hw
    hist = torch.empty((b, 256), device=dev, dtype=torch.int32) if high_contrast else None
    hist_ptr = None if hist is None else hist.data_ptr()
    parts, scaled = _minmax_images(maps, out_hw, hist)
    if scaled is None:
        src_ptrs, src_dt = [m.data_ptr() for m in maps], native.dtype_code(maps[0].dtype)
    else:
        offs = np.cumsum([0] + [h * w for h, w in hws[:-1]])
        src_ptrs, src_dt = [scaled.data_ptr() + 4 * int(o) for o in offs], native.DTYPE_F32
    ptrs, hw_arr = _ptrs_hw(src_ptrs, hws)
    u8 = torch.empty(int(sum(h * w for h, w in hws)), device=dev, dtype=torch.uint8)
    _launch(dev, "mdpt_post_u8_hist_images", ptrs.ctypes.data, hw_arr.ctypes.data, src_dt, b, parts.data_ptr(), int(bool(reverse)), u8.data_ptr(), hist_ptr)
    eq = None
    if high_contrast:
        eq = torch.empty((b, 256), device=dev, dtype=torch.uint8)
        _launch(dev, "mdpt_post_equalize_lut", hist.data_ptr(), b, None, 0, 255, eq.data_ptr())
    out = torch.empty(u8.numel() * 3, device=dev, dtype=torch.uint8)
    _launch(dev, "mdpt_post_colorize_images", u8.data_ptr(), hw_arr.ctypes.data, b, None if eq is None else eq.data_ptr(),
            None if cmap is None else cmap.data_ptr(), 3, out.data_ptr())
    return _views(out, hws, (3,))


# ---- the still-image demo's display tail (run_image.py) and the 3D viewer's edge alpha (run_3dviewer.py)


def plane_sample_points(hw, samples_per_side: int = 16, jitter_scale: float = 0.75, rng=np.random) -> np.ndarray:
    """int32 [N,2] (x, y) pixel samples of an [h,w] map for the plane of best fit, drawn as the reference's plane_fit.get_xyz_samples draws
    them: a min(n, side) grid of cell centres, jittered by clip(randn, -1, 1) * half a cell * jitter_scale (x first, then y, two randn calls),
    scaled by (w-1, h-1) and rounded. With np.random.seed(s) beforehand these are the reference's own points. rng: anything with randn
    (np.random, a RandomState) or standard_normal (a Generator)."""
    h, w = int(hw[0]), int(hw[1])
    n = int(samples_per_side)
    if h <= 0 or w <= 0 or n <= 0:
        raise ValueError(f"plane_sample_points: bad map size {tuple(hw)} or samples_per_side {samples_per_side}")
    randn = getattr(rng, "randn", None) or (lambda *shape: rng.standard_normal(shape))
    x_step, y_step = 1.0 / n, 1.0 / n
    jitter_scale = np.clip(jitter_scale, 0.0, 1.0)
    xs = x_step * (0.5 + np.arange(min(n, w), dtype=np.float32))
    ys = y_step * (0.5 + np.arange(min(n, h), dtype=np.float32))
    xgrid, ygrid = np.meshgrid(xs, ys)
    xgrid += np.clip(randn(*xgrid.shape), -1, 1) * (x_step / 2.0) * jitter_scale
    ygrid += np.clip(randn(*ygrid.shape), -1, 1) * (y_step / 2.0) * jitter_scale
    xy_norm = np.dstack((xgrid, ygrid)).reshape(-1, 2)
    return np.int32(np.round(xy_norm * np.float32((w - 1, h - 1))))


def _sample_table(sample_xy, b: int, h: int, w: int, samples_per_side: int, jitter_scale: float, dev, what: str) -> tuple[Tensor, int, bool]:
    """the int32 (x, y) sample points on the device -> (points, N, one set per image). None: plane_sample_points per image, in batch order."""
    if sample_xy is None:
        pts = np.stack([plane_sample_points((h, w), samples_per_side, jitter_scale) for _ in range(b)])
        return torch.from_numpy(pts).to(dev), pts.shape[1], True
    if isinstance(sample_xy, torch.Tensor) and sample_xy.device.type == "cuda":
        pts = sample_xy.detach()
        if pts.dtype.is_floating_point or pts.dtype == torch.bool:
            raise TypeError(f"{what}: sample_xy must hold integer pixel positions, got {pts.dtype}")
        pts = pts.to(dev, torch.int32).contiguous()  # (device points are clamped into the map by the kernel; they are not read back)
    else:
        arr = sample_xy.numpy() if isinstance(sample_xy, torch.Tensor) else np.asarray(sample_xy)
        if arr.dtype.kind not in "iu":
            raise TypeError(f"{what}: sample_xy must hold integer pixel positions, got {arr.dtype}")
        if arr.size and (arr[..., 0].min() < 0 or arr[..., 0].max() >= w or arr[..., 1].min() < 0 or arr[..., 1].max() >= h):
            raise ValueError(f"{what}: sample_xy has points outside the {h}x{w} map")
        pts = torch.from_numpy(np.ascontiguousarray(arr, dtype=np.int32)).to(dev)
    if pts.dim() == 2 and pts.shape[1] == 2 and pts.shape[0] > 0:
        return pts, pts.shape[0], False
    if pts.dim() == 3 and pts.shape[0] == b and pts.shape[2] == 2 and pts.shape[1] > 0:
        return pts, pts.shape[1], True
    raise ValueError(f"{what}: sample_xy must be [N,2] or [{b},N,2], got {tuple(pts.shape)}")


def _batch_maps(prediction, what: str) -> Tensor:
    """a [B,h,w] (or [h,w]) CUDA depth tensor -> contiguous [B,h,w] in fp32 / bf16 / fp16"""
    _need_cuda([prediction], what)
    x = prediction.detach()
    if x.dim() == 2:
        x = x[None]
    if x.dim() != 3 or x.numel() == 0:
        raise RuntimeError(f"{what} expects BxHxW, got {tuple(prediction.shape)}")
    if x.dtype not in (torch.float32, torch.bfloat16, torch.float16):
        x = x.to(torch.float32)
    return x.contiguous()


def plane_of_best_fit(depth: Tensor, samples_per_side: int = 16, jitter_scale: float = 0.75, sample_xy=None) -> Tensor:
    """[H,W] or [B,H,W] depth on the device -> fp32 plane images of the same shape, the reference's plane_fit.estimate_plane_of_best_fit per
    image: z at the sample points (sample_xy: [N,2] or [B,N,2] ints, host or device; None: plane_sample_points per image in batch order), the
    known x / y means, the sample z mean, and the normal of the smallest singular value of the centred samples (the smallest eigenvector of their
    fp64 Gram matrix, by Jacobi; the sign does not matter). One workgroup per image fits, one launch evaluates. A constant map gives the constant
    plane (the reference divides by a zero normal there)."""
    x = _batch_maps(depth, "plane_of_best_fit").to(torch.float32)
    b, h, w = x.shape
    dev = x.device
    pts, n, per_image = _sample_table(sample_xy, b, h, w, samples_per_side, jitter_scale, dev, "plane_of_best_fit")
    coef = torch.empty((b, 4), device=dev, dtype=torch.float64)
    _launch(dev, "mdpt_post_plane_fit", x.data_ptr(), native.DTYPE_F32, b, h, w, None, pts.data_ptr(), n, int(per_image), coef.data_ptr())
    out = torch.empty((b, h, w), device=dev, dtype=torch.float32)
    _launch(dev, "mdpt_post_plane_eval", coef.data_ptr(), b, h, w, out.data_ptr())
    return out.view(depth.shape)


def _threshold(threshold) -> tuple[float, float]:
    tmin, tmax = (float(v) for v in threshold)
    if not (0.0 <= tmin <= tmax <= 1.0):
        raise ValueError(f"threshold must be (min, max) with 0 <= min <= max <= 1, got {tuple(threshold)}")
    return tmin, tmax


def _plane_removed(x: Tensor, target_wh, plane_removal: float, threshold, samples_per_side: int, sample_xy, hist: bool, what: str):
    """run_image.py's steps up to the threshold for every image: remove_inf(scale_prediction) + min/max, the plane fit on the normalized map,
    min/max of dn - f plane -> (prepared map, its parts, plane coef, vparts, hist or None, out h, out w)"""
    tmin, tmax = _threshold(threshold)
    dev = x.device
    b, h, w = x.shape
    oh, ow = (h, w) if target_wh is None else (int(target_wh[1]), int(target_wh[0]))
    if oh <= 0 or ow <= 0:
        raise ValueError(f"{what}: bad target size {target_wh}")
    dt = native.dtype_code(x.dtype)
    pts, n, per_image = _sample_table(sample_xy, b, oh, ow, samples_per_side, 0.75, dev, what)
    prepared = torch.empty((b, oh, ow), device=dev, dtype=x.dtype)
    parts = torch.empty((b, native.POST_SEG_PARTS, 2), device=dev, dtype=torch.int32)
    hist_t = torch.empty((b, 256), device=dev, dtype=torch.int32) if hist else None
    _launch(dev, "mdpt_post_display_prep", x.data_ptr(), dt, b, h, w, prepared.data_ptr(), oh, ow, parts.data_ptr(),
            None if hist_t is None else hist_t.data_ptr())
    coef = torch.empty((b, 4), device=dev, dtype=torch.float64)
    _launch(dev, "mdpt_post_plane_fit", prepared.data_ptr(), dt, b, oh, ow, parts.data_ptr(), pts.data_ptr(), n, int(per_image), coef.data_ptr())
    vparts = torch.empty((b, native.POST_SEG_PARTS, 2), device=dev, dtype=torch.float64)
    f = float(plane_removal)
    _launch(dev, "mdpt_post_plane_minmax", prepared.data_ptr(), dt, b, oh, ow, parts.data_ptr(), coef.data_ptr(), f, vparts.data_ptr())
    return dict(x=prepared, dt=dt, parts=parts, coef=coef, f=f, vparts=vparts, tmin=tmin, tmax=tmax, hist=hist_t, hw=(oh, ow))


def depth_to_display(prediction: Tensor, target_wh: tuple[int, int] | None = None, plane_removal: float = 0.0, threshold=(0.0, 1.0),
                     reverse: bool = False, high_contrast: bool = False, lut=None, samples_per_side: int = 16, sample_xy=None) -> Tensor:
    """[B,h,w] depth prediction -> uint8 [B,H,W,3] BGR, the still-image demo's display loop (run_image.py:185-195, 323-343) for every image:
    scale_prediction (target_wh given) -> remove_inf -> normalize_01 -> plane of best fit of that -> dn - plane_removal * plane -> normalize_01 ->
    clip((v - min) / max(0.001, max - min), 0, 1) -> round(255 t) -> histogram_equalization(u8, min, max) (high_contrast) -> 255 - x (reverse)
    -> colormap (lut; gray when None). Steps after the plane are fp64 as in the reference's numpy. The equalization comes BEFORE the reverse
    here, as in run_image.py (depth_to_color follows run_video.py, which reverses first). sample_xy as for plane_of_best_fit, at the display
    size; row b equals the call on prediction[b:b+1] with image b's points bit for bit. Five launches, six with high_contrast; nothing is read back."""
    _threshold(threshold)
    x = _batch_maps(prediction, "depth_to_display")
    dev = x.device
    cmap = _cmap_tensor(lut, dev)
    if reverse:  # cmap[255 - e] as one table: the reverse after the equalization costs no pass
        cmap = (torch.arange(256, device=dev, dtype=torch.uint8)[:, None].expand(256, 3) if cmap is None else cmap).flip(0).contiguous()
    s = _plane_removed(x, target_wh, plane_removal, threshold, samples_per_side, sample_xy, high_contrast, "depth_to_display")
    b = x.shape[0]
    oh, ow = s["hw"]
    hist = s["hist"]
    u8 = torch.empty((b, oh, ow), device=dev, dtype=torch.uint8)
    _launch(dev, "mdpt_post_threshold", s["x"].data_ptr(), s["dt"], b, oh, ow, s["parts"].data_ptr(), s["coef"].data_ptr(), s["f"], s["vparts"].data_ptr(),
            s["tmin"], s["tmax"], native.POST_U8, 0, u8.data_ptr(), None if hist is None else hist.data_ptr())
    eq = None
    if high_contrast:
        vmin, vmax = equalization_range(s["tmin"], s["tmax"])
        table = None if (vmin, vmax) == (0, 255) else torch.from_numpy(threshold_bin_table(vmin, vmax).copy()).to(dev)
        eq = torch.empty((b, 256), device=dev, dtype=torch.uint8)
        _launch(dev, "mdpt_post_equalize_lut", hist.data_ptr(), b, None if table is None else table.data_ptr(), vmin, vmax, eq.data_ptr())
    out = torch.empty((b, oh, ow, 3), device=dev, dtype=torch.uint8)
    _launch(dev, "mdpt_post_colorize", u8.data_ptr(), b, oh * ow, None if eq is None else eq.data_ptr(), None if cmap is None else cmap.data_ptr(), 3,
            out.data_ptr())
    return out


def depth_for_saving(prediction: Tensor, plane_removal: float = 0.0, threshold=(0.0, 1.0), reverse: bool = False, samples_per_side: int = 16,
                     sample_xy=None) -> Tensor:
    """[B,h,w] depth prediction -> fp32 [B,h,w], the still-image demo's .npy save path (run_image.py:350-358) at model resolution for every image:
    remove_inf -> normalize_01 -> minus plane_removal * its plane of best fit -> normalize_01 -> clip((v - min) / max(0.001, max - min), 0, 1)
    -> 1 - t (reverse), in fp64, rounded to fp32 once. sample_xy as for plane_of_best_fit. Four launches."""
    _threshold(threshold)
    x = _batch_maps(prediction, "depth_for_saving")
    s = _plane_removed(x, None, plane_removal, threshold, samples_per_side, sample_xy, False, "depth_for_saving")
    b, h, w = x.shape
    out = torch.empty((b, h, w), device=x.device, dtype=torch.float32)
    _launch(x.device, "mdpt_post_threshold", s["x"].data_ptr(), s["dt"], b, h, w, s["parts"].data_ptr(), s["coef"].data_ptr(), s["f"],
            s["vparts"].data_ptr(), s["tmin"], s["tmax"], native.POST_F32, int(bool(reverse)), out.data_ptr(), None)
    return out


@functools.lru_cache(maxsize=16)
def _blur_weights(blur_kernel_size: int, blur_weight: float) -> np.ndarray:
    """the viewer's Gaussian (run_3dviewer.py:490-505): exp(-(i^2 + j^2) 0.01 / blur_weight) over i, j in -pad..pad, over its max, in fp32"""
    ks_pad = blur_kernel_size // 2
    ksize = 1 + 2 * ks_pad
    idx_1d = torch.linspace(-ks_pad, ks_pad, ksize, dtype=torch.float32)
    xy_idx = torch.stack(torch.meshgrid(idx_1d, idx_1d, indexing="ij"))
    gauss = torch.exp(-torch.sum(torch.square(xy_idx) * (0.01 / blur_weight), dim=0))
    out = np.ascontiguousarray((gauss / gauss.max()).numpy(), dtype=np.float32)
    out.setflags(write=False)
    return out


def _edge_args(h: int, w: int, blur_kernel_size, blur_weight, what: str) -> tuple[np.ndarray, int]:
    k, bw = int(blur_kernel_size), float(blur_weight)
    if k < 0 or 1 + 2 * (k // 2) > 15:
        raise ValueError(f"{what}: blur_kernel_size must be 0..15 (an odd kernel of at most 15), got {blur_kernel_size}")
    if not bw > 0.0:
        raise ValueError(f"{what}: blur_weight must be positive, got {blur_weight}")
    ksize = 1 + 2 * (k // 2)
    need = max(2, k // 2 + 1)
    if h < need or w < need:
        raise RuntimeError(f"{what}: a {h}x{w} map is too small for the reflect padding of a {ksize}x{ksize} blur and the 3x3 Sobel (sides of at least {need})")
    return _blur_weights(k, bw), ksize


def _edge_mag(x: Tensor, parts: Tensor | None, blur_kernel_size, blur_weight, what: str) -> tuple[Tensor, Tensor]:
    b, h, w = x.shape
    weights, ksize = _edge_args(h, w, blur_kernel_size, blur_weight, what)
    mag = torch.empty((b, h, w), device=x.device, dtype=torch.float32)
    mag_max = torch.empty(b, device=x.device, dtype=torch.int32)
    _launch(x.device, "mdpt_post_edge_mag", x.data_ptr(), b, h, w, None if parts is None else parts.data_ptr(), weights.ctypes.data, ksize,
            mag.data_ptr(), mag_max.data_ptr())
    return mag, mag_max


def depth_edge_mask(depth: Tensor, blur_kernel_size: int = 5, blur_weight: float = 1.0) -> Tensor:
    """[H,W] or [B,H,W] depth on the device -> uint8 of the same shape, the 3D viewer's default alpha (run_3dviewer.py:455-505) per image: a
    Gaussian blur (exp(-(i^2 + j^2) 0.01 / blur_weight) over its max, size 1 + 2 (k // 2)) and the 3x3 Sobel [[3,10,3],[0,0,0],[-3,-10,-3]]
    (and its transpose), both cross-correlations with reflect padding, mag = sqrt(dx^2 + dy^2), ~round(255 mag / max(mag)). A flat map (max 0)
    gives 255 everywhere (the reference's 0 / 0 there is NaN, whose conversion to uint8 is undefined); so does a map holding a NaN. Sides must
    exceed the reflect pads (at least max(2, k // 2 + 1)), as torch requires. Two launches."""
    if isinstance(depth, torch.Tensor) and depth.dim() in (2, 3):  # (sizes and filter arguments are checked before the device)
        _edge_args(depth.shape[-2], depth.shape[-1], blur_kernel_size, blur_weight, "depth_edge_mask")
    x = _batch_maps(depth, "depth_edge_mask").to(torch.float32)
    mag, mag_max = _edge_mag(x, None, blur_kernel_size, blur_weight, "depth_edge_mask")
    b, h, w = x.shape
    out = torch.empty((b, h, w), device=x.device, dtype=torch.uint8)
    _launch(x.device, "mdpt_post_edge_mask", mag.data_ptr(), mag_max.data_ptr(), b, h * w, out.data_ptr())
    return out.view(depth.shape)


def pack_depth_u24_frames(predictions: Tensor, is_metric: bool = False, lossy: bool = False, alpha="edges", blur_kernel_size: int = 5,
                          blur_weight: float = 1.0) -> Tensor:
    """[B,H,W] depth predictions -> uint8 [B,H,W,4] BGRA, the 3D viewer's 24-bit frames (run_3dviewer.py:576-593) for every image: BGR equal to
    pack_depth_u24 of each image bit for bit, and alpha
      "edges": depth_edge_mask of the map as packed (normalize_01 of it for relative models; the viewer's default, no mask file),
      a uint8 [H,W] or [B,H,W] CUDA tensor: passed through (the viewer's --mask_path),
      None: 0.
    Packing and alpha are one pass: two launches without edges, four with."""
    if isinstance(alpha, str) and alpha != "edges":
        raise ValueError(f"pack_depth_u24_frames: alpha must be 'edges', a uint8 mask tensor or None, got {alpha!r}")
    if isinstance(alpha, str) and isinstance(predictions, torch.Tensor) and predictions.dim() in (2, 3):
        _edge_args(predictions.shape[-2], predictions.shape[-1], blur_kernel_size, blur_weight, "pack_depth_u24_frames")
    x = _batch_maps(predictions, "pack_depth_u24_frames").to(torch.float32)
    b, h, w = x.shape
    dev = x.device
    mask = None
    if alpha is not None and not isinstance(alpha, str):
        if not isinstance(alpha, torch.Tensor) or alpha.device.type != "cuda" or alpha.dtype != torch.uint8:
            raise TypeError("pack_depth_u24_frames: a mask alpha must be a uint8 CUDA tensor")
        if tuple(alpha.shape) not in ((h, w), (b, h, w)):
            raise ValueError(f"pack_depth_u24_frames: mask of shape {tuple(alpha.shape)} for {b} maps of {h}x{w}")
        mask = alpha.detach().contiguous()
    parts = None
    if not is_metric:
        parts = torch.empty((b, native.POST_SEG_PARTS, 2), device=dev, dtype=torch.int32)
        _launch(dev, "mdpt_post_minmax_seg", x.data_ptr(), native.DTYPE_F32, b, h, w, None, h, w, parts.data_ptr(), None)
    mag = mag_max = None
    if isinstance(alpha, str):
        mag, mag_max = _edge_mag(x, parts, blur_kernel_size, blur_weight, "pack_depth_u24_frames")
    out = torch.empty((b, h, w, 4), device=dev, dtype=torch.uint8)
    _launch(dev, "mdpt_post_pack_u24_alpha", x.data_ptr(), b, h * w, None if parts is None else parts.data_ptr(), int(bool(lossy)),
            None if mag is None else mag.data_ptr(), None if mag_max is None else mag_max.data_ptr(), None if mask is None else mask.data_ptr(),
            int(mask is not None and mask.dim() == 3), out.data_ptr())
    return out


# ---- depth masking: the reference's experiments/depth_masking.py (background removal by depth)


def _display_photos(images_bgr, b: int, what: str) -> Tensor:
    """uint8 [B,ih,iw,3] (or [ih,iw,3] for one map) CUDA photos of the display batch"""
    _need_cuda([images_bgr], what, "images_bgr must be a uint8 CUDA tensor")
    x = images_bgr.detach()
    if x.dim() == 3:
        x = x[None]
    if x.dtype != torch.uint8 or x.dim() != 4 or x.shape[3] != 3 or x.shape[1] == 0 or x.shape[2] == 0:
        raise TypeError(f"{what}: images_bgr must be uint8 [B,H,W,3] or [H,W,3] BGR, got {x.dtype} {tuple(images_bgr.shape)}")
    if x.shape[0] != b:
        raise ValueError(f"{what}: {b} predictions but {x.shape[0]} images")
    return x.contiguous()


def depth_mask_display(prediction: Tensor, images_bgr: Tensor, target_wh: tuple[int, int] | None, plane_removal: float = 0.0, threshold=(0.0, 1.0),
                       invert: bool = False, samples_per_side: int = 16, sample_xy=None) -> tuple[Tensor, Tensor]:
    """[B,h,w] depth prediction and uint8 [B,ih,iw,3] BGR photos (or [ih,iw,3] for B = 1) on the device -> (mask uint8 [B,H,W], composite uint8
    [B,H,W,3]) at the display size target_wh = (W, H) (None: the map's size), the display loop of the reference's depth masking demo
    (experiments/depth_masking.py:189-199, 314-332) for every image: n = normalize_01(d - plane_removal * plane) in fp64, d = normalize_01(
    remove_inf(scale_prediction(x))) as depth_to_display prepares it (its plane fit, sample_xy as there, at the display size); mask = 255 where
    threshold[0] <= n <= threshold[1], else 0 (NaN: 0); invert: 255 - mask. The composite is the photo resized to (W, H) where the mask is 255 and
    the reference's CheckerPattern() (169 / 214, 32-px tiles, centred) where it is 0. The photo resize restates cv2.resize(INTER_LINEAR) on uint8
    by its scalar fixed-point formula (weights round(2048 w), (v + 2^21) >> 22); cv2's SIMD and IPP paths round differently, so a composite byte
    may differ from a given cv2 build's by 1. Mask and checker bytes do not depend on that. Four launches; nothing is read back."""
    _threshold(threshold)
    b = prediction.shape[0] if isinstance(prediction, torch.Tensor) and prediction.dim() == 3 else 1
    photos = _display_photos(images_bgr, b, "depth_mask_display")
    x = _batch_maps(prediction, "depth_mask_display")
    if photos.device != x.device:
        raise RuntimeError(f"depth_mask_display: the prediction is on {x.device} but the images are on {photos.device}")
    s = _plane_removed(x, target_wh, plane_removal, threshold, samples_per_side, sample_xy, False, "depth_mask_display")
    oh, ow = s["hw"]
    dev = x.device
    mask = torch.empty((b, oh, ow), device=dev, dtype=torch.uint8)
    comp = torch.empty((b, oh, ow, 3), device=dev, dtype=torch.uint8)
    _launch(dev, "mdpt_post_mask_display", s["x"].data_ptr(), s["dt"], b, oh, ow, s["parts"].data_ptr(), s["coef"].data_ptr(), s["f"], s["vparts"].data_ptr(),
            s["tmin"], s["tmax"], int(bool(invert)), photos.data_ptr(), photos.shape[1], photos.shape[2], mask.data_ptr(), comp.data_ptr())
    return mask, comp


def _cutout_photos(images_bgr, n: int, what: str) -> tuple[list, bool]:
    """a list of uint8 HxWx3 BGR host arrays or CUDA tensors (not a mix), one per prediction -> (photos, on_device)"""
    if not isinstance(images_bgr, (list, tuple)):
        raise TypeError(f"{what} expects a list of uint8 HxWx3 BGR images (ndarrays or CUDA tensors), got {type(images_bgr)}")
    if len(images_bgr) != n:
        raise ValueError(f"{what}: {n} predictions but {len(images_bgr)} images")
    n_dev = sum(isinstance(f, torch.Tensor) for f in images_bgr)
    if 0 < n_dev < len(images_bgr):
        raise TypeError(f"{what} expects host arrays or device tensors, not a mix of both")
    on_device = n_dev > 0
    for f in images_bgr:
        if on_device:
            ok = f.dtype == torch.uint8 and f.dim() == 3 and f.shape[2] == 3 and f.device.type == "cuda"
        else:
            ok = isinstance(f, np.ndarray) and f.dtype == np.uint8 and f.ndim == 3 and f.shape[2] == 3
        if not ok:
            raise TypeError(f"{what} expects OpenCV-style uint8 HxWx3 BGR images (cv2.imread output), or uint8 HxWx3 CUDA tensors")
        if f.shape[0] == 0 or f.shape[1] == 0:
            raise ValueError(f"{what} got an empty image ({f.shape[0]}x{f.shape[1]})")
    if on_device and len({f.device for f in images_bgr}) != 1:
        raise RuntimeError(f"{what}: the image tensors are on different devices")
    return [f.detach().contiguous() if on_device else f for f in images_bgr], on_device


def _stage_photos(photos: list[np.ndarray], dev) -> tuple[Tensor, list[int]]:
    """host photos -> one device buffer through pinned memory (numpy copies into a pinned buffer, one non-blocking copy on the current stream; the
    caching host allocator keeps the pinned block until that copy has run) -> (the buffer, the address of each photo in it, 16-byte aligned)"""
    offs, at = [], 0
    for f in photos:
        offs.append(at)
        at += (f.size + 15) // 16 * 16
    pinned = torch.empty(at, dtype=torch.uint8, pin_memory=True)
    host = pinned.numpy()
    for f, o in zip(photos, offs):
        host[o:o + f.size].reshape(f.shape)[...] = f  # (handles non-contiguous views: numpy does the strided copy)
    with torch.cuda.device(dev):
        staged = torch.empty(at, dtype=torch.uint8, device=dev)
        staged.copy_(pinned, non_blocking=True)
    return staged, [staged.data_ptr() + o for o in offs]


def _cutout_samples(sample_xy, maps: list[Tensor], what: str):
    """per-image [N,2] point sets -> list (None: drawn later, per image in list order)"""
    if sample_xy is None:
        return [None] * len(maps)
    sets = list(sample_xy.unbind(0)) if isinstance(sample_xy, torch.Tensor) else (list(sample_xy) if isinstance(sample_xy, (list, tuple)) else
                                                                                  list(np.asarray(sample_xy)))
    if len(sets) != len(maps):
        raise ValueError(f"{what}: {len(maps)} predictions but {len(sets)} sample point sets")
    return sets


def _size_group_batch(maps: list[Tensor]) -> Tensor:
    """contiguous [h,w] maps of one size -> [B,h,w]: a view when they lie back to back in ONE storage (rows of a [B,h,w] tensor, a chunk of
    inference_images), else a stacked copy. Separate allocations may sit back to back in memory, but a view across them would reach past the
    first one's storage."""
    first = maps[0]
    h, w = first.shape
    base = first.untyped_storage().data_ptr()
    step = h * w * first.element_size()
    if all(m.untyped_storage().data_ptr() == base and m.data_ptr() == first.data_ptr() + j * step for j, m in enumerate(maps)):
        return first.as_strided((len(maps), h, w), (h * w, w, 1))
    return torch.stack(maps)


def depth_mask_images(predictions, images_bgr, plane_removal: float = 0.0, threshold=(0.0, 1.0), invert: bool = False, samples_per_side: int = 16,
                      sample_xy=None) -> list[tuple[Tensor, Tensor]]:
    """Depth maps and the photos they came from -> one (cutout uint8 [ih,iw,4] BGRA, mask uint8 [ih,iw]) per photo, in order, at each photo's own
    size: the save path of the reference's depth masking demo (experiments/depth_masking.py:341-361). For every map: p = normalize_01(remove_inf(x))
    at model resolution (as depth_for_saving prepares it), n = normalize_01(p - plane_removal * plane) in fp64 with its own plane fit, s =
    cv2.resize(n, (iw, ih)) (INTER_LINEAR on CV_64F, restated: fp32 weights, fp64 sums), mask = 255 where threshold[0] <= s <= threshold[1] (NaN: 0),
    255 - mask with invert, cutout = (BGR AND mask, alpha = mask).
    predictions: a [B,h,w] tensor or a list of [1,h,w] / [h,w] maps whose sizes may differ (DPTModel.inference_images returns one). images_bgr: a
    list of uint8 HxWx3 BGR host arrays (staged through pinned memory) or CUDA tensors (read in place). sample_xy: None (plane_sample_points per
    map, in list order) or one [N,2] int point set per map. Maps of one size share one prep / fit / min-max chain; the cutouts are one launch per 32
    photos; nothing is read back or synchronised. Element k equals the call on map k and photo k alone, bit for bit. The cutouts are views into one
    allocation, the masks into another."""
    tmin, tmax = _threshold(threshold)
    what = "depth_mask_images"
    if isinstance(predictions, torch.Tensor):
        n = predictions.shape[0] if predictions.dim() == 3 else -1
    elif isinstance(predictions, (list, tuple)):
        n = len(predictions)
    else:
        raise TypeError(f"{what} expects a list of depth tensors or a BxHxW tensor, got {type(predictions)}")
    photos, on_device = _cutout_photos(images_bgr, n, what) if n >= 0 else (None, False)
    maps = _prediction_list(predictions, what)
    dev = maps[0].device
    if on_device and photos[0].device != dev:
        raise RuntimeError(f"{what}: the predictions are on {dev} but the images are on {photos[0].device}")
    sets = _cutout_samples(sample_xy, maps, what)
    # groups of equal map size (first-appearance order); the sample points of each, checked and drawn before anything is launched
    groups: dict[tuple[int, int], list[int]] = {}
    for k, m in enumerate(maps):
        groups.setdefault(tuple(m.shape), []).append(k)
    drawn = [plane_sample_points(m.shape, samples_per_side) if s is None else s for m, s in zip(maps, sets)]
    tables = {}
    for (h, w), idx in groups.items():
        pts = [drawn[k] for k in idx]
        if len({tuple(p.shape) for p in pts}) != 1:
            raise ValueError(f"{what}: the sample point sets of the {h}x{w} maps differ in shape: {[tuple(p.shape) for p in pts]}")
        stacked = torch.stack([torch.as_tensor(p) for p in pts]) if any(isinstance(p, torch.Tensor) for p in pts) else np.stack([np.asarray(p) for p in pts])
        if isinstance(stacked, torch.Tensor) and stacked.device.type == "cuda" and any(not isinstance(p, torch.Tensor) or p.device.type != "cuda" for p in pts):
            raise TypeError(f"{what}: sample_xy mixes host and device point sets")
        tables[(h, w)] = _sample_table(stacked, len(idx), h, w, samples_per_side, 0.75, dev, what)[0]
    # the map side: one chain per size group
    order, stats = [], []
    for (h, w), idx in groups.items():
        x = _size_group_batch([maps[k] for k in idx])
        s = _plane_removed(x, None, plane_removal, threshold, samples_per_side, tables[(h, w)], False, what)
        for j, k in enumerate(idx):
            order.append(k)
            stats.append((s["x"].data_ptr() + j * h * w * s["x"].element_size(), s["parts"][j].data_ptr(), s["coef"][j].data_ptr(), s["vparts"][j].data_ptr(), s))
    # outputs: photo k at a 16-pixel aligned offset of one allocation
    hws = [tuple(int(v) for v in f.shape[0:2]) for f in photos]
    offs, at = [], 0
    for ih, iw in hws:
        offs.append(at)
        at += (ih * iw + 15) // 16 * 16
    bgra = torch.empty(at * 4, device=dev, dtype=torch.uint8)
    mask = torch.empty(at, device=dev, dtype=torch.uint8)
    staged = None
    if on_device:
        img_ptrs = [f.data_ptr() for f in photos]
    else:
        staged, img_ptrs = _stage_photos(photos, dev)
    arr = lambda v, t: np.ascontiguousarray(np.asarray(v, dtype=t))  # noqa: E731
    map_ptrs = arr([stats[i][0] for i in range(len(order))], np.uint64)
    map_hw = arr([maps[k].shape for k in order], np.int32).reshape(-1)
    parts = arr([st[1] for st in stats], np.uint64)
    coef = arr([st[2] for st in stats], np.uint64)
    vparts = arr([st[3] for st in stats], np.uint64)
    img_arr = arr([img_ptrs[k] for k in order], np.uint64)
    img_hw = arr([hws[k] for k in order], np.int32).reshape(-1)
    off_arr = arr([offs[k] for k in order], np.int64)
    _launch(dev, "mdpt_post_mask_cutout_images", map_ptrs.ctypes.data, map_hw.ctypes.data, native.dtype_code(maps[0].dtype), parts.ctypes.data,
            coef.ctypes.data, vparts.ctypes.data, float(plane_removal), img_arr.ctypes.data, img_hw.ctypes.data, off_arr.ctypes.data, len(order), tmin, tmax,
            int(bool(invert)), bgra.data_ptr(), mask.data_ptr())
    del staged  # (the caching allocator reuses it in stream order only)
    return [(bgra[4 * o:4 * (o + ih * iw)].view(ih, iw, 4), mask[o:o + ih * iw].view(ih, iw)) for o, (ih, iw) in zip(offs, hws)]


# ---- block norm tiles: the reference's experiments/block_norm_visualization.py


def _block_maps(maps, what: str) -> list:
    """a list of [B,h,w] maps (sizes may differ between maps) or one [L,B,h,w] tensor -> list of [B,h,w] tensors, shapes checked (host-side only)"""
    if isinstance(maps, torch.Tensor):
        if maps.dim() != 4:
            raise RuntimeError(f"{what} expects a list of [B,h,w] maps or one [L,B,h,w] tensor, got {tuple(maps.shape)}")
        maps = list(maps.unbind(0))
    elif not isinstance(maps, (list, tuple)):
        raise TypeError(f"{what} expects a list of [B,h,w] maps or one [L,B,h,w] tensor, got {type(maps)}")
    if len(maps) == 0:
        raise ValueError(f"{what} got no maps")
    for m in maps:
        if not isinstance(m, torch.Tensor):
            raise TypeError(f"{what} expects tensors, got {type(m)}")
        if m.dim() != 3 or m.numel() == 0:
            raise RuntimeError(f"{what} expects [B,h,w] maps, got {tuple(m.shape)}")
    if len({m.shape[0] for m in maps}) != 1:
        raise ValueError(f"{what}: the maps differ in batch size: {[m.shape[0] for m in maps]}")
    return list(maps)


def block_norm_display(maps, max_token_hw=None, lut=None):
    """Per-block token maps -> display tiles, BlockData.__init__ and the tile enlargement of the reference's experiments/block_norm_visualization.py
    (:137-147, :207-233) for every block and image at once. maps: a list of fp32 [B,h_l,w_l] CUDA maps - the norms or channel planes
    DPTModel.block_norms returns - or one [L,B,h,w] tensor. -> (tiles, minmax):
      tiles   uint8 [L,B,H,W], or [L,B,H,W,3] BGR through the colormap LUT `lut` (as apply_colormap takes it) when one is given; (H, W) =
              max_token_hw, by default the largest map. Every (block, image) is normalised by its OWN min / max in fp32 exactly as numpy does it,
              u8 = round_half_even(((n - min) / (max - min)) * 255) with a true division, and a smaller map is enlarged by the nearest index
              dst // factor. Only whole factors are taken (all SwinV2's stages produce; every nearest rule, cv2.INTER_NEAREST_EXACT included,
              agrees there): any other ratio raises ValueError.
      minmax  fp32 [L,B,2], each map's {min, max}: the norm range of the script's hover label.
    A constant map (the reference divides 0 / 0) and a map holding a NaN (whose min and max are NaN, and are reported as such) give an all-zero
    tile: the reference's NaN -> uint8 conversion is undefined. One launch per 32 maps whatever B is (one more for the colormap); nothing is read
    back."""
    what = "block_norm_display"
    ms = _block_maps(maps, what)
    hws = [(int(m.shape[1]), int(m.shape[2])) for m in ms]
    if max_token_hw is None:
        th, tw = max(h for h, _ in hws), max(w for _, w in hws)
    else:
        th, tw = int(max_token_hw[0]), int(max_token_hw[1])
    if th <= 0 or tw <= 0:
        raise ValueError(f"{what}: bad tile size {max_token_hw}")
    for l, (h, w) in enumerate(hws):
        if th % h or tw % w:
            raise ValueError(f"{what}: map {l} is {h}x{w}, which does not divide the {th}x{tw} tile by whole factors")
    _need_cuda(ms, what, "expected CUDA tensors")
    if len({m.device for m in ms}) != 1:
        raise RuntimeError(f"{what}: the maps are on different devices")
    ms = [m.detach().to(torch.float32).contiguous() for m in ms]
    dev = ms[0].device
    cmap = _cmap_tensor(lut, dev)
    n_maps, b = len(ms), ms[0].shape[0]
    ptrs, hw_arr = _ptrs_hw([m.data_ptr() for m in ms], hws)
    tiles = torch.empty((n_maps, b, th, tw), device=dev, dtype=torch.uint8)
    minmax = torch.empty((n_maps, b, 2), device=dev, dtype=torch.float32)
    _launch(dev, "mdpt_post_block_norm_tiles", ptrs.ctypes.data, hw_arr.ctypes.data, n_maps, b, th, tw, tiles.data_ptr(), minmax.data_ptr())
    if cmap is None:
        return tiles, minmax
    out = torch.empty((n_maps, b, th, tw, 3), device=dev, dtype=torch.uint8)
    _launch(dev, "mdpt_post_colorize", tiles.data_ptr(), n_maps * b, th * tw, None, cmap.data_ptr(), 3, out.data_ptr())
    return out, minmax


# ---- depth-to-mesh: the client half of the reference's 3D viewer, its "Save 3D Model" (demo_helpers/3dviewer/*.js, JavaScript on the CPU there)

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
    import ctypes
    lib = native.load()
    nx, ny = ctypes.c_int32(), ctypes.c_int32()
    native.check(lib, lib.mdpt_post_mesh_grid(w, h, t, ctypes.byref(nx), ctypes.byref(ny)))
    return w, h, nx.value, ny.value


def mesh_plane_grid(image_wh, target_num_faces=MESH_TARGET_FACES, jitter_pct: float = 0.0, rng=np.random):
    """-> (nx, ny, vertex_xy | None): the viewer's plane grid for a photo of image_wh = (w, h) (3dviewer/mesh.js:184-200, through
    mdpt_post_mesh_grid) and, with jitter_pct > 0, its jittered float64 [nx ny, 2] vertex table for depth_frames_to_mesh(vertex_xy=...), drawn by
    apply_mesh_jitter's rule (mesh.js:258-283): every vertex off the border (|x| != 1 and |y| != 1), in index order, moves by
    (cos(angle) offset max_x, sin(angle) offset max_y) with offset = random(), angle = random() 2 pi (two draws per vertex, in that order) and
    max = jitter_pct x step x 0.5 x 0.9. rng: anything with random(size) - np.random, a RandomState, a Generator; the viewer's own Math.random
    cannot be reproduced. The viewer starts with jitter 1 (index.html:514)."""
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
        import ctypes
        lib, i32 = native.load(), 2 ** 31 - 1
        try:  # the library's own limits and words (host arithmetic: no device call)
            native.check(lib, lib.mdpt_post_mesh_scratch_bytes(1, max(-i32, min(nx, i32)), max(-i32, min(ny, i32)), ctypes.byref(ctypes.c_size_t())))
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
    import ctypes
    import math
    lib = native.load()
    need = ctypes.c_size_t()
    native.check(lib, lib.mdpt_post_mesh_scratch_bytes(b, nx, ny, ctypes.byref(need)))
    scratch = torch.empty(need.value // 4, device=dev, dtype=torch.int32)
    xyz = torch.empty((b, nv, 3), device=dev, dtype=torch.float32)
    uv = torch.empty((b, nv, 2), device=dev, dtype=torch.float32)
    faces = torch.empty((b, nv, 1) if mode == "points" else (b, nf, 3), device=dev, dtype=torch.int32)
    counts = torch.empty((b, 2), device=dev, dtype=torch.int32)
    bounds = torch.empty((b, 2, 3), device=dev, dtype=torch.float32)
    _launch(dev, "mdpt_post_mesh", frames.data_ptr(), b, fh, fw, nx, ny, None if table is None else table.data_ptr(), pa, pb,
            math.tan(fov_deg * 0.5 * (math.pi / 180.0)), x_scale, y_scale, edge_threshold, int(bool(is_metric)), MESH_MODES[mode], xyz.data_ptr(),
            uv.data_ptr(), faces.data_ptr(), counts.data_ptr(), bounds.data_ptr(), scratch.data_ptr(), need.value)
    return xyz, uv, faces, counts, bounds


def mesh_views(xyz: Tensor, uv: Tensor, faces: Tensor, counts: Tensor, bounds: Tensor) -> list[tuple[Tensor, Tensor, Tensor, Tensor]]:
    """depth_frames_to_mesh's slabs -> per image (xyz [kv,3], uv [kv,2], faces [kf,3 or 1], bounds [2,3]): views of the kept entries. Reads counts
    once (the only synchronisation of the mesh path)."""
    if counts.dim() != 2 or counts.shape[1] != 2 or not (xyz.shape[0] == uv.shape[0] == faces.shape[0] == bounds.shape[0] == counts.shape[0]):
        raise ValueError("mesh_views: expected the five tensors depth_frames_to_mesh returns")
    kept = counts.cpu().tolist()
    return [(xyz[i, :kv], uv[i, :kv], faces[i, :kf], bounds[i]) for i, (kv, kf) in enumerate(kept)]


# ---- rendering of depth meshes: the step of the reference's 3D viewer that needs a browser with WebGL there (3dviewer/index.html:1158-1228)

RENDER_CULL = ("back", "none")
RENDER_MAX_SCRATCH_BYTES = 1 << 30
# mdpt_texture of include/mdpt.h
_TEXTURE_RECORD = np.dtype([("bgr", "<u8"), ("h", "<i4"), ("w", "<i4")])


def _render_args(xyz, uv, faces, counts, view_proj, out_wh, cull, point_size, max_scratch_bytes, what: str):
    """everything render_mesh can check without the device -> (b, nv, nf, points, V, views float64 [b,V,16] host array or CUDA tensor, w, h)"""
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
    if int(max_scratch_bytes) <= 0:
        raise ValueError(f"{what}: max_scratch_bytes must be positive, got {max_scratch_bytes}")
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
    return b, nv, int(faces.shape[1]), points, int(views.shape[-2]), views, w, h, point_size


def render_mesh(xyz: Tensor, uv: Tensor, faces: Tensor, counts: Tensor, textures_bgr, view_proj, out_wh, cull: str = "back", point_size: float = 1.0,
                return_depth: bool = False, return_face_ids: bool = False, max_scratch_bytes: int = RENDER_MAX_SCRATCH_BYTES, fill_holes=None):
    """The slabs depth_frames_to_mesh returns (its bounds are not needed), read in place with their device-side counts, rendered from V viewpoints
    each: what the reference's 3D viewer draws with WebGL (3dviewer/index.html:1158-1228 render_3d, the mesh shaders of shaders.js) and saves frame
    by frame through canvas.toDataURL(). textures_bgr: one uint8 [h,w,3] BGR image per mesh, any sizes - host arrays (staged through pinned memory)
    or CUDA tensors (read in place; a strided view is copied) - the photo, or a depth_to_color image for the viewer's "depth as texture".
    view_proj: [V,16] (shared by the meshes) or [B,V,16], the reference's layout, clip = [x, y, z, 1] M: orbit_camera.viewer_view_proj /
    swing_views / stereo_views make them. out_wh = (w, h). cull: "back" = the viewer's gl.enable(CULL_FACE), "none" draws both windings. The mode
    follows faces.shape[-1]: 3 triangles, 1 points (squares of point_size pixels).
    -> color uint8 [B,V,h,w,4] BGRA (covered pixels alpha 255, background 0,0,0,0) and, as asked, depth fp32 [B,V,h,w] (the clip-space w: the
    distance along the view axis for the perspective camera; background +inf) and face ids int32 [B,V,h,w] (index in the kept-face order,
    background -1): a tuple when more than the colour is asked for. Nothing is read back, nothing synchronises; the result is bit-deterministic.
    The arithmetic (include/mdpt.h, mdpt_post_render): vertices in fp64 snapped to 1/256 pixel, int64 edge functions with the top-left fill rule,
    a uint64 z-buffer merged with integer atomic min, perspective-correct fp64 barycentrics, bilinear texture sample, one rounding. Deviations from
    GL: a face with a vertex at w <= 0 is dropped, not clipped against the near plane; mipmapped minification (LINEAR_MIPMAP_LINEAR,
    textures.js:200) and anti-aliasing are NOT reproduced (level 0, one sample per pixel). Four launches per chunk of views; the views are chunked
    so that the scratch (8 bytes per output pixel and 24 per vertex, per mesh and view) stays within max_scratch_bytes where one view allows.
    fill_holes: None, or the band of fill_holes below, applied to every view after the render: the colour and, when asked for, the depth are the
    filled ones (exactly what fill_holes makes of this call's result without it); face ids stay -1 on filled pixels."""
    what = "render_mesh"
    if fill_holes is not None:
        band = _fill_band(fill_holes, what, "fill_holes")
        out = render_mesh(xyz, uv, faces, counts, textures_bgr, view_proj, out_wh, cull, point_size, True, return_face_ids, max_scratch_bytes)
        filled = _fill_holes(out[0], out[1], band, return_depth, max_scratch_bytes)
        out = ((filled[0], filled[1]) if return_depth else (filled,)) + tuple(out[2:])
        return out[0] if len(out) == 1 else out
    b, nv, nf, points, n_views, views, w, h, point_size = _render_args(xyz, uv, faces, counts, view_proj, out_wh, cull, point_size, max_scratch_bytes, what)
    photos, on_device = _cutout_photos(textures_bgr, b, what)
    _need_cuda([xyz, uv, faces, counts], what)
    dev = xyz.device
    if any(t.device != dev for t in (uv, faces, counts)) or (on_device and photos[0].device != dev):
        raise RuntimeError(f"{what}: the tensors are on different devices")
    xyz, uv, faces, counts = (t.detach().contiguous() for t in (xyz, uv, faces, counts))
    if isinstance(views, np.ndarray):
        views = torch.from_numpy(np.array(np.broadcast_to(views, (b, n_views, 16))))
    views = views.to(dev, torch.float64).expand(b, n_views, 16).contiguous()
    staged = None
    if on_device:
        tex_ptrs = [f.data_ptr() for f in photos]
    else:
        staged, tex_ptrs = _stage_photos(photos, dev)
    records = np.zeros(b, dtype=_TEXTURE_RECORD)
    records["bgr"], records["h"], records["w"] = tex_ptrs, [f.shape[0] for f in photos], [f.shape[1] for f in photos]
    table = _upload_records(records, dev)
    import ctypes
    lib = native.load()
    per_view = ctypes.c_size_t()
    native.check(lib, lib.mdpt_post_render_scratch_bytes(b, 1, nv, nf, h, w, ctypes.byref(per_view)))
    chunk = max(1, min(n_views, int(max_scratch_bytes) // per_view.value, 65535 // b))
    if b > 65535:
        raise ValueError(f"{what}: at most 65535 meshes per call, got {b}")
    color = torch.empty((b, n_views, h, w, 4), device=dev, dtype=torch.uint8)
    depth = torch.empty((b, n_views, h, w), device=dev, dtype=torch.float32) if return_depth else None
    ids = torch.empty((b, n_views, h, w), device=dev, dtype=torch.int32) if return_face_ids else None
    scratch = torch.empty(chunk * per_view.value // 8, device=dev, dtype=torch.int64)
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
                table.data_ptr(), vp.data_ptr(), nvw, h, w, int(cull == "back"), point_size, c.data_ptr(), None if d is None else d.data_ptr(),
                None if i is None else i.data_ptr(), scratch.data_ptr(), nvw * per_view.value)
        if not whole:
            color[:, v0:v0 + nvw] = c
            if depth is not None:
                depth[:, v0:v0 + nvw] = d
            if ids is not None:
                ids[:, v0:v0 + nvw] = i
    del staged  # (the caching allocator reuses it in stream order only)
    out = (color,) + ((depth,) if return_depth else ()) + ((ids,) if return_face_ids else ())
    return out[0] if len(out) == 1 else out


# ---- hole filling of rendered views: depth-banded push-pull (not in the reference, whose viewer shows the holes)

FILL_BAND = 0.1  # a user-facing choice, not a measured optimum


def _fill_band(band, what: str, name: str = "band") -> float:
    if isinstance(band, bool) or not isinstance(band, (int, float, np.integer, np.floating)):
        raise TypeError(f"{what}: {name} must be a number in [0, 1], got {type(band)}")
    band = float(band)
    if not 0.0 <= band <= 1.0:
        raise ValueError(f"{what}: {name} must be in [0, 1], got {band}")
    return band


def fill_holes(color: Tensor, depth: Tensor, band: float = FILL_BAND, return_depth: bool = False, max_scratch_bytes: int = RENDER_MAX_SCRATCH_BYTES):
    """The holes of rendered views filled on the device: hierarchical (push-pull) hole filling with a preference for the far side, for what
    render_mesh leaves as background - the ground behind every foreground object once the camera leaves the photo's viewpoint (the mesh's edge
    threshold cuts those faces away on purpose) and everything outside the photo's frustum. Not in the reference, whose viewer shows the holes.
    color: uint8 [...,h,w,4] BGRA, depth: fp32 [...,h,w] with the same leading dims (render_mesh's colour and depth: clip-space w, +inf on the
    background), CUDA tensors on one device. A pixel is valid iff alpha != 0 and 0 < depth < inf; valid pixels come back byte for byte, the others
    take the mean of the valid pixels around them through an image pyramid (include/mdpt.h, mdpt_post_fill_holes, has the definition), alpha 255.
    Wherever up to four pyramid nodes are combined, only those whose depth is at least (1 - band) times the farthest one's are kept: a
    disocclusion is background, so it is continued from the background side of the hole and not from the object that uncovered it. band = 1 is
    plain push-pull, band = 0 keeps the farthest only; the default of 0.1 is a choice, not a measured optimum. With an orthographic camera w is
    constant and the band does nothing. An image without a valid pixel stays background (0,0,0,0, depth +inf).
    -> the filled colour [...,h,w,4] and, with return_depth, the filled depth [...,h,w] (a tuple). Nothing is read back, nothing synchronises; no
    atomics, bit-deterministic; the number of launches follows from (h, w) alone (9 for 1920x1080). The images are chunked so that the scratch
    (16 bytes per pyramid node above the image: about 16 / 3 bytes per pixel) stays within max_scratch_bytes where one image allows."""
    what = "fill_holes"
    for t, name in ((color, "color"), (depth, "depth")):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{what}: {name} must be a tensor, got {type(t)}")
    if color.dtype != torch.uint8 or color.dim() < 3 or color.shape[-1] != 4 or 0 in color.shape:
        raise ValueError(f"{what}: color must be uint8 [...,h,w,4] BGRA, got {color.dtype} {tuple(color.shape)}")
    if depth.dtype != torch.float32 or tuple(depth.shape) != tuple(color.shape[:-1]):
        raise ValueError(f"{what}: depth must be float32 {list(color.shape[:-1])}, got {depth.dtype} {tuple(depth.shape)}")
    band = _fill_band(band, what)
    h, w = int(color.shape[-3]), int(color.shape[-2])
    if not (0 < w <= 32768 and 0 < h <= 32768):
        raise ValueError(f"{what}: images must have sides of 1 .. 32768, got {h}x{w}")
    if int(max_scratch_bytes) <= 0:
        raise ValueError(f"{what}: max_scratch_bytes must be positive, got {max_scratch_bytes}")
    _need_cuda([color, depth], what)
    dev = color.device
    if depth.device != dev:
        raise RuntimeError(f"{what}: the tensors are on different devices")
    lead = tuple(color.shape[:-3])
    src_c, src_d = color.detach().reshape(-1, h, w, 4).contiguous(), depth.detach().reshape(-1, h, w).contiguous()
    n = int(src_c.shape[0])
    import ctypes
    lib = native.load()
    per_image = ctypes.c_size_t()
    native.check(lib, lib.mdpt_post_fill_scratch_bytes(1, h, w, ctypes.byref(per_image)))
    chunk = max(1, min(n, int(max_scratch_bytes) // per_image.value, 65535))
    out_c = torch.empty_like(src_c)
    out_d = torch.empty_like(src_d) if return_depth else None
    scratch = torch.empty(chunk * per_image.value // 16, 4, device=dev, dtype=torch.float32)
    for n0 in range(0, n, chunk):
        k = min(chunk, n - n0)
        _launch(dev, "mdpt_post_fill_holes", src_c[n0:].data_ptr(), src_d[n0:].data_ptr(), k, h, w, band, out_c[n0:].data_ptr(),
                None if out_d is None else out_d[n0:].data_ptr(), scratch.data_ptr(), k * per_image.value)
    out_c = out_c.reshape(*lead, h, w, 4)
    return (out_c, out_d.reshape(*lead, h, w)) if return_depth else out_c


_fill_holes = fill_holes  # (render_mesh's argument of that name hides the function there)


# ---- tiled high-resolution inference: the maps of overlapping tiles of one photo put together into one map at the photo's resolution

TILE_ALIGN = ("affine", "none")
# mdpt_tile of include/mdpt.h
_TILE_RECORD = np.dtype([("map", "<u8"), ("h", "<i4"), ("w", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("x2", "<i4"), ("y2", "<i4")])


def _tile_boxes_checked(boxes, image_hw, what: str) -> tuple[list[tuple[int, int, int, int]], int, int]:
    """(x1, y1, x2, y2) pixel boxes, half-open, inside the image_hw = (H, W) photo (host-side only) -> (boxes, H, W)"""
    if not hasattr(image_hw, "__len__") or len(image_hw) != 2:
        raise TypeError(f"{what}: image_hw must be (H, W), got {image_hw!r}")
    ih, iw = int(image_hw[0]), int(image_hw[1])
    if ih <= 0 or iw <= 0 or ih >= 2 ** 31 or iw >= 2 ** 31:
        raise ValueError(f"{what}: bad photo size {ih}x{iw}")
    if not isinstance(boxes, (list, tuple, np.ndarray)) or len(boxes) == 0:
        raise ValueError(f"{what} expects a non-empty list of (x1, y1, x2, y2) boxes, got {boxes!r}")
    out = []
    for k, b in enumerate(boxes):
        if not hasattr(b, "__len__") or len(b) != 4 or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in b):
            raise TypeError(f"{what}: box {k} must be four ints (x1, y1, x2, y2), got {b!r}")
        x1, y1, x2, y2 = (int(v) for v in b)
        if not (0 <= x1 < x2 <= iw and 0 <= y1 < y2 <= ih):
            raise ValueError(f"{what}: box {k} ({x1}, {y1})-({x2}, {y2}) is empty or outside the {ih}x{iw} photo")
        out.append((x1, y1, x2, y2))
    return out, ih, iw


def _upload_records(records: np.ndarray, dev) -> Tensor:
    """a host record array -> device bytes through pinned memory, one non-blocking copy on the current stream (as _stage_photos)"""
    raw = records.view(np.uint8).reshape(-1)
    pinned = torch.empty(raw.size, dtype=torch.uint8, pin_memory=True)
    pinned.numpy()[...] = raw
    with torch.cuda.device(dev):
        staged = torch.empty(raw.size, dtype=torch.uint8, device=dev)
        staged.copy_(pinned, non_blocking=True)
    return staged


def stitch_tiles(tile_maps, boxes, image_hw, guide=None, align: str = "affine", feather=None, return_fit: bool = False):
    """The depth maps of overlapping tiles of one photo -> one fp32 [1,H,W] map at the photo's resolution (not in the reference: its
    .readme_assets/results_explainer.md says why tiles cannot simply be pasted - every forward has its own scale and shift, "Results are
    scene-specific!" - and names the cure under "Fitting to (more) known data", a least-squares fit of the two terms, without code for it).
    tile_maps: [1,h,w] / [h,w] CUDA maps of one dtype and any sizes, as DPTModel.inference_regions returns them; boxes: each map's
    (x1, y1, x2, y2) pixel box in the photo, half-open; image_hw = (H, W). align="affine" fits every tile to `guide` - a [1,gh,gw] / [gh,gw] CUDA map
    of the WHOLE photo, e.g. its inference at model size - over the tile's own box with one scale and one shift (least squares over one sample per
    tile-map pixel, the guide sampled bilinearly at the pixel's centre; samples that are not finite are skipped; a tile the fit cannot use - flat,
    negatively correlated, fewer than two samples - takes the guide's mean over its box, a tile without any sample is left out); align="none" blends
    the maps as they are. The tiles are resized to their boxes by cv2.resize's INTER_LINEAR rule and blended with weights that ramp over `feather`
    pixels from every tile edge that is not the photo's own border (default: the smallest overlap between neighbouring boxes, 0 for one tile). A
    pixel no tile covers is NaN. fp64 arithmetic rounded once; bit-deterministic; three launches (fit, solve, blend), nothing read back, no
    synchronisation. return_fit: -> (map, fit fp64 [T,2] {scale, shift}, sums fp64 [T,6] {n, Sx, Sy, Sxx, Sxy, Syy}), both None with align="none"."""
    what = "stitch_tiles"
    if align not in TILE_ALIGN:
        raise ValueError(f"{what}: align must be 'affine' or 'none', got {align!r}")
    if align == "affine" and guide is None:
        raise ValueError(f"{what}: align='affine' fits the tiles to a guide map of the whole photo: pass guide=, or align='none'")
    boxes, ih, iw = _tile_boxes_checked(boxes, image_hw, what)
    if not isinstance(tile_maps, (list, tuple)):
        raise TypeError(f"{what} expects a list of [1,h,w] / [h,w] tile maps, got {type(tile_maps)}")
    if len(tile_maps) != len(boxes):
        raise ValueError(f"{what}: {len(tile_maps)} tile maps but {len(boxes)} boxes")
    if feather is None:
        from .tiling import smallest_overlap
        feather = smallest_overlap(boxes)
    feather = float(feather)
    if not (0.0 <= feather < float("inf")):
        raise ValueError(f"{what}: feather must be finite and >= 0, got {feather}")
    maps = _prediction_list(list(tile_maps), what)
    dev = maps[0].device
    g = None
    if align == "affine":
        g = _prediction_list([guide], what + " (guide)")[0]
        if g.device != dev:
            raise RuntimeError(f"{what}: the tiles are on {dev} but the guide is on {g.device}")
    import ctypes
    n_tiles = len(maps)
    records = np.zeros(n_tiles, dtype=_TILE_RECORD)
    records["map"] = [m.data_ptr() for m in maps]
    records["h"], records["w"] = [m.shape[0] for m in maps], [m.shape[1] for m in maps]
    for k, name in enumerate(("x1", "y1", "x2", "y2")):
        records[name] = [b[k] for b in boxes]
    table = _upload_records(records, dev)
    dt = native.dtype_code(maps[0].dtype)
    fit = sums = None
    if g is not None:
        lib = native.load()
        need = ctypes.c_size_t()
        native.check(lib, lib.mdpt_post_tile_scratch_bytes(records.ctypes.data, n_tiles, ctypes.byref(need)))
        scratch = torch.empty(max(need.value // 8, 1), device=dev, dtype=torch.float64)
        fit = torch.empty((n_tiles, 2), device=dev, dtype=torch.float64)
        sums = torch.empty((n_tiles, 6), device=dev, dtype=torch.float64)
        _launch(dev, "mdpt_post_tile_fit", records.ctypes.data, table.data_ptr(), n_tiles, dt, g.data_ptr(), native.dtype_code(g.dtype), g.shape[0], g.shape[1],
                ih, iw, fit.data_ptr(), sums.data_ptr(), scratch.data_ptr(), need.value)
    out = torch.empty((1, ih, iw), device=dev, dtype=torch.float32)
    _launch(dev, "mdpt_post_tile_blend", records.ctypes.data, table.data_ptr(), n_tiles, dt, ih, iw, None if fit is None else fit.data_ptr(),
            None if sums is None else sums.data_ptr(), feather, out.data_ptr())
    del table  # (the caching allocator reuses it in stream order only)
    return (out, fit, sums) if return_fit else out


# ---- true depth from ground truth: align predictions to measured depth maps, score them, map them to true depth

ALIGN_SPACES = {"inverse": native.ALIGN_INVERSE, "depth": native.ALIGN_DEPTH}
ALIGN_METHODS = {"lstsq": native.ALIGN_LSTSQ, "median": native.ALIGN_MEDIAN}
DEPTH_METRIC_NAMES = ("n", "n_bad", "abs_rel", "sq_rel", "rmse", "rmse_log", "log10", "delta1", "delta2", "delta3", "silog")
assert len(DEPTH_METRIC_NAMES) == native.ALIGN_NUM_METRICS
# mdpt_depth_pair of include/mdpt.h
_PAIR_RECORD = np.dtype([("pred", "<u8"), ("ph", "<i4"), ("pw", "<i4"), ("truth", "<u8"), ("valid", "<u8"), ("H", "<i4"), ("W", "<i4")])


def _truth_maps(maps, n: int, dev, np_dtype, torch_dtype, what: str, name: str) -> tuple[list[int], list[tuple[int, int]], list]:
    """`n` [H,W] / [1,H,W] maps - a [B,H,W] tensor or array, or a list of per-image CUDA tensors or host arrays (not a mix; sizes may differ) ->
    (device address of each, its (H, W), what keeps the memory alive). Host arrays are staged as the cutout route stages photos."""
    if isinstance(maps, (torch.Tensor, np.ndarray)):
        if maps.ndim != 3:
            raise RuntimeError(f"{what}: {name} must be a list of [H,W] / [1,H,W] maps or a BxHxW batch, got {tuple(maps.shape)}")
        maps = list(maps)
    if not isinstance(maps, (list, tuple)):
        raise TypeError(f"{what}: {name} must be a list of maps or a BxHxW batch, got {type(maps)}")
    if len(maps) != n:
        raise ValueError(f"{what}: {n} predictions but {len(maps)} {name} maps")
    n_dev = sum(isinstance(m, torch.Tensor) for m in maps)
    if 0 < n_dev < n or (n_dev == 0 and not all(isinstance(m, np.ndarray) for m in maps)):
        raise TypeError(f"{what}: {name} must be host arrays or device tensors, not a mix of both")
    flat = []
    for m in maps:
        m = m[0] if m.ndim == 3 and m.shape[0] == 1 else m
        if m.ndim != 2 or m.shape[0] == 0 or m.shape[1] == 0:
            raise RuntimeError(f"{what}: {name} maps must be non-empty [H,W] or [1,H,W], got {tuple(m.shape)}")
        flat.append(m)
    hws = [(int(m.shape[0]), int(m.shape[1])) for m in flat]
    if n_dev:
        _need_cuda(flat, what, f"expected {name} on the device")
        if any(m.device != dev for m in flat):
            raise RuntimeError(f"{what}: the predictions are on {dev} but a {name} map is not")
        keep = [(m.detach() != 0 if torch_dtype == torch.uint8 else m.detach()).to(torch_dtype).contiguous() for m in flat]
        return [m.data_ptr() for m in keep], hws, keep
    host = [np.ascontiguousarray(m != 0 if np_dtype == np.uint8 else m, dtype=np_dtype).view(np.uint8).reshape(h, -1) for m, (h, _) in zip(flat, hws)]
    staged, ptrs = _stage_photos(host, dev)
    return ptrs, hws, [staged]


def _truth_range(truth_range, what: str) -> tuple[float, float]:
    lo, hi = truth_range
    lo, hi = float("-inf") if lo is None else float(lo), float("inf") if hi is None else float(hi)
    if not lo <= hi:
        raise ValueError(f"{what}: the range ({lo}, {hi}) is empty or NaN")
    return lo, hi


def _align_choice(table: dict, key, what: str, name: str) -> int:
    if key not in table:
        raise ValueError(f"{what}: {name} must be one of {sorted(table)}, got {key!r}")
    return table[key]


def _align_pairs(predictions, truths, valid, what: str):
    """-> (maps, records, the uploaded table, (H, W) per pair, whatever must outlive the launches): what fit_true_depth and depth_metrics take as
    `staged` to share one staging of the truths and one table (DPTModel.evaluate_depth)"""
    maps = _prediction_list(predictions, what)
    dev = maps[0].device
    tptr, hws, keep_t = _truth_maps(truths, len(maps), dev, np.float32, torch.float32, what, "truth")
    vptr, keep_v = [0] * len(maps), []
    if isinstance(valid, (list, tuple)) and len(valid) != len(maps):
        raise ValueError(f"{what}: {len(maps)} predictions but {len(valid)} valid maps")
    given = None if valid is None else [k for k, m in enumerate(valid) if m is not None]  # (a list may hold None: that pair has no mask)
    if given:
        some, vhws, keep_v = _truth_maps([valid[k] for k in given], len(given), dev, np.uint8, torch.uint8, what, "valid")
        if vhws != [hws[k] for k in given]:
            raise ValueError(f"{what}: every valid map must have its truth's size")
        for k, ptr in zip(given, some):
            vptr[k] = ptr
    records = _pair_records(maps, hws, tptr, vptr)
    return maps, records, _upload_records(records, dev), hws, (keep_t, keep_v)


def _pair_records(maps: list[Tensor], hws, tptr=None, vptr=None) -> np.ndarray:
    if any(h * w >= 2 ** 31 for h, w in hws):
        raise ValueError("a map of 2^31 pixels or more is not supported")
    records = np.zeros(len(maps), dtype=_PAIR_RECORD)
    records["pred"] = [m.data_ptr() for m in maps]
    records["ph"], records["pw"] = [m.shape[0] for m in maps], [m.shape[1] for m in maps]
    records["H"], records["W"] = [h for h, _ in hws], [w for _, w in hws]
    if tptr is not None:
        records["truth"], records["valid"] = tptr, vptr
    return records


def _align_scratch(records: np.ndarray, dev) -> tuple[Tensor, int]:
    import ctypes
    lib = native.load()
    need = ctypes.c_size_t()
    native.check(lib, lib.mdpt_post_align_scratch_bytes(records.ctypes.data, len(records), ctypes.byref(need)))
    return torch.empty(max(need.value // 8, 1), device=dev, dtype=torch.float64), need.value


def fit_true_depth(predictions, truths, valid=None, space: str = "inverse", method: str = "lstsq", truth_range=(None, None), return_sums: bool = False, *,
                   staged=None):
    """Fit every prediction to its ground truth with one scale A and one shift B -> fp64 [P,2] {A, B} on the device (not in the reference: its
    .readme_assets/results_explainer.md gives depth = 1 / (A V + B) and names both fits under "Fitting to (more) known data", without code).
    predictions: a [B,h,w] CUDA tensor or a list of [1,h,w] / [h,w] CUDA maps of one dtype and any sizes (as DPTModel.inference_images returns).
    truths: one measured depth map per prediction, at its own resolution - a batch or a list of CUDA tensors or of host arrays (staged through
    pinned memory); zero, negative, NaN and inf mean "no measurement". valid: optional maps of the truths' sizes, non-zero where the truth counts
    (a batch, or a list that may hold None for a pair without a mask).
    truth_range = (min, max) leaves out measurements outside it (None: no bound). One sample per truth pixel: the prediction is sampled
    bilinearly at the pixel's centre. space="inverse" fits A v + B to 1 / truth (relative-depth models), "depth" to truth itself (metric heads).
    method="lstsq": least squares; "median": A = mad(t) / mad(v), B = med(t) - A med(v) with exact medians of the float32 samples (robust to
    outliers; MiDaS's normalisation). A pair the fit cannot use (fewer than two samples, a flat prediction, A <= 0) gets A = 0 and B = the
    mean / median of t, a pair without samples A = B = 0. fp64, bit-deterministic, 2 (lstsq) or 11 (median) launches for the whole call, nothing
    read back. return_sums: -> (fit, sums fp64 [P,6]: {n, Sv, St, Svv, Svt, Stt} or {n, med v, med t, mad v, mad t, 0}). staged: what
    _align_pairs returned for these very arguments (evaluate_depth stages the truths and uploads the table once for fit and metrics)."""
    what = "fit_true_depth"
    sp, me = _align_choice(ALIGN_SPACES, space, what, "space"), _align_choice(ALIGN_METHODS, method, what, "method")
    tmin, tmax = _truth_range(truth_range, what)
    maps, records, table, _, keep = _align_pairs(predictions, truths, valid, what) if staged is None else staged
    dev = maps[0].device
    scratch, need = _align_scratch(records, dev)
    fit = torch.empty((len(maps), 2), device=dev, dtype=torch.float64)
    sums = torch.empty((len(maps), 6), device=dev, dtype=torch.float64)
    _launch(dev, "mdpt_post_align_fit", records.ctypes.data, table.data_ptr(), len(maps), native.dtype_code(maps[0].dtype), sp, me, tmin, tmax,
            fit.data_ptr(), sums.data_ptr(), scratch.data_ptr(), need)
    del table, keep  # (the caching allocator reuses them in stream order only)
    return (fit, sums) if return_sums else fit


def depth_metrics(predictions, truths, fit=None, valid=None, space: str = "inverse", truth_range=(None, None), *, staged=None) -> Tensor:
    """The standard depth metrics of every prediction against its ground truth -> fp64 [P,11] on the device, columns DEPTH_METRIC_NAMES: n (samples),
    n_bad (samples whose A v + B is not positive, left out), AbsRel, SqRel, RMSE, RMSE-log, log10, delta1..3, SILog. Arguments and samples as
    fit_true_depth; fit: its [P,2] result (None: A = 1, B = 0 - a metric head scored as it is, with space="depth"). The aligned depth is
    1 / (A v + B) in inverse space and A v + B in depth space. A pair without scored samples gets NaN metrics. Two launches, nothing read back."""
    what = "depth_metrics"
    sp = _align_choice(ALIGN_SPACES, space, what, "space")
    tmin, tmax = _truth_range(truth_range, what)
    maps, records, table, _, keep = _align_pairs(predictions, truths, valid, what) if staged is None else staged
    dev = maps[0].device
    fit = _fit_checked(fit, len(maps), dev, what)
    scratch, need = _align_scratch(records, dev)
    out = torch.empty((len(maps), native.ALIGN_NUM_METRICS), device=dev, dtype=torch.float64)
    _launch(dev, "mdpt_post_align_metrics", records.ctypes.data, table.data_ptr(), len(maps), native.dtype_code(maps[0].dtype), sp, tmin, tmax,
            None if fit is None else fit.data_ptr(), out.data_ptr(), scratch.data_ptr(), need)
    del table, keep
    return out


def _fit_checked(fit, n: int, dev, what: str):
    if fit is None:
        return None
    _need_cuda([fit], what, "expected fit on the device")
    if fit.shape != (n, 2) or fit.device != dev:
        raise RuntimeError(f"{what}: fit must be [{n},2] on {dev}, got {tuple(fit.shape)} on {fit.device}")
    return fit.detach().to(torch.float64).contiguous()


def true_depth(predictions, fit, target_hws=None, space: str = "inverse", clamp=(None, None)):
    """Predictions -> true depth maps, fp32: each prediction resized bilinearly to its target (H, W) (target_hws: one per prediction; None: the
    prediction's own size), then 1 / (A v + B) in inverse space (+inf where A v + B <= 0) or A v + B in depth space, then clamped to
    clamp = (min, max) where given - one fused launch, fp64 arithmetic rounded once. fit: fit_true_depth's [P,2] (None: A = 1, B = 0). A [B,h,w]
    tensor with one common target size returns a [B,H,W] tensor, anything else a list of [1,H,W] maps (views of one allocation)."""
    what = "true_depth"
    sp = _align_choice(ALIGN_SPACES, space, what, "space")
    dmin, dmax = _truth_range(clamp, what)
    maps = _prediction_list(predictions, what)
    dev = maps[0].device
    fit = _fit_checked(fit, len(maps), dev, what)
    if target_hws is None:
        hws = [(m.shape[0], m.shape[1]) for m in maps]
    else:
        hws = [(int(hw[0]), int(hw[1])) for hw in target_hws]
        if len(hws) != len(maps):
            raise ValueError(f"{what}: {len(maps)} predictions but {len(hws)} target sizes")
        if any(h <= 0 or w <= 0 for h, w in hws):
            raise ValueError(f"{what}: target sizes must be positive, got {hws}")
    records = _pair_records(maps, hws)
    offsets = np.zeros(len(maps), dtype=np.int64)
    offsets[1:] = np.cumsum([h * w for h, w in hws], dtype=np.int64)[:-1]
    # one upload: the records (40 bytes each, so any count of them ends 8-byte aligned) and the offsets behind them
    table = _upload_records(np.concatenate([records.view(np.uint8).reshape(-1), offsets.view(np.uint8)]), dev)
    out = torch.empty(int(sum(h * w for h, w in hws)), device=dev, dtype=torch.float32)
    _launch(dev, "mdpt_post_align_apply", records.ctypes.data, table.data_ptr(), len(maps), native.dtype_code(maps[0].dtype), sp,
            None if fit is None else fit.data_ptr(), offsets.ctypes.data, table.data_ptr() + records.nbytes, dmin, dmax, out.data_ptr())
    del table
    if isinstance(predictions, torch.Tensor) and len(set(hws)) == 1:
        return out.view(len(maps), *hws[0])
    return _views(out, hws)


def mesh_depth_range(fit_ab, prediction_minmax) -> tuple[float, float]:
    """A fitted (A, B) of ONE image -> the (min_depth, max_depth) pair that makes depth_frames_to_mesh place its vertices at true depth. The mesh reads
    the 24-bit packed frame, V = (x - lo) / (hi - lo) with (lo, hi) = prediction_minmax, the prediction's min and max, and evaluates
    1 / (V (1 / min_depth - 1 / max_depth) + 1 / max_depth) (relative models). True depth is 1 / (A x + B) = 1 / (V A (hi - lo) + A lo + B), so
    max_depth = 1 / (A lo + B) and min_depth = 1 / (A hi + B): the algebra closes exactly, up to the 2^-24 quantisation of V. Host-side floats
    (the caller reads the fit and the min / max back once). Raises where the fit puts either end at or behind the camera (A hi + B or
    A lo + B <= 0) or is degenerate (A <= 0)."""
    a, b = float(fit_ab[0]), float(fit_ab[1])
    lo, hi = float(prediction_minmax[0]), float(prediction_minmax[1])
    far, near = a * lo + b, a * hi + b
    if not (a > 0.0 and lo < hi and far > 0.0 and near > 0.0):
        raise ValueError(f"mesh_depth_range: fit A={a}, B={b} over predictions [{lo}, {hi}] has no positive depth range")
    return 1.0 / near, 1.0 / far


# ---- photo-guided upsampling: the fast guided filter with the photo as guide (not in the reference: every demo there resizes its map bilinearly)

# mdpt_guided_pair of include/mdpt.h
_GUIDED_RECORD = np.dtype([("map", "<u8"), ("h", "<i4"), ("w", "<i4"), ("photo", "<u8"), ("pitch", "<i8"), ("H", "<i4"), ("W", "<i4"), ("out", "<u8"),
                           ("scratch_off", "<i8")])


def _guided_checked(predictions, images_bgr, radius, eps, what: str) -> tuple[int, float]:
    """everything guided_upsample_images can refuse from shapes and values alone, before any tensor has to be on the device"""
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 0 <= int(radius) <= native.GUIDED_MAX_RADIUS:
        raise ValueError(f"{what}: radius must be an int in 0 .. {native.GUIDED_MAX_RADIUS} (cells of the map), got {radius!r}")
    eps = float(eps)
    if not 0.0 < eps < float("inf"):
        raise ValueError(f"{what}: eps must be finite and > 0, got {eps}")
    if isinstance(predictions, torch.Tensor):
        shapes = [tuple(predictions.shape[1:])] * predictions.shape[0] if predictions.dim() == 3 else None
    elif isinstance(predictions, (list, tuple)):
        shapes = [tuple(p.shape[-2:]) if isinstance(p, torch.Tensor) and p.dim() in (2, 3) else None for p in predictions]
    else:
        shapes = None
    if shapes is None or not isinstance(images_bgr, (list, tuple)):
        return int(radius), eps  # (_prediction_list / _cutout_photos name what is wrong)
    if len(images_bgr) != len(shapes):
        raise ValueError(f"{what}: {len(shapes)} predictions but {len(images_bgr)} images")
    for k, (f, hw) in enumerate(zip(images_bgr, shapes)):
        if not isinstance(f, (np.ndarray, torch.Tensor)):
            continue
        if f.dtype != (torch.uint8 if isinstance(f, torch.Tensor) else np.uint8) or f.ndim != 3 or f.shape[2] != 3:
            raise ValueError(f"{what}: image {k} is not a uint8 HxWx3 BGR photo (shape {tuple(f.shape)}, dtype {f.dtype}): the guide is the BGR photo itself")
        if hw is not None and (f.shape[0] < hw[0] or f.shape[1] < hw[1]):
            raise ValueError(f"{what}: photo {k} of {f.shape[0]}x{f.shape[1]} is smaller than its {hw[0]}x{hw[1]} map: guided upsampling only enlarges "
                             "(to shrink a map use scale_prediction / scale_prediction_images)")
    return int(radius), eps


def guided_upsample_images(predictions, images_bgr, radius: int = 8, eps: float = 1e-4, return_coefficients: bool = False):
    """Depth maps and the photos they came from -> one fp32 [1,H_i,W_i] map per photo, in order, at each photo's own size, with the photo as the
    guide of the enlargement (not in the reference, whose demos resize bilinearly; He & Sun's fast guided filter): where scale_prediction_images turns
    a depth edge into a ramp several photo pixels wide, the result follows the photo's own edges. The photo averaged over the cell of each map pixel
    (pixel (Y, X) belongs to cell (Y h // H, X w // W)) is the guide g at map resolution; per cell, over the window of the cells within `radius` in
    both axes (clipped to the map, mean = sum / its own count): Sigma = mean(g g^T) - mean(g) mean(g)^T + eps I,
    a = Sigma^-1 (mean(g p) - mean(g) mean(p)), b = mean(p) - a . mean(g); (a, b) are window-averaged once more, resampled bilinearly at every photo
    pixel's centre, and q = a_B B / 255 + a_G G / 255 + a_R R / 255 + b. eps is the variance (of a 0 .. 1 guide) below which the photo's texture is
    ignored; radius 0 gives the bilinear resize, a flat photo the window mean of the map.
    predictions: a [B,h,w] tensor or a list of [1,h,w] / [h,w] CUDA maps of one dtype whose sizes may differ (DPTModel.inference_images returns one).
    images_bgr: one uint8 HxWx3 BGR photo per map, none smaller than its map: host arrays (staged through pinned memory) or CUDA tensors read in
    place - a sliced view photo[y1:y2, x1:x2] is read through its row pitch, no copy. fp64 arithmetic rounded to fp32 once; bit-deterministic; every
    pair independent of the others; six launches for the whole call, nothing read back, no synchronisation. The outputs are views into one
    allocation. return_coefficients: -> (maps, [fp64 [h_i,w_i,4] mean coefficients (a_B, a_G, a_R, b) per pair])."""
    what = "guided_upsample_images"
    radius, eps = _guided_checked(predictions, images_bgr, radius, eps, what)
    n = predictions.shape[0] if isinstance(predictions, torch.Tensor) and predictions.dim() == 3 else (len(predictions) if isinstance(predictions, (list, tuple)) else -1)
    checked, on_device = _cutout_photos(images_bgr, n, what) if n >= 0 else (None, False)
    maps = _prediction_list(predictions, what)
    dev = maps[0].device
    keep = None
    if on_device:
        if checked[0].device != dev:
            raise RuntimeError(f"{what}: the predictions are on {dev} but the images are on {checked[0].device}")
        # a view whose pixels are packed and whose rows are at least a row apart is read in place through its pitch; anything else as its packed copy
        in_place = [f.stride(2) == 1 and f.stride(1) == 3 and f.stride(0) >= 3 * f.shape[1] for f in images_bgr]
        keep = [f.detach() if ok else c for f, c, ok in zip(images_bgr, checked, in_place)]
        img_ptrs, pitches = [f.data_ptr() for f in keep], [int(f.stride(0)) for f in keep]
    else:
        keep, img_ptrs = _stage_photos(checked, dev)
        pitches = [3 * f.shape[1] for f in checked]
    hws = [(int(f.shape[0]), int(f.shape[1])) for f in checked]
    if any(h * w >= 2 ** 31 for h, w in hws):
        raise ValueError(f"{what}: a photo of 2^31 pixels or more is not supported")
    import ctypes
    lib = native.load()
    records = np.zeros(len(maps), dtype=_GUIDED_RECORD)
    records["map"] = [m.data_ptr() for m in maps]
    records["h"], records["w"] = [m.shape[0] for m in maps], [m.shape[1] for m in maps]
    records["photo"], records["pitch"] = img_ptrs, pitches
    records["H"], records["W"] = [h for h, _ in hws], [w for _, w in hws]
    need, at = ctypes.c_size_t(), 0
    for k in range(len(maps)):  # (a pair's region is what the call asks for its record alone; the regions lie end to end)
        native.check(lib, lib.mdpt_post_guided_scratch_bytes(records[k:k + 1].ctypes.data, 1, ctypes.byref(need)))
        records["scratch_off"][k] = at
        at += need.value
    out = torch.empty(int(sum(h * w for h, w in hws)), device=dev, dtype=torch.float32)
    offs = np.cumsum([0] + [h * w for h, w in hws[:-1]], dtype=np.int64)
    records["out"] = [out.data_ptr() + 4 * int(o) for o in offs]
    scratch = torch.empty(at // 8, device=dev, dtype=torch.float64)
    coeffs = torch.empty(4 * int(sum(m.numel() for m in maps)), device=dev, dtype=torch.float64) if return_coefficients else None
    table = _upload_records(records, dev)
    _launch(dev, "mdpt_post_guided_upsample", records.ctypes.data, table.data_ptr(), len(maps), native.dtype_code(maps[0].dtype), radius, eps,
            scratch.data_ptr(), at, None if coeffs is None else coeffs.data_ptr())
    del table, keep, scratch  # (the caching allocator reuses them in stream order only)
    result = _views(out, hws)
    if not return_coefficients:
        return result
    return result, [c[0] for c in _views(coeffs, [tuple(m.shape) for m in maps], (4,))]
