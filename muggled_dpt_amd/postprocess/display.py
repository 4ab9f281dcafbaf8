"""The tensor helpers of the reference's muggled_dpt/demo_helpers/postprocess.py (scale_prediction :22-29, normalize_01 :63-74, convert_to_uint8 :79-91), the 24-bit
packing of run_3dviewer.py:576-590, the per-image display tail of its video / image demos (histogram_equalization :107-145, the colormap LUT of
toadui/colormaps.py:237-259, depth_to_color: the per-frame loop of run_video.py:348-361 over a batch), the *_images variants. Kernels: csrc/post_display.inc."""

from __future__ import annotations

import functools

import numpy as np
import torch
from torch import Tensor

from .. import native
from ._common import _batch_maps, _cmap_tensor, _dev_f32, _dev_u8, _launch, _prediction_list, _target_hw, _views, packed_offsets, ptr


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
    _launch(x.device, "mdpt_post_normalize", x.data_ptr(), x.numel(), ptr(mm), out.data_ptr(), native.POST_U24, int(bool(lossy)))
    return out


def remove_inf_tensor(data: Tensor, inf_replacement_value: float = 0.0, in_place: bool = True) -> Tensor:
    """postprocess.py:34-40 (plain torch indexing on whatever device the tensor lives on; not a kernel of ours)."""
    data = data if in_place else data.clone()
    data[data.isinf()] = inf_replacement_value
    return data


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


def equalize_lut(hist: Tensor, b: int, vmin: int, vmax: int, dev) -> Tensor:
    """int32 [b,256] histograms -> uint8 [b,256] equalization LUTs: cv2.equalizeHist's for (0, 255), else np.histogram's through threshold_bin_table"""
    table = None if (vmin, vmax) == (0, 255) else torch.from_numpy(threshold_bin_table(vmin, vmax).copy()).to(dev)
    lut = torch.empty((b, 256), device=dev, dtype=torch.uint8)
    _launch(dev, "mdpt_post_equalize_lut", hist.data_ptr(), b, ptr(table), vmin, vmax, lut.data_ptr())
    return lut


def histogram_equalization(depth_uint8: Tensor, min_pct: float = 0.0, max_pct: float = 1.0) -> Tensor:
    """uint8 [H,W] or [B,H,W] on the device -> same shape, every image equalized on its own (postprocess.py:107-145): cv2.equalizeHist for the
    full range, the np.histogram branch otherwise. One histogram pass, one LUT launch, one apply pass; nothing visits the host."""
    x = _dev_u8(depth_uint8, "histogram_equalization")
    x3 = x if x.dim() == 3 else x[None]
    vmin, vmax = equalization_range(min_pct, max_pct)
    b = x3.shape[0]
    hist = torch.zeros((b, 256), device=x.device, dtype=torch.int32)
    _launch(x.device, "mdpt_post_histogram", x3.data_ptr(), b, x3[0].numel(), hist.data_ptr())
    lut = equalize_lut(hist, b, vmin, vmax, x.device)
    out = torch.empty_like(x3)
    _launch(x.device, "mdpt_post_colorize", x3.data_ptr(), b, x3[0].numel(), lut.data_ptr(), None, 1, out.data_ptr())
    return out.view(x.shape)


def apply_colormap(depth_uint8: Tensor, lut=None) -> Tensor:
    """uint8 [H,W] or [B,H,W] -> uint8 [...,H,W,3] BGR through a 1x256x3 BGR LUT (ndarray or tensor), or gray when lut is None:
    cv2.LUT(cv2.cvtColor(x, GRAY2BGR), lut) (toadui/colormaps.py:237-259)."""
    x = _dev_u8(depth_uint8, "apply_colormap")
    cmap = _cmap_tensor(lut, x.device)
    x3 = x if x.dim() == 3 else x[None]
    out = torch.empty((*x.shape, 3), device=x.device, dtype=torch.uint8)
    _launch(x.device, "mdpt_post_colorize", x3.data_ptr(), x3.shape[0], x3[0].numel(), None, ptr(cmap), 3, out.data_ptr())
    return out


def depth_to_color(prediction: Tensor, target_wh: tuple[int, int] | None = None, reverse: bool = False, high_contrast: bool = False, lut=None) -> Tensor:
    """[B,h,w] depth prediction -> uint8 [B,H,W,3] BGR display frames, the per-frame loop of run_video.py:348-361 for every image at once:
    scale_prediction (target_wh given) -> convert_to_uint8 -> 255 - x (reverse) -> histogram_equalization (high_contrast) -> colormap (lut; gray
    when None). Image b's frame equals that composition on prediction[b:b+1] bit for bit (its own min / max and histogram). Four launches at
    most: resize + per-image min/max (also clears the histogram), uint8 + histogram, LUT, equalize-and-colormap as one lookup."""
    x = _batch_maps(prediction, "depth_to_color")
    dev = x.device
    cmap = _cmap_tensor(lut, dev)
    b, h, w = x.shape
    dt = native.dtype_code(x.dtype)
    src, src_dt, oh, ow = x, dt, h, w
    scaled_ptr = hist_ptr = eq_ptr = None
    if target_wh is not None:
        oh, ow = int(target_wh[1]), int(target_wh[0])
        src, src_dt = torch.empty((b, oh, ow), device=dev, dtype=torch.float32), native.DTYPE_F32
        scaled_ptr = src.data_ptr()
    parts = torch.empty((b, native.POST_SEG_PARTS, 2), device=dev, dtype=torch.int32)
    if high_contrast:
        hist = torch.empty((b, 256), device=dev, dtype=torch.int32)
        hist_ptr = hist.data_ptr()
    _launch(dev, "mdpt_post_minmax_seg", x.data_ptr(), dt, b, h, w, scaled_ptr, oh, ow, parts.data_ptr(), hist_ptr)
    n = oh * ow
    u8 = torch.empty((b, oh, ow), device=dev, dtype=torch.uint8)
    _launch(dev, "mdpt_post_u8_hist_seg", src.data_ptr(), src_dt, b, n, parts.data_ptr(), int(bool(reverse)), u8.data_ptr(), hist_ptr)
    if high_contrast:
        eq = torch.empty((b, 256), device=dev, dtype=torch.uint8)  # (the per-frame call of a video loop: the parent's statements, no helper)
        _launch(dev, "mdpt_post_equalize_lut", hist_ptr, b, None, 0, 255, eq.data_ptr())
        eq_ptr = eq.data_ptr()
    out = torch.empty((b, oh, ow, 3), device=dev, dtype=torch.uint8)
    _launch(dev, "mdpt_post_colorize", u8.data_ptr(), b, n, eq_ptr, cmap.data_ptr() if lut is not None else None, 3, out.data_ptr())
    return out


def _minmax_images(maps: list[Tensor], out_hw, hist: Tensor | None):
    """mdpt_post_minmax_images: per-image min/max partials, and (out_hw given) every map resized into one packed fp32 buffer -> (parts, scaled)"""
    dev = maps[0].device
    b = len(maps)
    ptrs, in_hw = np.asarray([m.data_ptr() for m in maps], dtype=np.uint64), np.asarray([m.shape for m in maps], dtype=np.int32).reshape(-1)
    scaled = o_hw = None
    if out_hw is not None:
        o_hw = np.asarray(out_hw, dtype=np.int32).reshape(-1)
        scaled = torch.empty(int(sum(h * w for h, w in out_hw)), device=dev, dtype=torch.float32)
    parts = torch.empty((b, native.POST_SEG_PARTS, 2), device=dev, dtype=torch.int32)
    _launch(dev, "mdpt_post_minmax_images", ptrs.ctypes.data, in_hw.ctypes.data, native.dtype_code(maps[0].dtype), b, ptr(scaled),
            o_hw.ctypes.data if out_hw is not None else None, parts.data_ptr(), ptr(hist))
    return parts, scaled


def scale_prediction_images(predictions, target_whs) -> list[Tensor]:
    """scale_prediction for images of different sizes: predictions (a list of [1,h,w] / [h,w] maps whose sizes may differ, as DPTModel.inference_images returns, or a
    [B,h,w] tensor) and one (w, h) per image -> a list of [1,H_i,W_i] maps in the predictions' dtype. Element i equals scale_prediction(prediction i, target_whs[i]) bit
    for bit. One launch per 32 images; the outputs are views into one allocation."""
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
    out_hw = None if target_whs is None else _target_hw(target_whs, b, "depth_to_color_images")
    hws = [tuple(m.shape) for m in maps] if out_hw is None else out_hw
    hist = torch.empty((b, 256), device=dev, dtype=torch.int32) if high_contrast else None
    parts, scaled = _minmax_images(maps, out_hw, hist)
    offs, total = packed_offsets([h * w for h, w in hws])
    if scaled is None:
        src_ptrs, src_dt = [m.data_ptr() for m in maps], native.dtype_code(maps[0].dtype)
    else:
        src_ptrs, src_dt = [scaled.data_ptr() + 4 * o for o in offs], native.DTYPE_F32
    ptrs, hw_arr = np.asarray(src_ptrs, dtype=np.uint64), np.asarray(hws, dtype=np.int32).reshape(-1)
    u8 = torch.empty(total, device=dev, dtype=torch.uint8)
    _launch(dev, "mdpt_post_u8_hist_images", ptrs.ctypes.data, hw_arr.ctypes.data, src_dt, b, parts.data_ptr(), int(bool(reverse)), u8.data_ptr(), ptr(hist))
    eq = equalize_lut(hist, b, 0, 255, dev) if high_contrast else None
    out = torch.empty(total * 3, device=dev, dtype=torch.uint8)
    _launch(dev, "mdpt_post_colorize_images", u8.data_ptr(), hw_arr.ctypes.data, b, ptr(eq), ptr(cmap), 3, out.data_ptr())
    return _views(out, hws, (3,))
