"""The still-image demo's display loop and save path (depth_to_display / depth_for_saving, run_image.py:185-195, 323-358, the plane fit of demo_helpers/plane_fit.py),
the 3D viewer's edge alpha (depth_edge_mask / pack_depth_u24_frames, run_3dviewer.py:455-505, 576-593); mask.py starts from _plane_removed too. Kernels: csrc/post_still.inc."""

from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np
import torch
from torch import Tensor

from .. import native
from ._common import _batch_maps, _cmap_tensor, _launch, ptr
from .display import equalization_range, equalize_lut


def plane_sample_points(hw, samples_per_side: int = 16, jitter_scale: float = 0.75, rng=np.random) -> np.ndarray:
    """int32 [N,2] (x, y) pixel samples of an [h,w] map for the plane of best fit, drawn as the reference's plane_fit.get_xyz_samples draws them: a min(n, side) grid of
    cell centres, jittered by clip(randn, -1, 1) * half a cell * jitter_scale (x first, then y, two randn calls), scaled by (w-1, h-1) and rounded. With np.random.seed(s)
    beforehand these are the reference's own points. rng: anything with randn (np.random, a RandomState) or standard_normal (a Generator)."""
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


def plane_of_best_fit(depth: Tensor, samples_per_side: int = 16, jitter_scale: float = 0.75, sample_xy=None) -> Tensor:
    """[H,W] or [B,H,W] depth on the device -> fp32 plane images of the same shape, the reference's plane_fit.estimate_plane_of_best_fit per image: z at the sample points
    (sample_xy: [N,2] or [B,N,2] ints, host or device; None: plane_sample_points per image in batch order), the known x / y means, the sample z mean, and the normal of
    the smallest singular value of the centred samples (the smallest eigenvector of their fp64 Gram matrix, by Jacobi; the sign does not matter). One workgroup per image
    fits, one launch evaluates. A constant map gives the constant plane (the reference divides by a zero normal there)."""
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


class PlaneMap(namedtuple("PlaneMap", "x dt b oh ow parts coef f vparts tmin tmax hist")):
    """csrc's PlaneMap: the prepared [b,oh,ow] map and its min/max parts, the plane and its weight f, the parts of dn - f plane, the threshold, the histograms"""
    __slots__ = ()

    def args(self) -> tuple:  # (the argument run mdpt_post_threshold and mdpt_post_mask_display begin with)
        return (self.x.data_ptr(), self.dt, self.b, self.oh, self.ow, self.parts.data_ptr(), self.coef.data_ptr(), self.f, self.vparts.data_ptr(), self.tmin, self.tmax)


def _plane_removed(x: Tensor, target_wh, plane_removal: float, threshold, samples_per_side: int, sample_xy, hist: bool, what: str) -> PlaneMap:
    """run_image.py's steps up to the threshold for every image: remove_inf(scale_prediction) + min/max, the plane fit on the normalized map, min/max of dn - f plane"""
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
    _launch(dev, "mdpt_post_display_prep", x.data_ptr(), dt, b, h, w, prepared.data_ptr(), oh, ow, parts.data_ptr(), ptr(hist_t))
    coef = torch.empty((b, 4), device=dev, dtype=torch.float64)
    _launch(dev, "mdpt_post_plane_fit", prepared.data_ptr(), dt, b, oh, ow, parts.data_ptr(), pts.data_ptr(), n, int(per_image), coef.data_ptr())
    vparts = torch.empty((b, native.POST_SEG_PARTS, 2), device=dev, dtype=torch.float64)
    f = float(plane_removal)
    _launch(dev, "mdpt_post_plane_minmax", prepared.data_ptr(), dt, b, oh, ow, parts.data_ptr(), coef.data_ptr(), f, vparts.data_ptr())
    return PlaneMap(prepared, dt, b, oh, ow, parts, coef, f, vparts, tmin, tmax, hist_t)


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
    u8 = torch.empty((s.b, s.oh, s.ow), device=dev, dtype=torch.uint8)
    _launch(dev, "mdpt_post_threshold", *s.args(), native.POST_U8, 0, u8.data_ptr(), ptr(s.hist))
    eq = equalize_lut(s.hist, s.b, *equalization_range(s.tmin, s.tmax), dev) if high_contrast else None
    out = torch.empty((s.b, s.oh, s.ow, 3), device=dev, dtype=torch.uint8)
    _launch(dev, "mdpt_post_colorize", u8.data_ptr(), s.b, s.oh * s.ow, ptr(eq), ptr(cmap), 3, out.data_ptr())
    return out


def depth_for_saving(prediction: Tensor, plane_removal: float = 0.0, threshold=(0.0, 1.0), reverse: bool = False, samples_per_side: int = 16, sample_xy=None) -> Tensor:
    """[B,h,w] depth prediction -> fp32 [B,h,w], the still-image demo's .npy save path (run_image.py:350-358) at model resolution for every image:
    remove_inf -> normalize_01 -> minus plane_removal * its plane of best fit -> normalize_01 -> clip((v - min) / max(0.001, max - min), 0, 1)
    -> 1 - t (reverse), in fp64, rounded to fp32 once. sample_xy as for plane_of_best_fit. Four launches."""
    _threshold(threshold)
    x = _batch_maps(prediction, "depth_for_saving")
    s = _plane_removed(x, None, plane_removal, threshold, samples_per_side, sample_xy, False, "depth_for_saving")
    out = torch.empty((s.b, s.oh, s.ow), device=x.device, dtype=torch.float32)
    _launch(x.device, "mdpt_post_threshold", *s.args(), native.POST_F32, int(bool(reverse)), out.data_ptr(), None)
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
    _launch(x.device, "mdpt_post_edge_mag", x.data_ptr(), b, h, w, ptr(parts), weights.ctypes.data, ksize, mag.data_ptr(), mag_max.data_ptr())
    return mag, mag_max


def depth_edge_mask(depth: Tensor, blur_kernel_size: int = 5, blur_weight: float = 1.0) -> Tensor:
    """[H,W] or [B,H,W] depth on the device -> uint8 of the same shape, the 3D viewer's default alpha (run_3dviewer.py:455-505) per image: a Gaussian blur (exp(-(i^2 +
    j^2) 0.01 / blur_weight) over its max, size 1 + 2 (k // 2)) and the 3x3 Sobel [[3,10,3],[0,0,0],[-3,-10,-3]] (and its transpose), both cross-correlations with reflect
    padding, mag = sqrt(dx^2 + dy^2), ~round(255 mag / max(mag)). A flat map (max 0) gives 255 everywhere (the reference's 0 / 0 there is NaN, whose conversion to uint8
    is undefined); so does a map holding a NaN. Sides must exceed the reflect pads (at least max(2, k // 2 + 1)), as torch requires. Two launches."""
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
    _launch(dev, "mdpt_post_pack_u24_alpha", x.data_ptr(), b, h * w, ptr(parts), int(bool(lossy)), ptr(mag), ptr(mag_max), ptr(mask),
            int(mask is not None and mask.dim() == 3), out.data_ptr())
    return out
