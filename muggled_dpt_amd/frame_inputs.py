"""The host side of the uint8 frame routes of DPTModel (inference, inference_batch, inference_images, inference_regions): the reference's crop
rule, the argument checks, what the fused im2col kernel can read in place, and the forward plans. Every route is a list of uint8 [h,w,3] views -
host ndarray views or device tensors - and everything here only looks at shapes, strides and types: pure host code, no native binding, nothing that
needs a device. muggled_dpt_amd.dpt_model re-exports these names."""

from __future__ import annotations

import numpy as np
import torch
from torch import Tensor


def is_cropping(crop_xy1xy2_norm) -> bool:
    """Whether a normalised ((x1, y1), (x2, y2)) box leaves anything out (the reference's CropData.is_cropping, run_3dviewer.py): a side
    spanning less than 0.999 of the image crops."""
    (x1, y1), (x2, y2) = crop_xy1xy2_norm
    return bool((x2 - x1) < 0.999 or (y2 - y1) < 0.999)


def crop_slices_from_norm(image_shape, crop_xy1xy2_norm, minimum_crop_xy=(5, 5)) -> tuple[slice, slice]:
    """Normalised ((x1, y1), (x2, y2)) -> (y_slice, x_slice) in pixels, by the reference's rule (demo_helpers/crop_ui.py,
    make_crop_slices_from_xy1xy2_norm): the corners times (w, h) as a float32 product, rounded half to even, clipped to [0, w] x [0, h]; a side
    shorter than its minimum falls back to the image's full extent. Corners are not reordered (a reversed box gives an empty slice, as there)."""
    full_h, full_w = int(image_shape[0]), int(image_shape[1])
    norm = np.asarray(crop_xy1xy2_norm, dtype=np.float32)
    if norm.shape != (2, 2):
        raise TypeError(f"a normalised crop is ((x1, y1), (x2, y2)), got shape {norm.shape}")
    limits = np.array([full_w, full_h], dtype=np.int32)
    px = np.clip(np.round(norm * limits.astype(np.float32)).astype(np.int32), 0, limits)
    (x1, y1), (x2, y2) = px.tolist()
    if abs(x2 - x1) < minimum_crop_xy[0]:
        x1, x2 = 0, full_w
    if abs(y2 - y1) < minimum_crop_xy[1]:
        y1, y2 = 0, full_h
    return slice(y1, y2), slice(x1, x2)


def _is_crop(crop) -> bool:
    """a crop argument: a (y_slice, x_slice) pair, or ((x1, y1), (x2, y2)) in normalised units"""
    if not isinstance(crop, (tuple, list)) or len(crop) != 2:
        return False
    if all(isinstance(c, slice) for c in crop):
        return True
    real = lambda v: isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool)  # noqa: E731
    return all(isinstance(c, (tuple, list, np.ndarray)) and len(c) == 2 and all(real(v) for v in c) for c in crop)


def _crop_box(image_hw, crop) -> tuple[int, int, int, int]:
    """A crop argument on an image of (h, w) -> the pixel box (x1, y1, x2, y2), half-open; None is the full image. Slices mean what they mean
    in image[y_slice, x_slice] (negative and open ends included); a normalised box goes through crop_slices_from_norm. Host-side only."""
    h, w = int(image_hw[0]), int(image_hw[1])
    if crop is None:
        return 0, 0, w, h
    if not _is_crop(crop):
        raise TypeError(f"a crop is ((x1, y1), (x2, y2)) in normalised units or a (y_slice, x_slice) pair, got {crop!r}")
    ys, xs = crop if isinstance(crop[0], slice) else crop_slices_from_norm((h, w), crop)
    (y1, y2, sy), (x1, x2, sx) = ys.indices(h), xs.indices(w)
    if sy != 1 or sx != 1:
        raise ValueError(f"crop slices must have step 1, got {ys}, {xs}")
    if x2 <= x1 or y2 <= y1:
        raise ValueError(f"the crop {crop!r} of a {h}x{w} image is empty")
    return x1, y1, x2, y2


def _crop_host(image_bgr, crop):
    """image_bgr[y_slice, x_slice] of a host image as a view (nothing is copied; the staging copy reads the box's bytes only)"""
    if not (isinstance(image_bgr, np.ndarray) and image_bgr.ndim == 3):
        raise TypeError("a crop needs an OpenCV-style uint8 HxWx3 BGR image (cv2.imread output)")
    x1, y1, x2, y2 = _crop_box(image_bgr.shape[0:2], crop)
    return image_bgr[y1:y2, x1:x2]


def _row_pitch(t: Tensor) -> int:
    """bytes between the rows of a uint8 [..., h, w, 3] device tensor that _in_place() accepted (a single row has no pitch: packed)"""
    return int(t.stride(-3)) if t.shape[-3] > 1 else 3 * int(t.shape[-2])


def _in_place(t: Tensor) -> bool:
    """Whether the im2col kernel can read a uint8 [h,w,3] / [B,h,w,3] device tensor where it lies: innermost strides (3, 1), rows at least a
    row apart ([..., pitch, 3, 1]), frames any positive distance apart. Sliced views of packed tensors are of this kind."""
    if t.stride(-1) != 1 or t.stride(-2) != 3 or (t.shape[-3] > 1 and t.stride(-3) < 3 * t.shape[-2]):
        return False
    return t.dim() == 3 or t.shape[0] == 1 or t.stride(0) > 0


def _check_frames(images_bgr):
    """Argument checks of DPTModel.inference_batch (host-side only, nothing touches a GPU) -> (frames, on_device, (H, W)): frames is the
    ndarray / list as given, or a [B,H,W,3] CUDA tensor the kernel can read in place (_in_place: as given, e.g. a sliced view; any other
    layout is made contiguous)."""
    if isinstance(images_bgr, torch.Tensor):
        if images_bgr.dtype != torch.uint8 or images_bgr.dim() != 4 or images_bgr.shape[3] != 3:
            raise TypeError(f"inference_batch expects uint8 BxHxWx3 BGR frames, got a {images_bgr.dtype} tensor of shape {tuple(images_bgr.shape)}")
        if images_bgr.shape[0] == 0:
            raise ValueError("inference_batch got no frames")
        if images_bgr.device.type != "cuda":
            images_bgr = images_bgr.numpy()
        else:
            return images_bgr if _in_place(images_bgr) else images_bgr.contiguous(), True, tuple(images_bgr.shape[1:3])
    if isinstance(images_bgr, np.ndarray):
        if images_bgr.dtype != np.uint8 or images_bgr.ndim != 4 or images_bgr.shape[3] != 3:
            raise TypeError(f"inference_batch expects uint8 BxHxWx3 BGR frames, got a {images_bgr.dtype} array of shape {images_bgr.shape}")
        if images_bgr.shape[0] == 0:
            raise ValueError("inference_batch got no frames")
        return images_bgr, False, images_bgr.shape[1:3]
    if not isinstance(images_bgr, (list, tuple)):
        raise TypeError(f"inference_batch expects a uint8 [B,H,W,3] ndarray / CUDA tensor or a list of HxWx3 uint8 arrays, got {type(images_bgr)}")
    if len(images_bgr) == 0:
        raise ValueError("inference_batch got no frames")
    for f in images_bgr:
        if not (isinstance(f, np.ndarray) and f.dtype == np.uint8 and f.ndim == 3 and f.shape[2] == 3):
            raise TypeError("inference_batch expects OpenCV-style uint8 HxWx3 BGR frames (cv2.imread output)")
    shapes = {f.shape for f in images_bgr}
    if len(shapes) != 1:
        raise ValueError(f"inference_batch needs frames of one size, got {sorted(shapes)}")
    return list(images_bgr), False, images_bgr[0].shape[0:2]


def _check_images(images_bgr, batch_size) -> tuple[list, bool]:
    """Argument checks of DPTModel.inference_images (host-side only, nothing touches a GPU) -> (images, on_device): a list of uint8 HxWx3
    ndarrays, or of uint8 HxWx3 CUDA tensors the kernel can read in place (_in_place; any other layout is made contiguous)."""
    if isinstance(batch_size, bool) or not isinstance(batch_size, (int, np.integer)):
        raise TypeError(f"inference_images: batch_size must be an int, got {type(batch_size)}")
    if batch_size < 1:
        raise ValueError(f"inference_images: batch_size must be at least 1, got {batch_size}")
    if not isinstance(images_bgr, (list, tuple)):
        raise TypeError(f"inference_images expects a list of uint8 HxWx3 BGR images (ndarrays or CUDA tensors), got {type(images_bgr)}")
    if len(images_bgr) == 0:
        raise ValueError("inference_images got no images")
    n_dev = sum(isinstance(f, torch.Tensor) for f in images_bgr)
    if 0 < n_dev < len(images_bgr):
        raise TypeError("inference_images expects host arrays or device tensors, not a mix of both")
    on_device = n_dev > 0
    for f in images_bgr:
        if on_device:
            ok = f.dtype == torch.uint8 and f.dim() == 3 and f.shape[2] == 3 and f.device.type == "cuda"
        else:
            ok = isinstance(f, np.ndarray) and f.dtype == np.uint8 and f.ndim == 3 and f.shape[2] == 3
        if not ok:
            raise TypeError("inference_images expects OpenCV-style uint8 HxWx3 BGR images (cv2.imread output), or uint8 HxWx3 CUDA tensors")
        if f.shape[0] == 0 or f.shape[1] == 0:
            raise ValueError(f"inference_images got an empty image ({f.shape[0]}x{f.shape[1]})")
    if on_device and len({f.device for f in images_bgr}) != 1:
        raise RuntimeError("inference_images: the device tensors are on different devices")
    return [(f if _in_place(f) else f.contiguous()) if on_device else f for f in images_bgr], on_device


def _check_crops(crops, n_images: int) -> list:
    """The `crops` argument of DPTModel.inference_images -> one crop (or None) per image: None, one crop for all, or a list of one per image."""
    if crops is None or _is_crop(crops):
        return [crops] * n_images
    if not isinstance(crops, (list, tuple)) or not all(c is None or _is_crop(c) for c in crops):
        raise TypeError("crops is one crop for all images or a list of one crop (or None) per image; a crop is ((x1, y1), (x2, y2)) in normalised "
                        "units or a (y_slice, x_slice) pair")
    if len(crops) != n_images:
        raise ValueError(f"{n_images} images but {len(crops)} crops")
    return list(crops)


def _check_regions(regions, image_shapes) -> list[tuple[int, int, int, int, int]]:
    """The `regions` argument of DPTModel.inference_regions (host-side only): (image_index, x1, y1, x2, y2) pixel boxes, half-open, inside their image."""
    if not isinstance(regions, (list, tuple, np.ndarray)):
        raise TypeError(f"inference_regions expects a list of (image_index, x1, y1, x2, y2) boxes, got {type(regions)}")
    if len(regions) == 0:
        raise ValueError("inference_regions got no regions")
    out = []
    for k, r in enumerate(regions):
        if not hasattr(r, "__len__") or len(r) != 5 or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in r):
            raise TypeError(f"region {k} must be five ints (image_index, x1, y1, x2, y2), got {r!r}")
        i, x1, y1, x2, y2 = (int(v) for v in r)
        if not 0 <= i < len(image_shapes):
            raise IndexError(f"region {k}: image index {i} is outside [0, {len(image_shapes)})")
        h, w = int(image_shapes[i][0]), int(image_shapes[i][1])
        if not (0 <= x1 < x2 <= w and 0 <= y1 < y2 <= h):
            raise ValueError(f"region {k}: box ({x1}, {y1})-({x2}, {y2}) is empty or outside its {h}x{w} image")
        out.append((i, x1, y1, x2, y2))
    return out


def region_chunks(regions, scaled_hw, batch_size: int):
    """Forward plan of DPTModel.inference_regions (pure host code): image_chunks on the BOX sizes - the reference applies its size rule to the
    cropped frame - so the indices are region indices."""
    return image_chunks([(y2 - y1, x2 - x1) for _, x1, y1, x2, y2 in regions], scaled_hw, batch_size)


def image_chunks(sizes_hw, scaled_hw, batch_size: int) -> list[tuple[tuple[int, int], list[int]]]:
    """Forward plan of DPTModel.inference_images (pure host code): image sizes [(h, w), ...] and the size rule scaled_hw(h, w) -> model
    tensor (H, W) -> [((H, W), [image indices]), ...]. A group is every image with the same tensor size, groups in order of first appearance,
    indices in input order; each group is cut into chunks of at most batch_size images, one batched forward each."""
    groups: dict[tuple[int, int], list[int]] = {}
    for i, (h, w) in enumerate(sizes_hw):
        groups.setdefault(tuple(int(v) for v in scaled_hw(int(h), int(w))), []).append(i)
    return [(hw, idx[k:k + batch_size]) for hw, idx in groups.items() for k in range(0, len(idx), batch_size)]
