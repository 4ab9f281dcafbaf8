"""What the feature modules share, each rule once: the device checks (no CPU implementation: host arrays raise), the launch on the current torch stream,
nullable pointers, scratch-size queries and the chunk rule, the pinned upload, packed-buffer offsets and their views, the record tables of mdpt.h's structs."""

from __future__ import annotations

import ctypes

import numpy as np
import torch
from torch import Tensor

from .. import native

# the host tables of the per-item entry points, one numpy record per struct of include/mdpt.h (csrc/mdpt_post_*.cpp static_assert the layouts, field by field:
# MDPT_SAME_RECORD of csrc/mdpt_post_checks.h)
TILE_RECORD = np.dtype([("map", "<u8"), ("h", "<i4"), ("w", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("x2", "<i4"), ("y2", "<i4")])  # mdpt_tile
PAIR_RECORD = np.dtype([("pred", "<u8"), ("ph", "<i4"), ("pw", "<i4"), ("truth", "<u8"), ("valid", "<u8"), ("H", "<i4"), ("W", "<i4")])  # mdpt_depth_pair
GUIDED_RECORD = np.dtype([("map", "<u8"), ("h", "<i4"), ("w", "<i4"), ("photo", "<u8"), ("pitch", "<i8"), ("H", "<i4"), ("W", "<i4"), ("out", "<u8"),
                          ("scratch_off", "<i8")])  # mdpt_guided_pair
TEXTURE_RECORD = np.dtype([("bgr", "<u8"), ("h", "<i4"), ("w", "<i4")])  # mdpt_texture
REFOCUS_RECORD = np.dtype([("map", "<u8"), ("h", "<i4"), ("w", "<i4"), ("photo", "<u8"), ("pitch", "<i8"), ("H", "<i4"), ("W", "<i4"), ("out", "<u8"),
                           ("scratch_off", "<i8"), ("tile_off", "<i8")])  # mdpt_refocus_pair
NORMALS_RECORD = np.dtype([("map", "<u8"), ("h", "<i4"), ("w", "<i4"), ("photo", "<u8"), ("pitch", "<i8"), ("H", "<i4"), ("W", "<i4"), ("normals", "<u8"),
                           ("encoded", "<u8"), ("relit", "<u8"), ("scratch_off", "<i8"), ("tile_off", "<i8"), ("kx", "<f8"), ("ky", "<f8"), ("step", "<i4"),
                           ("pad", "<i4")])  # mdpt_normals_pair
SHADOWS_RECORD = np.dtype([("map", "<u8"), ("h", "<i4"), ("w", "<i4"), ("photo", "<u8"), ("pitch", "<i8"), ("H", "<i4"), ("W", "<i4"), ("gh", "<i4"), ("gw", "<i4"),
                           ("ao", "<u8"), ("vis", "<u8"), ("relit", "<u8"), ("scratch_off", "<i8"), ("tile_off", "<i8"), ("gtile_off", "<i8"), ("kx", "<f8"),
                           ("ky", "<f8"), ("step", "<i4"), ("pad", "<i4")])  # mdpt_shadows_pair
# (mdpt_segment_image and mdpt_segment_photo, for muggled_dpt_amd/segment.py; csrc/mdpt_segment.cpp asserts the layouts)
SEGMENT_RECORD = np.dtype([("map", "<u8"), ("h", "<i4"), ("w", "<i4"), ("labels", "<u8"), ("scratch_off", "<i8"), ("region_off", "<i8"), ("tile_off", "<i8"),
                           ("pixel_off", "<i8")])
SEGMENT_PHOTO_RECORD = np.dtype([("labels", "<u8"), ("h", "<i4"), ("w", "<i4"), ("photo", "<u8"), ("pitch", "<i8"), ("H", "<i4"), ("W", "<i4"), ("bgra", "<u8"),
                                 ("mask", "<u8"), ("region_off", "<i8"), ("regions", "<i4"), ("pad", "<i4")])
# (mdpt_localfit_pair, for muggled_dpt_amd/local_align.py; csrc/mdpt_localfit.cpp asserts the layout)
LOCALFIT_RECORD = np.dtype([("pred", "<u8"), ("ph", "<i4"), ("pw", "<i4"), ("truth", "<u8"), ("valid", "<u8"), ("H", "<i4"), ("W", "<i4"), ("gh", "<i4"), ("gw", "<i4"),
                            ("cell_off", "<i8"), ("scratch_off", "<i8"), ("out", "<u8")])


def _need_cuda(tensors, what: str, expected: str = "expected a CUDA tensor") -> None:
    """There is no CPU implementation: anything among `tensors` that is not a CUDA tensor raises."""
    if not all(isinstance(t, torch.Tensor) and t.device.type == "cuda" for t in tensors):
        raise RuntimeError(f"{what}: {expected} (muggled_dpt_amd post-processing runs on the MI355X only, no CPU fallback)")


def _dev_f32(t, what: str) -> Tensor:
    _need_cuda([t], what)
    return t.detach().to(torch.float32).contiguous()


def _dev_u8(t, what: str) -> Tensor:
    _need_cuda([t], what)
    if t.dtype != torch.uint8 or t.dim() not in (2, 3) or t.numel() == 0:
        raise TypeError(f"{what}: expected a uint8 HxW or BxHxW tensor, got {t.dtype} {tuple(t.shape)}")
    return t.detach().contiguous()


def _launch(dev, fn, *args):
    lib = native.load()
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        native.check(lib, getattr(lib, fn)(*args, stream))


def ptr(t):
    """the device address of an optional tensor: None (a NULL argument) stays None"""
    return None if t is None else t.data_ptr()


def scratch_bytes(symbol: str, *args) -> int:
    """what an mdpt_post_*_scratch_bytes entry point asks for these arguments (host arithmetic: no device call)"""
    lib, need = native.load(), ctypes.c_size_t()
    native.check(lib, getattr(lib, symbol)(*args, ctypes.byref(need)))
    return need.value


def scratch_chunk(n: int, per_item: int, max_scratch_bytes, what: str, cap: int = 65535) -> int:
    """how many of `n` items one launch takes so that its scratch stays within the budget where one item allows, and within the grid's cap"""
    if int(max_scratch_bytes) <= 0:
        raise ValueError(f"{what}: max_scratch_bytes must be positive, got {max_scratch_bytes}")
    return max(1, min(n, int(max_scratch_bytes) // per_item, cap))


def packed_offsets(counts, align: int = 1) -> tuple[list[int], int]:
    """items of `counts` elements laid end to end, each starting at a multiple of `align` -> (where each starts, the padded total); _views undoes it"""
    offs, at = [], 0
    for c in counts:
        offs.append(at)
        at += (int(c) + align - 1) // align * align
    return offs, at


def _views(flat: Tensor, hws, tail=(), align: int = 1) -> list[Tensor]:
    """a packed buffer -> its [1,h,w,*tail] items (packed_offsets over h w, in units of one `tail`)"""
    step = int(np.prod(tail, dtype=np.int64))
    offs, _ = packed_offsets([h * w for h, w in hws], align)
    return [flat[o * step:(o + h * w) * step].view(1, h, w, *tail) for o, (h, w) in zip(offs, hws)]


def _to_device(pinned: Tensor, dev) -> Tensor:
    """a filled pinned buffer -> its device copy, non-blocking on the current stream; keep it until the launch is enqueued (reuse is in stream order only)"""
    with torch.cuda.device(dev):
        staged = torch.empty(pinned.numel(), dtype=torch.uint8, device=dev)
        staged.copy_(pinned, non_blocking=True)
    return staged


def upload(arrays, dev, align: int = 1) -> tuple[Tensor, list[int]]:
    """host arrays (photos, maps; strided views included: numpy does the copy) -> (one device buffer, the `align`ed device address of each in it)"""
    offs, total = packed_offsets([a.nbytes for a in arrays], align)
    pinned = torch.empty(total, dtype=torch.uint8, pin_memory=True)
    host = pinned.numpy()
    for a, o in zip(arrays, offs):
        host[o:o + a.nbytes].view(a.dtype).reshape(a.shape)[...] = a
    staged = _to_device(pinned, dev)
    return staged, [staged.data_ptr() + o for o in offs]


def _upload_records(records: np.ndarray, dev) -> Tensor:
    """a host record table -> its device copy (one array needs no offsets: every per-item entry point pays this on each call)"""
    raw = records.view(np.uint8).reshape(-1)
    pinned = torch.empty(raw.size, dtype=torch.uint8, pin_memory=True)
    pinned.numpy()[...] = raw
    return _to_device(pinned, dev)


def record_table(dtype: np.dtype, maps, lead=("map", "h", "w"), ptrs=None, **columns) -> np.ndarray:
    """one zeroed record per item of `maps` ([h,w,...]): `lead` takes its device address (`ptrs` for host items), h and w; `columns` fill fields by name"""
    records = np.zeros(len(maps), dtype=dtype)
    records[lead[0]], records[lead[1]], records[lead[2]] = ptrs or [m.data_ptr() for m in maps], [m.shape[0] for m in maps], [m.shape[1] for m in maps]
    for name, values in columns.items():
        records[name] = values
    return records


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


def prediction_count(predictions) -> int:
    """B of a [B,h,w] tensor, len of a list, -1 for anything else (_prediction_list then names what is wrong)"""
    if isinstance(predictions, torch.Tensor):
        return predictions.shape[0] if predictions.dim() == 3 else -1
    return len(predictions) if isinstance(predictions, (list, tuple)) else -1


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


def _photo_list(images_bgr, n: int, what: str) -> tuple[list, bool]:
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


def _photo_pointers(images_bgr, photos, on_device: bool, dev, what: str):
    """_photo_list's photos for kernels that read a photo byte by byte through its row pitch -> (what must stay alive until the launch, the device address and
    the pitch in bytes of each). A CUDA view whose pixels are packed and whose rows are at least a row apart is read in place; anything else as its packed
    copy; host photos go through one pinned upload."""
    if on_device:
        if photos[0].device != dev:
            raise RuntimeError(f"{what}: the predictions are on {dev} but the images are on {photos[0].device}")
        in_place = [f.stride(2) == 1 and f.stride(1) == 3 and f.stride(0) >= 3 * f.shape[1] for f in images_bgr]
        keep = [f.detach() if ok else c for f, c, ok in zip(images_bgr, photos, in_place)]
        return keep, [f.data_ptr() for f in keep], [int(f.stride(0)) for f in keep]
    keep, img_ptrs = upload(photos, dev, 16)
    return keep, img_ptrs, [3 * f.shape[1] for f in photos]


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
