"""The filling of the holes a moved camera uncovers in rendered views (fill_holes: depth-banded push-pull; not in the reference, whose viewer shows
the holes; render_mesh and DPTModel.render_views take it as an option). Kernels: csrc/post_fill.inc."""

from __future__ import annotations

import numpy as np
import torch
from torch import Tensor

from ._common import _launch, _need_cuda, ptr, scratch_bytes, scratch_chunk

RENDER_MAX_SCRATCH_BYTES = 1 << 30  # the default scratch budget of render_mesh and fill_holes
FILL_BAND = 0.1  # a user-facing choice, not a measured optimum


def _fill_band(band, what: str, name: str = "band") -> float:
    if isinstance(band, bool) or not isinstance(band, (int, float, np.integer, np.floating)):
        raise TypeError(f"{what}: {name} must be a number in [0, 1], got {type(band)}")
    band = float(band)
    if not 0.0 <= band <= 1.0:
        raise ValueError(f"{what}: {name} must be in [0, 1], got {band}")
    return band


def fill_holes(color: Tensor, depth: Tensor, band: float = FILL_BAND, return_depth: bool = False, max_scratch_bytes: int = RENDER_MAX_SCRATCH_BYTES):
    """The holes of rendered views filled on the device: hierarchical (push-pull) hole filling with a preference for the far side, for what render_mesh leaves as
    background - the ground behind every foreground object once the camera leaves the photo's viewpoint (the mesh's edge threshold cuts those faces away on purpose) and
    everything outside the photo's frustum. Not in the reference, whose viewer shows the holes. color: uint8 [...,h,w,4] BGRA, depth: fp32 [...,h,w] with the same leading
    dims (render_mesh's colour and depth: clip-space w, +inf on the background), CUDA tensors on one device. A pixel is valid iff alpha != 0 and 0 < depth < inf; valid
    pixels come back byte for byte, the others take the mean of the valid pixels around them through an image pyramid (include/mdpt.h, mdpt_post_fill_holes, has the
    definition), alpha 255. Wherever up to four pyramid nodes are combined, only those whose depth is at least (1 - band) times the farthest one's are kept: a
    disocclusion is background, so it is continued from the background side of the hole and not from the object that uncovered it. band = 1 is plain push-pull, band = 0
    keeps the farthest only; the default of 0.1 is a choice, not a measured optimum. With an orthographic camera w is constant and the band does nothing. An image without
    a valid pixel stays background (0,0,0,0, depth +inf). -> the filled colour [...,h,w,4] and, with return_depth, the filled depth [...,h,w] (a tuple). Nothing is read
    back, nothing synchronises; no atomics, bit-deterministic; the number of launches follows from (h, w) alone (9 for 1920x1080). The images are chunked so that the
    scratch (16 bytes per pyramid node above the image: about 16 / 3 bytes per pixel) stays within max_scratch_bytes where one image allows."""
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
    scratch_chunk(1, 1, max_scratch_bytes, what)  # (the budget is checked before the device is)
    _need_cuda([color, depth], what)
    dev = color.device
    if depth.device != dev:
        raise RuntimeError(f"{what}: the tensors are on different devices")
    lead = tuple(color.shape[:-3])
    src_c, src_d = color.detach().reshape(-1, h, w, 4).contiguous(), depth.detach().reshape(-1, h, w).contiguous()
    n = int(src_c.shape[0])
    per_image = scratch_bytes("mdpt_post_fill_scratch_bytes", 1, h, w)
    chunk = scratch_chunk(n, per_image, max_scratch_bytes, what)
    out_c = torch.empty_like(src_c)
    out_d = torch.empty_like(src_d) if return_depth else None
    scratch = torch.empty(chunk * per_image // 16, 4, device=dev, dtype=torch.float32)
    for n0 in range(0, n, chunk):
        k = min(chunk, n - n0)
        _launch(dev, "mdpt_post_fill_holes", src_c[n0:].data_ptr(), src_d[n0:].data_ptr(), k, h, w, band, out_c[n0:].data_ptr(),
                ptr(out_d[n0:] if return_depth else None), scratch.data_ptr(), k * per_image)
    out_c = out_c.reshape(*lead, h, w, 4)
    return (out_c, out_d.reshape(*lead, h, w)) if return_depth else out_c
