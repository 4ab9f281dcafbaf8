"""The tiles of the reference's block norm viewer (block_norm_display: experiments/block_norm_visualization.py). Kernels: csrc/post_block_norms.inc."""

import numpy as np
import torch

from ._common import _cmap_tensor, _launch, _need_cuda


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
    ms = list(maps)
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
    ptrs, hw_arr = np.asarray([m.data_ptr() for m in ms], dtype=np.uint64), np.asarray(hws, dtype=np.int32).reshape(-1)
    tiles = torch.empty((n_maps, b, th, tw), device=dev, dtype=torch.uint8)
    minmax = torch.empty((n_maps, b, 2), device=dev, dtype=torch.float32)
    _launch(dev, "mdpt_post_block_norm_tiles", ptrs.ctypes.data, hw_arr.ctypes.data, n_maps, b, th, tw, tiles.data_ptr(), minmax.data_ptr())
    if cmap is None:
        return tiles, minmax
    out = torch.empty((n_maps, b, th, tw, 3), device=dev, dtype=torch.uint8)
    _launch(dev, "mdpt_post_colorize", tiles.data_ptr(), n_maps * b, th * tw, None, cmap.data_ptr(), 3, out.data_ptr())
    return out, minmax
