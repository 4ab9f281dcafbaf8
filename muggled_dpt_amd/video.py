"""Temporally stable video depth (not in the reference: its run_video.py:348-361 normalises every frame on its own, so a clip pumps in brightness
and shimmers). The relative-depth families return each map up to a scale and a shift of its own; video_fit aligns every frame of a clip to the
frame before it, video_filter averages what is left of the noise over time, video_display shows the result with a range carried from frame to
frame. A clip of any length streams through in batches: VideoDepthState carries the chain across calls, on the device, and nothing is read back.
Kernels: csrc/post_video.inc (mdpt_post_video_*); the arithmetic is written out in include/mdpt.h.

Temporally smoothed histogram equalisation (depth_to_color's high_contrast) is out of scope: video_display has no equalisation. Output quality on
real video is unverified - no checkpoint can be loaded where this was written; the tests hold the arithmetic and synthetic scenes only."""

from __future__ import annotations

import dataclasses

import torch
from torch import Tensor

from . import native
from .postprocess._common import _batch_maps, _cmap_tensor, _launch, _need_cuda, ptr, scratch_bytes

__all__ = ["VideoDepthState", "video_fit", "video_filter", "video_display", "stabilize_video"]

FIT_ROUNDS, FIT_C, CUT_CORR = 3, 2.0, 0.5
FILTER_ALPHA, FILTER_TAU = 0.3, 3.0
RANGE_RATE = 0.1


@dataclasses.dataclass(frozen=True)
class VideoDepthState:
    """What a clip carries from one call to the next; every field is a device tensor and no function here reads one back. The functions return a
    new state and leave the one they were given as it is, so a chunk can be replayed from the state before it.
    raw [h,w] (the frames' dtype): the last raw frame (the fit's partner of the next frame 0); out fp32 [h,w]: the last filtered frame; ab fp64 [2]:
    the chain's (A, B); display_range fp32 [2]: the carried (lo, hi); started int32 [2]: {chain, display range} - 0 = nothing before."""

    raw: Tensor
    out: Tensor
    ab: Tensor
    display_range: Tensor
    started: Tensor

    @staticmethod
    def empty(hw: tuple[int, int], dtype: torch.dtype, device) -> "VideoDepthState":
        """the state before a clip's first frame: frame 0 of the next call starts the chain and the display range"""
        h, w = int(hw[0]), int(hw[1])
        return VideoDepthState(raw=torch.zeros((h, w), device=device, dtype=dtype), out=torch.zeros((h, w), device=device, dtype=torch.float32),
                               ab=torch.tensor([1.0, 0.0], device=device, dtype=torch.float64), display_range=torch.zeros(2, device=device, dtype=torch.float32),
                               started=torch.zeros(2, device=device, dtype=torch.int32))


def _state_for(x: Tensor, state, what: str) -> VideoDepthState:
    """the state a call on frames x [T,h,w] works from: `state`, checked against the frames, or the empty one"""
    if state is None:
        return VideoDepthState.empty(x.shape[1:], x.dtype, x.device)
    if not isinstance(state, VideoDepthState):
        raise TypeError(f"{what}: state must be a VideoDepthState or None, got {type(state)}")
    _need_cuda([state.raw, state.out, state.ab, state.display_range, state.started], what)
    if tuple(state.out.shape) != tuple(x.shape[1:]) or state.out.device != x.device:
        raise ValueError(f"{what}: the state is of {tuple(state.out.shape)} frames on {state.out.device}, these are {tuple(x.shape[1:])} on {x.device}")
    return state


def _check_table(table, t: int, dev, what: str) -> Tensor:
    _need_cuda([table], what)
    if table.dtype != torch.float64 or tuple(table.shape) != (t, 4) or table.device != dev:
        raise ValueError(f"{what}: the table must be video_fit's fp64 [{t}, 4] on {dev}, got {table.dtype} {tuple(table.shape)} on {table.device}")
    return table.contiguous()


def _scratch(t: int, h: int, w: int, oh: int, ow: int, dev) -> Tensor:
    return torch.empty(scratch_bytes("mdpt_post_video_scratch_bytes", t, h, w, oh, ow) // 8, device=dev, dtype=torch.float64)


def video_fit(frames: Tensor, state: VideoDepthState | None = None, rounds: int = FIT_ROUNDS, c: float = FIT_C, cut_corr: float = CUT_CORR,
              return_sums: bool = False):
    """[T,h,w] depth maps (fp32 / bf16 / fp16) -> the fp64 table [T,4] {A, B, sigma, cut} on the device: A_t P_t + B_t is frame t in the units of the
    clip's last anchor frame, sigma_t the residual scale of its fit in those units, cut = 1 where the chain re-anchors (A = 1, B = 0, sigma = 0).
    Frame t is fitted to frame t - 1, frame 0 to the state's raw last frame (no state: frame 0 is a start), by least squares reweighted `rounds`
    times (0 .. 8) with the Cauchy weight 1 / (1 + r^2 / (c s)^2), r and s the residual and its scale of the round before: a moving object drags a
    plain least-squares fit, and a smooth weight keeps the result a continuous function of the pixels. A pair is a cut when it has fewer than two
    finite samples, a flat frame, a scale <= 0, a result that is not finite, or a correlation below cut_corr (0.5: a choice for the user to make,
    not a measured optimum); so is a frame whose composed scale leaves [2^-20, 2^20].
    All T fits run as one set of 2 (rounds + 1) + 1 launches whatever T. return_sums: -> (table, sums fp64 [rounds + 1, T, 6]), every round's
    weighted {n, Sx, Sy, Sxx, Sxy, Syy}. The state is not changed; stabilize_video returns the next one."""
    _check_fit_args(rounds, c, cut_corr)
    table, _, sums = _fit(_batch_maps(frames, "video_fit"), state, rounds, c, cut_corr, return_sums)
    return (table, sums) if return_sums else table


def _check_fit_args(rounds, c, cut_corr, what: str = "video_fit") -> None:
    if isinstance(rounds, bool) or not isinstance(rounds, int) or not 0 <= rounds <= 8:
        raise ValueError(f"{what}: rounds must be an integer 0 .. 8, got {rounds!r}")
    if not (float(c) > 0.0 and float(c) < float("inf")):
        raise ValueError(f"{what}: c must be finite and > 0, got {c!r}")
    if not 0.0 <= float(cut_corr) <= 1.0:
        raise ValueError(f"{what}: cut_corr must be in [0, 1], got {cut_corr!r}")


def _check_filter_args(alpha, tau, what: str = "video_filter") -> None:
    if not 0.0 < float(alpha) <= 1.0:
        raise ValueError(f"{what}: alpha must be in (0, 1], got {alpha!r}")
    if not (float(tau) >= 0.0 and float(tau) < float("inf")):
        raise ValueError(f"{what}: tau must be finite and >= 0, got {tau!r}")


def _fit(x: Tensor, state, rounds, c, cut_corr, return_sums):
    what = "video_fit"
    st = _state_for(x, state, what)
    if st.raw.dtype != x.dtype:
        raise ValueError(f"{what}: the state holds a {st.raw.dtype} frame, these are {x.dtype}")
    t, h, w = x.shape
    dev = x.device
    table = torch.empty((t, 4), device=dev, dtype=torch.float64)
    ab = torch.empty(2, device=dev, dtype=torch.float64)
    sums = torch.empty((rounds + 1, t, 6), device=dev, dtype=torch.float64) if return_sums else None
    scratch = _scratch(t, h, w, 0, 0, dev)
    _launch(dev, "mdpt_post_video_fit", x.data_ptr(), native.dtype_code(x.dtype), t, h, w, st.raw.contiguous().data_ptr(), st.ab.data_ptr(),
            st.started.data_ptr(), rounds, float(c), float(cut_corr), table.data_ptr(), ab.data_ptr(), ptr(sums), scratch.data_ptr(), scratch.numel() * 8)
    return table, ab, sums


def video_filter(frames: Tensor, table: Tensor, state: VideoDepthState | None = None, alpha: float = FILTER_ALPHA, tau: float = FILTER_TAU) -> Tensor:
    """[T,h,w] depth maps and their video_fit table -> fp32 [T,h,w], aligned and filtered over time. Per pixel, in frame order, from the state's last
    output: s = A_t p + B_t, d = s - o_prev, g = d^2 / (d^2 + (tau sigma_t)^2), o = o_prev + (alpha + (1 - alpha) g) d in fp64, rounded once to fp32.
    Differences well below tau sigma (noise) are averaged with weight alpha, differences well above it (motion) pass through; at a start or a cut,
    and where o_prev or p is not finite, o = s (a pixel that is not finite passes through and restarts on the next frame); alpha = 1: o = s
    throughout, alignment only. alpha in (0, 1] and tau >= 0 are choices for the user. One launch: parallel over pixels, the frames in order
    inside each thread."""
    _check_filter_args(alpha, tau)
    x = _batch_maps(frames, "video_filter")
    st = _state_for(x, state, "video_filter")
    t, h, w = x.shape
    tab = _check_table(table, t, x.device, "video_filter")
    out = torch.empty((t, h, w), device=x.device, dtype=torch.float32)
    _launch(x.device, "mdpt_post_video_filter", x.data_ptr(), native.dtype_code(x.dtype), t, h, w, tab.data_ptr(), st.out.contiguous().data_ptr(), float(alpha),
            float(tau), out.data_ptr())
    return out


def video_display(stable: Tensor, table: Tensor, state: VideoDepthState | None = None, target_wh: tuple[int, int] | None = None, reverse: bool = False,
                  lut=None, range_rate: float = RANGE_RATE):
    """fp32 [T,h,w] stabilised maps -> (uint8 [T,H,W,3] BGR display frames, the state with the new display range): postprocess.depth_to_color
    without equalisation (optional bilinear resize to target_wh, uint8, 255 - x, colormap; gray when lut is None), normalised by a carried range in
    place of each frame's own min / max: lo_t = lo_{t-1} + range_rate (m_t - lo_{t-1}), hi alike, m_t / M_t the frame's min / max; the frame's own
    at a start or a cut (the table's flag) and without a range in the state; values outside the range clamp to 0 / 255. range_rate in (0, 1]
    (0.1: a choice for the user); 1 takes every frame's own min / max, and the frames then equal depth_to_color(stable, target_wh, reverse, False,
    lut) bit for bit. Four launches, three of them depth_to_color's own kernels. No histogram equalisation (high_contrast): smoothing it over time
    is out of scope."""
    what = "video_display"
    if not 0.0 < float(range_rate) <= 1.0:
        raise ValueError(f"{what}: range_rate must be in (0, 1], got {range_rate!r}")
    if target_wh is not None and (int(target_wh[0]) <= 0 or int(target_wh[1]) <= 0):
        raise ValueError(f"{what}: target_wh must be positive, got {target_wh}")
    _need_cuda([stable], what)
    if stable.dim() != 3 or stable.dtype != torch.float32 or stable.numel() == 0:
        raise ValueError(f"{what} expects video_filter's fp32 [T,h,w], got {stable.dtype} {tuple(stable.shape)}")
    x = stable.detach().contiguous()
    st = _state_for(x, state, what)
    dev = x.device
    t, h, w = x.shape
    tab = _check_table(table, t, dev, what)
    cmap = _cmap_tensor(lut, dev)
    oh, ow = (0, 0) if target_wh is None else (int(target_wh[1]), int(target_wh[0]))
    out = torch.empty((t, oh or h, ow or w, 3), device=dev, dtype=torch.uint8)
    new_range = torch.empty(2, device=dev, dtype=torch.float32)
    scratch = _scratch(t, h, w, oh, ow, dev)
    _launch(dev, "mdpt_post_video_display", x.data_ptr(), t, h, w, tab.data_ptr(), st.display_range.data_ptr(), st.started.data_ptr() + 4, oh, ow,
            int(bool(reverse)), ptr(cmap), float(range_rate), out.data_ptr(), None, new_range.data_ptr(), scratch.data_ptr(), scratch.numel() * 8)
    started = st.started.clone()
    started[1] = 1
    return out, dataclasses.replace(st, display_range=new_range, started=started)


def stabilize_video(frames: Tensor, state: VideoDepthState | None = None, rounds: int = FIT_ROUNDS, c: float = FIT_C, cut_corr: float = CUT_CORR,
                    alpha: float = FILTER_ALPHA, tau: float = FILTER_TAU):
    """video_fit + video_filter on one batch of a clip -> (stable fp32 [T,h,w], table fp64 [T,4], the state for the next batch). Feeding a clip in
    batches of any sizes gives the bits of feeding it whole. The state passed in is not changed (a batch can be replayed from it); the display
    range it carries goes through as it is - video_display returns the state that advances it:

        state = None
        for batch in batches:                       # [T,h,w] maps, e.g. DPTModel.inference_batch's
            stable, table, state = stabilize_video(batch, state)
            bgr, state = video_display(stable, table, state, target_wh=(1920, 1080), lut=lut)
    """
    _check_fit_args(rounds, c, cut_corr, "stabilize_video")
    _check_filter_args(alpha, tau, "stabilize_video")
    x = _batch_maps(frames, "stabilize_video")
    st = _state_for(x, state, "stabilize_video")
    table, ab, _ = _fit(x, st, rounds, c, cut_corr, False)
    stable = video_filter(x, table, st, alpha, tau)
    started = st.started.clone()
    started[0] = 1
    return stable, table, VideoDepthState(raw=x[-1].clone(), out=stable[-1].clone(), ab=ab, display_range=st.display_range, started=started)
