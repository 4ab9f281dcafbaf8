"""Locally varying true-depth alignment (not in the reference): depth completion from a relative-depth map and sparse measurements. postprocess.fit_true_depth
turns a prediction into true depth with ONE scale and shift per image, depth = 1 / (A v + B) - the right tool for a handful of known points. A measured depth map
with hundreds to millions of samples (a LiDAR sweep, a structure-from-motion point set, a cheap sensor) shows more: the error of a DPT map against the truth drifts
across the frame, and one (A, B) leaves that drift in the result however many samples were given. fit_true_depth_local fits (A, B) per cell of a grid over the
truth, pulls sparse windows towards the image's global fit, smooths the fits as the guided filter smooths its coefficients, and true_depth_local applies the
coefficient field; DPTModel.inference_completed starts from the photos. postprocess.depth_metrics(completed, truths, fit=None, space="depth") scores the result.
Kernels: csrc/post_localfit.inc (mdpt_localfit_*); the definition is written out in include/mdpt.h and restated in numpy in tests/local_align_restate.py.

Not done here: edge-aware (photo-guided) propagation of the coefficients, robust reweighting of outlier measurements, a median variant, per-node confidence maps,
temporal coherence across frames. Output quality on real photographs and real sensors is unverified: no checkpoint can be loaded where this was written; the
tests hold the definition and synthetic scenes only."""

from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np
import torch
from torch import Tensor

from . import native
from .postprocess._common import LOCALFIT_RECORD, _launch, _prediction_list, _upload_records, _views, packed_offsets, scratch_bytes
from .postprocess.align import ALIGN_SPACES, _align_choice, _truth_range, align_pairs

__all__ = ["LOCAL_GRID_HW", "LOCAL_RADIUS", "LOCAL_PRIOR", "LocalDepthFit", "fit_true_depth_local", "true_depth_local"]

# user-facing choices, not measured optima: a grid of 12 x 16 cells, windows of 3 x 3 cells, a prior worth four samples
LOCAL_GRID_HW, LOCAL_RADIUS, LOCAL_PRIOR = (12, 16), 1, 4.0


@dataclass
class LocalDepthFit:
    """What fit_true_depth_local returns, all on the device, nothing read back. coeffs: one fp64 [gh_i,gw_i,2] field {A, B} per pair (views into one allocation).
    fit: fp64 [P,2], the global (A0, B0) of every pair (what postprocess.fit_true_depth gives); sums: fp64 [P,6], the global {n, Sv, St, Svv, Svt, Stt}; moments:
    one fp64 [gh_i,gw_i,6] table per pair, the same six sums per cell (views into one allocation). grids: the (gh, gw) of every pair."""
    coeffs: list
    fit: Tensor
    sums: Tensor
    moments: list
    grids: list
    _flat: Tensor = field(repr=False, default=None)


def _grids(grid_hw, hws, what: str) -> list[tuple[int, int]]:
    """one (gh, gw) for all pairs or a list with one per pair -> a checked list"""
    def is_int(v):
        return isinstance(v, (int, np.integer)) and not isinstance(v, bool)
    if isinstance(grid_hw, (list, tuple)) and len(grid_hw) == 2 and all(is_int(v) for v in grid_hw):
        grids = [tuple(grid_hw)] * len(hws)
    elif isinstance(grid_hw, (list, tuple)) and all(isinstance(g, (list, tuple)) and len(g) == 2 and all(is_int(v) for v in g) for g in grid_hw):
        grids = [tuple(g) for g in grid_hw]
    else:
        raise ValueError(f"{what}: grid_hw must be (gh, gw) or a list of one (gh, gw) per pair, got {grid_hw!r}")
    if len(grids) != len(hws):
        raise ValueError(f"{what}: {len(hws)} pairs but {len(grids)} grids")
    cap = native.LOCALFIT_MAX_GRID
    for k, ((gh, gw), (h, w)) in enumerate(zip(grids, hws)):
        if not (1 <= gh <= min(h, cap) and 1 <= gw <= min(w, cap)):
            raise ValueError(f"{what}: grid {gh}x{gw} of pair {k} must be 1 .. {cap} cells an axis and no more than the {h}x{w} pixels of its truth")
    return [(int(gh), int(gw)) for gh, gw in grids]


def _local_checked(radius, prior, what: str) -> tuple[int, float]:
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 0 <= int(radius) <= native.LOCALFIT_MAX_RADIUS:
        raise ValueError(f"{what}: radius must be an int in 0 .. {native.LOCALFIT_MAX_RADIUS} cells, got {radius!r}")
    prior = float(prior)
    if not (prior >= 0.0 and math.isfinite(prior)):
        raise ValueError(f"{what}: prior must be finite and >= 0 pseudo-samples, got {prior}")
    return int(radius), prior


def _local_records(pair_records: np.ndarray, grids) -> tuple[np.ndarray, list[int], int]:
    """mdpt_depth_pair records + the grids -> (mdpt_localfit_pair records with cell_off filled, the cell offsets, the cells of the call)"""
    records = np.zeros(len(pair_records), dtype=LOCALFIT_RECORD)
    for name in pair_records.dtype.names:
        records[name] = pair_records[name]
    records["gh"], records["gw"] = [g[0] for g in grids], [g[1] for g in grids]
    cell_offs, cells = packed_offsets([gh * gw for gh, gw in grids])
    records["cell_off"] = cell_offs
    return records, cell_offs, cells


def fit_true_depth_local(predictions, truths, valid=None, *, space: str = "inverse", grid_hw=LOCAL_GRID_HW, radius: int = LOCAL_RADIUS, prior: float = LOCAL_PRIOR,
                         truth_range=(None, None)) -> LocalDepthFit:
    """Fit every prediction to its measured depth map with a scale A and a shift B that vary over the frame -> LocalDepthFit, on the device. predictions, truths, valid,
    space and truth_range are postprocess.fit_true_depth's, and so are the samples: one per truth pixel that holds a measurement, the prediction sampled bilinearly at
    its centre, t = 1 / truth (space="inverse") or truth ("depth"). grid_hw = (gh, gw) cells over the truth, one pair for all or a list with one per pair (1 .. 256 an
    axis, no more than the truth's pixels): truth pixel (Y, X) belongs to cell (Y gh // H, X gw // W), and every cell gets the six sums {n, Sv, St, Svv, Svt, Stt} of
    its samples. The global fit (A0, B0) comes from their total by fit_true_depth's least-squares rule. Node (j, i) is fitted to the sums of the cells within `radius`
    of it (clipped to the grid) plus `prior` pseudo-samples distributed like the image's own (prior G / n_G term by term); a window without a sample, or one the rule
    cannot use (fewer than two samples, a flat prediction, A <= 0), takes (A0, B0). The coefficient of a node is the mean of the window fits over the same window.
    prior = 0 is the pure local fit, a large prior the global fit everywhere. The defaults (12 x 16 cells, radius 1, prior 4) are user-facing choices, not
    measured optima. fp64 throughout, no atomics, bit-deterministic, every pair independent of the others; five launches whatever the number of pairs, nothing read
    back, no synchronisation. Limits: see this module's docstring."""
    what = "fit_true_depth_local"
    sp = _align_choice(ALIGN_SPACES, space, what, "space")
    tmin, tmax = _truth_range(truth_range, what)
    radius, prior = _local_checked(radius, prior, what)
    maps, pair_records, _, hws, keep = align_pairs(predictions, truths, valid, what)
    if len(maps) > 65535:
        raise ValueError(f"{what}: {len(maps)} pairs, a call takes 1 .. 65535")
    grids = _grids(grid_hw, hws, what)
    dev = maps[0].device
    records, cell_offs, cells = _local_records(pair_records, grids)
    records["scratch_off"], need = packed_offsets([scratch_bytes("mdpt_localfit_scratch_bytes", records[k:k + 1].ctypes.data, 1) for k in range(len(maps))])
    flat = torch.empty(cells * 8 + len(maps) * 8, device=dev, dtype=torch.float64)  # coefficients [cells,2], moments [cells,6], fit [P,2], sums [P,6]
    coeffs, moments = flat[:cells * 2], flat[cells * 2:cells * 8]
    fit, sums = flat[cells * 8:cells * 8 + 2 * len(maps)].view(-1, 2), flat[cells * 8 + 2 * len(maps):].view(-1, 6)
    scratch = torch.empty(need // 8, device=dev, dtype=torch.float64)
    table = _upload_records(records, dev)
    _launch(dev, "mdpt_localfit_fit", records.ctypes.data, table.data_ptr(), len(maps), native.dtype_code(maps[0].dtype), sp, radius, prior, tmin, tmax,
            moments.data_ptr(), fit.data_ptr(), sums.data_ptr(), coeffs.data_ptr(), scratch.data_ptr(), need)
    del table, scratch, keep  # (the caching allocator reuses them in stream order only)
    return LocalDepthFit([coeffs[2 * o:2 * (o + gh * gw)].view(gh, gw, 2) for o, (gh, gw) in zip(cell_offs, grids)], fit, sums,
                         [moments[6 * o:6 * (o + gh * gw)].view(gh, gw, 6) for o, (gh, gw) in zip(cell_offs, grids)], grids, flat)


def true_depth_local(predictions, local_fit: LocalDepthFit, target_hws=None, space: str = "inverse", clamp=(None, None)) -> list[Tensor]:
    """Predictions and their LocalDepthFit -> true depth maps, a list of fp32 [1,H_i,W_i] (views of one allocation). Per pixel of the target (H, W) (target_hws: one
    per prediction; None: the prediction's own size) the coefficients (A, B) are the field resampled bilinearly at the pixel's centre, v the prediction resampled
    the same way, then postprocess.true_depth's arithmetic: 1 / (A v + B) in inverse space (+inf where A v + B <= 0) or A v + B in depth space, clamped to
    clamp = (min, max) where given - one fused launch for all pairs, fp64 arithmetic rounded once; a non-finite prediction propagates."""
    what = "true_depth_local"
    if not isinstance(local_fit, LocalDepthFit):
        raise TypeError(f"{what} expects the LocalDepthFit of fit_true_depth_local, got {type(local_fit)}")
    sp = _align_choice(ALIGN_SPACES, space, what, "space")
    dmin, dmax = _truth_range(clamp, what)
    maps = _prediction_list(predictions, what)
    if len(maps) != len(local_fit.grids):
        raise ValueError(f"{what}: {len(maps)} predictions but a fit of {len(local_fit.grids)} pairs")
    dev = maps[0].device
    if local_fit._flat.device != dev:
        raise RuntimeError(f"{what}: the predictions are on {dev} but the fit is on {local_fit._flat.device}")
    if target_hws is None:
        hws = [(int(m.shape[0]), int(m.shape[1])) for m in maps]
    else:
        hws = [(int(hw[0]), int(hw[1])) for hw in target_hws]
        if len(hws) != len(maps):
            raise ValueError(f"{what}: {len(maps)} predictions but {len(hws)} target sizes")
        if any(h <= 0 or w <= 0 for h, w in hws):
            raise ValueError(f"{what}: target sizes must be positive, got {hws}")
    if any(h * w >= 2 ** 31 for h, w in hws):
        raise ValueError(f"{what}: a map of 2^31 pixels or more is not supported")
    offs, total = packed_offsets([h * w for h, w in hws])
    out = torch.empty(total, device=dev, dtype=torch.float32)
    records = np.zeros(len(maps), dtype=LOCALFIT_RECORD)
    records["pred"], records["ph"], records["pw"] = [m.data_ptr() for m in maps], [m.shape[0] for m in maps], [m.shape[1] for m in maps]
    records["H"], records["W"] = [h for h, _ in hws], [w for _, w in hws]
    records["gh"], records["gw"] = [g[0] for g in local_fit.grids], [g[1] for g in local_fit.grids]
    records["cell_off"] = packed_offsets([gh * gw for gh, gw in local_fit.grids])[0]
    records["out"] = [out.data_ptr() + 4 * o for o in offs]
    table = _upload_records(records, dev)
    _launch(dev, "mdpt_localfit_apply", records.ctypes.data, table.data_ptr(), len(maps), native.dtype_code(maps[0].dtype), sp, local_fit._flat.data_ptr(), dmin, dmax)
    del table
    return _views(out, hws)
