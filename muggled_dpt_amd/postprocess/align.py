"""Predictions aligned to measured depth maps, the standard metrics and true depth (fit_true_depth / depth_metrics / true_depth; not in the reference, which
only describes the fit; DPTModel.evaluate_depth makes the whole call); mesh_depth_range carries a fit over to the mesh. Kernels: csrc/post_align.inc."""

from __future__ import annotations

import numpy as np
import torch
from torch import Tensor

from .. import native
from ._common import PAIR_RECORD, _launch, _need_cuda, _prediction_list, _upload_records, _views, packed_offsets, ptr, scratch_bytes, upload

ALIGN_SPACES = {"inverse": native.ALIGN_INVERSE, "depth": native.ALIGN_DEPTH}
ALIGN_METHODS = {"lstsq": native.ALIGN_LSTSQ, "median": native.ALIGN_MEDIAN}
DEPTH_METRIC_NAMES = ("n", "n_bad", "abs_rel", "sq_rel", "rmse", "rmse_log", "log10", "delta1", "delta2", "delta3", "silog")
assert len(DEPTH_METRIC_NAMES) == native.ALIGN_NUM_METRICS


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
    staged, ptrs = upload([np.ascontiguousarray(m != 0 if np_dtype == np.uint8 else m, dtype=np_dtype) for m in flat], dev, 16)
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


def align_pairs(predictions, truths, valid, what: str):
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
        for k, address in zip(given, some):
            vptr[k] = address
    records = _pair_records(maps, hws, tptr, vptr)
    return maps, records, _upload_records(records, dev), hws, (keep_t, keep_v)


def _pair_records(maps: list[Tensor], hws, tptr=None, vptr=None) -> np.ndarray:
    if any(h * w >= 2 ** 31 for h, w in hws):
        raise ValueError("a map of 2^31 pixels or more is not supported")
    records = np.zeros(len(maps), dtype=PAIR_RECORD)  # (column by column, not through record_table: fit_true_depth pays this on every call)
    records["pred"] = [m.data_ptr() for m in maps]
    records["ph"], records["pw"] = [m.shape[0] for m in maps], [m.shape[1] for m in maps]
    records["H"], records["W"] = [h for h, _ in hws], [w for _, w in hws]
    if tptr is not None:
        records["truth"], records["valid"] = tptr, vptr
    return records


def _align_scratch(records: np.ndarray, dev) -> tuple[Tensor, int]:
    need = scratch_bytes("mdpt_post_align_scratch_bytes", records.ctypes.data, len(records))
    return torch.empty(max(need // 8, 1), device=dev, dtype=torch.float64), need


def fit_true_depth(predictions, truths, valid=None, space: str = "inverse", method: str = "lstsq", truth_range=(None, None), return_sums: bool = False, *, staged=None):
    """Fit every prediction to its ground truth with one scale A and one shift B -> fp64 [P,2] {A, B} on the device (not in the reference: its
    .readme_assets/results_explainer.md gives depth = 1 / (A V + B) and names both fits under "Fitting to (more) known data", without code). predictions: a [B,h,w] CUDA
    tensor or a list of [1,h,w] / [h,w] CUDA maps of one dtype and any sizes (as DPTModel.inference_images returns). truths: one measured depth map per prediction, at its
    own resolution - a batch or a list of CUDA tensors or of host arrays (staged through pinned memory); zero, negative, NaN and inf mean "no measurement". valid:
    optional maps of the truths' sizes, non-zero where the truth counts (a batch, or a list that may hold None for a pair without a mask). truth_range = (min, max) leaves
    out measurements outside it (None: no bound). One sample per truth pixel: the prediction is sampled bilinearly at the pixel's centre. space="inverse" fits A v + B to
    1 / truth (relative-depth models), "depth" to truth itself (metric heads). method="lstsq": least squares; "median": A = mad(t) / mad(v), B = med(t) - A med(v) with
    exact medians of the float32 samples (robust to outliers; MiDaS's normalisation). A pair the fit cannot use (fewer than two samples, a flat prediction, A <= 0) gets A
    = 0 and B = the mean / median of t, a pair without samples A = B = 0. fp64, bit-deterministic, 2 (lstsq) or 11 (median) launches for the whole call, nothing read
    back. return_sums: -> (fit, sums fp64 [P,6]: {n, Sv, St, Svv, Svt, Stt} or {n, med v, med t, mad v, mad t, 0}). staged: what align_pairs returned for these very
    arguments (evaluate_depth stages the truths and uploads the table once for fit and metrics)."""
    what = "fit_true_depth"
    sp, me = _align_choice(ALIGN_SPACES, space, what, "space"), _align_choice(ALIGN_METHODS, method, what, "method")
    tmin, tmax = _truth_range(truth_range, what)
    maps, records, table, _, keep = align_pairs(predictions, truths, valid, what) if staged is None else staged
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
    maps, records, table, _, keep = align_pairs(predictions, truths, valid, what) if staged is None else staged
    dev = maps[0].device
    fit = _fit_checked(fit, len(maps), dev, what)
    scratch, need = _align_scratch(records, dev)
    out = torch.empty((len(maps), native.ALIGN_NUM_METRICS), device=dev, dtype=torch.float64)
    _launch(dev, "mdpt_post_align_metrics", records.ctypes.data, table.data_ptr(), len(maps), native.dtype_code(maps[0].dtype), sp, tmin, tmax,
            ptr(fit), out.data_ptr(), scratch.data_ptr(), need)
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
    offs, total = packed_offsets([h * w for h, w in hws])
    offsets = np.asarray(offs, dtype=np.int64)
    # one upload: the records (40 bytes each, so any count of them ends 8-byte aligned) and the offsets behind them
    table, (d_records, d_offsets) = upload([records.view(np.uint8), offsets], dev)
    out = torch.empty(total, device=dev, dtype=torch.float32)
    _launch(dev, "mdpt_post_align_apply", records.ctypes.data, d_records, len(maps), native.dtype_code(maps[0].dtype), sp, ptr(fit),
            offsets.ctypes.data, d_offsets, dmin, dmax, out.data_ptr())
    del table
    if isinstance(predictions, torch.Tensor) and len(set(hws)) == 1:
        return out.view(len(maps), *hws[0])
    return _views(out, hws)


def mesh_depth_range(fit_ab, prediction_minmax) -> tuple[float, float]:
    """A fitted (A, B) of ONE image -> the (min_depth, max_depth) pair that makes depth_frames_to_mesh place its vertices at true depth. The mesh reads the 24-bit packed
    frame, V = (x - lo) / (hi - lo) with (lo, hi) = prediction_minmax, the prediction's min and max, and evaluates 1 / (V (1 / min_depth - 1 / max_depth) + 1 / max_depth)
    (relative models). True depth is 1 / (A x + B) = 1 / (V A (hi - lo) + A lo + B), so max_depth = 1 / (A lo + B) and min_depth = 1 / (A hi + B): the algebra closes
    exactly, up to the 2^-24 quantisation of V. Host-side floats (the caller reads the fit and the min / max back once). Raises where the fit puts either end at or behind
    the camera (A hi + B or A lo + B <= 0) or is degenerate (A <= 0)."""
    a, b = float(fit_ab[0]), float(fit_ab[1])
    lo, hi = float(prediction_minmax[0]), float(prediction_minmax[1])
    far, near = a * lo + b, a * hi + b
    if not (a > 0.0 and lo < hi and far > 0.0 and near > 0.0):
        raise ValueError(f"mesh_depth_range: fit A={a}, B={b} over predictions [{lo}, {hi}] has no positive depth range")
    return 1.0 / near, 1.0 / far
