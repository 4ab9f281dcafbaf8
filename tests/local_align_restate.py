"""fp64 numpy restatement of the locally varying true-depth alignment (local_align.fit_true_depth_local / true_depth_local: mdpt_localfit_*) for the tests,
written from the definition in include/mdpt.h; samples, solve rule and resampler are tests/align_restate.py's. Cell sums are math.fsum's (correctly rounded), so a
device sum in ANY order lies within n 2^-52 sum|terms| of them. `real` = the floating type of everything after the cell sums (np.float64; np.longdouble
for the tests' noise estimate); `rng` adds the cells of every window in a random order instead of dj outer, di inner, ascending."""
import math

import numpy as np

from tests import align_restate as ar


def cell_of(n_cells: int, n: int) -> np.ndarray:
    """the cell of every pixel along an axis of n pixels: X n_cells // n"""
    return (np.arange(n, dtype=np.int64) * n_cells) // n


def cell_moments(pred, truth, valid=None, space="inverse", grid=(1, 1), truth_range=(None, None)):
    """-> (M [gh, gw, 6] = {n, Sv, St, Svv, Svt, Stt} per cell, abs [gh, gw, 6] = sum |term|, the per-sample terms [6][n] and the cell index of every sample)"""
    g = np.asarray(truth, dtype=np.float32).astype(np.float64)
    H, W = g.shape
    gh, gw = grid
    v_all = ar.resample(pred, g.shape)
    lo = -np.inf if truth_range[0] is None else float(truth_range[0])
    hi = np.inf if truth_range[1] is None else float(truth_range[1])
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(g) & (g > 0.0) & (g >= lo) & (g <= hi) & np.isfinite(v_all)
    if valid is not None:
        ok &= np.asarray(valid) != 0
    cell = (cell_of(gh, H)[:, None] * gw + cell_of(gw, W)[None, :])[ok]
    v, gg = v_all[ok], g[ok]
    with np.errstate(over="ignore"):
        t = 1.0 / gg if space == "inverse" else gg.copy()
    # (the samples are align_restate.samples': the same mask in the same row-major order)
    v2, t2, _ = ar.samples(pred, truth, valid, space, truth_range)
    assert np.array_equal(v, v2) and np.array_equal(t, t2)
    terms = [np.ones_like(v), v, t, v * v, v * t, t * t]
    M, A = np.zeros((gh * gw, 6)), np.zeros((gh * gw, 6))
    for c in range(gh * gw):
        pick = cell == c
        for k in range(6):
            M[c, k] = math.fsum(terms[k][pick].tolist())
            A[c, k] = math.fsum(np.abs(terms[k][pick]).tolist())
    return M.reshape(gh, gw, 6), A.reshape(gh, gw, 6), terms, cell


def solve(s, real=np.float64):
    """the align solve rule on sums of type `real` -> (A, B, degenerate)"""
    n, sv, st, svv, svt = (real(x) for x in s[:5])
    if n == 0:
        return real(0.0), real(0.0), True
    var = n * svv - sv * sv
    with np.errstate(all="ignore"):
        a = (n * svt - sv * st) / var
    if n >= 2 and var > 0 and np.isfinite(a) and a > 0:
        return a, (st - a * sv) / n, False
    return real(0.0), st / n, True


def window(j, i, gh, gw, radius):
    """the cells of node (j, i)'s clipped window, dj outer, di inner, ascending"""
    return [(jj, ii) for jj in range(max(j - radius, 0), min(j + radius, gh - 1) + 1) for ii in range(max(i - radius, 0), min(i + radius, gw - 1) + 1)]


def branch_margin_ok(margins, rel=1e-6) -> bool:
    """no window's var or A (its numerator) within `rel` of zero relative to its terms, apart from the exactly degenerate ones (n < 2, or var == 0 exactly)"""
    return all(m["n"] < 2 or m["var"] == 0.0 or (abs(m["var"]) > rel * m["var_scale"] and abs(m["num"]) > rel * m["num_scale"]) for m in margins)


def fit_from_moments(M, radius=1, prior=4.0, real=np.float64, rng=None):
    """cell moments [gh, gw, 6] -> dict(G [6], global (A0, B0), window fits [gh, gw, 2], coeffs [gh, gw, 2], margins: per window with a sample its n, var = n Svv - Sv^2
    and num = n Svt - Sv St with the size of their terms, for the branch condition). rng: add every sum's terms in a random order."""
    gh, gw = M.shape[:2]
    M = M.astype(real)

    def total(rows):
        rows = list(rows)
        if rng is not None:
            rows = [rows[k] for k in rng.permutation(len(rows))]
        acc = np.zeros(rows[0].shape, dtype=real)
        for r in rows:
            acc = acc + r
        return acc

    G = total(M.reshape(-1, 6))
    a0, b0, _ = solve(G, real)
    wfit = np.zeros((gh, gw, 2), dtype=real)
    margins = []
    for j in range(gh):
        for i in range(gw):
            s = total(M[jj, ii] for jj, ii in window(j, i, gh, gw, radius))
            a, b = a0, b0
            if s[0] > 0:
                if prior > 0 and G[0] > 0:
                    s = s + real(prior) * (G / G[0])
                wa, wb, degenerate = solve(s, real)
                if not degenerate:
                    a, b = wa, wb
                n, sv, st, svv, svt = s[:5]
                margins.append(dict(node=(j, i), n=float(n), var=float(n * svv - sv * sv), var_scale=float(n * svv), num=float(n * svt - sv * st),
                                    num_scale=float(abs(n * svt) + abs(sv * st))))
            wfit[j, i] = (a, b)
    coeffs = np.zeros((gh, gw, 2), dtype=real)
    for j in range(gh):
        for i in range(gw):
            cells = window(j, i, gh, gw, radius)
            coeffs[j, i] = total(wfit[jj, ii] for jj, ii in cells) / real(len(cells))
    return dict(G=G, fit=(a0, b0), wfit=wfit, coeffs=coeffs, margins=margins)


def fit(pred, truth, valid=None, space="inverse", grid=(1, 1), radius=1, prior=4.0, truth_range=(None, None)):
    M, A, _, _ = cell_moments(pred, truth, valid, space, grid, truth_range)
    out = fit_from_moments(M, radius, prior)
    out["M"], out["abs"] = M, A
    return out


def field_at(coeffs, hw) -> np.ndarray:
    """the coefficient field resampled at the centre of every pixel of an hw = (H, W) map -> [H, W, 2] (align_restate.resample per coefficient)"""
    c = np.asarray(coeffs, dtype=np.float64)
    return np.stack([ar.resample(c[..., 0], hw), ar.resample(c[..., 1], hw)], axis=-1)


def apply(pred, coeffs, hw=None, space="inverse", clamp=(None, None), return_q=False):
    """true depth in fp64 (the caller rounds to float32): align_restate.apply's arithmetic with (A, B) per pixel"""
    p = np.asarray(pred, dtype=np.float64)
    hw = p.shape if hw is None else tuple(hw)
    ab = field_at(coeffs, hw)
    v = ar.resample(p, hw)
    with np.errstate(all="ignore"):
        q = ab[..., 0] * v + ab[..., 1]
        d = np.where(q <= 0.0, np.inf, 1.0 / np.where(q == 0.0, 1.0, q)) if space == "inverse" else q
    d = np.where(np.isnan(q), np.nan, d)
    if clamp[0] is not None and np.isfinite(clamp[0]):
        d = np.where(d < clamp[0], clamp[0], d)
    if clamp[1] is not None and np.isfinite(clamp[1]):
        d = np.where(d > clamp[1], clamp[1], d)
    return (d, q) if return_q else d


def drift_scene(h=96, w=128, every=8, share=0.25, seed=0, pred_hw=None):
    """The prototype's scene: a prediction v in [1, 2], a truth whose inverse is A v + B with A drifting 0.30 -> 0.50 left to right and B 0.20 -> 0.30 top to
    bottom; measurements on every `every`-th row, a `share` of that row's pixels -> (pred fp32, dense truth fp32, valid uint8)"""
    rng = np.random.default_rng(seed)
    ph, pw = pred_hw or (h, w)
    yy, xx = np.mgrid[0:ph, 0:pw]
    pred = (1.5 + 0.35 * np.sin(xx / 9.0) * np.cos(yy / 7.0) + 0.15 * rng.uniform(-1.0, 1.0, (ph, pw))).astype(np.float32)
    v = ar.resample(pred, (h, w))
    a = 0.30 + 0.20 * (np.arange(w) + 0.5) / w
    b = 0.20 + 0.10 * (np.arange(h) + 0.5) / h
    truth = (1.0 / (a[None, :] * v + b[:, None])).astype(np.float32)
    valid = np.zeros((h, w), dtype=np.uint8)
    rows = np.arange(every // 2, h, every)
    valid[rows] = rng.uniform(0.0, 1.0, (rows.size, w)) < share
    return pred, truth, valid


def abs_rel(depth, truth, mask) -> float:
    d, g = np.asarray(depth, dtype=np.float64)[mask], np.asarray(truth, dtype=np.float64)[mask]
    return float(np.mean(np.abs(d - g) / g))
