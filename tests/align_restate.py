"""fp64 numpy restatement of the true-depth block (postprocess.fit_true_depth / depth_metrics / true_depth: mdpt_post_align_*) for the tests: the
sample rule, both fits, the metrics and the apply step, written from the formulas of include/mdpt.h. Sums are math.fsum's (correctly rounded), so
a device sum in ANY order lies within n 2^-52 sum|terms| of them."""
import math

import numpy as np

METRICS = 11


def sample_positions(n_out: int, n_in: int):
    """output pixel centres in the source: u = (X + 0.5) n_in / n_out - 0.5 clamped to [0, n_in - 1] -> (i0, i1, weight of i1)"""
    u = (np.arange(n_out, dtype=np.float64) + 0.5) * float(n_in) / float(n_out) - 0.5
    u = np.minimum(np.maximum(u, 0.0), float(n_in - 1))
    i0 = np.floor(u).astype(np.int64)
    return i0, np.minimum(i0 + 1, n_in - 1), u - i0


def resample(pred: np.ndarray, hw) -> np.ndarray:
    """the prediction at the centre of every pixel of an hw = (H, W) map: bilinear, fp64 weights, rows first (top and bottom rows are each
    interpolated along x, then the two along y)"""
    p = np.asarray(pred, dtype=np.float64)
    y0, y1, ay = sample_positions(hw[0], p.shape[0])
    x0, x1, ax = sample_positions(hw[1], p.shape[1])
    with np.errstate(invalid="ignore", over="ignore"):
        top = p[y0][:, x0] * (1.0 - ax) + p[y0][:, x1] * ax
        bot = p[y1][:, x0] * (1.0 - ax) + p[y1][:, x1] * ax
        return top * (1.0 - ay[:, None]) + bot * ay[:, None]


def samples(pred, truth, valid=None, space="inverse", truth_range=(None, None)):
    """-> (v, t, g) of the samples that count, in row-major truth order, fp64"""
    g = np.asarray(truth, dtype=np.float32).astype(np.float64)
    v = resample(pred, g.shape)
    lo = -np.inf if truth_range[0] is None else float(truth_range[0])
    hi = np.inf if truth_range[1] is None else float(truth_range[1])
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(g) & (g > 0.0) & (g >= lo) & (g <= hi) & np.isfinite(v)
    if valid is not None:
        ok &= np.asarray(valid) != 0
    v, g = v[ok], g[ok]
    with np.errstate(over="ignore"):
        t = 1.0 / g if space == "inverse" else g.copy()
    return v, t, g


def _fsum(x) -> float:
    return math.fsum(np.asarray(x, dtype=np.float64).tolist())


def solve(n, sv, st, svv, svt):
    """the tile fit's solve rule"""
    if n == 0:
        return 0.0, 0.0
    var = n * svv - sv * sv
    with np.errstate(all="ignore"):
        a = np.float64(n * svt - sv * st) / np.float64(var)
    if n >= 2 and var > 0 and np.isfinite(a) and a > 0:
        return float(a), float((st - a * sv) / n)
    return 0.0, st / n


def fit_lstsq(v, t):
    """-> ((A, B), sums [6], abs_terms [6]: sum |term| of every sum, for the summation-order bound)"""
    terms = [np.ones_like(v), v, t, v * v, v * t, t * t]
    sums = np.array([_fsum(x) for x in terms])
    return solve(*sums[:5]), sums, np.array([_fsum(np.abs(x)) for x in terms])


def f32_key(x) -> np.ndarray:
    """float32 -> uint32 keys whose unsigned order is the float order, -0.0 before +0.0"""
    b = np.asarray(x, dtype=np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def median32(x32: np.ndarray) -> float:
    """the exact median of float32 values: the middle order statistic, or for even n ((double)lo + (double)hi) 0.5"""
    s = np.sort(np.asarray(x32, dtype=np.float32))
    n = s.size
    return (float(s[(n - 1) // 2]) + float(s[n // 2])) * 0.5


def fit_median(v, t):
    """-> ((A, B), sums [6] = {n, med v, med t, mad v, mad t, 0}, abs_terms [2]: sum |x - med| of v and t)"""
    n = v.size
    if n == 0:
        return (0.0, 0.0), np.zeros(6), np.zeros(2)
    v32, t32 = v.astype(np.float32).astype(np.float64), t.astype(np.float32).astype(np.float64)
    mv, mt = median32(v32), median32(t32)
    dev_v, dev_t = _fsum(np.abs(v32 - mv)), _fsum(np.abs(t32 - mt))
    mad_v, mad_t = dev_v / n, dev_t / n
    a, b = 0.0, mt
    if mad_v > 0:
        cand = mad_t / mad_v
        if np.isfinite(cand) and cand > 0:
            a, b = cand, mt - cand * mv
    return (a, b), np.array([n, mv, mt, mad_v, mad_t, 0.0]), np.array([dev_v, dev_t])


def fit(pred, truth, valid=None, space="inverse", method="lstsq", truth_range=(None, None)):
    v, t, _ = samples(pred, truth, valid, space, truth_range)
    return fit_lstsq(v, t) if method == "lstsq" else fit_median(v, t)


def metric_terms(v, g, ab=(1.0, 0.0), space="inverse", log=np.log, log10=np.log10):
    """-> (n, n_bad, dict of the per-sample terms over the scored samples, q of every sample, ratio r of the scored ones)"""
    q = ab[0] * v + ab[1]
    good = q > 0.0
    qg, g = q[good], g[good]
    d = 1.0 / qg if space == "inverse" else qg
    diff = d - g
    e = log(d) - log(g)
    r = np.maximum(d / g, g / d)
    terms = dict(abs_rel=np.abs(diff) / g, sq_rel=diff * diff / g, sq=diff * diff, e2=e * e, l10=np.abs(log10(d) - log10(g)),
                 d1=(r < 1.25).astype(np.float64), d2=(r < 1.5625).astype(np.float64), d3=(r < 1.953125).astype(np.float64), e=e)
    return v.size, int(v.size - good.sum()), terms, q, r


def metrics_from_sums(n, n_bad, s) -> np.ndarray:
    out = np.full(METRICS, np.nan)
    out[0], out[1] = n, n_bad
    m = n - n_bad
    if m > 0:
        me = s["e"] / m
        out[2:] = [s["abs_rel"] / m, s["sq_rel"] / m, math.sqrt(s["sq"] / m), math.sqrt(s["e2"] / m), s["l10"] / m, s["d1"] / m, s["d2"] / m,
                   s["d3"] / m, 100.0 * math.sqrt(max(s["e2"] / m - me * me, 0.0))]
    return out


def metrics(pred, truth, ab=(1.0, 0.0), valid=None, space="inverse", truth_range=(None, None), log=np.log, log10=np.log10):
    """-> (metrics [11], abs_sums: dict of sum |term| for the summation-order bound, q, r)"""
    v, _, g = samples(pred, truth, valid, space, truth_range)
    n, n_bad, terms, q, r = metric_terms(v, g, ab, space, log, log10)
    sums = {k: _fsum(x) for k, x in terms.items()}
    return metrics_from_sums(n, n_bad, sums), {k: _fsum(np.abs(x)) for k, x in terms.items()}, q, r


def apply(pred, ab, hw=None, space="inverse", clamp=(None, None)) -> np.ndarray:
    """true depth in fp64 (the caller rounds to float32)"""
    p = np.asarray(pred, dtype=np.float64)
    v = resample(p, p.shape if hw is None else hw)
    with np.errstate(all="ignore"):
        q = ab[0] * v + ab[1]
        d = np.where(q <= 0.0, np.inf, 1.0 / np.where(q == 0.0, 1.0, q)) if space == "inverse" else q
    d = np.where(np.isnan(q), np.nan, d)
    if clamp[0] is not None and np.isfinite(clamp[0]):
        d = np.where(d < clamp[0], clamp[0], d)
    if clamp[1] is not None and np.isfinite(clamp[1]):
        d = np.where(d > clamp[1], clamp[1], d)
    return d


def ulps(a: np.ndarray, b: np.ndarray) -> int:
    """the largest distance in float32 steps between two float32 arrays; NaN must meet NaN, inf the same inf"""
    a, b = np.asarray(a, dtype=np.float32).ravel(), np.asarray(b, dtype=np.float32).ravel()
    assert np.array_equal(np.isnan(a), np.isnan(b)), "NaN positions differ"
    keep = ~np.isnan(a)
    ka, kb = f32_key(a[keep]).astype(np.int64), f32_key(b[keep]).astype(np.int64)
    return int(np.abs(ka - kb).max()) if keep.any() else 0
