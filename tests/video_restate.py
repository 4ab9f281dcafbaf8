"""fp64 numpy restatement of the video block (muggled_dpt_amd.video: mdpt_post_video_*) for the tests, written from the definitions of
include/mdpt.h: the reweighted fit of a frame to the one before, the chain, the temporal filter, the carried display range. Sums are math.fsum's
(correctly rounded), so a device sum in ANY order lies within n 2^-52 sum|terms| of them; frames are walked by a Python loop."""
import math

import numpy as np

RUN, EXACT, CUT, START = 0, 1, 2, 3


def _fsum(x) -> float:
    return math.fsum(np.asarray(x, dtype=np.float64).ravel().tolist())


def pair_sums(x, y, before=None, c=2.0):
    """the weighted {n, Sx, Sy, Sxx, Sxy, Syy} of x = frame t, y = frame t - 1 over the pixels where both are finite -> (sums [6], sum |term| [6]);
    before = (a, b, s2) of the round before (None: round 0, weights 1)"""
    x, y = np.asarray(x, dtype=np.float64).ravel(), np.asarray(y, dtype=np.float64).ravel()
    ok = np.isfinite(x) & np.isfinite(y)
    x, y = x[ok], y[ok]
    w = np.ones_like(x)
    if before is not None:
        a, b, s2 = before
        r = (a * x + b) - y
        w = 1.0 / (1.0 + (r * r) / ((c * c) * s2))
    wx, wy = w * x, w * y
    terms = [w, wx, wy, wx * x, wx * y, wy * y]
    return np.array([_fsum(v) for v in terms]), np.array([_fsum(np.abs(v)) for v in terms])


def solve(sums, first: bool, final: bool, cut_corr: float = 0.5):
    """-> (a, b, s2, status) of one round's sums; first: n counts the samples; final: the last round (the correlation rule applies)"""
    n, sx, sy, sxx, sxy, syy = (float(v) for v in sums)
    var, cov = n * sxx - sx * sx, n * sxy - sx * sy
    with np.errstate(all="ignore"):
        a = float(np.float64(cov) / np.float64(var))
        b = float((np.float64(sy) - a * sx) / np.float64(n))
        s2 = float(np.fmax(0.0, (np.float64(syy) - a * sxy - b * sy) / np.float64(n)))
    if (first and not n >= 2.0) or not var > 0.0 or not a > 0.0 or not (math.isfinite(a) and math.isfinite(b) and math.isfinite(s2)):
        return a, b, s2, CUT
    status = EXACT if s2 <= 2.0 ** -40 * syy / n else RUN
    if final or status == EXACT:
        var_y = n * syy - sy * sy
        if not var_y > 0.0 or cov * cov < (cut_corr * cut_corr) * (var * var_y):
            status = CUT
    return a, b, s2, status


def fit_pair(x, y, rounds=3, c=2.0, cut_corr=0.5, feed=None):
    """the fit of frame x to the frame y before it -> ((a, b, s2, status), sums [rounds + 1, 6], sum |term| [rounds + 1, 6]). A kept fit (exact, cut)
    repeats its sums in the rounds left. feed [rounds + 1, 6]: another implementation's sums; round k then weights with the fit solved from
    feed[k - 1] in place of this one's own, so that each round's sums can be compared on their own."""
    sums, mags, rec, before = [], [], None, None
    for k in range(rounds + 1):
        if rec is not None and rec[3] != RUN:
            sums.append(sums[-1])
            mags.append(mags[-1])
            continue
        s, m = pair_sums(x, y, before, c)
        sums.append(s)
        mags.append(m)
        rec = solve(s if feed is None else feed[k], k == 0, k == rounds, cut_corr)
        before = rec[:3]
    return rec, np.array(sums), np.array(mags)


def chain(recs, ab=(1.0, 0.0)):
    """the records of T pairs (status START: no pair), composed in order from ab -> (table [T, 4] {A, B, sigma, cut}, the last (A, B))"""
    A, B = float(ab[0]), float(ab[1])
    table = np.zeros((len(recs), 4))
    for t, (a, b, s2, status) in enumerate(recs):
        cut = status >= CUT
        An, Bn, sg = 1.0, 0.0, 0.0
        if not cut:
            with np.errstate(all="ignore"):
                An, Bn, sg = float(np.float64(A) * a), float(np.float64(A) * b + B), float(np.float64(A) * math.sqrt(s2))
            cut = not (math.isfinite(An) and math.isfinite(Bn) and math.isfinite(sg)) or An < 2.0 ** -20 or An > 2.0 ** 20
            if cut:
                An, Bn, sg = 1.0, 0.0, 0.0
        table[t] = An, Bn, sg, float(cut)
        A, B = An, Bn
    return table, (A, B)


def fit(frames, prev=None, ab=(1.0, 0.0), rounds=3, c=2.0, cut_corr=0.5, feed=None):
    """frames [T,h,w], prev = the raw frame before frame 0 (None: frame 0 is a start) -> (table [T, 4], (A, B), sums [rounds + 1, T, 6],
    sum |term| [rounds + 1, T, 6]); feed [rounds + 1, T, 6] as for fit_pair"""
    frames = np.asarray(frames)
    T = frames.shape[0]
    recs, sums, mags = [], np.zeros((rounds + 1, T, 6)), np.zeros((rounds + 1, T, 6))
    for t in range(T):
        y = prev if t == 0 else frames[t - 1]
        if y is None:
            recs.append((1.0, 0.0, 0.0, START))
            continue
        rec, sums[:, t], mags[:, t] = fit_pair(frames[t], y, rounds, c, cut_corr, None if feed is None else np.asarray(feed)[:, t])
        recs.append(rec)
    table, ab_out = chain(recs, ab)
    return table, ab_out, sums, mags


def temporal_filter(frames, table, prev_out=None, alpha=0.3, tau=3.0) -> np.ndarray:
    """-> float32 [T,h,w]; prev_out = the float32 output before frame 0 (None: whatever, frame 0 must then be a cut)"""
    frames = np.asarray(frames)
    out = np.zeros(frames.shape, dtype=np.float32)
    o = np.zeros(frames.shape[1:], dtype=np.float32) if prev_out is None else np.asarray(prev_out, dtype=np.float32)
    for t in range(frames.shape[0]):
        A, B, sg, cut = (float(v) for v in table[t])
        p = frames[t].astype(np.float64)
        with np.errstate(all="ignore"):
            s = A * p + B
            op = o.astype(np.float64)
            d = s - op
            d2, ts2 = d * d, (tau * sg) * (tau * sg)
            den = d2 + ts2
            g = np.where(den > 0.0, d2 / np.where(den > 0.0, den, 1.0), 0.0)
            k = alpha + (1.0 - alpha) * g
            filtered = np.where(k != 1.0, (op + k * d).astype(np.float32), s.astype(np.float32))
            plain = s.astype(np.float32)
        use = np.isfinite(o) & np.isfinite(p) & (cut == 0.0)
        o = np.where(use, filtered, plain).astype(np.float32)
        out[t] = o
    return out


def display_ranges(frames, table, range_in=None, rate=0.1) -> np.ndarray:
    """frames float32 [T,H,W] at display size -> float32 [T, 2] {lo_t, hi_t}; range_in = the carried range (None: none)"""
    lo = hi = np.float32(0.0)
    have = range_in is not None
    if have:
        lo, hi = np.float32(range_in[0]), np.float32(range_in[1])
    out = np.zeros((len(frames), 2), dtype=np.float32)
    for t, f in enumerate(frames):
        m, M = np.float32(np.min(f)), np.float32(np.max(f))  # (numpy's min / max propagate a NaN, as the device's do)
        if not have or table[t][3] != 0.0 or rate == 1.0 or not all(np.isfinite(v) for v in (m, M, lo, hi)):
            lo, hi = m, M
        else:
            lo = np.float32(float(lo) + rate * (float(m) - float(lo)))
            hi = np.float32(float(hi) + rate * (float(M) - float(hi)))
        have = True
        out[t] = lo, hi
    return out


def display(frames, ranges, reverse=False, lut=None):
    """frames float32 [T,H,W] and their ranges -> (uint8 BGR [T,H,W,3], ties bool [T,H,W]). The device normalises in fp32 - (x - lo) / (hi - lo), clamped
    to [0, 1] (NaN: 0), times 255, truncated - and so does this, step by step; a value within 1e-6 of a uint8 step (1 .. 255; what clamps has no step to cross) is reported as a tie."""
    frames = np.asarray(frames, dtype=np.float32)
    q = np.zeros(frames.shape, dtype=np.uint8)
    ties = np.zeros(frames.shape, dtype=bool)
    for t, f in enumerate(frames):
        lo, hi = np.float32(ranges[t][0]), np.float32(ranges[t][1])
        with np.errstate(all="ignore"):
            v = (f - lo) / np.float32(hi - lo)
            v = np.where(np.isnan(v), np.float32(0.0), np.minimum(np.maximum(v, np.float32(0.0)), np.float32(1.0))).astype(np.float32)
            scaled = np.float32(255.0) * v
            exact = np.nan_to_num(255.0 * (f.astype(np.float64) - float(lo)) / (float(hi) - float(lo)), nan=0.5, posinf=1e9, neginf=-1e9)
        q[t] = scaled.astype(np.int32).astype(np.uint8)
        ties[t] = (np.abs(exact - np.rint(exact)) < 1e-6) & (exact > 0.5) & (exact < 255.5) & (f != hi)  # (0 and below, above 255: clamped; x == hi: exactly 1)
    if reverse:
        q = (255 - q.astype(np.int32)).astype(np.uint8)
    table = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1) if lut is None else np.asarray(lut, dtype=np.uint8).reshape(256, 3)
    return table[q], ties


# ---- the synthetic clip of the tests: a static background seen through a scale and a shift per frame, noise, and a moving block


def scene(T=12, hw=(24, 32), block=(8, 6), value=8.0, step=2, noise=0.02, seed=0):
    """-> (frames float64 [T,h,w], scales [T], shifts [T], rows: the block's rows): frame t = scale_t (background + block + noise) + shift_t,
    scale_t = exp(N(0, 0.15)), shift_t = N(0, 0.5); the background is a ramp plus a sine, the block (value 8) moves `step` pixels a frame"""
    rng = np.random.default_rng(seed)
    h, w = hw
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    background = 1.0 + 2.0 * xx / w + 1.0 * yy / h + 0.5 * np.sin(xx / 3.0) * np.cos(yy / 4.0)
    scales, shifts = np.exp(rng.normal(0.0, 0.15, T)), rng.normal(0.0, 0.5, T)
    y0 = (h - block[1]) // 2
    frames = np.zeros((T, h, w))
    for t in range(T):
        s = background + rng.normal(0.0, noise, hw)
        x0 = 2 + step * t
        assert x0 + block[0] <= w, "the block leaves the frame"
        s[y0:y0 + block[1], x0:x0 + block[0]] = value
        frames[t] = scales[t] * s + shifts[t]
    return frames, scales, shifts, slice(y0, y0 + block[1])
