"""postprocess.fit_true_depth / depth_metrics / true_depth (mdpt_post_align_*) against the fp64 restatement tests/align_restate.py.

Inputs: predictions are uniform in [1, 2] rounded to the dtype; a truth pixel is 1 / (0.37 v + 0.25 + e), v the prediction at the pixel (the
restatement's sampling, used here only to BUILD inputs), e ~ N(0, 0.01), stored as float32 - so t = 1 / truth = 0.37 v + 0.25 + e and the
cancellation in var = n Svv - Sv^2 is about 28 x (mean of v^2 2.33 against its variance 1 / 12). About 30 % of the truth pixels are zero, NaN or
masked off, a few predictions are NaN or inf. One call holds an enlarging pair (13 x 10 -> 37 x 29), a reducing one (16 x 12 -> 9 x 7), a truth
of 50 x 47 = 2350 valid pixels (two chunks of 2048), pairs with no and with one sample, a constant prediction, a prediction on both sides of zero,
and pairs with an even and an odd count. The median call adds four-sample pairs whose two middle values lie on either side of every digit boundary
of the 32-bit keys (bits 8, 16, 24 and the sign: -0.0 / +0.0), so the select's two rank tracks part at every pass; bf16 predictions tie heavily.

Bounds. Counts are exact. Sums against math.fsum's within n 2^-52 sum|terms|, the worst case of ANY summation order. A and B within 1e-9 relative:
the tolerance the tile fit holds for this solve on this evidence (random reorderings of the fp64 sums moved scale and shift by at most 1.1e-12 on a
CPU over 200 trials with n <= 4096, at the same 28 x cancellation; n <= 2350 here). Medians bit-equal: both sides take exact order statistics
of bit-identical IEEE samples. The arithmetic metrics (AbsRel, SqRel, RMSE, the deltas) under the summation-order bound of their sums, carried
through the division and the square root. The log metrics (RMSE-log, log10, SILog) at a relative bound derived on the CPU, never from the device:
every log / log10 result of the restatement is moved by +-2 fp64 ulp (the device's log need not be correctly rounded) - all up for d and down for g,
the reverse, and random signs - and the bound is 4 x the largest relative movement of the three metrics over the cases of this file that share a
fit (the restatement's own, or the shifted one, where q comes close to zero). Measured on a CPU: largest movement 4.8e-15 with the own fit, bound
1.9e-14; 8.3e-12 with the shifted fit, bound 3.3e-11; the test recomputes both and uses the recomputed bound. The
conditions the counts need are asserted on the CPU when a case is built: no ratio max(d / g, g / d) within 1e-9 relative of a delta threshold, no
q = A v + B within 1e-12 of zero. True depth within one fp32 ulp of float32(the restatement): the device computes in fp64 and rounds once, one ulp
covers a last-bit difference of the fp64 value at a rounding tie; judged with the device's own fit fed to the restatement and with the
restatement's fit (fit error 1e-9 is far below an fp32 ulp of 6e-8: still one ulp, at ties only)."""
import functools

import numpy as np
import pytest
import torch

from muggled_dpt_amd import postprocess as pp
from tests import align_restate as ar

pytestmark = pytest.mark.gpu

DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
A0, B0, NOISE = 0.37, 0.25, 0.01


def _round(x: np.ndarray, dtype) -> np.ndarray:
    """the values as the dtype stores them, as float32"""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dtype).float().numpy()


def _key_floats(keys) -> np.ndarray:
    k = np.asarray(keys, dtype=np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def _pair(rng, dtype, phw, thw, invalid=0.3, lo=1.0, hi=2.0, const=None, keep=None, spoil=None):
    """-> (pred, truth, valid): keep = exactly this many measurements stay (the rest zero); spoil = 'nan' / 'inf': one prediction pixel"""
    pred = np.full(phw, const, dtype=np.float64) if const is not None else rng.uniform(lo, hi, phw)
    pred = _round(pred, dtype)
    if spoil:
        pred[phw[0] // 2, phw[1] // 2] = np.nan if spoil == "nan" else np.inf
    v = ar.resample(np.where(np.isfinite(pred), pred, 1.5), thw)
    truth = (1.0 / (A0 * v + B0 + rng.normal(0.0, NOISE, thw))).astype(np.float32)
    valid = np.ones(thw, dtype=np.uint8)
    if keep is not None:
        off = rng.permutation(truth.size)[keep:]
        truth.reshape(-1)[off] = 0.0
    elif invalid > 0:
        kind = rng.uniform(0.0, 1.0, thw)
        truth[kind < invalid / 3] = 0.0
        truth[(kind >= invalid / 3) & (kind < 2 * invalid / 3)] = np.nan
        valid[(kind >= 2 * invalid / 3) & (kind < invalid)] = 0
    return pred, truth, valid


@functools.lru_cache(maxsize=None)
def _case(dt: str, method: str):
    """-> dict(preds, truths, valids: float32 / uint8 arrays, names, ref: per pair the restatement's ((A, B), sums, abs_terms))"""
    dtype = DTYPES[dt]
    rng = np.random.default_rng(7)
    pairs = {
        "up": _pair(rng, dtype, (13, 10), (37, 29), spoil="nan"),
        "down": _pair(rng, dtype, (16, 12), (9, 7), spoil="inf"),
        "two_chunks": _pair(rng, dtype, (13, 10), (50, 47), invalid=0.0),
        "none": _pair(rng, dtype, (5, 6), (8, 9), keep=0),
        "one": _pair(rng, dtype, (5, 6), (8, 9), keep=1),
        "constant": _pair(rng, dtype, (6, 5), (12, 11), const=1.5),
        "signs": _pair(rng, dtype, (9, 8), (20, 21), lo=-0.5, hi=1.5),
        "even": _pair(rng, dtype, (7, 7), (11, 13), keep=40),
        "odd": _pair(rng, dtype, (7, 7), (11, 13), keep=41),
    }
    if method == "median":
        # the two middle keys of four samples on either side of a digit boundary; truth at the prediction's size, so v = pred exactly
        for name, b in (("bit8", 0xBF800100), ("bit16", 0xBF810000), ("bit24", 0xBF000000), ("sign", None)):
            four = _key_floats([b - 2, b - 1, b, b + 1]) if b else np.array([-1e-3, -0.0, 0.0, 1e-3], dtype=np.float32)
            pred = _round(four.reshape(2, 2), dtype)
            truth = (1.0 / (A0 * np.array([[1.0, 1.3], [1.6, 1.9]]) + B0)).astype(np.float32)
            pairs[name] = (pred, truth, np.ones((2, 2), dtype=np.uint8))
    case = dict(names=list(pairs), preds=[p[0] for p in pairs.values()], truths=[p[1] for p in pairs.values()], valids=[p[2] for p in pairs.values()],
                dtype=dtype)
    case["ref"] = [ar.fit(p, t, m, method=method) for p, t, m in zip(case["preds"], case["truths"], case["valids"])]
    for a in case["preds"] + case["truths"] + case["valids"]:
        a.setflags(write=False)
    n = {k: r[1][0] for k, r in zip(case["names"], case["ref"])}
    assert n["two_chunks"] == 2350 and n["none"] == 0 and n["one"] == 1 and n["even"] == 40 and n["odd"] == 41 and 0.55 < n["up"] / (37 * 29) < 0.8
    return case


def _dev_preds(case, idx=None):
    idx = range(len(case["preds"])) if idx is None else idx
    return [torch.from_numpy(np.array(case["preds"][i])).to(case["dtype"]).cuda()[None] for i in idx]


def _sel(case, key, idx=None):
    return [case[key][i] for i in (range(len(case["preds"])) if idx is None else idx)]


def _fit(case, method, idx=None, **kw):
    fit, sums = pp.fit_true_depth(_dev_preds(case, idx), _sel(case, "truths", idx), _sel(case, "valids", idx), method=method, return_sums=True, **kw)
    assert fit.dtype == sums.dtype == torch.float64 and fit.is_cuda
    return fit.cpu().numpy(), sums.cpu().numpy()


@pytest.mark.parametrize("dt", list(DTYPES))
def test_least_squares_fit_against_the_restatement(dt):
    case = _case(dt, "lstsq")
    fit, sums = _fit(case, "lstsq")
    ref_fit = np.array([r[0] for r in case["ref"]])
    ref_sums, abs_terms = np.array([r[1] for r in case["ref"]]), np.array([r[2] for r in case["ref"]])
    assert np.array_equal(sums[:, 0], ref_sums[:, 0])
    err, bound = np.abs(sums - ref_sums), ref_sums[:, :1] * 2.0 ** -52 * abs_terms
    print(f"{dt}: sums err / bound max {np.max(err / np.maximum(bound, 1e-300)):.3g}")
    assert np.all(err <= bound)
    rel = np.abs(fit - ref_fit) / np.maximum(np.abs(ref_fit), 1e-300)
    print(f"{dt}: fit rel err max {rel.max():.3g}; A {dict(zip(case['names'], np.round(ref_fit[:, 0], 4)))}")
    assert np.all(np.abs(fit - ref_fit) <= 1e-9 * np.abs(ref_fit))
    by = dict(zip(case["names"], ref_fit))
    assert by["none"].tolist() == [0.0, 0.0] and by["one"][0] == 0.0 and by["constant"][0] == 0.0 and by["constant"][1] > 0
    for name in ("up", "down", "two_chunks", "signs", "even", "odd"):
        assert abs(by[name][0] - A0) < 0.05 and abs(by[name][1] - B0) < 0.05, name


@pytest.mark.parametrize("dt", list(DTYPES))
def test_median_fit_against_the_restatement(dt):
    case = _case(dt, "median")
    fit, sums = _fit(case, "median")
    ref_fit = np.array([r[0] for r in case["ref"]])
    ref_sums, dev_terms = np.array([r[1] for r in case["ref"]]), np.array([r[2] for r in case["ref"]])
    # n and both medians bit for bit (-0.0 == +0.0 would pass array_equal: compare the bits)
    assert np.array_equal(sums[:, :3].view(np.uint64), ref_sums[:, :3].view(np.uint64)), (sums[:, :3], ref_sums[:, :3])
    assert np.all(sums[:, 5] == 0.0)
    # mad = S / n: S under the summation-order bound, then one division
    n = np.maximum(ref_sums[:, :1], 1.0)
    err, bound = np.abs(sums[:, 3:5] - ref_sums[:, 3:5]), (n * 2.0 ** -52 * dev_terms) / n + 2.0 ** -52 * ref_sums[:, 3:5]
    print(f"{dt}: mad err / bound max {np.max(err / np.maximum(bound, 1e-300)):.3g}")
    assert np.all(err <= bound)
    rel = np.abs(fit - ref_fit) / np.maximum(np.abs(ref_fit), 1e-300)
    print(f"{dt}: median fit rel err max {rel.max():.3g}; A {dict(zip(case['names'], np.round(ref_fit[:, 0], 4)))}")
    assert np.all(np.abs(fit - ref_fit) <= 1e-9 * np.abs(ref_fit))
    by = dict(zip(case["names"], ref_fit))
    assert by["none"].tolist() == [0.0, 0.0] and by["one"][0] == 0.0 and by["constant"][0] == 0.0
    assert abs(by["two_chunks"][0] - A0) < 0.05 and abs(by["two_chunks"][1] - B0) < 0.05
    if dt == "fp32":  # the middle keys straddle the boundary: the median lies between two float32 neighbours
        k = case["names"].index("bit16")
        lo, hi = _key_floats([0xBF810000 - 1, 0xBF810000])
        assert sums[k, 1] == (float(lo) + float(hi)) * 0.5 and np.float32(sums[k, 1]) != sums[k, 1]
        k = case["names"].index("sign")
        assert sums[k, 1] == 0.0 and not np.signbit(sums[k, 1])


def test_median_of_the_truth_stream_parts_its_tracks_at_every_digit_boundary():
    """The digit pairs of the median case straddle the boundaries in the v stream; here the t stream does (depth space: t = truth, float32 as
    given), in one call with a pair whose valid entry is None. Bit-equal medians, A and B within 1e-9."""
    preds, truths = [], []
    for b in (0xBF800100, 0xBF810000, 0xBF000000):
        preds.append(np.array([[1.0, 1.3], [1.6, 1.9]], dtype=np.float32))
        truths.append(_key_floats([b - 2, b - 1, b, b + 1]).reshape(2, 2).copy())
    valids = [np.ones((2, 2), dtype=np.uint8), None, np.ones((2, 2), dtype=np.uint8)]
    ref = [ar.fit(p, t, space="depth", method="median") for p, t in zip(preds, truths)]
    fit, sums = pp.fit_true_depth([torch.from_numpy(p).cuda() for p in preds], truths, valids, space="depth", method="median", return_sums=True)
    fit, sums = fit.cpu().numpy(), sums.cpu().numpy()
    ref_fit, ref_sums = np.array([r[0] for r in ref]), np.array([r[1] for r in ref])
    assert np.array_equal(sums[:, :3].view(np.uint64), ref_sums[:, :3].view(np.uint64)), (sums, ref_sums)
    for k, b in enumerate((0xBF800100, 0xBF810000, 0xBF000000)):
        lo, hi = _key_floats([b - 1, b])
        assert sums[k, 2] == (float(lo) + float(hi)) * 0.5 and np.float32(sums[k, 2]) != sums[k, 2]
    assert np.all(np.abs(sums[:, 3:5] - ref_sums[:, 3:5]) <= 2.0 ** -51 * ref_sums[:, 3:5])  # (four exact terms, one division)
    assert np.all(ref_fit[:, 0] > 0) and np.all(np.abs(fit - ref_fit) <= 1e-9 * np.abs(ref_fit))
    # a mask on one pair only: the others are untouched, bit for bit
    valids = [None, np.array([[1, 1], [1, 0]], dtype=np.uint8), None]
    f2, s2 = pp.fit_true_depth([torch.from_numpy(p).cuda() for p in preds], truths, valids, space="depth", method="median", return_sums=True)
    s2 = s2.cpu().numpy()
    assert s2[1, 0] == 3 and np.array_equal(s2[[0, 2]].view(np.uint64), sums[[0, 2]].view(np.uint64))


class _MovedLog:
    """np.log / np.log10 with every result moved by +-2 ulp: signs = +1 / -1 per call in turn, or None for random signs"""

    def __init__(self, fn, signs, seed=0):
        self.fn, self.signs, self.calls, self.rng = fn, signs, 0, np.random.default_rng(seed)

    def __call__(self, x):
        y = self.fn(x)
        s = self.rng.choice([-1.0, 1.0], y.shape) if self.signs is None else self.signs[self.calls % len(self.signs)]
        self.calls += 1
        return y + s * 2.0 * np.spacing(np.abs(y))


LOG_COLUMNS = (5, 6, 10)  # RMSE-log, log10, SILog


def _metric_inputs(case, which):
    """the fit the metrics are evaluated with: the restatement's own, or one shifted so that part of the samples get q <= 0"""
    fits = np.array([r[0] for r in case["ref"]])
    if which == "shifted":
        fits = fits - np.array([0.0, 0.75])
    return fits


@functools.lru_cache(maxsize=None)
def _metric_refs(dt, which):
    """-> (fits, ref metrics [P, 11], abs_sums per pair, the largest relative movement of the log metrics under +-2 ulp of every log); asserts the
    conditions on the inputs that make the counts exact"""
    case = _case(dt, "lstsq")
    fits = _metric_inputs(case, which)
    refs, sums_abs, moved = [], [], 0.0
    for p, t, m, ab in zip(case["preds"], case["truths"], case["valids"], fits):
        ref, abs_sums, q, r = ar.metrics(p, t, tuple(ab), m)
        assert q.size == 0 or np.min(np.abs(q)) > 1e-12, "a q within 1e-12 of zero"
        for thr in (1.25, 1.5625, 1.953125):
            assert r.size == 0 or np.min(np.abs(r / thr - 1.0)) > 1e-9, "a ratio within 1e-9 of a delta threshold"
        for signs in ((1.0, -1.0), (-1.0, 1.0), None):
            alt = ar.metrics(p, t, tuple(ab), m, log=_MovedLog(np.log, signs, 1), log10=_MovedLog(np.log10, signs, 2))[0]
            for c in LOG_COLUMNS:
                if np.isfinite(ref[c]) and ref[c] != 0.0:
                    moved = max(moved, abs(alt[c] - ref[c]) / abs(ref[c]))
        refs.append(ref)
        sums_abs.append(abs_sums)
    return fits, np.array(refs), sums_abs, moved


def _metrics(case, fits, idx=None, **kw):
    fit = None if fits is None else torch.from_numpy(np.ascontiguousarray(fits[list(idx)] if idx is not None else fits)).cuda()
    out = pp.depth_metrics(_dev_preds(case, idx), _sel(case, "truths", idx), fit, _sel(case, "valids", idx), **kw)
    assert out.dtype == torch.float64 and out.shape[1] == 11
    return out.cpu().numpy()


@pytest.mark.parametrize("which", ["own", "shifted"])
@pytest.mark.parametrize("dt", list(DTYPES))
def test_metrics_against_the_restatement(dt, which):
    case = _case(dt, "lstsq")
    fits, ref, sums_abs, _ = _metric_refs(dt, which)
    moved = max(_metric_refs(d, which)[3] for d in DTYPES)  # (per fit: the shifted fit's q near zero must not loosen the own fit's bound)
    log_bound = 4.0 * moved
    print(f"{dt} {which}: largest movement of a log metric under +-2 ulp logs {moved:.3g}, bound {log_bound:.3g}")
    assert 0.0 < log_bound < 1e-10
    got = _metrics(case, fits)
    assert np.array_equal(got[:, :2], ref[:, :2])
    if which == "shifted":
        assert ref[:, 1].max() > 100 and np.any((ref[:, 1] > 0) & (ref[:, 1] < ref[:, 0]))
    for k, name in enumerate(case["names"]):
        m = ref[k, 0] - ref[k, 1]
        if m == 0:
            assert np.isnan(got[k, 2:]).all() and np.isnan(ref[k, 2:]).all(), name
            continue
        eps = m * 2.0 ** -52
        s = sums_abs[k]
        # means: the sum's bound over m, plus the division's rounding; RMSE = sqrt(mean): half the relative bound, plus the root's rounding
        for c, key in ((2, "abs_rel"), (3, "sq_rel"), (7, "d1"), (8, "d2"), (9, "d3")):
            assert abs(got[k, c] - ref[k, c]) <= eps * s[key] / m + 2.0 ** -52 * abs(ref[k, c]), (name, key, got[k, c], ref[k, c])
        assert got[k, 7] == ref[k, 7] and got[k, 8] == ref[k, 8] and got[k, 9] == ref[k, 9], name  # (integer numerators: exact)
        assert abs(got[k, 4] - ref[k, 4]) <= (0.5 * eps + 2.0 ** -51) * ref[k, 4], (name, "rmse")
        for c in LOG_COLUMNS:
            err = abs(got[k, c] - ref[k, c])
            print(f"  {name} col {c}: ref {ref[k, c]:.6g} rel err {err / max(abs(ref[k, c]), 1e-300):.3g}")
            assert err <= log_bound * abs(ref[k, c]), (name, c, got[k, c], ref[k, c])
    # fit=None is A = 1, B = 0
    ones = np.tile(np.array([1.0, 0.0]), (len(case["names"]), 1))
    assert np.array_equal(_metrics(case, None), _metrics(case, ones), equal_nan=True)


@pytest.mark.parametrize("dt", list(DTYPES))
def test_true_depth_within_one_ulp(dt):
    case = _case(dt, "lstsq")
    ref_fit = np.array([r[0] for r in case["ref"]])
    fit_dev = pp.fit_true_depth(_dev_preds(case), case["truths"], case["valids"])
    hws = [t.shape for t in case["truths"]]
    for kw in (dict(), dict(clamp=(1.2, 1.9)), dict(space="depth", clamp=(None, 0.9))):
        outs = pp.true_depth(_dev_preds(case), fit_dev, hws, **kw)
        assert len({o.untyped_storage().data_ptr() for o in outs}) == 1
        for k, (name, o) in enumerate(zip(case["names"], outs)):
            assert o.shape == (1, *hws[k]) and o.dtype == torch.float32
            for ab in (fit_dev[k].cpu().numpy(), ref_fit[k]):
                want = ar.apply(case["preds"][k], tuple(ab), hws[k], **kw).astype(np.float32)
                assert ar.ulps(o[0].cpu().numpy(), want) <= 1, (name, kw)
    outs = pp.true_depth(_dev_preds(case), fit_dev, hws)
    by = dict(zip(case["names"], outs))
    assert torch.isnan(by["up"]).any() and torch.isinf(by["none"]).all()  # a NaN prediction propagates; A = B = 0: q = 0 -> +inf
    # the default target is the prediction's own size, where the resize is the identity
    own = pp.true_depth(_dev_preds(case), fit_dev)
    k = case["names"].index("two_chunks")
    want = (1.0 / (fit_dev[k, 0].item() * case["preds"][k].astype(np.float64) + fit_dev[k, 1].item())).astype(np.float32)
    assert ar.ulps(own[k][0].cpu().numpy(), want) <= 1


@pytest.mark.parametrize("method", ["lstsq", "median"])
def test_pairs_are_independent_and_runs_repeat_bit_for_bit(method):
    case = _case("bf16", method)
    fit, sums = _fit(case, method)
    again = _fit(case, method)
    assert np.array_equal(fit.view(np.uint64), again[0].view(np.uint64)) and np.array_equal(sums.view(np.uint64), again[1].view(np.uint64))
    fits = np.array([r[0] for r in case["ref"]])
    met = _metrics(case, fits)
    assert np.array_equal(met, _metrics(case, fits), equal_nan=True)
    hws = [t.shape for t in case["truths"]]
    fit_dev = torch.from_numpy(fits).cuda()
    maps = pp.true_depth(_dev_preds(case), fit_dev, hws)
    for k, name in enumerate(case["names"]):
        f1, s1 = _fit(case, method, [k])
        assert np.array_equal(f1.view(np.uint64), fit[k:k + 1].view(np.uint64)) and np.array_equal(s1.view(np.uint64), sums[k:k + 1].view(np.uint64)), name
        assert np.array_equal(_metrics(case, fits, [k]), met[k:k + 1], equal_nan=True), name
        alone = pp.true_depth(_dev_preds(case, [k]), fit_dev[k:k + 1], [hws[k]])[0]
        assert torch.equal(alone.view(torch.int32), maps[k].view(torch.int32)), name
    # reversed order: every pair keeps its results
    rev = list(range(len(case["names"])))[::-1]
    f2, s2 = _fit(case, method, rev)
    assert np.array_equal(f2[::-1].view(np.uint64), fit.view(np.uint64)) and np.array_equal(s2[::-1].view(np.uint64), sums.view(np.uint64))


@pytest.mark.parametrize("method", ["lstsq", "median"])
def test_batch_input_equals_list_input(method):
    rng = np.random.default_rng(3)
    trip = [_pair(rng, torch.float16, (9, 8), (20, 21)) for _ in range(3)]
    preds = torch.from_numpy(np.stack([t[0] for t in trip])).to(torch.float16).cuda()
    truths = torch.from_numpy(np.stack([t[1] for t in trip])).cuda()
    valid = torch.from_numpy(np.stack([t[2] for t in trip])).cuda()
    for v_batch, v_list in ((valid, [t[2] for t in trip]), (None, None)):
        a = pp.fit_true_depth(preds, truths, v_batch, method=method, return_sums=True)
        b = pp.fit_true_depth([p[None] for p in preds], [t[1] for t in trip], v_list, method=method, return_sums=True)  # device maps, host truths
        assert torch.equal(a[0].view(torch.int64), b[0].view(torch.int64)) and torch.equal(a[1].view(torch.int64), b[1].view(torch.int64))
        ma = pp.depth_metrics(preds, truths, a[0], v_batch)
        mb = pp.depth_metrics(list(preds), list(truths), a[0], None if v_batch is None else list(valid.bool()))
        assert torch.equal(ma.view(torch.int64), mb.view(torch.int64))
    da = pp.true_depth(preds, a[0], [(20, 21)] * 3)
    db = pp.true_depth(list(preds), a[0], [(20, 21)] * 3)
    assert da.shape == (3, 20, 21) and isinstance(db, list) and torch.equal(da, torch.cat(db))
    # truth_range leaves out what a mask leaves out
    lo, hi = 0.9, 1.3
    t_np = np.stack([t[1] for t in trip])
    inside = (t_np >= lo) & (t_np <= hi)
    c = pp.fit_true_depth(preds, truths, method=method, truth_range=(lo, hi), return_sums=True)
    d = pp.fit_true_depth(preds, truths, torch.from_numpy(inside).cuda(), method=method, return_sums=True)
    assert torch.equal(c[0].view(torch.int64), d[0].view(torch.int64)) and torch.equal(c[1].view(torch.int64), d[1].view(torch.int64))
    assert 0 < c[1][0, 0].item() < a[1][0, 0].item()


def test_evaluate_depth_is_inference_images_plus_the_three_calls():
    from muggled_dpt_amd import make_depthanythingv2_dpt_from_original_state_dict as make
    from tests.helpers import synthetic_model
    model = make(synthetic_model("tiny")[0])[1].to("cuda", torch.bfloat16)
    rng = np.random.default_rng(21)
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in [(120, 160), (97, 61), (64, 64)]]
    truths = [np.where(rng.uniform(0, 1, f.shape[:2]) < 0.3, 0.0, rng.uniform(0.5, 5.0, f.shape[:2])).astype(np.float32) for f in images]
    valid = [rng.uniform(0, 1, f.shape[:2]) < 0.9 for f in images]
    for method in ("lstsq", "median"):
        fit, metrics, maps = model.evaluate_depth(images, truths, valid, method=method, truth_range=(0.6, None), max_side_length=112, batch_size=2)
        preds = model.inference_images(images, 112, True, 2)
        want_fit = pp.fit_true_depth(preds, truths, valid, "inverse", method, (0.6, None))
        want_metrics = pp.depth_metrics(preds, truths, want_fit, valid, "inverse", (0.6, None))
        want_maps = pp.true_depth(preds, want_fit, [t.shape for t in truths])
        assert torch.equal(fit.view(torch.int64), want_fit.view(torch.int64)) and torch.equal(metrics.view(torch.int64), want_metrics.view(torch.int64))
        assert metrics[:, 0].min().item() > 1000
        for i, f in enumerate(images):
            assert maps[i].shape == (1, *f.shape[:2]) and torch.equal(maps[i].view(torch.int32), want_maps[i].view(torch.int32))
