"""The chunk boundaries of chunk_reduce (csrc/post_common.inc), the one scaffold under the tile fit, the least-squares fit, the mean absolute
deviation of the median fit and the depth metrics: a chunk is 2048 samples, 256 threads x 8 strided samples. Sample counts 1 (1 x 1), 255 (1 x 255:
a thread without a sample), 2048 (32 x 64: exactly one full chunk), 2049 (3 x 683: a second chunk holding one sample) and 4096 (2 x 2048: two full
chunks); the prediction (the tile fit: the guide) has about a quarter of each side; every sample is valid. Through the public entry points, in one
call per dtype (the tile fit: one call per size, a single tile that is the whole photo).

Inputs and bounds are those of tests/test_gpu_align.py and tests/test_gpu_tiles.py (their _pair / guide construction, their assertions on the
"two_chunks" pair / in test_fit_and_blend_against_the_restatement): counts exact, sums within n 2^-52 sum|terms| of math.fsum's, A and B (s and t)
within 1e-9 relative, medians bit-equal, the metrics under the summation-order bound and the recomputed log bound, the blend within one fp32 ulp.
One sample cannot be anything but degenerate (n < 2): there the restatement's scale is exactly 0, `<= 1e-9 |0|` asks the device for exactly 0 too,
and the closeness to the generating (0.37, 0.25) (the tile fit: a positive scale, all its test asks) is asserted from 255 samples on. Asserted
on the CPU when a case is built: every restatement is finite, and non-degenerate from 255 samples on. Running a whole call twice gives equal bits."""
import functools

import numpy as np
import pytest
import torch

from muggled_dpt_amd import postprocess as pp
from tests import align_restate as ar
from tests import test_gpu_align as ta
from tests import tile_restate as tr

pytestmark = pytest.mark.gpu

DTYPES = ta.DTYPES
SIZES = ((1, 1), (1, 255), (32, 64), (3, 683), (2, 2048))
COUNTS = [h * w for h, w in SIZES]
assert COUNTS == [1, 255, 2048, 2049, 4096]


def _quarter(hw):
    return tuple(max(1, -(-s // 4)) for s in hw)


@functools.lru_cache(maxsize=None)
def _case(dt: str, method: str):
    rng = np.random.default_rng(11)
    trip = [ta._pair(rng, DTYPES[dt], _quarter(hw), hw, invalid=0.0) for hw in SIZES]
    case = dict(names=[f"{h}x{w}" for h, w in SIZES], preds=[t[0] for t in trip], truths=[t[1] for t in trip], valids=[t[2] for t in trip], dtype=DTYPES[dt])
    case["ref"] = [ar.fit(p, t, m, method=method) for p, t, m in zip(case["preds"], case["truths"], case["valids"])]
    for a in case["preds"] + case["truths"] + case["valids"]:
        a.setflags(write=False)
    for k, (ab, sums, terms) in enumerate(case["ref"]):
        assert sums[0] == COUNTS[k] and np.isfinite(ab).all() and np.isfinite(sums).all() and np.isfinite(terms).all()
        if COUNTS[k] == 1:
            assert ab[0] == 0.0 and ab[1] > 0.0  # (one sample: the degenerate rule, B = t)
        else:
            assert abs(ab[0] - ta.A0) < 0.05 and abs(ab[1] - ta.B0) < 0.05, (case["names"][k], ab)
    return case


def _bits(*arrays):
    return [np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32) for a in arrays]


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(_bits(*a), _bits(*b)))


@pytest.mark.parametrize("dt", list(DTYPES))
def test_least_squares_fit_at_the_chunk_boundaries(dt):
    case = _case(dt, "lstsq")
    fit, sums = ta._fit(case, "lstsq")
    ref_fit = np.array([r[0] for r in case["ref"]])
    ref_sums, abs_terms = np.array([r[1] for r in case["ref"]]), np.array([r[2] for r in case["ref"]])
    assert np.array_equal(sums[:, 0].view(np.uint64), ref_sums[:, 0].view(np.uint64))
    err, bound = np.abs(sums - ref_sums), ref_sums[:, :1] * 2.0 ** -52 * abs_terms
    print(f"{dt}: sums err / bound per pair {np.max(err / np.maximum(bound, 1e-300), axis=1)}")
    assert np.all(err <= bound)
    print(f"{dt}: fit rel err per pair {np.max(np.abs(fit - ref_fit) / np.maximum(np.abs(ref_fit), 1e-300), axis=1)}")
    assert np.all(np.abs(fit - ref_fit) <= 1e-9 * np.abs(ref_fit))
    assert _same(ta._fit(case, "lstsq"), (fit, sums))


@pytest.mark.parametrize("dt", list(DTYPES))
def test_median_fit_at_the_chunk_boundaries(dt):
    case = _case(dt, "median")
    fit, sums = ta._fit(case, "median")
    ref_fit = np.array([r[0] for r in case["ref"]])
    ref_sums, dev_terms = np.array([r[1] for r in case["ref"]]), np.array([r[2] for r in case["ref"]])
    assert np.array_equal(sums[:, :3].view(np.uint64), ref_sums[:, :3].view(np.uint64)), (sums[:, :3], ref_sums[:, :3])
    assert np.all(sums[:, 5] == 0.0)
    n = np.maximum(ref_sums[:, :1], 1.0)
    err, bound = np.abs(sums[:, 3:5] - ref_sums[:, 3:5]), (n * 2.0 ** -52 * dev_terms) / n + 2.0 ** -52 * ref_sums[:, 3:5]
    print(f"{dt}: mad err / bound per pair {np.max(err / np.maximum(bound, 1e-300), axis=1)}")
    assert np.all(err <= bound)
    print(f"{dt}: median fit rel err per pair {np.max(np.abs(fit - ref_fit) / np.maximum(np.abs(ref_fit), 1e-300), axis=1)}")
    assert np.all(np.abs(fit - ref_fit) <= 1e-9 * np.abs(ref_fit))
    assert _same(ta._fit(case, "median"), (fit, sums))


@functools.lru_cache(maxsize=None)
def _metric_refs(dt):
    """as tests/test_gpu_align.py::_metric_refs, with the restatement's own fits"""
    case = _case(dt, "lstsq")
    fits = np.array([r[0] for r in case["ref"]])
    refs, sums_abs, moved = [], [], 0.0
    for p, t, m, ab in zip(case["preds"], case["truths"], case["valids"], fits):
        ref, abs_sums, q, r = ar.metrics(p, t, tuple(ab), m)
        assert np.isfinite(ref).all() and ref[1] == 0 and np.min(np.abs(q)) > 1e-12, "a q within 1e-12 of zero"
        for thr in (1.25, 1.5625, 1.953125):
            assert np.min(np.abs(r / thr - 1.0)) > 1e-9, "a ratio within 1e-9 of a delta threshold"
        for signs in ((1.0, -1.0), (-1.0, 1.0), None):
            alt = ar.metrics(p, t, tuple(ab), m, log=ta._MovedLog(np.log, signs, 1), log10=ta._MovedLog(np.log10, signs, 2))[0]
            for c in ta.LOG_COLUMNS:
                if ref[c] != 0.0:
                    moved = max(moved, abs(alt[c] - ref[c]) / abs(ref[c]))
        refs.append(ref)
        sums_abs.append(abs_sums)
    return fits, np.array(refs), sums_abs, moved


@pytest.mark.parametrize("dt", list(DTYPES))
def test_metrics_at_the_chunk_boundaries(dt):
    case = _case(dt, "lstsq")
    fits, ref, sums_abs, _ = _metric_refs(dt)
    log_bound = 4.0 * max(_metric_refs(d)[3] for d in DTYPES)
    print(f"{dt}: log bound {log_bound:.3g}")
    assert 0.0 < log_bound < 1e-10
    got = ta._metrics(case, fits)
    assert np.array_equal(got[:, :2], ref[:, :2])
    for k, name in enumerate(case["names"]):
        m = ref[k, 0] - ref[k, 1]
        eps = m * 2.0 ** -52
        s = sums_abs[k]
        for c, key in ((2, "abs_rel"), (3, "sq_rel"), (7, "d1"), (8, "d2"), (9, "d3")):
            assert abs(got[k, c] - ref[k, c]) <= eps * s[key] / m + 2.0 ** -52 * abs(ref[k, c]), (name, key, got[k, c], ref[k, c])
        assert got[k, 7] == ref[k, 7] and got[k, 8] == ref[k, 8] and got[k, 9] == ref[k, 9], name
        assert abs(got[k, 4] - ref[k, 4]) <= (0.5 * eps + 2.0 ** -51) * ref[k, 4], (name, "rmse")
        for c in ta.LOG_COLUMNS:
            err = abs(got[k, c] - ref[k, c])
            print(f"  {name} col {c}: ref {ref[k, c]:.6g} rel err {err / max(abs(ref[k, c]), 1e-300):.3g}")
            assert err <= log_bound * abs(ref[k, c]), (name, c, got[k, c], ref[k, c])
    assert np.array_equal(ta._metrics(case, fits).view(np.uint64), got.view(np.uint64))


PHOTO, GUIDE, FEATHER = (24, 40), (6, 10), 3.0  # the photo's one tile is fitted to a guide of a quarter of the photo's sides


@functools.lru_cache(maxsize=None)
def _tile_case(k: int, dt: str):
    """tests/test_gpu_tiles.py::_case for one tile of SIZES[k] samples that covers the whole photo"""
    dtype, mhw = DTYPES[dt], SIZES[k]
    rng = np.random.default_rng(13 + k)
    boxes = [(0, 0, PHOTO[1], PHOTO[0])]
    guide = ta._round(0.37 * rng.uniform(1.0, 2.0, GUIDE) + 2.5, dtype)
    y = tr.guide_samples(guide, boxes[0], mhw, PHOTO)
    maps = [ta._round((y - 2.5 - rng.normal(0.0, 0.05, mhw)) / 0.37, dtype)]
    case = dict(hw=PHOTO, boxes=boxes, feather=FEATHER, maps=maps, guide=guide, dtype=dtype)
    case["ref"] = tr.fit(maps, boxes, guide, PHOTO)
    for v in maps + [guide]:
        v.setflags(write=False)
    ref_fit, ref_sums, abs_terms = case["ref"]
    assert ref_sums[0, 0] == COUNTS[k] and np.isfinite(ref_fit).all() and np.isfinite(ref_sums).all() and np.isfinite(abs_terms).all()
    assert (ref_fit[0, 0] == 0.0 and ref_fit[0, 1] > 0.0) if COUNTS[k] == 1 else ref_fit[0, 0] > 0.0, ref_fit
    return case


def _stitch(case):
    dev = lambda a: torch.from_numpy(np.array(a)).to(case["dtype"]).cuda()[None]
    out, fit, sums = pp.stitch_tiles([dev(m) for m in case["maps"]], case["boxes"], case["hw"], guide=dev(case["guide"]), align="affine",
                                     feather=case["feather"], return_fit=True)
    return out[0].cpu().numpy(), fit.cpu().numpy(), sums.cpu().numpy()


@pytest.mark.parametrize("dt", list(DTYPES))
def test_tile_fit_at_the_chunk_boundaries(dt):
    for k, name in enumerate(f"{h}x{w}" for h, w in SIZES):
        case = _tile_case(k, dt)
        out, fit, sums = _stitch(case)
        ref_fit, ref_sums, abs_terms = case["ref"]
        assert out.shape == PHOTO and fit.shape == ref_fit.shape and sums.shape == ref_sums.shape
        assert np.array_equal(sums[:, 0], ref_sums[:, 0])
        err, bound = np.abs(sums - ref_sums), ref_sums[:, :1] * 2.0 ** -52 * abs_terms
        print(f"{name} {dt}: sums err / bound max {np.max(err / np.maximum(bound, 1e-300)):.3g}, fit {fit[0]} ref {ref_fit[0]}")
        assert np.all(err <= bound)
        assert np.all(np.abs(fit - ref_fit) <= 1e-9 * np.abs(ref_fit))
        for st, empty in ((fit, sums[:, 0] == 0), (ref_fit, ref_sums[:, 0] == 0)):  # the blend alone, then end to end
            want = tr.blend(case["maps"], case["boxes"], PHOTO, st, empty, FEATHER).astype(np.float32)
            assert tr.ulps(out, want) <= 1, name
        assert np.isfinite(out).all() and 2.0 < out.min() and out.max() < 4.0
        assert _same(_stitch(case), (out, fit, sums)), name
