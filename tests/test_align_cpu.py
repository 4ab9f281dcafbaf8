"""The true-depth block without a GPU: the fp64 restatement tests/align_restate.py against closed forms, the key order of the radix select, the
Python argument checks and the C entry points' host-side checks (which launch nothing)."""
import ctypes
import math

import numpy as np
import pytest
import torch

from muggled_dpt_amd import native
from muggled_dpt_amd import postprocess as pp
from tests import align_restate as ar


def test_the_explainers_ball_is_four_metres_away():
    """results_explainer.md: normalised V = 0.375 with d_min = 3, d_max = 5 -> 1 / (V (1/3 - 1/5) + 1/5) = 4 m; the same through the fit of two
    exact measurements (V = 1 at 3 m, V = 0 at 5 m) and through the mesh helper's inverse"""
    a, b = 1.0 / 3.0 - 1.0 / 5.0, 1.0 / 5.0
    pred = np.array([[0.0, 1.0, 0.375]])
    d = ar.apply(pred, (a, b))
    assert abs(d[0, 2] - 4.0) < 1e-14 and abs(d[0, 0] - 5.0) < 1e-14 and abs(d[0, 1] - 3.0) < 1e-14
    (fa, fb), sums, _ = ar.fit(pred, np.array([[5.0, 3.0, 0.0]], dtype=np.float32))  # (0: the ball itself is not measured)
    assert sums[0] == 2 and abs(fa - a) < 1e-15 and abs(fb - b) < 1e-15
    assert abs(ar.apply(pred, (fa, fb))[0, 2] - 4.0) < 1e-13
    lo, hi = pp.mesh_depth_range((fa, fb), (0.0, 1.0))
    assert abs(lo - 3.0) < 1e-13 and abs(hi - 5.0) < 1e-13
    # a prediction in raw units x = 7 V + 2: the fit absorbs the units, the mesh range is unchanged
    lo, hi = pp.mesh_depth_range((fa / 7.0, fb - 2.0 * fa / 7.0), (2.0, 9.0))
    assert abs(lo - 3.0) < 1e-12 and abs(hi - 5.0) < 1e-12
    with pytest.raises(ValueError):
        pp.mesh_depth_range((0.0, 0.2), (0.0, 1.0))
    with pytest.raises(ValueError):
        pp.mesh_depth_range((1.0, -0.5), (0.0, 1.0))


@pytest.mark.parametrize("method", ["lstsq", "median"])
@pytest.mark.parametrize("space", ["inverse", "depth"])
def test_truth_built_from_the_model_returns_the_model(space, method):
    rng = np.random.default_rng(0)
    A, B = 0.37, 0.25
    pred = rng.uniform(1.0, 2.0, (9, 7))
    # the truth at the prediction's own size: the sample positions are the pixel centres, v = pred exactly
    assert np.array_equal(ar.resample(pred, pred.shape), pred)
    q = A * pred + B
    truth = (1.0 / q if space == "inverse" else q).astype(np.float32)
    (a, b), sums, _ = ar.fit(pred, truth, space=space, method=method)
    # float32 truths: t carries 2^-24 relative rounding (the median fit also rounds v to float32)
    assert sums[0] == 63 and abs(a - A) < 1e-5 and abs(b - B) < 1e-5
    m, _, _, _ = ar.metrics(pred, truth, (a, b), space=space)
    assert m[0] == 63 and m[1] == 0 and m[2] < 1e-5 and m[7] == 1.0 and m[8] == 1.0 and m[9] == 1.0 and m[4] < 1e-4 and m[10] < 1e-3
    # ... and exactly, where the truth is exact in float32: v in {1, 3}, t = 0.25 v + 0.25 in {0.5, 1}, truth = 1 / t in {2, 1}
    pred = np.array([[1.0, 3.0, 3.0, 1.0, 1.0]])
    truth = np.array([[2.0, 1.0, 1.0, 2.0, 2.0]], dtype=np.float32)
    (a, b), _, _ = ar.fit(pred, truth, method=method)
    assert (a, b) == (0.25, 0.25)
    m, _, _, _ = ar.metrics(pred, truth, (a, b))
    assert m[2] == 0.0 and m[3] == 0.0 and m[4] == 0.0 and m[5] == 0.0 and m[6] == 0.0 and m[7] == 1.0 and m[10] == 0.0


def test_sample_rule_leaves_out_what_it_must():
    pred = np.array([[1.0, 2.0], [np.nan, 4.0]])
    truth = np.array([[1.0, 0.0, np.nan, 2.0], [np.inf, -1.0, 3.0, 4.0], [5.0, 6.0, 7.0, 8.0], [9.0, 10.0, 11.0, 12.0]], dtype=np.float32)
    v, t, g = ar.samples(pred, truth)
    # a tap that is NaN makes the sample NaN even at weight 0 (0 x NaN): only column 3, whose two taps are column 1 of the prediction, is finite
    assert g.tolist() == [2.0, 4.0, 8.0, 12.0] and v.tolist() == [2.0, 2.5, 3.5, 4.0]
    assert np.array_equal(t, 1.0 / g)
    valid = np.ones((4, 4), dtype=np.uint8)
    valid[0, 3] = 0
    assert ar.samples(pred, truth, valid)[2].tolist() == [4.0, 8.0, 12.0]
    assert ar.samples(pred, truth, truth_range=(3.0, 8.0))[2].tolist() == [4.0, 8.0]
    assert ar.samples(pred, truth, truth_range=(None, 3.5), space="depth")[1].tolist() == [2.0]
    pred = np.array([[1.0, 2.0], [3.0, 4.0]])  # (all finite: what the truth itself leaves out)
    assert ar.samples(pred, truth)[2].tolist() == [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0, 10.0, 11.0, 12.0]
    # downsampling reads between source pixels: 4 -> 2 samples at u = 0.5 and 2.5
    assert ar.resample(np.array([[0.0, 1.0, 2.0, 3.0]]), (1, 2)).tolist() == [[0.5, 2.5]]
    # upsampling clamps at the border: 2 -> 4 samples at u = -0.25 -> 0, 0.25, 0.75, 1.25 -> 1
    assert ar.resample(np.array([[0.0, 1.0]]), (1, 4)).tolist() == [[0.0, 0.25, 0.75, 1.0]]


def test_median_rule_even_odd_ties():
    f = np.float32
    assert ar.median32(np.array([3, 1, 2], dtype=f)) == 2.0
    assert ar.median32(np.array([4, 1, 3, 2], dtype=f)) == 2.5
    assert ar.median32(np.array([1, 5, 5, 5, 9, 5], dtype=f)) == 5.0
    assert ar.median32(np.array([7], dtype=f)) == 7.0
    lo, hi = f(1.0), np.nextafter(f(1.0), f(2.0))
    assert ar.median32(np.array([lo, hi], dtype=f)) == (float(lo) + float(hi)) * 0.5  # between two float32 neighbours: exact in fp64 only
    # mad and the fit: v = {1, 2, 3, 4, 10}, t = 2 v + 1 -> med v = 3, mad v = (2 + 1 + 0 + 1 + 7) / 5 = 2.2, mad t = 4.4, A = 2, B = 1
    v = np.array([1.0, 2.0, 3.0, 4.0, 10.0])
    (a, b), sums, _ = ar.fit_median(v, 2.0 * v + 1.0)
    assert sums.tolist() == [5, 3.0, 7.0, 2.2, 4.4, 0.0] and a == 2.0 and b == 1.0
    # degenerate: a constant prediction, one sample, no sample
    assert ar.fit_median(np.full(4, 1.5), np.array([1.0, 2.0, 3.0, 4.0]))[0] == (0.0, 2.5)
    assert ar.fit_median(np.array([1.5]), np.array([3.0]))[0] == (0.0, 3.0)
    assert ar.fit_median(np.zeros(0), np.zeros(0))[0] == (0.0, 0.0)
    assert ar.fit_lstsq(np.full(4, 1.5), np.array([1.0, 2.0, 3.0, 4.0]))[0] == (0.0, 2.5)
    assert ar.fit_lstsq(np.array([1.0, 2.0]), np.array([2.0, 1.0]))[0] == (0.0, 1.5)  # negatively correlated


def test_key_order():
    f = np.float32
    vals = np.array([-np.inf, -3.5, -1.0, -np.finfo(f).tiny, -1e-45, -0.0, 0.0, 1e-45, np.finfo(f).tiny, 1.0, 3.5, np.inf], dtype=f)
    keys = ar.f32_key(vals)
    assert np.all(np.diff(keys.astype(np.int64)) > 0)
    assert keys[5] == 0x7FFFFFFF and keys[6] == 0x80000000  # -0.0 directly before +0.0
    rng = np.random.default_rng(1)
    x = rng.standard_normal(4096).astype(f) * f(100.0)
    order = np.argsort(ar.f32_key(x), kind="stable")
    assert np.array_equal(x[order], np.sort(x))


def test_metrics_closed_forms():
    # one sample, d = 2 g: AbsRel 1, SqRel g, RMSE g, RMSE-log ln 2, log10 log10 2, delta1 0 (ratio 2 >= 1.25^3 = 1.953125), SILog 0
    pred, truth = np.array([[0.25]]), np.array([[2.0]], dtype=np.float32)
    m, _, q, r = ar.metrics(pred, truth)
    assert q.tolist() == [0.25] and r.tolist() == [2.0]
    assert m[:5].tolist() == [1, 0, 1.0, 2.0, 2.0] and abs(m[5] - math.log(2.0)) < 1e-15 and abs(m[6] - math.log10(2.0)) < 1e-15
    assert m[7:].tolist() == [0.0, 0.0, 0.0, 0.0]
    # q <= 0 is bad and left out; nothing left: NaN
    m, _, _, _ = ar.metrics(np.array([[1.0, 2.0]]), np.array([[1.0, 0.4]], dtype=np.float32), (1.0, -1.0))
    assert m[0] == 2 and m[1] == 1 and abs(m[2] - 1.5) < 1e-7  # the second sample: d = 1, g = 0.4
    m, _, _, _ = ar.metrics(np.array([[1.0]]), np.array([[1.0]], dtype=np.float32), (1.0, -1.0))
    assert m[0] == 1 and m[1] == 1 and np.isnan(m[2:]).all()
    # apply: q <= 0 -> +inf, the clamp, NaN stays
    d = ar.apply(np.array([[1.0, 2.0, 4.0]]), (1.0, -2.0), clamp=(None, 10.0))
    assert d.tolist() == [[10.0, 10.0, 0.5]] and np.isnan(ar.apply(np.array([[np.nan]]), (1.0, -2.0), clamp=(0.0, 10.0))).all()
    assert ar.apply(np.array([[1.0, 2.0, 4.0]]), (1.0, -2.0)).tolist() == [[np.inf, np.inf, 0.5]]
    assert ar.apply(np.array([[1.0, 2.0]]), (1.0, -2.0), space="depth", clamp=(0.0, None)).tolist() == [[0.0, 0.0]]


def test_python_argument_checks_need_no_gpu():
    p = [torch.zeros(1, 4, 4)]
    t = [np.ones((8, 8), dtype=np.float32)]
    with pytest.raises(ValueError, match="space"):
        pp.fit_true_depth(p, t, space="log")
    with pytest.raises(ValueError, match="method"):
        pp.fit_true_depth(p, t, method="ransac")
    with pytest.raises(ValueError, match="range"):
        pp.fit_true_depth(p, t, truth_range=(5.0, 1.0))
    with pytest.raises(ValueError, match="range"):
        pp.true_depth(p, None, clamp=(float("nan"), None))
    for call in (lambda: pp.fit_true_depth(p, t), lambda: pp.depth_metrics(p, t), lambda: pp.true_depth(p, None)):
        with pytest.raises(RuntimeError, match="CUDA"):  # host predictions: there is no CPU implementation
            call()
    assert len(pp.DEPTH_METRIC_NAMES) == native.ALIGN_NUM_METRICS == ar.METRICS


def _pairs(rows):
    t = np.zeros(len(rows), dtype=pp._PAIR_RECORD)
    for k, r in enumerate(rows):
        t[k] = r
    return t


def test_c_entry_points_check_on_the_host_and_launch_nothing():
    """Pointers are plain numbers here: a call that got past its checks would fault, so every call must return its error first."""
    lib = native.load()
    A = 0x10000  # an aligned, non-null address that is never read
    inf = float("inf")
    assert pp._PAIR_RECORD.itemsize == 40
    good = _pairs([(A, 13, 10, A, A, 37, 29), (A, 16, 12, A, 0, 50, 47)])
    need = ctypes.c_size_t()
    assert lib.mdpt_post_align_scratch_bytes(good.ctypes.data, 2, ctypes.byref(need)) == 0
    assert need.value == 2 * 2 * 11 * 8 + 2 * (1024 + 16) * 4  # 50 x 47 = 2350 pixels: two chunks of 2048

    def fit_rc(table, P=None, dt=native.DTYPE_F32, space=0, method=0, rng=(-inf, inf), fit=A, sums=A, scratch=A, nbytes=1 << 20, tdev=A):
        return lib.mdpt_post_align_fit(table.ctypes.data, tdev, len(table) if P is None else P, dt, space, method, rng[0], rng[1], fit, sums, scratch, nbytes, None)

    def metrics_rc(table, P=None, dt=native.DTYPE_F32, space=0, rng=(-inf, inf), fit=A, out=A, scratch=A, nbytes=1 << 20, tdev=A):
        return lib.mdpt_post_align_metrics(table.ctypes.data, tdev, len(table) if P is None else P, dt, space, rng[0], rng[1], fit, out, scratch, nbytes, None)

    offs = np.array([0, 37 * 29], dtype=np.int64)

    def apply_rc(table, P=None, dt=native.DTYPE_F32, space=0, fit=A, offsets=offs, odev=A, clamp=(-inf, inf), out=A, tdev=A):
        return lib.mdpt_post_align_apply(table.ctypes.data, tdev, len(table) if P is None else P, dt, space, fit,
                                         None if offsets is None else offsets.ctypes.data, odev, clamp[0], clamp[1], out, None)

    bad_tables = {
        "null prediction": _pairs([(0, 13, 10, A, 0, 37, 29)]), "misaligned prediction": _pairs([(A + 2, 13, 10, A, 0, 37, 29)]),
        "prediction size": _pairs([(A, 0, 10, A, 0, 37, 29)]), "truth size": _pairs([(A, 13, 10, A, 0, 37, -1)]),
        "too large": _pairs([(A, 13, 10, A, 0, 46341, 46341)]),
    }
    for word, table in bad_tables.items():
        for rc in (fit_rc(table), metrics_rc(table), apply_rc(table, offsets=offs[:1])):
            assert rc == -1 and lib.mdpt_last_error(), word
    for word, table in {"null truth": _pairs([(A, 13, 10, 0, 0, 37, 29)]), "misaligned truth": _pairs([(A, 13, 10, A + 2, 0, 37, 29)])}.items():
        assert fit_rc(table) == -1 and metrics_rc(table) == -1, word
        assert b"truth" in lib.mdpt_last_error()
    nan = float("nan")
    for kw in (dict(P=0), dict(P=70000), dict(dt=7), dict(space=2), dict(method=2), dict(rng=(2.0, 1.0)), dict(rng=(nan, 1.0)), dict(rng=(0.0, nan)),
               dict(fit=0), dict(fit=A + 4), dict(sums=0), dict(sums=A + 4), dict(scratch=0), dict(scratch=A + 4), dict(nbytes=need.value - 1), dict(tdev=0),
               dict(tdev=A + 4)):
        assert fit_rc(good, **kw) == -1, kw
        assert lib.mdpt_last_error()
    for kw in (dict(P=0), dict(P=70000), dict(dt=7), dict(space=-1), dict(rng=(2.0, 1.0)), dict(rng=(nan, nan)), dict(fit=A + 4), dict(out=0), dict(out=A + 4),
               dict(scratch=0), dict(nbytes=need.value - 1), dict(tdev=0), dict(tdev=A + 4)):
        assert metrics_rc(good, **kw) == -1, kw
    for kw in (dict(P=0), dict(dt=7), dict(space=2), dict(fit=A + 4), dict(offsets=None), dict(offsets=np.array([0, -1], dtype=np.int64)), dict(odev=0),
               dict(odev=A + 4), dict(clamp=(2.0, 1.0)), dict(clamp=(nan, inf)), dict(out=0), dict(out=A + 2), dict(tdev=0), dict(tdev=A + 4)):
        assert apply_rc(good, **kw) == -1, kw
    assert lib.mdpt_post_align_scratch_bytes(None, 2, ctypes.byref(need)) == -1 and lib.mdpt_post_align_scratch_bytes(good.ctypes.data, 2, None) == -1
    assert lib.mdpt_post_align_scratch_bytes(good.ctypes.data, 0, ctypes.byref(need)) == -1
