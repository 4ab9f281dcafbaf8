"""The locally varying true-depth alignment without a GPU: the restatement (tests/local_align_restate.py) on the prototype's scene and on inputs whose answer is
known; the argument checks of muggled_dpt_amd.local_align; the exported entry points, which refuse bad arguments before they touch a device pointer; the record
table's layout; the scratch query.

The scene: 96 x 128, the truth's inverse is A v + B with A drifting 0.30 -> 0.50 left to right and B 0.20 -> 0.30 top to bottom, measurements on every eighth row
at 25 % (382 samples, 3 %), grid 6 x 8, radius 1. Hold-out AbsRel (every pixel without a measurement) measured with the restatement: global fit 0.0918, local fit
0.0157 (prior 0, 0.17 of the global) and 0.0206 (prior 4, 0.22); the test asks for at most one third."""
import ctypes

import numpy as np
import pytest
import torch

from muggled_dpt_amd import local_align, native
from muggled_dpt_amd.postprocess import _common
from tests import align_restate as ar
from tests import local_align_restate as lr


def test_the_local_fit_removes_the_drift_a_global_fit_leaves_on_the_prototype_scene():
    pred, truth, valid = lr.drift_scene()
    n = int(valid.sum())
    assert 300 <= n <= 500
    hold = valid == 0
    ab = ar.fit(pred, truth, valid)[0]
    glob = lr.abs_rel(ar.apply(pred, ab, truth.shape), truth, hold)
    for prior in (0.0, 4.0):
        f = lr.fit(pred, truth, valid, grid=(6, 8), radius=1, prior=prior)
        assert f["G"][0] == n and lr.branch_margin_ok(f["margins"])
        loc = lr.abs_rel(lr.apply(pred, f["coeffs"], truth.shape), truth, hold)
        print(f"prior {prior}: hold-out AbsRel global {glob:.4f}, local {loc:.4f} ({loc / glob:.3f} of it)")
        assert loc <= glob / 3.0


def _noisy(seed=3, phw=(11, 9), thw=(30, 26), invalid=0.3):
    rng = np.random.default_rng(seed)
    pred = rng.uniform(1.0, 2.0, phw).astype(np.float32)
    v = ar.resample(pred, thw)
    truth = (1.0 / (0.37 * v + 0.25 + rng.normal(0.0, 0.01, thw))).astype(np.float32)
    truth[rng.uniform(0.0, 1.0, thw) < invalid] = 0.0
    return pred, truth


def test_a_one_by_one_grid_is_the_global_fit():
    pred, truth = _noisy()
    (a, b), sums, _ = ar.fit(pred, truth)
    for radius, prior in ((0, 0.0), (1, 0.0), (3, 4.0)):
        f = lr.fit(pred, truth, grid=(1, 1), radius=radius, prior=prior)
        assert np.array_equal(f["M"][0, 0], sums) and tuple(f["fit"]) == (a, b)
        if prior == 0.0:
            assert f["coeffs"][0, 0].tolist() == [a, b]  # the one window is the image
        else:
            assert np.allclose(f["coeffs"][0, 0], [a, b], rtol=1e-12, atol=0.0)  # (n + prior) samples distributed as the n are
    assert np.array_equal(lr.apply(pred, np.array([[[a, b]]]), truth.shape), ar.apply(pred, (a, b), truth.shape))


def test_a_large_prior_gives_the_global_fit_in_every_node():
    pred, truth = _noisy()
    f = lr.fit(pred, truth, grid=(5, 4), radius=1, prior=1e12)
    a, b = f["fit"]
    assert np.all(np.abs(f["wfit"] - [a, b]) <= 1e-9 * np.abs([a, b])) and np.all(np.abs(f["coeffs"] - [a, b]) <= 1e-9 * np.abs([a, b]))
    free = lr.fit(pred, truth, grid=(5, 4), radius=1, prior=0.0)
    assert np.max(np.abs(free["wfit"][..., 0] - a)) > 1e-3 * a  # without the prior the nodes differ


def test_a_radius_that_covers_the_grid_gives_one_coefficient_everywhere():
    pred, truth = _noisy()
    for prior in (0.0, 4.0):
        f = lr.fit(pred, truth, grid=(4, 3), radius=64, prior=prior)
        assert np.all(f["wfit"] == f["wfit"][0, 0]) and np.all(f["coeffs"] == f["coeffs"][0, 0])
        assert np.all(np.abs(f["coeffs"][0, 0] - f["fit"]) <= 1e-9 * np.abs(f["fit"]))  # every window is the image


def test_an_empty_window_takes_the_global_fit_exactly():
    pred, truth = _noisy()
    truth[:12] = 0.0  # cell rows 0 and 1 of 5 (6 pixels each) are empty: with radius 0 node row 0, 1; with radius 1 node row 0
    for radius, rows in ((0, 2), (1, 1)):
        for prior in (0.0, 4.0):
            f = lr.fit(pred, truth, grid=(5, 4), radius=radius, prior=prior)
            assert np.all(f["M"][:2, :, 0] == 0) and np.all(f["M"][2:, :, 0] > 0)
            assert np.all(f["wfit"][:rows] == np.array(f["fit"])) and not np.any(f["wfit"][rows:, :, 0] == f["fit"][0])


def test_a_truth_affine_in_v_per_cell_region_is_reproduced():
    rng = np.random.default_rng(5)
    pred = rng.uniform(1.0, 2.0, (24, 32)).astype(np.float32)
    a = np.where(np.arange(32) < 16, 0.3, 0.5)[None, :]  # two regions of 4 x 4 cells each on an 8 x 8 grid
    for space in ("inverse", "depth"):
        t = a * pred.astype(np.float64) + 0.2
        truth = (1.0 / t if space == "inverse" else t).astype(np.float32)
        f = lr.fit(pred, truth, space=space, grid=(8, 8), radius=1, prior=0.0)
        # a window wholly inside one region sees an exactly affine truth (up to its float32 rounding): nodes 0..2 and 5..7 across
        assert np.allclose(f["wfit"][:, :3], [0.3, 0.2], rtol=0.0, atol=1e-5) and np.allclose(f["wfit"][:, 5:], [0.5, 0.2], rtol=0.0, atol=1e-5)
        assert np.allclose(f["coeffs"][:, :2], [0.3, 0.2], rtol=0.0, atol=1e-5) and np.allclose(f["coeffs"][:, 6:], [0.5, 0.2], rtol=0.0, atol=1e-5)
        d = lr.apply(pred, f["coeffs"], space=space)
        inside = np.ones((24, 32), bool)
        inside[:, 6:26] = False  # pixels whose four taps lie in columns 0..1 or 6..7
        assert np.allclose(d[inside], truth[inside], rtol=1e-4)


def test_cells_follow_the_integer_rule_and_uneven_cells_hold_every_pixel_once():
    assert lr.cell_of(3, 10).tolist() == [0, 0, 0, 0, 1, 1, 1, 2, 2, 2] and lr.cell_of(4, 37).tolist().count(0) == 10
    pred, truth = _noisy(thw=(37, 29), invalid=0.0)
    f = lr.fit(pred, truth, grid=(4, 3))
    assert f["M"][..., 0].sum() == 37 * 29 and f["M"][..., 0].tolist() == [[100, 100, 90], [90, 90, 81], [90, 90, 81], [90, 90, 81]]  # rows 10, 9, 9, 9 and columns 10, 10, 9


def test_python_arguments_are_checked_before_anything_runs():
    maps, truths = [torch.zeros(1, 4, 5)], [np.ones((8, 9), np.float32)]
    for bad in (dict(space="linear"), dict(radius=-1), dict(radius=65), dict(radius=1.5), dict(radius=True), dict(prior=-1.0), dict(prior=float("nan")),
                dict(prior=float("inf")), dict(truth_range=(2.0, 1.0))):
        with pytest.raises(ValueError, match="fit_true_depth_local"):
            local_align.fit_true_depth_local(maps, truths, **bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # there is no CPU implementation: host maps raise
        local_align.fit_true_depth_local(maps, truths)
    for bad in ((0, 4), (4, 10), (9, 1), (257, 1), (2.0, 2), [(2, 2), (2, 2)], "12x16"):
        with pytest.raises(ValueError, match="grid"):
            local_align._grids(bad, [(8, 9)], "fit_true_depth_local")
    assert local_align._grids((2, 3), [(8, 9), (5, 5)], "f") == [(2, 3), (2, 3)] and local_align._grids([(8, 9), [1, 1]], [(8, 9), (5, 5)], "f") == [(8, 9), (1, 1)]
    with pytest.raises(TypeError, match="LocalDepthFit"):
        local_align.true_depth_local(maps, object())
    assert "not\n    measured optima" in local_align.fit_true_depth_local.__doc__ or "not measured optima" in " ".join(local_align.fit_true_depth_local.__doc__.split())
    for word in ("Edge-aware".lower(), "robust reweighting", "median variant", "confidence", "temporal coherence", "unverified: no checkpoint can be loaded"):
        assert word in " ".join(local_align.__doc__.split()), word
    import muggled_dpt_amd.postprocess as package  # nothing new in the recorded package surface
    assert not hasattr(package, "fit_true_depth_local") and not hasattr(package, "LOCALFIT_RECORD")


def _records(sizes, ptr=4096):
    """sizes: (ph, pw, H, W, gh, gw) per pair -> (records with running cell_off and scratch_off, the scratch bytes)"""
    rec = np.zeros(len(sizes), dtype=_common.LOCALFIT_RECORD)
    cells = at = 0
    for k, (ph, pw, H, W, gh, gw) in enumerate(sizes):
        rec[k] = (ptr, ph, pw, ptr, 0, H, W, gh, gw, cells, at, ptr)  # (not device addresses: nothing may be launched with them)
        chunks = (-(-H // gh) * -(-W // gw) + 2047) // 2048
        at += (gh * gw * chunks * 6 + gh * gw * 2) * 8
        cells += gh * gw
    return rec, at


def test_entry_points_are_exported_and_refuse_bad_arguments_without_a_device():
    lib = native.load()
    names = ("mdpt_localfit_scratch_bytes", "mdpt_localfit_fit", "mdpt_localfit_apply")
    for name in names:
        assert name in native.SYMBOLS and hasattr(lib, name)
    assert {s for s in native.SYMBOLS if s.startswith("mdpt_localfit_")} == set(names)
    assert "post_localfit.inc" in native.HEADERS and "mdpt_localfit.cpp" in native.SOURCES
    assert (native.LOCALFIT_MAX_GRID, native.LOCALFIT_MAX_RADIUS, native.LOCALFIT_CHUNK) == (256, 64, 2048)
    assert lib.mdpt_abi_version() == 6 == native.ABI_VERSION
    sizes = [(13, 10, 37, 29, 4, 3), (16, 12, 9, 7, 9, 7), (13, 10, 50, 47, 1, 1), (5, 5, 300, 200, 2, 2)]
    rec, total = _records(sizes)
    need = ctypes.c_size_t()
    assert lib.mdpt_localfit_scratch_bytes(rec.ctypes.data, 4, ctypes.byref(need)) == 0 and need.value == total
    assert total == ((12 * 6 + 24) + (63 * 6 + 126) + (2 * 6 + 2) + (4 * 8 * 6 + 8)) * 8  # (50 x 47 on one cell: two chunks; 150 x 100 a cell: eight)

    def changed(field, k, value, base=rec):
        r = base.copy()
        r[field][k] = value
        return r

    huge, _ = _records([(5, 5, 65536, 32768, 1, 1)])
    for r, n, out, word in ((None, 4, need, b"records_host"), (rec, 0, need, b"n ="), (rec, 65536, need, b"n ="), (rec, 4, None, b"bytes"), (huge, 1, need, b"2^31"),
                            (changed("H", 1, 0), 4, need, b"size"), (changed("pw", 0, -1), 4, need, b"size"), (changed("gh", 0, 0), 4, need, b"grid"),
                            (changed("gw", 0, 30), 4, need, b"grid"), (changed("gh", 3, 257), 4, need, b"grid")):
        assert lib.mdpt_localfit_scratch_bytes(None if r is None else r.ctypes.data, n, None if out is None else ctypes.byref(out)) == native_invalid(), (n, word)
        assert word in lib.mdpt_last_error(), (word, lib.mdpt_last_error())

    p, big = 4096, 1 << 30

    def fit(r=rec, dev=p, n=4, dtype=0, space=0, radius=1, prior=4.0, tmin=float("-inf"), tmax=float("inf"), moments=p, ab=p, sums=p, coeffs=p, scratch=p, nbytes=big):
        return lib.mdpt_localfit_fit(None if r is None else r.ctypes.data, dev, n, dtype, space, radius, prior, tmin, tmax, moments, ab, sums, coeffs, scratch, nbytes, None)

    for kw, word in ((dict(r=None), b"records_host"), (dict(dev=None), b"records_dev"), (dict(scratch=None), b"scratch"), (dict(moments=None), b"moments_f64"),
                     (dict(ab=None), b"fit_f64"), (dict(sums=None), b"sums_f64"), (dict(coeffs=None), b"coeffs_f64"), (dict(n=0), b"n ="), (dict(n=65536), b"n ="),
                     (dict(dtype=7), b"dtype"), (dict(space=2), b"space"), (dict(radius=-1), b"radius"), (dict(radius=65), b"radius"), (dict(prior=-0.5), b"prior"),
                     (dict(prior=float("nan")), b"prior"), (dict(prior=float("inf")), b"prior"), (dict(tmin=2.0, tmax=1.0), b"truth range"),
                     (dict(tmin=float("nan")), b"truth range"), (dict(r=changed("H", 1, 0)), b"size"), (dict(r=changed("ph", 2, 0)), b"size"),
                     (dict(r=huge, n=1), b"2^31"), (dict(r=changed("gh", 0, 38)), b"grid"), (dict(r=changed("gw", 1, 8)), b"grid"), (dict(r=changed("gw", 3, 0)), b"grid"),
                     (dict(r=changed("gh", 3, 257)), b"grid"), (dict(r=changed("pred", 0, 0)), b"prediction"), (dict(r=changed("pred", 0, 4098)), b"prediction"),
                     (dict(r=changed("truth", 2, 0)), b"truth"), (dict(r=changed("truth", 2, 4098)), b"truth"), (dict(r=changed("cell_off", 2, 74)), b"cell_off"),
                     (dict(moments=4100), b"misaligned"), (dict(coeffs=4100), b"misaligned"), (dict(dev=4100), b"misaligned"), (dict(scratch=4100), b"misaligned"),
                     (dict(nbytes=total - 8), b"scratch region"), (dict(r=changed("scratch_off", 1, 4)), b"scratch region"),
                     (dict(r=changed("scratch_off", 1, -8)), b"scratch region"), (dict(r=changed("scratch_off", 1, 0)), b"overlap")):
        assert fit(**kw) == native_invalid(), kw
        assert word in lib.mdpt_last_error(), (kw, lib.mdpt_last_error())

    def apply(r=rec, dev=p, n=4, dtype=0, space=0, coeffs=p, dmin=float("-inf"), dmax=float("inf")):
        return lib.mdpt_localfit_apply(None if r is None else r.ctypes.data, dev, n, dtype, space, coeffs, dmin, dmax, None)

    for kw, word in ((dict(r=None), b"records_host"), (dict(dev=None), b"records_dev"), (dict(coeffs=None), b"coeffs_f64"), (dict(n=0), b"n ="), (dict(dtype=3), b"dtype"),
                     (dict(space=-1), b"space"), (dict(dmin=2.0, dmax=1.0), b"clamp"), (dict(dmax=float("nan")), b"clamp"), (dict(coeffs=4100), b"misaligned"),
                     (dict(r=changed("W", 0, 0)), b"size"), (dict(r=huge, n=1), b"2^31"), (dict(r=changed("gh", 0, 0)), b"grid"), (dict(r=changed("gw", 0, 257)), b"grid"),
                     (dict(r=changed("pred", 1, 0)), b"prediction"), (dict(r=changed("cell_off", 1, 0)), b"cell_off"), (dict(r=changed("out", 3, 0)), b"out"),
                     (dict(r=changed("out", 3, 4098)), b"out")):
        assert apply(**kw) == native_invalid(), kw
        assert word in lib.mdpt_last_error(), (kw, lib.mdpt_last_error())


def native_invalid() -> int:
    """MDPT_E_INVALID of include/mdpt.h"""
    import re
    return int(re.search(r"#define MDPT_E_INVALID\s+\(?(-?\d+)\)?", open(native.HEADERS[-1]).read()).group(1))


def test_the_record_table_has_the_layout_of_its_struct():
    r = _common.LOCALFIT_RECORD
    assert r.itemsize == 72
    assert {n: r.fields[n][1] for n in r.names} == {"pred": 0, "ph": 8, "pw": 12, "truth": 16, "valid": 24, "H": 32, "W": 36, "gh": 40, "gw": 44, "cell_off": 48,
                                                    "scratch_off": 56, "out": 64}
    p = _common.PAIR_RECORD  # the first seven fields are mdpt_depth_pair's, at its offsets
    assert all(r.fields[n][1] == p.fields[n][1] and r.fields[n][0] == p.fields[n][0] for n in p.names)
    header = open(native.HEADERS[-1]).read()
    assert ("typedef struct mdpt_localfit_pair { const void* pred; int32_t ph, pw; const void* truth; const void* valid; int32_t H, W, gh, gw; "
            "int64_t cell_off, scratch_off; void* out; }") in header
    assert "#define MDPT_LOCALFIT_MAX_GRID 256" in header and "#define MDPT_LOCALFIT_MAX_RADIUS 64" in header and "#define MDPT_ABI_VERSION 6" in header
    assert "FIVE launches" in header and "mdpt_localfit_apply: ONE" in header
