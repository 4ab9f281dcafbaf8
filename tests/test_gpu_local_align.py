"""local_align.fit_true_depth_local / true_depth_local (mdpt_localfit_*) against the fp64 restatement tests/local_align_restate.py, on the smallest shapes that reach
every path.

Inputs are built as tests/test_gpu_align.py builds them: predictions uniform in [1, 2] rounded to the dtype, t = 0.37 v + 0.25 + e with e ~ N(0, 0.01), the truth
1 / t (inverse space) or t (depth space) as float32; about 30 % of the truth pixels zero, NaN or masked off (with valid = NULL the masked ones count), one NaN or
inf prediction pixel. One call holds: an enlarging pair (13 x 10 -> 37 x 29, grid 4 x 3: cells of 10 / 9 rows and 10 / 10 / 9 columns), a reducing pair (16 x 12 ->
9 x 7, grid 9 x 7: one pixel a cell), a 50 x 47 truth without an invalid pixel on a 1 x 1 grid (2350 samples: two chunks of 2048), a grid with an empty cell row,
pairs with no and with one sample, a constant prediction of 1.5 (var = 0 exactly), a prediction on both sides of zero. Every dtype, space and valid / NULL runs at
radius 1 and prior 0; fp32 runs again at radius 2, at radius 64 (which covers the 4 x 3 grid and every other), and with prior 4 at radius 0 and 1. The prior-4 calls
leave the one-sample pair out: its window and the prior are multiples of one sample, var cancels to rounding noise and its sign is nobody's to define.

Bounds. Counts exact. Cell and global sums within n 2^-52 sum|terms| of math.fsum's, the bound of ANY summation order. Global fit within 1e-9 relative (the align
tests' bound for this solve). Coefficient fields: the tolerance is 16 x the restatement's own noise, recomputed by every test - the largest relative movement of any
node's A or B between the restatement and (a) its np.longdouble run, (b) eight runs whose cell sums add their samples, and whose windows add their cells, in random
orders in plain fp64. Measured on a CPU over the cases of this file: noise 3.6e-13 .. 8.6e-13, so tolerances of 5.8e-12 .. 1.4e-11; measured on an MI355X: the device
differs from the restatement by at most 0.0091 of the tolerance (1.2e-13 relative). The branch condition is asserted on the CPU when a case is built: apart from the exactly
degenerate windows (n < 2, var == 0) none has var or A's numerator within 1e-6 relative of zero, so a device that takes the fallback where the restatement does not
fails. True depth: within one fp32 ulp of float32(the restatement's apply) when that is fed the device's own field; with the restatement's field within the
coefficient tolerance carried through q = A v + B and 1 / q (tol (|A v| + |B|) / |q| relative) plus that ulp, no q within 1e-9 of zero unless it is zero."""
import functools

import numpy as np
import pytest
import torch

from muggled_dpt_amd import local_align as la
from muggled_dpt_amd import postprocess as pp
from tests import align_restate as ar
from tests import local_align_restate as lr

pytestmark = pytest.mark.gpu

DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
A0, B0, NOISE = 0.37, 0.25, 0.01
TRIALS = 8


def _round(x: np.ndarray, dtype) -> np.ndarray:
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dtype).float().numpy()


def _pair(rng, dtype, space, phw, thw, grid, invalid=0.3, lo=1.0, hi=2.0, const=None, keep=None, spoil=None, empty_rows=None):
    """-> (pred, truth, valid, grid): test_gpu_align's _pair with the truth of either space"""
    pred = np.full(phw, const, dtype=np.float64) if const is not None else rng.uniform(lo, hi, phw)
    pred = _round(pred, dtype)
    if spoil:
        pred[phw[0] // 2, phw[1] // 2] = np.nan if spoil == "nan" else np.inf
    v = ar.resample(np.where(np.isfinite(pred), pred, 1.5), thw)
    t = A0 * v + B0 + rng.normal(0.0, NOISE, thw)
    truth = (1.0 / t if space == "inverse" else t).astype(np.float32)
    valid = np.ones(thw, dtype=np.uint8)
    if keep is not None:
        off = rng.permutation(truth.size)[keep:]
        truth.reshape(-1)[off] = 0.0
    elif invalid > 0:
        kind = rng.uniform(0.0, 1.0, thw)
        truth[kind < invalid / 3] = 0.0
        truth[(kind >= invalid / 3) & (kind < 2 * invalid / 3)] = np.nan
        valid[(kind >= 2 * invalid / 3) & (kind < invalid)] = 0
    if empty_rows is not None:
        truth[empty_rows[0]:empty_rows[1]] = 0.0
    return pred, truth, valid, grid


def _reordered_moments(terms, cell, cells, rng) -> np.ndarray:
    """the cell sums with every cell's samples added one by one in a random order, plain fp64"""
    M = np.zeros((cells, 6))
    for c in range(cells):
        idx = np.flatnonzero(cell == c)
        idx = idx[rng.permutation(idx.size)]
        for k in range(6):
            M[c, k] = np.cumsum(terms[k][idx])[-1] if idx.size else 0.0
    return M


@functools.lru_cache(maxsize=None)
def _case(dt: str, space: str, masked: bool, radius: int = 1, prior: float = 0.0):
    """-> dict(names, preds, truths, valids (None: NULL), grids, ref: the restatement per pair, tol: 16 x the restatement's noise)"""
    dtype = DTYPES[dt]
    rng = np.random.default_rng(11)
    pairs = {
        "up": _pair(rng, dtype, space, (13, 10), (37, 29), (4, 3), spoil="nan"),
        "down": _pair(rng, dtype, space, (16, 12), (9, 7), (9, 7), spoil="inf"),
        "two_chunks": _pair(rng, dtype, space, (13, 10), (50, 47), (1, 1), invalid=0.0),
        "empty_row": _pair(rng, dtype, space, (9, 8), (20, 21), (5, 3), empty_rows=(4, 8)),
        "none": _pair(rng, dtype, space, (5, 6), (8, 9), (2, 2), keep=0),
        "one": _pair(rng, dtype, space, (5, 6), (8, 9), (2, 2), keep=1),
        "constant": _pair(rng, dtype, space, (6, 5), (12, 11), (3, 2), const=1.5),
        "signs": _pair(rng, dtype, space, (9, 8), (20, 21), (2, 3), lo=-0.5, hi=1.5),
    }
    if prior > 0:
        del pairs["one"]
    case = dict(names=list(pairs), preds=[p[0] for p in pairs.values()], truths=[p[1] for p in pairs.values()],
                valids=[p[2] if masked else None for p in pairs.values()], grids=[p[3] for p in pairs.values()], dtype=dtype, space=space, radius=radius, prior=prior)
    for a in case["preds"] + case["truths"] + [v for v in case["valids"] if v is not None]:
        a.setflags(write=False)
    refs, noise = [], 0.0
    trial_rng = np.random.default_rng(5)
    for name, p, t, m, g in zip(case["names"], case["preds"], case["truths"], case["valids"], case["grids"]):
        M, A, terms, cell = lr.cell_moments(p, t, m, space, g)
        ref = lr.fit_from_moments(M, radius, prior)
        ref["M"], ref["abs"] = M, A
        ref["global"] = ar.fit_lstsq(*ar.samples(p, t, m, space)[:2])
        assert lr.branch_margin_ok(ref["margins"]), (name, [x for x in ref["margins"] if not lr.branch_margin_ok([x])])
        alts = [lr.fit_from_moments(M, radius, prior, real=np.longdouble)]
        alts += [lr.fit_from_moments(_reordered_moments(terms, cell, g[0] * g[1], trial_rng).reshape(*g, 6), radius, prior, rng=trial_rng) for _ in range(TRIALS)]
        for alt in alts:
            c = alt["coeffs"].astype(np.float64)
            assert np.array_equal(c == 0.0, ref["coeffs"] == 0.0), name  # (no branch moved)
            moved = np.abs(c - ref["coeffs"])[ref["coeffs"] != 0.0] / np.abs(ref["coeffs"][ref["coeffs"] != 0.0])
            noise = max(noise, float(moved.max()) if moved.size else 0.0)
        refs.append(ref)
    case["ref"], case["noise"], case["tol"] = refs, noise, 16.0 * noise
    by = dict(zip(case["names"], refs))
    assert by["two_chunks"]["G"][0] == 2350 and by["none"]["G"][0] == 0 and np.all(by["empty_row"]["M"][1, :, 0] == 0) and np.all(by["empty_row"]["M"][0, :, 0] > 0)
    assert "one" not in by or by["one"]["G"][0] == 1
    assert by["constant"]["fit"][0] == 0.0 and all(x["var"] == 0.0 for x in by["constant"]["margins"])
    assert by["up"]["M"][..., 0].max() <= 100 and 0.5 < by["up"]["G"][0] / (37 * 29) <= 1.0
    assert 0.0 < case["tol"] < 1e-9
    return case


def _dev_preds(case, idx=None):
    idx = range(len(case["preds"])) if idx is None else idx
    return [torch.from_numpy(np.array(case["preds"][i])).to(case["dtype"]).cuda()[None] for i in idx]


def _sel(case, key, idx=None):
    return [case[key][i] for i in (range(len(case["preds"])) if idx is None else idx)]


def _fit(case, idx=None, truths=None, **kw):
    valids = _sel(case, "valids", idx)
    fit = la.fit_true_depth_local(_dev_preds(case, idx), _sel(case, "truths", idx) if truths is None else truths, None if all(v is None for v in valids) else valids,
                                  space=case["space"], grid_hw=_sel(case, "grids", idx), radius=case["radius"], prior=case["prior"], **kw)
    assert isinstance(fit, la.LocalDepthFit) and fit.fit.dtype == fit.sums.dtype == torch.float64 and fit.fit.is_cuda
    assert len({c.untyped_storage().data_ptr() for c in fit.coeffs}) == 1 and all(c.dtype == torch.float64 and c.is_cuda for c in fit.coeffs + fit.moments)
    return fit


def _bits(fit) -> np.ndarray:
    return fit._flat.cpu().numpy().view(np.uint64)


def _check_against_the_restatement(case):
    fit = _fit(case)
    tol = case["tol"]
    worst = 0.0
    for k, (name, ref) in enumerate(zip(case["names"], case["ref"])):
        gh, gw = case["grids"][k]
        M, C = fit.moments[k].cpu().numpy(), fit.coeffs[k].cpu().numpy()
        assert M.shape == (gh, gw, 6) and C.shape == (gh, gw, 2) and fit.grids[k] == (gh, gw)
        assert np.array_equal(M[..., 0], ref["M"][..., 0]), name
        assert np.all(np.abs(M - ref["M"]) <= ref["M"][..., :1] * 2.0 ** -52 * ref["abs"]), name
        (a0, b0), gsums, gabs = ref["global"]
        sums, ab = fit.sums[k].cpu().numpy(), fit.fit[k].cpu().numpy()
        assert sums[0] == gsums[0] and np.all(np.abs(sums - gsums) <= gsums[0] * 2.0 ** -52 * gabs), name
        assert np.all(np.abs(ab - [a0, b0]) <= 1e-9 * np.abs([a0, b0])), (name, ab, a0, b0)
        want = ref["coeffs"]
        assert np.array_equal(C == 0.0, want == 0.0), name
        err = np.abs(C - want)
        assert np.all(err <= tol * np.abs(want)), (name, float(np.max(err / np.maximum(np.abs(want), 1e-300))), tol)
        worst = max(worst, float(np.max(err[want != 0.0] / np.abs(want[want != 0.0]))) if np.any(want != 0.0) else 0.0)
    print(f"{case['dtype']} {case['space']} r{case['radius']} prior {case['prior']}: restatement noise {case['noise']:.3g}, tolerance {tol:.3g}, device / tolerance {worst / tol:.3g}")
    return fit


@pytest.mark.parametrize("masked", [True, False], ids=["valid", "null"])
@pytest.mark.parametrize("space", ["inverse", "depth"])
@pytest.mark.parametrize("dt", list(DTYPES))
def test_fit_and_true_depth_against_the_restatement(dt, space, masked):
    case = _case(dt, space, masked)
    fit = _check_against_the_restatement(case)
    hws = [t.shape for t in case["truths"]]
    for kw in (dict(), dict(clamp=(0.5, 1.9))):
        outs = la.true_depth_local(_dev_preds(case), fit, hws, space=space, **kw)
        assert len({o.untyped_storage().data_ptr() for o in outs}) == 1
        for k, (name, o, ref) in enumerate(zip(case["names"], outs, case["ref"])):
            assert o.shape == (1, *hws[k]) and o.dtype == torch.float32
            got = o[0].cpu().numpy()
            own = lr.apply(case["preds"][k], fit.coeffs[k].cpu().numpy(), hws[k], space, **kw).astype(np.float32)
            assert ar.ulps(got, own) <= 1, (name, kw)
            if kw:
                continue
            d, q = lr.apply(case["preds"][k], ref["coeffs"], hws[k], space, return_q=True)
            ok = np.isfinite(q)
            assert np.all((np.abs(q[ok]) > 1e-9) | (q[ok] == 0.0)), name
            assert np.array_equal(np.isnan(got), np.isnan(d)) and np.array_equal(np.isinf(got), np.isinf(d)), name
            fin = np.isfinite(d) & np.isfinite(q)  # (an inf prediction gives q = inf and d = 0 or inf: equal, not bounded)
            rest = ~fin & ~np.isnan(d)
            assert np.array_equal(got[rest], d[rest].astype(np.float32)), name
            ab = lr.field_at(ref["coeffs"], hws[k])
            v = ar.resample(case["preds"][k], hws[k])
            with np.errstate(all="ignore"):
                size = np.abs(ab[..., 0] * v) + np.abs(ab[..., 1])
                bound = case["tol"] * size / np.abs(q) * np.abs(d) if space == "inverse" else case["tol"] * size
                bound = bound + np.spacing(np.abs(d).astype(np.float32)).astype(np.float64)
            assert np.all(np.abs(got.astype(np.float64)[fin] - d[fin]) <= bound[fin]), name
    by = dict(zip(case["names"], la.true_depth_local(_dev_preds(case), fit, hws, space=space)))
    assert torch.isnan(by["up"]).any() and (torch.isinf(by["none"]).all() if space == "inverse" else (by["none"] == 0).all())
    own_size = la.true_depth_local(_dev_preds(case), fit, space=space)  # the default target is the prediction's own size
    assert [tuple(o.shape[1:]) for o in own_size] == [p.shape for p in case["preds"]]


@pytest.mark.parametrize("radius,prior", [(2, 0.0), (64, 0.0), (0, 4.0), (1, 4.0)])
def test_other_radii_and_the_prior_against_the_restatement(radius, prior):
    case = _case("fp32", "inverse", True, radius, prior)
    fit = _check_against_the_restatement(case)
    if radius == 64:  # the window covers every grid: one coefficient a pair
        for c in fit.coeffs:
            flat = c.reshape(-1, 2)
            assert torch.equal(flat, flat[:1].expand_as(flat))
    if prior > 0:  # the empty cell row's nodes at radius 0 take the global fit itself
        k = case["names"].index("empty_row")
        if radius == 0:
            assert torch.equal(fit.coeffs[k][1].view(torch.int64), fit.fit[k].expand(3, 2).contiguous().view(torch.int64))


def test_the_same_call_twice_and_every_pair_alone_give_equal_bits():
    case = _case("bf16", "inverse", True)
    fit = _fit(case)
    assert np.array_equal(_bits(fit), _bits(_fit(case)))
    hws = [t.shape for t in case["truths"]]
    maps = la.true_depth_local(_dev_preds(case), fit, hws)
    again = la.true_depth_local(_dev_preds(case), fit, hws)
    for k, name in enumerate(case["names"]):
        assert torch.equal(maps[k].view(torch.int32), again[k].view(torch.int32)), name
        alone = _fit(case, [k])
        for part in ("coeffs", "moments"):
            assert torch.equal(getattr(alone, part)[0].view(torch.int64), getattr(fit, part)[k].view(torch.int64)), (name, part)
        assert torch.equal(alone.fit.view(torch.int64), fit.fit[k:k + 1].view(torch.int64)) and torch.equal(alone.sums.view(torch.int64), fit.sums[k:k + 1].view(torch.int64)), name
        one = la.true_depth_local(_dev_preds(case, [k]), alone, [hws[k]])[0]
        assert torch.equal(one.view(torch.int32), maps[k].view(torch.int32)), name
    rev = list(range(len(case["names"])))[::-1]  # reversed order: every pair keeps its results
    back = _fit(case, rev)
    for k, r in enumerate(rev):
        assert torch.equal(back.coeffs[k].view(torch.int64), fit.coeffs[r].view(torch.int64))


def test_host_truths_and_device_truths_give_equal_bits():
    case = _case("fp16", "depth", True)
    host = _fit(case)
    dev = _fit(case, truths=[torch.from_numpy(np.array(t)).cuda() for t in case["truths"]])
    assert np.array_equal(_bits(host), _bits(dev))
    masks = la.fit_true_depth_local(_dev_preds(case), case["truths"], [torch.from_numpy(np.array(v)).cuda() for v in case["valids"]], space="depth",
                                    grid_hw=case["grids"], radius=1, prior=0.0)
    assert np.array_equal(_bits(host), _bits(masks))


@pytest.mark.parametrize("dt", list(DTYPES))
def test_a_one_by_one_grid_without_prior_is_fit_true_depth(dt):
    case = _case(dt, "inverse", True)
    ones = [(1, 1)] * len(case["names"])
    fit = la.fit_true_depth_local(_dev_preds(case), case["truths"], case["valids"], grid_hw=ones, radius=1, prior=0.0)
    want, sums = pp.fit_true_depth(_dev_preds(case), case["truths"], case["valids"], return_sums=True)
    got = torch.stack([c[0, 0] for c in fit.coeffs])
    for have in (got, fit.fit):
        assert torch.all((have - want).abs() <= 1e-9 * want.abs()), (have, want)
    assert torch.equal(fit.sums[:, 0], sums[:, 0]) and torch.all((fit.sums - sums).abs() <= 1e-12 * sums.abs())
    hws = [t.shape for t in case["truths"]]
    for kw in (dict(), dict(space="depth", clamp=(None, 0.9))):
        mine, theirs = la.true_depth_local(_dev_preds(case), fit, hws, **kw), pp.true_depth(_dev_preds(case), want, hws, **kw)
        for name, a, b in zip(case["names"], mine, theirs):
            assert ar.ulps(a.cpu().numpy(), b.cpu().numpy()) <= 1, (name, kw)


def test_the_prototype_scene_on_the_device_loses_the_drift():
    pred, truth, valid = lr.drift_scene()
    hold = valid == 0
    preds = [torch.from_numpy(pred).cuda()[None]]
    glob = pp.true_depth(preds, pp.fit_true_depth(preds, [truth], [valid]), [truth.shape])[0][0].cpu().numpy()
    g = lr.abs_rel(glob, truth, hold)
    assert 300 <= int(valid.sum()) <= 500
    for prior in (0.0, 4.0):
        fit = la.fit_true_depth_local(preds, [truth], [valid], grid_hw=(6, 8), radius=1, prior=prior)
        loc = lr.abs_rel(la.true_depth_local(preds, fit, [truth.shape])[0][0].cpu().numpy(), truth, hold)
        print(f"prior {prior}: hold-out AbsRel global {g:.4f}, local {loc:.4f} ({loc / g:.3f} of it)")
        assert loc <= g / 3.0
    # depth_metrics scores a completed map as it is (fit=None, space="depth"): at the measured pixels the same one-third condition holds (the restatement:
    # AbsRel 0.0913 for the global fit, 0.0203 for prior 4)
    m = pp.depth_metrics(la.true_depth_local(preds, fit, [truth.shape]), [truth], None, [valid], space="depth")
    m_glob = pp.depth_metrics([torch.from_numpy(glob).cuda()[None]], [truth], None, [valid], space="depth")
    assert m[0, 0].item() == valid.sum() and m[0, 2].item() <= m_glob[0, 2].item() / 3.0
