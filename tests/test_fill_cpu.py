"""The numpy restatement of the depth-banded push-pull hole filling (tests/fill_restate.py) checked against what the definition implies, and the
cases of tests/test_gpu_fill.py held to at most 2 % unsafe pixels per image (a condition on the cases, not a tolerance)."""
import numpy as np
import pytest

from tests import fill_restate as fr


def _image(h, w, seed=0):
    rng = np.random.default_rng(seed)
    color = rng.integers(0, 256, size=(h, w, 4)).astype(np.uint8)
    color[..., 3] = 255
    return color, rng.uniform(1.0, 10.0, size=(h, w)).astype(np.float32)


def test_level_sizes_halve_rounding_up_to_one_node():
    assert fr.level_sizes(1, 1) == [(1, 1)]
    assert fr.level_sizes(5, 3) == [(5, 3), (3, 2), (2, 1), (1, 1)]
    assert fr.level_sizes(1, 7) == [(1, 7), (1, 4), (1, 2), (1, 1)]
    assert fr.level_sizes(130, 67)[3] == (17, 9)


@pytest.mark.parametrize("band", [0.0, 0.1, 0.37, 1.0])
def test_an_image_without_holes_is_returned_as_it_is(band):
    color, depth = _image(13, 22)
    color[..., 3] = np.random.default_rng(1).integers(1, 256, size=(13, 22))  # (any alpha but 0 is valid and is copied)
    r = fr.fill(color, depth, band)
    np.testing.assert_array_equal(r["color"], color)
    assert r["depth"].tobytes() == depth.tobytes() and r["safe"].all()


@pytest.mark.parametrize("band", [0.0, 0.1, 1.0])
@pytest.mark.parametrize("hw, at", [((9, 14), (3, 11)), ((1, 7), (0, 6)), ((5, 3), (4, 0)), ((33, 17), (32, 16))])
def test_one_valid_pixel_fills_the_whole_image(hw, at, band):
    color = np.zeros(hw + (4,), dtype=np.uint8)
    depth = np.full(hw, np.inf, dtype=np.float32)
    color[at], depth[at] = (17, 130, 251, 255), 3.7
    r = fr.fill(color, depth, band)
    assert (r["color"] == np.array([17, 130, 251, 255], dtype=np.uint8)).all()
    assert (r["depth"] == np.float32(3.7)).all() and r["safe"].all()


def _two_layers():
    """left: a red foreground at depth 1, right: a blue background at depth 4, a strip of holes between them (columns 9 .. 14 of 24)"""
    color = np.zeros((16, 24, 4), dtype=np.uint8)
    depth = np.full((16, 24), np.inf, dtype=np.float32)
    color[:, :9], depth[:, :9] = (0, 0, 255, 255), 1.0
    color[:, 15:], depth[:, 15:] = (255, 0, 0, 255), 4.0
    return color, depth


def test_the_band_keeps_the_foreground_out_of_a_disocclusion():
    color, depth = _two_layers()
    hole = color[..., 3] == 0
    r = fr.fill(color, depth, 0.25)
    assert (r["color"][hole] == np.array([255, 0, 0, 255], dtype=np.uint8)).all() and (r["depth"][hole] == 4.0).all()
    assert r["safe"].all()
    np.testing.assert_array_equal(r["color"][~hole], color[~hole])
    plain = fr.fill(color, depth, 1.0)
    assert (plain["color"][hole][:, 3] == 255).all()
    assert (plain["color"][hole] != np.array([255, 0, 0, 255], dtype=np.uint8)).any(axis=-1).any()  # without the band the red bleeds in


def test_an_empty_image_stays_background():
    rng = np.random.default_rng(3)
    color = rng.integers(0, 256, size=(11, 6, 4)).astype(np.uint8)
    depth = rng.uniform(1, 2, size=(11, 6)).astype(np.float32)
    color[:6, :, 3] = 0          # alpha 0 over a finite depth
    depth[6:] = np.inf           # alpha != 0 over an infinite depth
    depth[7, 2], depth[8, 3], depth[9, 1] = np.nan, 0.0, -1.0
    r = fr.fill(color, depth, 0.1)
    assert (r["color"] == 0).all() and np.isposinf(r["depth"]).all() and r["safe"].all()


def test_near_threshold_comparisons_are_flagged_and_exact_ties_at_band_zero_are_not():
    color = np.zeros((2, 2, 4), dtype=np.uint8)
    color[..., 3] = 255
    color[1, 1, 3] = 0
    depth = np.array([[10.0, 9.0 * (1 + 5e-7)], [5.0, np.inf]], dtype=np.float32)
    assert not fr.fill(color, depth, 0.1)["safe"][1, 1]  # 9 (1 + 5e-7) against 0.9 x 10
    assert fr.fill(color, depth, 0.3)["safe"].all()  # (7 is far from 5, 9 and 10)
    depth = np.array([[10.0, 10.0], [5.0, np.inf]], dtype=np.float32)
    r = fr.fill(color, depth, 0.0)
    assert r["safe"].all() and r["depth"][1, 1] == 10.0
    depth[0, 1] = np.nextafter(np.float32(10.0), np.float32(0.0))
    assert not fr.fill(color, depth, 0.0)["safe"][1, 1]


@pytest.mark.parametrize("family, band", fr.FAMILIES, ids=[f"{f}-{b}" for f, b in fr.FAMILIES])
@pytest.mark.parametrize("hw", fr.SIZES, ids=[f"{h}x{w}" for h, w in fr.SIZES])
def test_gpu_cases_are_mostly_safe(hw, family, band):
    color, depth = fr.case(*hw, family)
    refs = fr.reference(*hw, family, band)
    for i, r in enumerate(refs):
        share = float((~r["safe"]).mean())
        assert share <= 0.02, (hw, family, band, i, share)
        if family == "pow2":
            assert share == 0.0
            assert all(np.isin(d, (0.0, 1.0, 2.0, 4.0, 8.0)).all() for d in r["levels"])
    assert (refs[0]["color"] == 0).all() and np.isposinf(refs[0]["depth"]).all()
    np.testing.assert_array_equal(refs[1]["color"], color[1])
    valid = refs[2]["valid"]
    assert valid.any() and (hw == (1, 1) or not valid.all())
    assert (refs[2]["color"][..., 3] == 255).all() and np.isfinite(refs[2]["depth"]).all()
