"""The video block without a GPU: the rule itself (tests/video_restate.py) on a synthetic clip, the chain's re-anchoring, the cuts, the argument
checks of muggled_dpt_amd.video and the four exported entry points.

The clip (video_restate.scene, seed 0): a 24 x 32 ramp-plus-sine background, an 8 x 6 block of value 8 moving 2 px a frame, noise 0.02, and per
frame a scale exp(N(0, 0.15)) and a shift N(0, 0.5); 12 frames. Measured with this restatement (seeds 0 .. 3): three reweighted rounds recover
every pair's scale within 0.18 % (seed 0: 0.14 %), plain least squares (rounds = 0) misses every pair by at least 16.6 % (the block drags it). The
mean temporal standard deviation of the pixels outside the block's rows falls from 0.541 raw to 0.0191 aligned (28 x) and to 0.00898 after the
filter (a further 2.1 x); asserted: 10 x and 1.5 x."""
import ctypes

import numpy as np
import pytest
import torch

from muggled_dpt_amd import native, video
from tests import video_restate as vr


@pytest.fixture(scope="module")
def clip():
    frames, scales, shifts, rows = vr.scene(seed=0)
    frames.setflags(write=False)
    return frames, scales, rows


def _pair_scales(table):
    return table[1:, 0] / table[:-1, 0]


def test_reweighted_rounds_recover_the_scale_that_least_squares_misses(clip):
    frames, scales, _ = clip
    true = scales[:-1] / scales[1:]
    robust, *_ = vr.fit(frames, rounds=3)
    plain, *_ = vr.fit(frames, rounds=0, cut_corr=0.0)
    assert robust[:, 3].tolist() == [1.0] + [0.0] * 11 and plain[:, 3].tolist() == [1.0] + [0.0] * 11
    err_robust, err_plain = np.abs(_pair_scales(robust) / true - 1.0), np.abs(_pair_scales(plain) / true - 1.0)
    print(f"pair scale error: rounds=3 max {err_robust.max():.3%}, rounds=0 min {err_plain.min():.3%}")
    assert err_robust.max() < 0.01
    assert err_plain.min() > 0.10


def test_alignment_and_filter_quiet_the_static_pixels(clip):
    frames, _, rows = clip
    table, *_ = vr.fit(frames)
    keep = np.ones(frames.shape[1], dtype=bool)
    keep[rows] = False
    aligned = table[:, 0, None, None] * frames + table[:, 1, None, None]
    filtered = vr.temporal_filter(frames, table).astype(np.float64)
    raw_sd, aligned_sd, filtered_sd = (v[:, keep].std(0).mean() for v in (frames, aligned, filtered))
    print(f"temporal sd: raw {raw_sd:.4g}, aligned {aligned_sd:.4g}, filtered {filtered_sd:.4g}")
    assert raw_sd >= 10.0 * aligned_sd
    assert aligned_sd >= 1.5 * filtered_sd
    # the block itself is motion: where it arrives the filter lets it through (within the noise of the aligned frame)
    t, x0 = 5, 2 + 2 * 5
    assert np.all(np.abs(filtered[t, rows, x0 + 6:x0 + 8] - aligned[t, rows, x0 + 6:x0 + 8]) < 0.05 * 8.0)


def test_alpha_one_is_alignment_only(clip):
    frames, _, _ = clip
    table, *_ = vr.fit(frames)
    out = vr.temporal_filter(frames, table, alpha=1.0)
    assert np.array_equal(out, (table[:, 0, None, None] * frames + table[:, 1, None, None]).astype(np.float32))


def test_chain_re_anchors_when_the_scale_leaves_its_range():
    recs = [(1.0, 0.0, 0.0, vr.START)] + [(0.25, 0.5, 1e-4, vr.RUN)] * 12
    table, ab = vr.chain(recs)
    # 0.25^10 = 2^-20 is still inside, 0.25^11 is not: frame 11 re-anchors, frame 12 goes on from A = 1
    assert table[:, 3].tolist() == [1.0] + [0.0] * 10 + [1.0, 0.0]
    assert table[10, 0] == 2.0 ** -20 and table[11].tolist() == [1.0, 0.0, 0.0, 1.0] and table[12, 0] == 0.25 and ab == (0.25, 0.5)
    assert table[2, 1] == 0.25 * 0.5 + 0.5 and table[2, 2] == 0.25 * 1e-2
    up, _ = vr.chain([(1.0, 0.0, 0.0, vr.START)] + [(4.0, 0.0, 0.0, vr.RUN)] * 12)
    assert up[:, 3].tolist() == [1.0] + [0.0] * 10 + [1.0, 0.0] and up[10, 0] == 2.0 ** 20


def test_degenerate_pairs_are_cuts(clip):
    frames, _, _ = clip
    rng = np.random.default_rng(1)
    base = frames[0]
    cases = {"flat": np.full_like(base, 2.5), "anti": 10.0 - base, "nan": np.full_like(base, np.nan), "noise": rng.normal(0.0, 1.0, base.shape)}
    for name, frame in cases.items():
        table, *_ = vr.fit(np.stack([base, frame, base]))
        assert table[:, 3].tolist() == [1.0, 1.0, 1.0], name  # (the way into the odd frame and the way out of it)
        assert table[1].tolist() == [1.0, 0.0, 0.0, 1.0], name
    rec, sums, _ = vr.fit_pair(base, base)
    assert rec == (1.0, 0.0, 0.0, vr.EXACT) and np.array_equal(sums[0], sums[3])
    one = np.full_like(base, np.nan)
    one[0, 0] = 1.0
    assert vr.fit_pair(base, one)[0][3] == vr.CUT  # a single sample


def test_carried_range_follows_slowly_and_re_anchors_at_a_cut():
    frames = np.stack([np.linspace(lo, hi, 12, dtype=np.float32).reshape(3, 4) for lo, hi in ((0, 1), (0, 2), (1, 3), (5, 6))])
    table = np.zeros((4, 4))
    table[0, 3] = table[3, 3] = 1.0
    r = vr.display_ranges(frames, table, rate=0.5)
    assert r.tolist() == [[0.0, 1.0], [0.0, 1.5], [0.5, 2.25], [5.0, 6.0]]
    assert vr.display_ranges(frames, table, rate=1.0).tolist() == [[0.0, 1.0], [0.0, 2.0], [1.0, 3.0], [5.0, 6.0]]
    assert vr.display_ranges(frames[1:3], table[1:3], range_in=(0.0, 1.0), rate=0.5).tolist() == r[1:3].tolist()
    bgr, _ = vr.display(frames[1:2], r[1:2])
    assert bgr.shape == (1, 3, 4, 3) and bgr[0, 0, 0, 0] == 0 and bgr[0, -1, -1, 0] == 255  # (2 > hi = 1.5 clamps)


def test_python_arguments_are_checked_before_anything_runs():
    x = torch.zeros(2, 4, 5)
    for bad in (dict(rounds=-1), dict(rounds=9), dict(rounds=2.0), dict(rounds=True), dict(c=0.0), dict(c=float("nan")), dict(cut_corr=1.5), dict(cut_corr=-0.1)):
        with pytest.raises(ValueError, match="video_fit"):
            video.video_fit(x, **bad)
        with pytest.raises(ValueError, match="stabilize_video"):
            video.stabilize_video(x, **bad)
    table = torch.zeros(2, 4, dtype=torch.float64)
    for bad in (dict(alpha=0.0), dict(alpha=1.01), dict(alpha=float("nan")), dict(tau=-1.0), dict(tau=float("inf"))):
        with pytest.raises(ValueError, match="video_filter"):
            video.video_filter(x, table, **bad)
        with pytest.raises(ValueError, match="stabilize_video"):
            video.stabilize_video(x, **bad)
    for bad in (dict(range_rate=0.0), dict(range_rate=1.5), dict(target_wh=(0, 4))):
        with pytest.raises(ValueError, match="video_display"):
            video.video_display(x, table, **bad)
    # there is no CPU implementation: host tensors raise
    for call in (lambda: video.video_fit(x), lambda: video.video_filter(x, table), lambda: video.video_display(x, table), lambda: video.stabilize_video(x)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    assert "not a measured optimum" in video.video_fit.__doc__ and "out of scope" in video.video_display.__doc__


def test_entry_points_are_exported_and_the_scratch_query_rejects_bad_sizes():
    lib = native.load()
    for name in ("mdpt_post_video_scratch_bytes", "mdpt_post_video_fit", "mdpt_post_video_filter", "mdpt_post_video_display"):
        assert name in native.SYMBOLS and hasattr(lib, name)
    assert "post_video.inc" in native.HEADERS and list(native.HEADERS[:-1]) == sorted(native.HEADERS[:-1])
    need = ctypes.c_size_t()
    assert lib.mdpt_post_video_scratch_bytes(32, 504, 504, 0, 0, ctypes.byref(need)) == 0
    chunks = (504 * 504 + 2047) // 2048
    assert need.value == max(8 * (32 * chunks * 6 + 32 * 4), 2 * 32 * 64 * 2 * 4 + 32 * 504 * 504)
    assert lib.mdpt_post_video_scratch_bytes(2, 5, 7, 9, 11, ctypes.byref(need)) == 0
    assert need.value == (2 * 2 * 64 * 2 * 4 + 2 * 9 * 11 * 4 + 2 * 9 * 11 + 7) // 8 * 8
    for bad in ((0, 4, 4, 0, 0), (65536, 4, 4, 0, 0), (1, 0, 4, 0, 0), (1, 4, -1, 0, 0), (1, 65536, 65536, 0, 0), (1, 4, 4, 3, 0), (1, 4, 4, -1, -1),
                (1, 4, 4, 65536, 65536)):
        assert lib.mdpt_post_video_scratch_bytes(*bad, ctypes.byref(need)) != 0, bad
        assert lib.mdpt_last_error()
    assert lib.mdpt_post_video_scratch_bytes(1, 4, 4, 0, 0, None) != 0
    # the entry points check their scalars before they touch a pointer (4096 is not a device address: nothing may be launched with it)
    p = 4096
    assert lib.mdpt_post_video_fit(p, 0, 1, 4, 4, p, p, p, 9, 2.0, 0.5, p, p, None, p, 1 << 20, None) != 0 and b"rounds" in lib.mdpt_last_error()
    assert lib.mdpt_post_video_fit(p, 0, 1, 4, 4, p, p, p, 3, 2.0, 0.5, p, p, None, p, 8, None) != 0 and b"scratch" in lib.mdpt_last_error()
    assert lib.mdpt_post_video_filter(p, 0, 1, 4, 4, p, p, 0.0, 3.0, 8192, None) != 0 and b"alpha" in lib.mdpt_last_error()
    assert lib.mdpt_post_video_display(p, 1, 4, 4, p, p, p, 0, 0, 0, None, 0.0, p, None, p, p, 1 << 20, None) != 0 and b"range_rate" in lib.mdpt_last_error()
    assert lib.mdpt_abi_version() == 6
