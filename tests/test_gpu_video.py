"""muggled_dpt_amd.video (mdpt_post_video_*) against the fp64 restatement tests/video_restate.py.

Inputs: a ramp-plus-sine base map in [1, 4.5], per frame a scale exp(N(0, 0.15)), a shift N(0, 0.5), noise N(0, 0.05) (above 1e-2 of the signal) and,
where the map has room, a moving block of value 8; rounded to the dtype. Shapes: 13 x 10 (one partial chunk; 130 = 32 lanes of four pixels and a
tail of 2), 50 x 47 = 2350 samples (two reduction chunks; a tail of 2), 16 x 12 (a multiple of four: the 16- / 8-byte loads), 1 x 1 (every pair a
cut); T = 1, 2, 7. The noise keeps SSR / Syy >= 1e-4, so the identity s^2 = (Syy - a Sxy - b Sy) / n loses at most about 4 digits; asserted on the
CPU when a case is built.

Bounds. Sums of every round within n 2^-52 sum|terms| of math.fsum's, the worst case of ANY summation order; the weights of round k come from the
fit of round k - 1, so each round is compared with the restatement weighting from the DEVICE's sums of the round before (the same solve, the same
bits), which tests that round's summation on its own. A, B, sigma of the independent restatement within 1e-9 relative to max(|A|, |B|, 1), the bound
the align and tile fits hold for this solve (measured on the MI355X: at most 3.1e-14 over every case of this file; sums at most 0.01 of their bound).
Cut flags equal. The filter is bit-equal to the restatement fed the device's table - both compute in fp64 without contraction and round once - and
within one fp32 ulp when the restatement uses its own table. Display: range_rate = 1 is depth_to_color bit for bit; at 0.1 it equals the
restatement except where the restatement reports a tie (a value within 1e-6 of a uint8 step), asserted to be under 0.1 % of the pixels."""
import functools

import numpy as np
import pytest
import torch

from muggled_dpt_amd import postprocess as pp
from muggled_dpt_amd import video
from tests import video_restate as vr
from tests.align_restate import ulps

pytestmark = pytest.mark.gpu

DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
SHAPES = [(13, 10), (50, 47), (16, 12), (1, 1)]


def _round(x: np.ndarray, dtype) -> np.ndarray:
    """the values as the dtype stores them, as float32"""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dtype).float().numpy()


@functools.lru_cache(maxsize=None)
def _clip(dt: str, hw, T: int = 7, seed: int = 3):
    """-> (frames float32 [T,h,w] as the dtype stores them, read-only; the restatement's (table, ab, sums, mags))"""
    rng = np.random.default_rng(seed)
    h, w = hw
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    base = 1.0 + 2.0 * xx / max(w, 1) + 1.0 * yy / max(h, 1) + 0.5 * np.sin(xx / 3.0) * np.cos(yy / 4.0)
    frames = np.zeros((T, h, w))
    for t in range(T):
        s = base + rng.normal(0.0, 0.05, hw)
        if h >= 8 and w >= 8:
            x0 = min(1 + t, w - 3)
            s[h // 2:h // 2 + 3, x0:x0 + 3] = 8.0
        frames[t] = np.exp(rng.normal(0.0, 0.15)) * s + rng.normal(0.0, 0.5)
    frames = _round(frames, DTYPES[dt])
    frames.setflags(write=False)
    ref = vr.fit(frames)
    table, _, sums, _ = ref
    for t in range(1, T):
        if table[t, 3] == 0.0:
            n, syy = sums[-1, t, 0], sums[-1, t, 5]
            s2 = (table[t, 2] / table[t - 1, 0]) ** 2
            assert s2 * n / syy >= 1e-4, (dt, hw, t)
    return frames, ref


def _dev(frames, dt):
    return torch.from_numpy(np.array(frames)).to(DTYPES[dt]).cuda()


def _check_fit(frames, dt, ref=None, **kw):
    """device fit of `frames` against the restatement -> the device's table"""
    x = _dev(frames, dt)
    table, sums = video.video_fit(x, return_sums=True, **kw)
    assert table.dtype == sums.dtype == torch.float64 and table.is_cuda and tuple(table.shape) == (len(frames), 4)
    table, sums = table.cpu().numpy(), sums.cpu().numpy()
    ref_table, _, _, _ = ref if ref is not None else vr.fit(frames, **kw)
    _, _, fed_sums, fed_mags = vr.fit(frames, feed=sums, **kw)
    n = fed_sums[0, :, :1]
    err, bound = np.abs(sums - fed_sums), n * 2.0 ** -52 * fed_mags
    print(f"{dt} {frames.shape}: sums err / bound max {np.max(err / np.maximum(bound, 1e-300)):.3g}")
    assert np.array_equal(sums[0, :, 0], fed_sums[0, :, 0])
    assert np.all(err <= bound)
    assert np.array_equal(table[:, 3], ref_table[:, 3]), (table[:, 3], ref_table[:, 3])
    scale = np.maximum(np.maximum(np.abs(ref_table[:, 0]), np.abs(ref_table[:, 1])), 1.0)[:, None]
    rel = np.abs(table[:, :3] - ref_table[:, :3]) / scale
    print(f"{dt} {frames.shape}: A, B, sigma rel err max {rel.max():.3g}; cuts {ref_table[:, 3].tolist()}")
    assert np.all(rel <= 1e-9)
    return table


@pytest.mark.parametrize("hw", SHAPES)
@pytest.mark.parametrize("dt", list(DTYPES))
def test_fit_against_the_restatement(dt, hw):
    frames, ref = _clip(dt, hw)
    table = _check_fit(frames, dt, ref)
    assert table[0].tolist() == [1.0, 0.0, 0.0, 1.0]
    assert table[1:, 3].tolist() == ([1.0] * 6 if hw == (1, 1) else [0.0] * 6)


@pytest.mark.parametrize("T", [1, 2])
@pytest.mark.parametrize("rounds", [0, 3, 8])
def test_fit_of_short_clips_and_other_round_counts(T, rounds):
    frames, _ = _clip("fp32", (13, 10), T)
    _check_fit(frames, "fp32", rounds=rounds)


@pytest.mark.parametrize("dt", list(DTYPES))
def test_cuts_and_odd_pixels(dt):
    base, _ = _clip(dt, (13, 10))
    rng = np.random.default_rng(5)
    f = [np.array(base[0]), np.array(base[1]), np.array(base[1])]  # 2: identical to the frame before
    spoiled = np.array(base[2])
    spoiled[3, 4], spoiled[7, 1], spoiled[0, 0] = np.nan, np.inf, -np.inf  # 3: pixels that are not finite are left out
    f.append(spoiled)
    f.append(np.full_like(base[0], 2.5))          # 4: flat -> cut; 5: out of a flat frame -> cut
    f.append(np.array(base[3]))
    f.append(_round(10.0 - base[3], DTYPES[dt]))  # 6: anti-correlated (a <= 0) -> cut
    f.append(np.full_like(base[0], np.nan))       # 7: no samples -> cut; 8: out of it -> cut
    f.append(np.array(base[4]))
    f.append(_round(rng.normal(3.0, 1.0, base[0].shape), DTYPES[dt]))  # 9: uncorrelated -> cut
    frames = np.stack(f)
    table = _check_fit(frames, dt)
    assert table[:, 3].tolist() == [1.0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]
    assert table[2, 0] == table[1, 0] and table[2, 1] == table[1, 1]  # a = 1, b = 0 exactly
    rms = float(np.sqrt(np.mean(frames[2].astype(np.float64) ** 2)))
    assert table[2, 2] <= 2.0 ** -20 * rms


def test_chain_leaves_its_range_and_re_anchors():
    base, _ = _clip("fp32", (13, 10))
    frames = np.stack([(base[0].astype(np.float64) * 0.25 ** t).astype(np.float32) for t in range(13)])  # a_t = 4 exactly: A_10 = 2^20, A_11 beyond
    table = _check_fit(frames, "fp32")
    assert table[:, 3].tolist() == [1.0] + [0.0] * 10 + [1.0, 0.0] and table[10, 0] == 2.0 ** 20 and table[12, 0] == 4.0


@pytest.mark.parametrize("hw", SHAPES)
@pytest.mark.parametrize("dt", list(DTYPES))
def test_filter_against_the_restatement(dt, hw):
    frames, (ref_table, *_) = _clip(dt, hw)
    x = _dev(frames, dt)
    table = video.video_fit(x)
    out = video.video_filter(x, table)
    assert out.dtype == torch.float32 and tuple(out.shape) == frames.shape
    got = out.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), vr.temporal_filter(frames, table.cpu().numpy()).view(np.uint32))
    d = ulps(got, vr.temporal_filter(frames, ref_table))
    print(f"{dt} {hw}: filter against the restatement's own table: {d} ulp")
    assert d <= 1
    plain = video.video_filter(x, table, alpha=1.0).cpu().numpy()
    t64 = table.cpu().numpy()
    assert np.array_equal(plain, (t64[:, 0, None, None] * frames.astype(np.float64) + t64[:, 1, None, None]).astype(np.float32))
    other = video.video_filter(x, table, alpha=0.05, tau=0.5).cpu().numpy()
    assert np.array_equal(other.view(np.uint32), vr.temporal_filter(frames, t64, alpha=0.05, tau=0.5).view(np.uint32))


def test_filter_passes_pixels_that_are_not_finite_and_restarts_them():
    base, _ = _clip("fp32", (13, 10))
    frames = np.array(base)
    frames[2, 5, 5], frames[3, 0, 9], frames[4, 12, 0] = np.nan, np.inf, -np.inf
    x = _dev(frames, "fp32")
    table = video.video_fit(x)
    got = video.video_filter(x, table).cpu().numpy()
    want = vr.temporal_filter(frames, table.cpu().numpy())
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    t64 = table.cpu().numpy()
    assert np.isnan(got[2, 5, 5]) and np.isposinf(got[3, 0, 9]) and np.isneginf(got[4, 12, 0])
    assert got[3, 5, 5] == np.float32(t64[3, 0] * float(frames[3, 5, 5]) + t64[3, 1])  # the frame after: o = s


LUT = np.stack([np.arange(256)[::-1], (np.arange(256) * 7) % 256, np.arange(256)], axis=1).astype(np.uint8).reshape(1, 256, 3)


@pytest.mark.parametrize("target_wh, reverse, lut", [(None, False, None), ((29, 37), True, LUT), ((7, 5), False, LUT), (None, True, None)])
def test_display_with_rate_one_is_depth_to_color(target_wh, reverse, lut):
    frames, _ = _clip("fp32", (13, 10))
    x = _dev(frames, "fp32")
    stable, table, state = video.stabilize_video(x)
    got, new_state = video.video_display(stable, table, state, target_wh, reverse, lut, range_rate=1.0)
    want = pp.depth_to_color(stable, target_wh, reverse, False, lut)
    assert got.dtype == torch.uint8 and torch.equal(got, want)
    own = stable[-1] if target_wh is None else pp.scale_prediction(stable[-1:], target_wh)
    assert new_state.display_range.tolist() == [float(own.min()), float(own.max())] and new_state.started.tolist() == [1, 1]


@pytest.mark.parametrize("target_wh, reverse, lut", [(None, False, None), ((29, 37), True, LUT)])
def test_display_with_a_carried_range_against_the_restatement(target_wh, reverse, lut):
    frames, _ = _clip("fp32", (50, 47))
    cut = np.array(frames)
    cut[4] = _round(10.0 - cut[4], torch.float32)  # a cut in the middle: the range re-anchors at frames 4 and 5
    x = _dev(cut, "fp32")
    stable, table, state = video.stabilize_video(x)
    assert table[:, 3].tolist() == [1.0, 0.0, 0.0, 0.0, 1.0, 1.0, 0.0]
    got, new_state = video.video_display(stable, table, state, target_wh, reverse, lut)
    shown = (stable if target_wh is None else pp.scale_prediction(stable, target_wh)).cpu().numpy()
    ranges = vr.display_ranges(shown, table.cpu().numpy(), None, 0.1)
    want, ties = vr.display(shown, ranges, reverse, lut)
    assert ties.mean() < 1e-3
    got = got.cpu().numpy()
    differ = np.any(got != want, axis=-1)
    print(f"display {target_wh}: {int(differ.sum())} pixels differ, {int(ties.sum())} ties")
    assert not np.any(differ & ~ties)
    if lut is None:
        assert np.all(np.abs(got.astype(np.int32) - want.astype(np.int32))[differ] <= 1)
    assert new_state.display_range.cpu().numpy().tolist() == ranges[-1].tolist()
    assert not np.array_equal(ranges[2], [shown[2].min(), shown[2].max()]) and np.array_equal(ranges[5], [shown[5].min(), shown[5].max()])
    # the next batch goes on from the carried range
    t3 = table[:3].cpu().numpy().copy()
    t3[0, 3] = 0.0  # (frame 0 of the table is flagged a start; here only the range rule is under test)
    again_nocut, _ = video.video_display(stable[:3], torch.from_numpy(t3).cuda(), new_state, target_wh, reverse, lut)
    r3 = vr.display_ranges(shown[:3], t3, ranges[-1], 0.1)
    want3, ties3 = vr.display(shown[:3], r3, reverse, lut)
    assert not np.any(np.any(again_nocut.cpu().numpy() != want3, axis=-1) & ~ties3)


def _same_state(a, b):
    return all(torch.equal(getattr(a, k), getattr(b, k)) and getattr(a, k).dtype == getattr(b, k).dtype for k in ("raw", "out", "ab", "display_range", "started"))


@pytest.mark.parametrize("dt", list(DTYPES))
def test_streaming_in_batches_gives_the_bits_of_the_whole_clip(dt):
    frames, _ = _clip(dt, (50, 47))
    x = _dev(frames, dt)

    def run(sizes):
        state, outs, at = None, [], 0
        for n in sizes:
            before = None if state is None else {k: getattr(state, k).clone() for k in ("raw", "out", "ab", "display_range", "started")}
            stable, table, mid = video.stabilize_video(x[at:at + n], state)
            bgr, after = video.video_display(stable, table, mid, (29, 37), False, LUT)
            if state is not None:  # the state passed in is as it was, and a replay from it gives the same bits
                assert all(torch.equal(getattr(state, k), v) for k, v in before.items())
                again = video.stabilize_video(x[at:at + n], state)
                assert torch.equal(again[0], stable) and torch.equal(again[1], table) and _same_state(again[2], mid)
            outs.append((stable, table, bgr))
            state, at = after, at + n
        return [torch.cat([o[k] for o in outs]) for k in range(3)], state

    whole, state_whole = run([7])
    for sizes in ([3, 4], [1] * 7):
        parts, state_parts = run(sizes)
        for a, b in zip(whole, parts):
            assert a.dtype == b.dtype and torch.equal(a, b), sizes
        assert _same_state(state_whole, state_parts), sizes
    twice, state_twice = run([7])
    assert all(torch.equal(a, b) for a, b in zip(whole, twice)) and _same_state(state_whole, state_twice)
    assert state_whole.started.tolist() == [1, 1] and torch.equal(state_whole.raw, x[-1]) and torch.equal(state_whole.out, whole[0][-1])
    assert whole[1][0].tolist() == [1.0, 0.0, 0.0, 1.0] and whole[1][1:, 3].sum() == 0


def test_state_must_match_the_frames():
    frames, _ = _clip("fp32", (13, 10))
    x = _dev(frames, "fp32")
    _, _, state = video.stabilize_video(x)
    with pytest.raises(ValueError, match="state"):
        video.stabilize_video(x[:, :12], state)
    with pytest.raises(ValueError, match="state holds"):
        video.stabilize_video(x.half(), state)
    with pytest.raises(ValueError, match="table"):
        video.video_filter(x, torch.zeros(3, 4, dtype=torch.float64, device="cuda"))
