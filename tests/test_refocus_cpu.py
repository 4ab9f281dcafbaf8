"""The synthetic depth of field without a GPU: the properties of the restatement (tests/refocus_restate.py), which are the specification; the argument
checks of muggled_dpt_amd.refocus; the two exported entry points, which refuse bad arguments before they touch a device pointer."""
import ctypes
import math

import numpy as np
import pytest
import torch

from muggled_dpt_amd import native, refocus
from tests import refocus_restate as rr


def test_lattice_counts_against_the_row_formula():
    counts = rr.lattice_counts()
    assert counts.shape == (1025,) and counts[:5].tolist() == [1, 5, 9, 9, 13] and counts[1024] == 3209
    for k in range(1025):  # row dy of the disc holds 2 floor(sqrt(k - dy^2)) + 1 points
        r = math.isqrt(k)
        assert counts[k] == sum(2 * math.isqrt(k - dy * dy) + 1 for dy in range(-r, r + 1)), k
    assert all(int(c) % 4 == 1 for c in counts)  # the centre and four-fold symmetry: a disc mean never falls on a rounding boundary


def test_a_uniform_photo_comes_back_unchanged_whatever_the_map():
    rng = np.random.default_rng(0)
    photo = np.empty((23, 31, 3), np.uint8)
    photo[...] = (17, 200, 93)
    for space, p in (("inverse", rng.uniform(0.0, 5.0, (6, 8))), ("depth", rng.uniform(0.2, 9.0, (23, 31)))):
        out, rq, _ = rr.refocus(p.astype(np.float32), photo, focus=0.4 if space == "inverse" else 2.0, aperture=30.0, max_radius=7, space=space)
        assert rq.max() > 8 and np.array_equal(out, photo), space


def test_no_aperture_no_radius_or_a_flat_map_return_the_photo():
    rng = np.random.default_rng(1)
    photo = rng.integers(0, 256, (19, 27, 3), dtype=np.uint8)
    p = rng.uniform(0.0, 1.0, (5, 6)).astype(np.float32)
    for kw in (dict(aperture=0.0), dict(max_radius=0)):
        out, rq, _ = rr.refocus(p, photo, **kw)
        assert not rq.any() and np.array_equal(out, photo), kw
    flat = np.full((5, 6), 3.25, np.float32)
    out, rq, e32 = rr.refocus(flat, photo, focus=0.9, aperture=100.0)
    assert not rq.any() and not e32.any() and np.array_equal(out, photo)
    out, rq, _ = rr.refocus(np.full((5, 6), np.nan, np.float32), photo, aperture=100.0)
    assert not rq.any() and np.array_equal(out, photo)
    out, rq, _ = rr.refocus(p, photo, focus=0.5, aperture=2.0, focus_range=1.0)  # |e| <= 0.5 everywhere: all of it inside the sharp band
    assert not rq.any() and np.array_equal(out, photo)


def test_a_sharp_foreground_is_kept_and_the_background_is_the_disc_mean():
    """40 x 40, the map at photo size: a near 8 x 8 square (1) on a far background (0), focus on the square. Background: e = -1, r = 5, rq = 20, k = 25, N = 81."""
    rng = np.random.default_rng(2)
    photo = rng.integers(0, 256, (40, 40, 3), dtype=np.uint8)
    p = np.zeros((40, 40), np.float32)
    p[16:24, 16:24] = 1.0
    out, rq, e32 = rr.refocus(p, photo, focus=1.0, aperture=5.0, max_radius=5)
    assert np.array_equal(out[16:24, 16:24], photo[16:24, 16:24])  # every foreground pixel, byte for byte
    assert not rq[16:24, 16:24].any() and (rq[:16] == 20).all() and (e32[:16] == -1.0).all()
    d = np.arange(-5, 6)
    disc = (d[:, None] ** 2 + d[None, :] ** 2) <= 25
    assert disc.sum() == 81
    for y, x in ((7, 7), (5, 30), (33, 9), (34, 34), (20, 6)):  # farther than 5 from the square and from the border
        mean = photo[y - 5:y + 6, x - 5:x + 6].astype(np.float64)[disc].sum(axis=0) / 81.0
        assert np.array_equal(out[y, x], np.floor(mean + 0.5).astype(np.uint8)), (y, x)
    # and the reverse: focus on the background, the blurred square spreads over the sharp pixels around it
    out, rq, _ = rr.refocus(p, photo, focus=0.0, aperture=5.0, max_radius=5)
    assert not rq[:16].any() and (rq[16:24, 16:24] == 20).all()
    assert not np.array_equal(out[14, 20], photo[14, 20]) and np.array_equal(out[9, 20], photo[9, 20])


def test_a_pointed_focus_has_no_defocus_at_its_pixel():
    rng = np.random.default_rng(3)
    H, W = 21, 34
    for space, p in (("inverse", rng.uniform(-3.0, 3.0, (6, 5))), ("depth", rng.uniform(0.5, 20.0, (6, 5)))):
        for xy in ((0.0, 0.0), (1.0, 1.0), (0.37, 0.81)):
            rq, e32 = rr.defocus_planes(p.astype(np.float32), H, W, focus_xy=xy, aperture=50.0, space=space)
            at = (min(H - 1, int(xy[1] * H)), min(W - 1, int(xy[0] * W)))
            assert e32[at] == 0.0 and rq[at] == 0 and rq.any(), (space, xy)
    bad = rng.uniform(0.5, 20.0, (H, W)).astype(np.float32)
    bad[0, 0], bad[H - 1, W - 1] = -1.0, np.inf
    for xy in ((0.0, 0.0), (1.0, 1.0)):  # a pointed depth that is not > 0, or not finite: everything is in focus
        rq, e32 = rr.defocus_planes(bad, H, W, focus_xy=xy, aperture=50.0, space="depth")
        assert not rq.any() and not e32.any()
    rq, _ = rr.defocus_planes(bad, H, W, focus=3.0, aperture=50.0, space="depth")
    assert rq[H - 1, W - 1] == 0 and rq[0, 0] == min(64, math.floor(4 * 50.0 / 3.0))  # inf: in focus; a depth <= 0: infinitely far


def test_python_arguments_are_checked_before_anything_runs():
    maps = [torch.zeros(1, 4, 5), torch.zeros(1, 3, 3)]
    photos = [np.zeros((8, 9, 3), np.uint8), np.zeros((2, 2, 3), np.uint8)]  # (a photo may be smaller than its map)
    bad_calls = (dict(max_radius=33), dict(max_radius=-1), dict(max_radius=2.0), dict(max_radius=True), dict(aperture=-1.0), dict(aperture=float("nan")),
                 dict(aperture=float("inf")), dict(focus_range=-0.1), dict(focus_range=float("inf")), dict(focus=1.5), dict(focus=-0.1), dict(focus=float("nan")),
                 dict(focus=0.0, space="depth"), dict(focus=float("inf"), space="depth"), dict(space="linear"), dict(focus_xy=(0.5,)), dict(focus_xy=(0.5, 1.5)),
                 dict(focus_xy=(-0.1, 0.5)))
    for fn in (refocus.refocus_images, refocus.defocus_planes):
        for bad in bad_calls:
            with pytest.raises(ValueError, match=fn.__name__):
                fn(maps, photos, **bad)
        with pytest.raises(ValueError, match="2 predictions but 1 images"):
            fn(maps, photos[:1])
        with pytest.raises(ValueError, match="image 1 is not a uint8"):
            fn(maps, [photos[0], np.zeros((2, 2, 3), np.float32)])
        with pytest.raises(ValueError, match="image 0 is not a uint8"):
            fn(maps, [np.zeros((8, 9), np.uint8), photos[1]])
        with pytest.raises(RuntimeError, match="no CPU fallback"):  # there is no CPU implementation: host maps raise
            fn(maps, photos)
    assert "not measured optima" in refocus.refocus_images.__doc__ and "not inpainted" in refocus.__doc__ and "unverified" in refocus.__doc__


def _records(H=8, W=9, n=1):
    rec = np.zeros(n, dtype=refocus.REFOCUS_RECORD)
    rec["map"], rec["photo"], rec["out"] = 4096, 8192, 12288  # (not device addresses: nothing may be launched with them)
    rec["h"], rec["w"], rec["H"], rec["W"], rec["pitch"] = 4, 5, H, W, 3 * W
    per = 1024 + 8 * H * W
    rec["scratch_off"] = per * np.arange(n)
    rec["tile_off"] = ((H + 31) // 32) * ((W + 31) // 32) * np.arange(n)
    return rec


def test_entry_points_are_exported_and_refuse_bad_arguments_without_a_device():
    lib = native.load()
    for name in ("mdpt_post_refocus_scratch_bytes", "mdpt_post_refocus"):
        assert name in native.SYMBOLS and hasattr(lib, name)
    assert "post_refocus.inc" in native.HEADERS and native.REFOCUS_MAX_RADIUS == 32 and native.REFOCUS_TILE == 32
    assert lib.mdpt_abi_version() == 6 == native.ABI_VERSION
    need = ctypes.c_size_t()
    rec = _records(70, 33, 3)
    assert lib.mdpt_post_refocus_scratch_bytes(rec.ctypes.data, 3, 16, ctypes.byref(need)) == 0 and need.value == 3 * (1024 + 8 * 70 * 33)
    huge = _records(65536, 32768)
    for args, word in (((None, 1, 16), b"records"), ((rec.ctypes.data, 0, 16), b"n ="), ((rec.ctypes.data, 65536, 16), b"n ="), ((rec.ctypes.data, 3, 33), b"max_radius"),
                       ((rec.ctypes.data, 3, -1), b"max_radius"), ((huge.ctypes.data, 1, 16), b"2^31")):
        assert lib.mdpt_post_refocus_scratch_bytes(*args, ctypes.byref(need)) != 0 and word in lib.mdpt_last_error(), args
    assert lib.mdpt_post_refocus_scratch_bytes(rec.ctypes.data, 3, 16, None) != 0

    p, big = 4096, 1 << 30

    def call(r=rec, dev=p, n=3, dtype=0, space=0, focus=0.5, xy=None, aperture=32.0, focus_range=0.0, max_radius=16, scratch=p, nbytes=big, rq=p, e32=p):
        xy = None if xy is None else (ctypes.c_double * 2)(*xy)
        return lib.mdpt_post_refocus(None if r is None else r.ctypes.data, dev, n, dtype, space, focus, xy, aperture, focus_range, max_radius, scratch, nbytes, rq, e32, None)

    wrong_tiles = _records(70, 33, 3)
    wrong_tiles["tile_off"][2] = 5
    some_out = _records(70, 33, 3)
    some_out["out"][1] = 0
    no_out = _records(70, 33, 3)
    no_out["out"] = 0
    narrow = _records(70, 33, 3)
    narrow["pitch"][0] = 98
    for kw, word in ((dict(r=None), b"null"), (dict(dev=None), b"null"), (dict(scratch=None), b"null"), (dict(n=0), b"n ="), (dict(dtype=7), b"dtype"),
                     (dict(space=2), b"space"), (dict(max_radius=33), b"max_radius"), (dict(max_radius=-1), b"max_radius"), (dict(aperture=-1.0), b"aperture"),
                     (dict(aperture=float("nan")), b"aperture"), (dict(aperture=float("inf")), b"aperture"), (dict(focus_range=-1.0), b"focus_range"),
                     (dict(focus_range=float("inf")), b"focus_range"), (dict(focus=1.5), b"focus"), (dict(focus=float("nan")), b"focus"),
                     (dict(focus=0.0, space=1), b"focus"), (dict(xy=(0.5, 1.5)), b"focus_xy"), (dict(nbytes=3 * (1024 + 8 * 70 * 33) - 8), b"scratch"),
                     (dict(r=huge, n=1), b"2^31"), (dict(r=wrong_tiles), b"tile_off"), (dict(r=some_out), b"out"), (dict(r=no_out, rq=None, e32=None), b"radius_out"),
                     (dict(r=narrow), b"pitch"), (dict(scratch=4100), b"misaligned"), (dict(e32=4098), b"misaligned")):
        assert call(**kw) != 0, kw
        assert word in lib.mdpt_last_error(), (kw, lib.mdpt_last_error())


def test_the_record_table_has_the_layout_of_its_struct():
    r = refocus.REFOCUS_RECORD
    assert r.itemsize == 64
    assert {n: r.fields[n][1] for n in r.names} == {"map": 0, "h": 8, "w": 12, "photo": 16, "pitch": 24, "H": 32, "W": 36, "out": 40, "scratch_off": 48, "tile_off": 56}
    header = open(native.HEADERS[-1]).read()
    assert "typedef struct mdpt_refocus_pair { const void* map; int32_t h, w; const void* photo; int64_t pitch; int32_t H, W; void* out; int64_t scratch_off, tile_off; }" in header
    assert "#define MDPT_REFOCUS_MAX_RADIUS 32" in header and "#define MDPT_ABI_VERSION 6" in header
