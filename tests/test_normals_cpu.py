"""Surface normals and relighting without a GPU: the properties of the restatement (tests/normals_restate.py), which are the specification; the argument
checks of muggled_dpt_amd.relight; the two exported entry points, which refuse bad arguments before they touch a device pointer."""
import ctypes
import math

import numpy as np
import pytest
import torch

from muggled_dpt_amd import native, relight
from tests import normals_restate as nr


def test_a_fronto_parallel_map_faces_the_camera_in_both_spaces():
    for space, p in (("inverse", np.full((5, 7), 3.5, np.float32)), ("depth", np.full((5, 7), 3.5, np.float32)), ("depth", np.full((19, 26), 0.75))):
        for step in (1, 3):
            n, valid, _ = nr.normals(p, 19, 26, space=space, step=step)
            assert valid.all() and np.array_equal(n, np.broadcast_to([0.0, 0.0, 1.0], n.shape)), (space, step)
    # a 2 x 3 photo at step 3: no neighbour lies inside, everything is invalid
    n, valid, _ = nr.normals(np.full((2, 3), 1.0), 2, 3, space="depth", step=3)
    assert not valid.any() and not n.any()


def _plane_depth(n0, d, H, W, fov_deg):
    """the depth z of the plane n0 . P = d along the ray of every pixel: P = z (x kx, y ky, -1)"""
    kx, ky = nr.camera_scales(H, W, fov_deg)
    X, Y = np.arange(W, dtype=np.float64)[None, :], np.arange(H, dtype=np.float64)[:, None]
    x, y = 2.0 * (X + 0.5) / W - 1.0, 1.0 - 2.0 * (Y + 0.5) / H
    return d / (n0[0] * x * kx + n0[1] * y * ky - n0[2])


@pytest.mark.parametrize("step", [1, 3])
@pytest.mark.parametrize("edge_ratio", [1.0, 2.0, float("inf")])
def test_a_tilted_plane_gives_its_own_normal(step, edge_ratio):
    """Differences of points of a plane lie in the plane, whichever of the three differences the edge rule picks: the normal is the plane's on every
    valid pixel. Bound 1e-9 absolute (the issue's): z is rounded to 2^-53 relative, a tangent is the difference of two points |P| ~ 6 apart by
    |T| >= 0.03, an amplification of 200, so the direction errs by some 1e-13."""
    n0 = np.array([0.3, -0.2, 1.0])
    n0 /= np.sqrt((n0 * n0).sum())
    for H, W in ((21, 34), (30, 17)):
        z = _plane_depth(n0, -5.0, H, W, 50.0)
        assert z.min() > 0
        n, valid, _ = nr.normals(z, H, W, space="depth", fov_deg=50.0, step=step, edge_ratio=edge_ratio)
        worst = float(np.abs(n - n0)[valid].max())
        print(f"tilted plane {H}x{W} step {step} edge_ratio {edge_ratio}: worst |n - n0| = {worst:.3e}")
        assert valid.all() and worst < 1e-9


def test_a_depth_step_is_not_differenced_across():
    """two fronto-parallel planes, a depth step down the middle: with the edge rule every normal is (0, 0, 1); with central differences only, the pixels
    next to the step tilt - the property the feature exists for"""
    z = np.full((12, 20), 2.0)
    z[:, 10:] = 5.0
    for step in (1, 2):
        n, valid, _ = nr.normals(z, 12, 20, space="depth", step=step, edge_ratio=2.0)
        assert valid.all() and float(np.abs(n - [0.0, 0.0, 1.0]).max()) <= 1e-15
        n, valid, _ = nr.normals(z, 12, 20, space="depth", step=step, edge_ratio=float("inf"))
        off = np.abs(n - [0.0, 0.0, 1.0]).max(axis=-1) > 1e-3
        assert valid.all() and off[:, 10 - step:10 + step].all() and not off[:, :10 - step].any() and not off[:, 10 + step:].any()
    # the same through an enlarged inverse map: the step's own ramp (one map cell wide) is the only place that is not flat
    inv = np.full((6, 10), 1.0, np.float32)
    inv[:, 5:] = 0.0
    n, valid, _ = nr.normals(inv, 12, 20, space="inverse", step=1)
    assert valid.all() and np.array_equal(n[:, :8], np.broadcast_to([0.0, 0.0, 1.0], (12, 8, 3)))


def test_invalid_pixels_invalidate_themselves_and_redirect_their_neighbours():
    z = np.full((9, 11), 4.0)
    z[2, 3], z[5, 7], z[6, 2], z[4, 4] = np.nan, np.inf, 0.0, -1.0
    n, valid, _ = nr.normals(z, 9, 11, space="depth", step=1)
    bad = np.zeros((9, 11), bool)
    bad[2, 3] = bad[5, 7] = bad[6, 2] = bad[4, 4] = True
    assert np.array_equal(valid, ~bad) and not n[bad].any()
    assert np.array_equal(n[~bad], np.broadcast_to([0.0, 0.0, 1.0], n[~bad].shape))  # the neighbours took their other side
    enc = nr.encode(n)
    assert (enc[~bad] == (255, 128, 128)).all() and (enc[bad] == (128, 128, 128)).all()
    inv = np.array(z, np.float32)  # inverse space: zero and a negative value are ordinary values, NaN and inf are not
    _, valid, _ = nr.normals(inv, 9, 11, space="inverse", step=1)
    assert not valid[2, 3] and not valid[5, 7] and valid[6, 2] and valid[4, 4]
    # a pixel between two invalid neighbours on one axis has no tangent there
    z = np.full((5, 5), 4.0)
    z[2, 1] = z[2, 3] = np.nan
    _, valid, _ = nr.normals(z, 5, 5, space="depth", step=1)
    assert not valid[2, 2] and valid[1, 2] and valid[3, 1]
    assert not valid[2, 0] and not valid[2, 4]  # (the border on one side, an invalid neighbour on the other)


def test_shading_rules():
    rng = np.random.default_rng(0)
    photo = rng.integers(0, 256, (9, 11, 3), dtype=np.uint8)
    z = rng.uniform(2.0, 2.2, (9, 11))
    n, valid, P = nr.normals(z, 9, 11, space="depth", step=1)
    assert valid.all()
    behind = nr.shade(photo, n, valid, P, (0.0, 0.0, -1.0), ambient=0.35, diffuse=0.9)
    assert behind.shape == (1, 9, 11, 3) and np.array_equal(behind[0], np.floor(photo.astype(np.float64) * 0.35 + 0.5).astype(np.uint8))
    assert np.array_equal(nr.shade(photo, n, valid, P, (0.3, 0.4, 0.5), ambient=1.0, diffuse=0.0)[0], photo)
    bright = nr.shade(photo, n, valid, P, (0.0, 0.0, 1.0), ambient=1.0, diffuse=2.0)[0]
    assert (bright[photo >= 128] == 255).all() and bright.max() == 255 and (bright[photo == 0] == 0).all()  # the clamp
    flat = np.full((9, 11), 2.0)
    nf, vf, Pf = nr.normals(flat, 9, 11, space="depth", step=1)
    lit = nr.shade(photo, nf, vf, Pf, (0.0, 0.0, 2.0), ambient=0.25, diffuse=0.5)[0]  # n.l = 1 after the normalisation: shade 0.75
    assert np.array_equal(lit, np.floor(photo.astype(np.float64) * 0.75 + 0.5).astype(np.uint8))
    dull = nr.shade(photo, nf, vf, Pf, (0.2, 0.1, 1.0), 0.35, 0.9, 0.5, 0)
    shiny = nr.shade(photo, nf, vf, Pf, (0.2, 0.1, 1.0), 0.35, 0.9, 0.5, 5)
    plain = nr.shade(photo, nf, vf, Pf, (0.2, 0.1, 1.0), 0.35, 0.9, 0.0, 5)
    assert not np.array_equal(dull, shiny) and (dull >= shiny).all() and (shiny >= plain).all() and not np.array_equal(shiny, plain)
    three = nr.shade(photo, n, valid, P, [(0.0, 0.0, 1.0), (0.0, 0.0, -1.0), (1.0, 1.0, 1.0)])
    assert three.shape == (3, 9, 11, 3) and np.array_equal(three[1], behind[0])
    z[4, 5] = np.nan  # an invalid pixel keeps the photo's bytes
    n, valid, P = nr.normals(z, 9, 11, space="depth", step=1)
    assert np.array_equal(nr.shade(photo, n, valid, P, (0.0, 0.0, 1.0), 0.1, 0.2, 0.3, 2)[0, 4, 5], photo[4, 5])


def test_default_step_and_light_sweep():
    assert [relight.default_step(W, w) for W, w in ((504, 504), (1280, 504), (4032, 504), (100, 504), (7, 4), (20000, 504))] == [1, 3, 8, 1, 2, 16]
    assert all(relight.default_step(W, w) == nr.default_step(W, w) for W in (1, 5, 33, 640, 4032) for w in (1, 4, 37, 504))
    ring = relight.light_sweep(8, 30.0)
    assert ring.shape == (8, 3) and ring.dtype == np.float64 and np.allclose((ring * ring).sum(axis=1), 1.0, atol=1e-15)
    assert np.allclose(ring[:, 2], 0.5) and np.allclose(ring[0], (math.cos(math.radians(30.0)), 0.0, 0.5)) and np.allclose(ring.sum(axis=0)[:2], 0.0, atol=1e-12)
    assert np.allclose(relight.light_sweep(1, 90.0), [[0.0, 0.0, 1.0]])
    for bad in (dict(n=0), dict(n=2.0), dict(n=3, elevation_deg=91.0)):
        with pytest.raises(ValueError, match="light_sweep"):
            relight.light_sweep(**bad)


def test_python_arguments_are_checked_before_anything_runs():
    maps = [torch.zeros(1, 4, 5), torch.zeros(1, 3, 3)]
    photos = [np.zeros((8, 9, 3), np.uint8), np.zeros((2, 2, 3), np.uint8)]
    camera = (dict(space="linear"), dict(fov_deg=0.0), dict(fov_deg=180.0), dict(fov_deg=float("nan")), dict(min_depth=0.0), dict(min_depth=100.0),
              dict(max_depth=float("inf")), dict(step=0), dict(step=17), dict(step=2.0), dict(step=True), dict(edge_ratio=0.5), dict(edge_ratio=float("nan")))
    for bad in camera:
        with pytest.raises(ValueError, match="depth_normals"):
            relight.depth_normals(maps, **bad)
        with pytest.raises(ValueError, match="relight_images"):
            relight.relight_images(maps, photos, (0.0, 0.0, 1.0), **bad)
    for bad in (dict(ambient=-0.1), dict(ambient=float("inf")), dict(diffuse=-1.0), dict(diffuse=float("nan")), dict(specular=-1.0), dict(shininess_log2=11),
                dict(shininess_log2=-1), dict(shininess_log2=2.0)):
        with pytest.raises(ValueError, match="relight_images"):
            relight.relight_images(maps, photos, (0.0, 0.0, 1.0), **bad)
    for lights in ((0.0, 0.0, 0.0), (1.0, float("nan"), 0.0), (1.0, float("inf"), 0.0), (1.0, 2.0), np.zeros((0, 3)), np.ones((65, 3)), np.ones((2, 2, 3))):
        with pytest.raises(ValueError, match="light_dirs|light direction"):
            relight.relight_images(maps, photos, lights)
    for call in (lambda preds, imgs=None, target_hws=None: relight.depth_normals(preds, target_hws, imgs),
                 lambda preds, imgs=None, target_hws=None: relight.relight_images(preds, imgs, (0.0, 0.0, 1.0), target_hws=target_hws)):
        with pytest.raises(ValueError, match="2 predictions but 1 images"):
            call(maps, photos[:1])
        with pytest.raises(ValueError, match="image 1 is not a uint8"):
            call(maps, [photos[0], np.zeros((2, 2, 3), np.float32)])
        with pytest.raises(ValueError, match="2 predictions but 1 target sizes"):
            call(maps, target_hws=[(4, 4)])
        with pytest.raises(ValueError, match="target sizes must be positive"):
            call(maps, target_hws=[(4, 4), (0, 3)])
        with pytest.raises(ValueError, match="not both"):
            call(maps, photos, target_hws=[(4, 4), (3, 3)])
        with pytest.raises(RuntimeError, match="no CPU fallback"):  # there is no CPU implementation: host maps raise
            call(maps, photos)
    assert "not measured optima" in relight.depth_normals.__doc__ and "not measured optima" in relight.relight_images.__doc__
    assert all(word in relight.__doc__ for word in ("unverified", "gamma", "cast shadows", "fov_deg"))
    depth_space = relight.depth_normals  # depth space reads neither min_depth nor max_depth
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        depth_space(maps, space="depth", min_depth=0.0, max_depth=0.0)


def _records(H=8, W=9, n=1):
    rec = np.zeros(n, dtype=relight.NORMALS_RECORD)
    rec["map"], rec["photo"], rec["normals"], rec["encoded"], rec["relit"] = 4096, 8192, 12288, 16384, 20480  # (not device addresses: nothing may be launched)
    rec["h"], rec["w"], rec["H"], rec["W"], rec["pitch"], rec["step"], rec["kx"], rec["ky"] = 4, 5, H, W, 3 * W, 2, 0.4, 0.3
    rec["scratch_off"] = 1024 * np.arange(n)
    rec["tile_off"] = ((H + 31) // 32) * ((W + 31) // 32) * np.arange(n)
    return rec


def test_entry_points_are_exported_and_refuse_bad_arguments_without_a_device():
    lib = native.load()
    for name in ("mdpt_post_normals_scratch_bytes", "mdpt_post_normals"):
        assert name in native.SYMBOLS and hasattr(lib, name)
    assert "post_normals.inc" in native.HEADERS and (native.NORMALS_MAX_STEP, native.NORMALS_TILE, native.NORMALS_MAX_LIGHTS) == (16, 32, 64)
    assert lib.mdpt_abi_version() == 6 == native.ABI_VERSION
    need = ctypes.c_size_t()
    sizes = []
    for H, W in ((1, 1), (8, 9), (70, 33), (720, 1280), (3024, 4032)):  # monotone in the photo size (a header a pair: nothing per pixel is kept)
        rec = _records(H, W, 3)
        assert lib.mdpt_post_normals_scratch_bytes(rec.ctypes.data, 3, ctypes.byref(need)) == 0
        sizes.append(need.value)
    assert sizes == sorted(sizes) and sizes[0] == 3 * 1024
    rec, huge = _records(70, 33, 3), _records(65536, 32768)
    for args, word in (((None, 1), b"records"), ((rec.ctypes.data, 0), b"n ="), ((rec.ctypes.data, 65536), b"n ="), ((huge.ctypes.data, 1), b"2^31")):
        assert lib.mdpt_post_normals_scratch_bytes(*args, ctypes.byref(need)) != 0 and word in lib.mdpt_last_error(), args
    assert lib.mdpt_post_normals_scratch_bytes(rec.ctypes.data, 3, None) != 0

    p, big = 4096, 1 << 30

    def call(r=rec, dev=p, n=3, dtype=0, space=0, min_depth=50.0, max_depth=100.0, edge_ratio=2.0, lights=p, V=2, ambient=0.35, diffuse=0.9, specular=0.0,
             shininess_log2=4, scratch=p, nbytes=big):
        return lib.mdpt_post_normals(None if r is None else r.ctypes.data, dev, n, dtype, space, min_depth, max_depth, edge_ratio, lights, V, ambient, diffuse,
                                     specular, shininess_log2, scratch, nbytes, None)

    def changed(**fields):
        r = _records(70, 33, 3)
        for name, (k, v) in fields.items():
            r[name][k] = v
        return r

    no_out = _records(70, 33, 3)
    no_out["normals"] = no_out["encoded"] = no_out["relit"] = 0
    for kw, word in ((dict(r=None), b"null"), (dict(dev=None), b"null"), (dict(scratch=None), b"null"), (dict(n=0), b"n ="), (dict(dtype=7), b"dtype"),
                     (dict(space=2), b"space"), (dict(min_depth=0.0), b"min_depth"), (dict(min_depth=100.0), b"min_depth"), (dict(max_depth=float("inf")), b"min_depth"),
                     (dict(edge_ratio=0.5), b"edge_ratio"), (dict(edge_ratio=float("nan")), b"edge_ratio"), (dict(V=65), b"num_lights"), (dict(V=-1), b"num_lights"),
                     (dict(V=0), b"lights"), (dict(lights=None), b"lights"), (dict(ambient=-1.0), b"ambient"), (dict(diffuse=float("nan")), b"ambient"),
                     (dict(specular=float("inf")), b"ambient"), (dict(shininess_log2=11), b"shininess_log2"), (dict(shininess_log2=-1), b"shininess_log2"),
                     (dict(nbytes=3 * 1024 - 8), b"scratch"), (dict(r=huge, n=1), b"2^31"), (dict(r=changed(tile_off=(2, 5))), b"tile_off"),
                     (dict(r=changed(relit=(1, 0))), b"output"), (dict(r=changed(normals=(0, 0))), b"output"), (dict(r=changed(photo=(2, 0))), b"photo"),
                     (dict(r=no_out), b"no record has an output"), (dict(r=changed(pitch=(0, 98))), b"pitch"), (dict(r=changed(step=(1, 0))), b"step"),
                     (dict(r=changed(step=(1, 17))), b"step"), (dict(r=changed(kx=(0, 0.0))), b"kx"), (dict(r=changed(ky=(0, float("nan")))), b"kx"),
                     (dict(r=changed(normals=(0, 12290))), b"misaligned"), (dict(r=changed(scratch_off=(1, 0))), b"overlap"), (dict(scratch=4100), b"misaligned"),
                     (dict(lights=4100), b"misaligned")):
        assert call(**kw) != 0, kw
        assert word in lib.mdpt_last_error(), (kw, lib.mdpt_last_error())


def test_the_record_table_has_the_layout_of_its_struct():
    r = relight.NORMALS_RECORD
    assert r.itemsize == 104
    assert {n: r.fields[n][1] for n in r.names} == {"map": 0, "h": 8, "w": 12, "photo": 16, "pitch": 24, "H": 32, "W": 36, "normals": 40, "encoded": 48, "relit": 56,
                                                    "scratch_off": 64, "tile_off": 72, "kx": 80, "ky": 88, "step": 96, "pad": 100}
    header = open(native.HEADERS[-1]).read()
    assert ("typedef struct mdpt_normals_pair { const void* map; int32_t h, w; const void* photo; int64_t pitch; int32_t H, W; void* normals; void* encoded; "
            "void* relit; int64_t scratch_off, tile_off; double kx, ky; int32_t step, pad; }") in header
    assert "#define MDPT_NORMALS_MAX_STEP 16" in header and "#define MDPT_NORMALS_MAX_LIGHTS 64" in header and "#define MDPT_ABI_VERSION 6" in header
    assert not hasattr(__import__("muggled_dpt_amd.postprocess", fromlist=["x"]), "depth_normals")  # (the pinned surface of postprocess stays as it is)
