"""Cast shadows and ambient occlusion without a GPU: the properties of the restatement (tests/shadows_restate.py), which are the specification; the
condition on the scenes of tests/test_gpu_shadows.py; the argument checks of muggled_dpt_amd.relight; the two exported entry points, which refuse bad
arguments before they touch a device pointer."""
import ctypes

import numpy as np
import pytest
import torch

from muggled_dpt_amd import native, relight
from tests import normals_restate as nr
from tests import shadows_cases as sc
from tests import shadows_restate as sr


def test_a_flat_map_is_lit_and_open_everywhere():
    lights = [(-1.0, 1.0, 1.0), (0.0, 0.0, 1.0), (1.0, 0.5, 0.0), (0.3, 0.2, 0.4)]
    for space, p, grid in (("inverse", np.full((5, 7), 3.5, np.float32), None), ("depth", np.full((19, 26), 0.75), None), ("depth", np.full((5, 7), 2.0), (33, 40))):
        ao, vis, valid = sr.occlusion(p, 21, 34, lights, grid, space=space, shadow_reach=32, ao_reach=32)
        assert valid.all() and (ao == 1.0).all() and (vis == 1.0).all() and ao.dtype == np.float32 and vis.shape == (4, *ao.shape), space


def test_with_both_features_off_the_shading_is_the_relighting_byte_for_byte():
    for index in (2, 3, 4, 6):
        c = sc.CASES[index]
        p, photo = sc.make_case(index)
        camera = {k: v for k, v in c["kw"].items() if k in ("space", "fov_deg", "min_depth", "max_depth", "edge_ratio", "step")}
        shading = {k: v for k, v in c["kw"].items() if k in sc.SHADING}
        n, valid, P = nr.normals(p, *photo.shape[:2], **camera)
        want = nr.shade(photo, n, valid, P, c["lights"], **shading)
        for off in (dict(shadow_reach=0, ao_strength=0.0), dict(shadow_reach=0, ao_reach=0)):
            assert np.array_equal(sr.shade_images(p, photo, c["lights"], grid_hw=c["grid"], **camera, **shading, **off)[0], want), (index, off)
        assert not np.array_equal(sc.restated(index)[2], want)  # (and the features change the picture)


def _dilated(mask, r=1):
    padded = np.pad(mask, r)
    return np.any([padded[r + dy:r + dy + mask.shape[0], r + dx:r + dx + mask.shape[1]] for dy in range(-r, r + 1) for dx in range(-r, r + 1)], axis=0)


def test_a_plate_before_a_wall_shadows_the_wall_where_geometry_says():
    """A fronto-parallel wall at z = 10 (depth space) and a square plate at z = 8 before it, on a 40 x 48 grid, lit from the upper left. A wall point's ray
    towards the light reaches the plate's plane after 2 / Lz, displaced by 2 L_xy / L_z world units; a height field is solid behind its surface, so the ray
    is blocked iff its projection crosses the plate's footprint on the way. Predicted from the continuous geometry; the nodes with vis = 0 lie within one
    node of that region and cover it but for one node of its outline, and none lie on the lit side of the plate."""
    gh, gw, (i0, i1, j0, j1) = 40, 48, (12, 24, 16, 30)
    z = np.full((gh, gw), 10.0)
    z[i0:i1, j0:j1] = 8.0
    plate = z == 8.0
    light = nr.unit_lights((-1.0, 1.0, 1.5))[0]
    kx, ky = nr.camera_scales(gh, gw, 50.0)
    ao, vis, valid = sr.occlusion(z, gh, gw, light, space="depth", shadow_reach=32, shadow_bias=0.02)
    assert valid.all()
    dark = (vis[0] == 0.0) & ~plate
    I, J = np.mgrid[0:gh, 0:gw]
    x0, y0 = 2.0 * (J + 0.5) / gw - 1.0, 1.0 - 2.0 * (I + 0.5) / gh
    predicted = np.zeros((gh, gw), bool)
    for t in np.linspace(0.0, 2.0 / light[2], 400)[1:]:
        zr = 10.0 - t * light[2]
        jq = ((10.0 * x0 * kx + t * light[0]) / (zr * kx) + 1.0) / 2.0 * gw - 0.5
        iq = (1.0 - (10.0 * y0 * ky + t * light[1]) / (zr * ky)) / 2.0 * gh - 0.5
        predicted |= (iq >= i0 - 0.5) & (iq <= i1 - 0.5) & (jq >= j0 - 0.5) & (jq <= j1 - 0.5)
    predicted &= ~plate
    print(f"plate scene: {int(dark.sum())} wall nodes in shadow, {int(predicted.sum())} predicted, outside the dilated prediction "
          f"{int((dark & ~_dilated(predicted)).sum())}, missed inside the eroded one {int((~_dilated(~predicted | plate) & ~dark & ~plate).sum())}")
    assert predicted.sum() > 100 and not (dark & ~_dilated(predicted)).any()
    assert not (~_dilated(~predicted | plate) & ~dark & ~plate).any()  # (eroded by one node, the plate not counting as outside)
    assert not dark[:i0].any() and not dark[:, :j0].any()  # the lit side: above and left of the plate
    assert (vis[0][plate] == 1.0).all()  # nothing is before the plate
    # occlusion: the wall next to the plate's edge is darkened, the wall far from it is open, the plate's face is open
    ring = _dilated(plate) & ~plate
    assert (ao[ring] < 1.0).all() and (ao[~_dilated(plate, 10)] == 1.0).all() and (ao[plate] == 1.0).all()
    # a finite thickness lets the light pass behind the plate: fewer nodes in shadow, all of them among the solid block's
    thin = sr.occlusion(z, gh, gw, light, space="depth", shadow_reach=32, shadow_thickness=0.05)[1][0] == 0.0
    assert 0 < thin.sum() < dark.sum() and not (thin & ~dark).any()
    short = sr.occlusion(z, gh, gw, light, space="depth", shadow_reach=3)[1][0] == 0.0  # a short reach sees the near part only
    assert 0 < short.sum() < dark.sum() and not (short & ~dark).any()


def test_lights_behind_along_the_axis_and_grazing():
    z = np.full((9, 11), 4.0)
    z[3:6, 4:7] = 3.0
    ao, vis, valid = sr.occlusion(z, 9, 11, [(0.0, 0.0, 1.0), (1.0, 0.0, 0.0), (0.0, 0.0, -1.0)], space="depth", shadow_reach=8)
    assert vis[0][4, 5] == 1.0  # x0 = y0 = 0 at the centre of an odd grid: gx = gy = 0, lit
    assert (vis[1][3:6, :4] == 0.0).all() and (vis[1][3:6, 7:] == 1.0).all() and (vis[1][:3] == 1.0).all()  # grazing from the right: the block's left side is dark
    # a light straight behind the scene: its rays run into the solid behind the surface (the diffuse term of such a light is 0 whatever vis says)
    assert vis[2][4, 5] == 1.0 and (vis[2][:, 5] == [0, 0, 0, 1, 1, 0, 0, 0, 0]).all()


def test_the_gpu_cases_cover_what_they_claim():
    """a condition on the inputs of tests/test_gpu_shadows.py: in every non-degenerate scene some light leaves at least 5 % of the valid nodes in shadow and
    at least 5 % lit, and at least 5 % have ao < 1; the degenerate ones (smaller than a tile, flat) are named as such"""
    for index, c in enumerate(sc.CASES):
        shadowed, occluded = sc.coverage(index)
        print(f"case {index} {c['hw']} grid {c['grid']} -> {c['HW']} {c['holds']}: in shadow per light {[round(s, 3) for s in shadowed]}, ao < 1 on {occluded:.3f}")
        if c.get("degenerate"):
            continue
        assert any(0.05 <= s <= 0.95 for s in shadowed) and occluded >= 0.05, index
    assert (sc.restated(8)[3] == 1.0).all() and (sc.restated(8)[4] == 1.0).all()  # the flat map
    for index in (6, 7):
        valid = sc.restated(index)[5]
        assert 0 < (~valid).sum() < valid.size / 10
    assert sum(not c.get("degenerate") for c in sc.CASES) >= 6
    assert not np.array_equal(sc.restated(2)[4][0], sc.restated(3)[4][0])  # reach 5 and reach 32 differ under the same light


BAD_OCCLUSION = (dict(shadow_reach=-1), dict(shadow_reach=33), dict(shadow_reach=2.0), dict(shadow_reach=True), dict(ao_reach=33), dict(ao_reach=-1), dict(ao_reach=1.5),
                 dict(shadow_bias=-0.1), dict(shadow_bias=1.0), dict(shadow_bias=float("nan")), dict(shadow_thickness=-1.0), dict(shadow_thickness=float("nan")),
                 dict(ao_radius=0.0), dict(ao_radius=float("inf")), dict(ao_radius=float("nan")), dict(ao_bias=-0.1), dict(ao_bias=float("inf")),
                 dict(ao_strength=-1.0), dict(ao_strength=float("nan")), dict(grid_hw=(0, 4)), dict(grid_hw=(4,)), dict(grid_hw=[(4, 4)]), dict(grid_hw=(65536, 32768)),
                 dict(grid_hw=[(4, 4), (3, -1)]), dict(grid_hw=5))


def test_python_arguments_are_checked_before_anything_runs():
    maps = [torch.zeros(1, 4, 5), torch.zeros(1, 3, 3)]
    photos = [np.zeros((8, 9, 3), np.uint8), np.zeros((2, 2, 3), np.uint8)]
    camera = (dict(space="linear"), dict(fov_deg=0.0), dict(fov_deg=180.0), dict(min_depth=0.0), dict(max_depth=float("inf")), dict(edge_ratio=0.5),
              dict(edge_ratio=float("nan")))
    for bad in camera + BAD_OCCLUSION:
        with pytest.raises(ValueError, match="light_occlusion"):
            relight.light_occlusion(maps, (0.0, 0.0, 1.0), **bad)
        with pytest.raises(ValueError, match="shade_images"):
            relight.shade_images(maps, photos, (0.0, 0.0, 1.0), **bad)
    for bad in (dict(step=0), dict(step=17), dict(step=2.0), dict(ambient=-0.1), dict(diffuse=float("nan")), dict(specular=-1.0), dict(shininess_log2=11)):
        with pytest.raises(ValueError, match="shade_images"):
            relight.shade_images(maps, photos, (0.0, 0.0, 1.0), **bad)
    for lights in ((0.0, 0.0, 0.0), (1.0, float("nan"), 0.0), (1.0, 2.0), np.zeros((0, 3)), np.ones((65, 3))):
        with pytest.raises(ValueError, match="light_dirs|light direction"):
            relight.shade_images(maps, photos, lights)
        with pytest.raises(ValueError, match="light_dirs|light direction"):
            relight.light_occlusion(maps, lights)
    with pytest.raises(ValueError, match="2 predictions but 1 images"):
        relight.shade_images(maps, photos[:1], (0.0, 0.0, 1.0))
    with pytest.raises(ValueError, match="not both"):
        relight.shade_images(maps, photos, (0.0, 0.0, 1.0), target_hws=[(4, 4), (3, 3)])
    with pytest.raises(ValueError, match="2 predictions but 1 target sizes"):
        relight.light_occlusion(maps, target_hws=[(4, 4)])
    for call in (lambda: relight.shade_images(maps, photos, (0.0, 0.0, 1.0)), lambda: relight.light_occlusion(maps), lambda: relight.light_occlusion(maps, grid_hw=(7, 9))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):  # there is no CPU implementation: host maps raise
            call()
    assert "not measured optima" in relight.shade_images.__doc__ and "not measured optima" in relight.light_occlusion.__doc__
    assert all(word in relight.__doc__ for word in ("screen space", "outside the frame", "assumed", "at most 32", "gamma", "unverified"))


def _records(H=8, W=9, n=1, gh=6, gw=7):
    rec = np.zeros(n, dtype=relight.SHADOWS_RECORD)
    rec["map"], rec["photo"], rec["ao"], rec["vis"], rec["relit"] = 4096, 8192, 12288, 16384, 20480  # (not device addresses: nothing may be launched)
    rec["h"], rec["w"], rec["H"], rec["W"], rec["gh"], rec["gw"], rec["pitch"], rec["step"], rec["kx"], rec["ky"] = 4, 5, H, W, gh, gw, 3 * W, 2, 0.4, 0.3
    rec["scratch_off"] = 1024 * np.arange(n)
    rec["tile_off"] = ((H + 31) // 32) * ((W + 31) // 32) * np.arange(n)
    rec["gtile_off"] = ((gh + 31) // 32) * ((gw + 31) // 32) * np.arange(n)
    return rec


def test_entry_points_are_exported_and_refuse_bad_arguments_without_a_device():
    lib = native.load()
    for name in ("mdpt_post_shadows_scratch_bytes", "mdpt_post_shadows"):
        assert name in native.SYMBOLS and hasattr(lib, name)
    assert "post_shadows.inc" in native.HEADERS and (native.SHADOWS_MAX_REACH, native.SHADOWS_AO_DIRECTIONS) == (32, 8) == (sr.MAX_REACH, len(sr.AO_DIRECTIONS))
    assert list(native.HEADERS[:-1]) == sorted(native.HEADERS[:-1])
    assert lib.mdpt_abi_version() == 6 == native.ABI_VERSION
    need = ctypes.c_size_t()
    rec, huge, huge_grid = _records(70, 33, 3, 40, 70), _records(65536, 32768), _records(gh=65536, gw=32768)
    assert lib.mdpt_post_shadows_scratch_bytes(rec.ctypes.data, 3, ctypes.byref(need)) == 0 and need.value == 3 * 1024
    for args, word in (((None, 1), b"records"), ((rec.ctypes.data, 0), b"n ="), ((rec.ctypes.data, 65536), b"n ="), ((huge.ctypes.data, 1), b"2^31"),
                       ((huge_grid.ctypes.data, 1), b"working grid"), ((_records(gh=0).ctypes.data, 1), b"working grid")):
        assert lib.mdpt_post_shadows_scratch_bytes(*args, ctypes.byref(need)) != 0 and word in lib.mdpt_last_error(), args
    assert lib.mdpt_post_shadows_scratch_bytes(rec.ctypes.data, 3, None) != 0

    p, big = 4096, 1 << 30

    def call(r=rec, dev=p, n=3, dtype=0, space=0, min_depth=50.0, max_depth=100.0, edge_ratio=2.0, lights=p, V=2, ambient=0.35, diffuse=0.9, specular=0.0,
             shininess_log2=4, shadow_reach=32, shadow_bias=0.02, shadow_thickness=float("inf"), ao_reach=8, ao_radius=0.25, ao_bias=0.05, ao_strength=1.0,
             scratch=p, nbytes=big):
        return lib.mdpt_post_shadows(None if r is None else r.ctypes.data, dev, n, dtype, space, min_depth, max_depth, edge_ratio, lights, V, ambient, diffuse,
                                     specular, shininess_log2, shadow_reach, shadow_bias, shadow_thickness, ao_reach, ao_radius, ao_bias, ao_strength, scratch,
                                     nbytes, None)

    def changed(**fields):
        r = _records(70, 33, 3, 40, 70)
        for name, value in fields.items():
            if isinstance(value, tuple):
                r[name][value[0]] = value[1]
            else:
                r[name] = value
        return r

    for kw, word in ((dict(r=None), b"null"), (dict(dev=None), b"null"), (dict(scratch=None), b"null"), (dict(n=0), b"n ="), (dict(n=65536), b"n ="),
                     (dict(dtype=7), b"dtype"), (dict(space=2), b"space"), (dict(min_depth=0.0), b"min_depth"), (dict(max_depth=float("inf")), b"min_depth"),
                     (dict(edge_ratio=0.5), b"edge_ratio"), (dict(V=65), b"num_lights"), (dict(V=-1), b"num_lights"), (dict(V=0), b"lights"),
                     (dict(lights=None), b"lights"), (dict(ambient=-1.0), b"ambient"), (dict(specular=float("inf")), b"ambient"), (dict(shininess_log2=11), b"shininess_log2"),
                     (dict(shadow_reach=33), b"shadow_reach"), (dict(shadow_reach=-1), b"shadow_reach"), (dict(ao_reach=33), b"ao_reach"), (dict(ao_reach=-1), b"ao_reach"),
                     (dict(shadow_bias=1.0), b"shadow_bias"), (dict(shadow_bias=float("nan")), b"shadow_bias"), (dict(shadow_thickness=-1.0), b"shadow_thickness"),
                     (dict(shadow_thickness=float("nan")), b"shadow_thickness"), (dict(ao_radius=0.0), b"ao_radius"), (dict(ao_radius=float("inf")), b"ao_radius"),
                     (dict(ao_bias=-1.0), b"ao_bias"), (dict(ao_strength=float("nan")), b"ao_strength"), (dict(nbytes=3 * 1024 - 8), b"scratch"),
                     (dict(r=huge, n=1), b"2^31"), (dict(r=huge_grid, n=1), b"working grid"), (dict(r=changed(tile_off=(2, 5))), b"tile_off"),
                     (dict(r=changed(gtile_off=(2, 5))), b"gtile_off"), (dict(r=changed(relit=(1, 0))), b"output"), (dict(r=changed(ao=(0, 0))), b"output"),
                     (dict(r=changed(vis=(2, 0))), b"output"), (dict(r=changed(photo=(2, 0))), b"photo"), (dict(r=changed(ao=0, vis=0, relit=0)), b"no record has an output"),
                     (dict(r=changed(vis=0)), b"needs a plane"), (dict(r=changed(ao=0)), b"needs a plane"), (dict(r=changed(relit=0), V=0), b"lights"),
                     (dict(r=changed(pitch=(0, 98))), b"pitch"), (dict(r=changed(step=(1, 17))), b"step"), (dict(r=changed(kx=(0, 0.0))), b"kx"),
                     (dict(r=changed(ao=(0, 12290))), b"misaligned"), (dict(r=changed(vis=(1, 16385))), b"misaligned"), (dict(r=changed(scratch_off=(1, 0))), b"overlap"),
                     (dict(scratch=4100), b"misaligned"), (dict(lights=4100), b"misaligned"), (dict(r=changed(gh=(1, 0))), b"working grid")):
        assert call(**kw) != 0, kw
        assert word in lib.mdpt_last_error(), (kw, lib.mdpt_last_error())


def test_the_record_table_has_the_layout_of_its_struct():
    r = relight.SHADOWS_RECORD
    assert r.itemsize == 120
    assert {n: r.fields[n][1] for n in r.names} == {"map": 0, "h": 8, "w": 12, "photo": 16, "pitch": 24, "H": 32, "W": 36, "gh": 40, "gw": 44, "ao": 48, "vis": 56,
                                                    "relit": 64, "scratch_off": 72, "tile_off": 80, "gtile_off": 88, "kx": 96, "ky": 104, "step": 112, "pad": 116}
    header = open(native.HEADERS[-1]).read()
    assert ("typedef struct mdpt_shadows_pair { const void* map; int32_t h, w; const void* photo; int64_t pitch; int32_t H, W, gh, gw; void* ao; void* vis; "
            "void* relit; int64_t scratch_off, tile_off, gtile_off; double kx, ky; int32_t step, pad; }") in header
    assert "#define MDPT_SHADOWS_MAX_REACH 32" in header and "#define MDPT_SHADOWS_AO_DIRECTIONS 8" in header and "#define MDPT_ABI_VERSION 6" in header
    assert relight.NORMALS_RECORD.itemsize == 104  # (mdpt_normals_pair is untouched)
