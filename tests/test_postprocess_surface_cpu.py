"""The public surface of muggled_dpt_amd.postprocess is what tests/golden/postprocess_surface.json recorded from the single-file module before it became
a package (`python tests/test_postprocess_surface_cpu.py` rewrites the file from whatever is importable: only ever run on purpose), and the helpers of
postprocess/_common.py that replaced the per-feature copies give what the old expressions gave. No GPU."""
import ctypes
import inspect
import json
import os
import re

import numpy as np
import pytest

from muggled_dpt_amd import native
from muggled_dpt_amd import postprocess as pp

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "postprocess_surface.json")
NOT_OURS = {"np", "torch", "Tensor", "functools", "native", "annotations"}
PRIVATE = ("_PAIR_RECORD", "_TILE_RECORD", "_GUIDED_RECORD", "_size_group_batch", "_blur_weights")


def surface(module) -> dict:
    """{names, signatures of the callables among them, values of the constants} - modules (the package's own files) are not names of the surface"""
    names = sorted(n for n in dir(module) if not n.startswith("_") and n not in NOT_OURS and not inspect.ismodule(getattr(module, n)))
    # (a module as a default, rng=np.random, prints with the path it was loaded from: only its name is kept)
    calls = {n: re.sub(r"<module '([\w.]+)' from '[^']*'>", r"<module '\1'>", str(inspect.signature(getattr(module, n)))) for n in names if callable(getattr(module, n))}
    consts = {n: json.loads(json.dumps(getattr(module, n))) for n in names if n not in calls}
    return {"names": names, "signatures": calls, "constants": consts}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


def test_exports_exactly_the_recorded_names(golden):
    assert surface(pp)["names"] == golden["names"]
    assert sorted(pp.__all__) == golden["names"]


def test_signatures_are_the_recorded_ones(golden):
    assert surface(pp)["signatures"] == golden["signatures"]


def test_constants_have_the_recorded_values(golden):
    got = surface(pp)["constants"]
    assert got == golden["constants"]
    for prefix in ("MESH_", "FILL_BAND", "RENDER_", "TILE_ALIGN", "ALIGN_", "DEPTH_METRIC_NAMES"):
        assert any(n.startswith(prefix) for n in got), prefix


def test_private_names_the_tests_use_resolve():
    for name in PRIVATE:
        assert getattr(pp, name) is not None


# ---- the helpers of _common.py against the expressions they replaced, written out


@pytest.mark.parametrize("counts", [[7], [1, 17, 5], [16, 32, 48], [1], [17], [37 * 53, 21 * 29, 64 * 48, 1, 17]])
def test_packed_offsets_equal_the_old_expressions(counts):
    from muggled_dpt_amd.postprocess._common import packed_offsets

    offs, total = packed_offsets(counts)
    assert offs == [int(v) for v in np.cumsum([0] + counts[:-1])] and total == sum(counts)  # depth_to_color_images, guided_upsample_images
    old = np.zeros(len(counts), dtype=np.int64)
    old[1:] = np.cumsum(counts, dtype=np.int64)[:-1]  # true_depth
    assert offs == old.tolist()
    old16, at = [], 0
    for c in counts:  # _stage_photos, depth_mask_images
        old16.append(at)
        at += (c + 15) // 16 * 16
    assert packed_offsets(counts, 16) == (old16, at)
    assert all(type(o) is int for o in offs)


def test_views_is_the_inverse_of_packed_offsets():
    import torch

    from muggled_dpt_amd.postprocess._common import _views, packed_offsets

    hws = [(3, 5), (1, 1), (2, 17)]
    for align, tail in ((1, ()), (1, (3,)), (16, ()), (16, (4,))):
        step = int(np.prod(tail, dtype=np.int64))
        offs, total = packed_offsets([h * w for h, w in hws], align)
        flat = torch.arange(total * step)
        views = _views(flat, hws, tail, align)
        assert [tuple(v.shape) for v in views] == [(1, h, w, *tail) for h, w in hws]
        assert [int(v.reshape(-1)[0]) for v in views] == [o * step for o in offs]


def test_scratch_bytes_equals_the_direct_call():
    from muggled_dpt_amd.postprocess._common import scratch_bytes

    lib = native.load()
    need = ctypes.c_size_t()
    native.check(lib, lib.mdpt_post_fill_scratch_bytes(1, 9, 270, ctypes.byref(need)))
    assert scratch_bytes("mdpt_post_fill_scratch_bytes", 1, 9, 270) == need.value > 0
    with pytest.raises(native.MdptError):
        scratch_bytes("mdpt_post_fill_scratch_bytes", 1, 0, 270)


def test_record_tables_have_the_layout_of_their_structs():
    """item sizes and field offsets of the seven record structs of include/mdpt.h (the MDPT_SAME_RECORD asserts of csrc/mdpt_post_*.cpp)"""
    from muggled_dpt_amd.postprocess._common import (GUIDED_RECORD, NORMALS_RECORD, PAIR_RECORD, REFOCUS_RECORD, SHADOWS_RECORD, TEXTURE_RECORD, TILE_RECORD,
                                                     record_table)

    class Map:
        def __init__(self, ptr, h, w):
            self.shape, self._ptr = (h, w), ptr

        def data_ptr(self):
            return self._ptr

    maps = [Map(4096, 3, 5), Map(8192, 7, 2)]
    expected = {
        "tile": (TILE_RECORD, 32, {"map": 0, "h": 8, "w": 12, "x1": 16, "y1": 20, "x2": 24, "y2": 28}),
        "pair": (PAIR_RECORD, 40, {"pred": 0, "ph": 8, "pw": 12, "truth": 16, "valid": 24, "H": 32, "W": 36}),
        "guided": (GUIDED_RECORD, 56, {"map": 0, "h": 8, "w": 12, "photo": 16, "pitch": 24, "H": 32, "W": 36, "out": 40, "scratch_off": 48}),
        "texture": (TEXTURE_RECORD, 16, {"bgr": 0, "h": 8, "w": 12}),
        "refocus": (REFOCUS_RECORD, 64, {"map": 0, "h": 8, "w": 12, "photo": 16, "pitch": 24, "H": 32, "W": 36, "out": 40, "scratch_off": 48, "tile_off": 56}),
        "normals": (NORMALS_RECORD, 104, {"map": 0, "h": 8, "w": 12, "photo": 16, "pitch": 24, "H": 32, "W": 36, "normals": 40, "encoded": 48, "relit": 56,
                                          "scratch_off": 64, "tile_off": 72, "kx": 80, "ky": 88, "step": 96, "pad": 100}),
        "shadows": (SHADOWS_RECORD, 120, {"map": 0, "h": 8, "w": 12, "photo": 16, "pitch": 24, "H": 32, "W": 36, "gh": 40, "gw": 44, "ao": 48, "vis": 56, "relit": 64,
                                          "scratch_off": 72, "tile_off": 80, "gtile_off": 88, "kx": 96, "ky": 104, "step": 112, "pad": 116}),
    }
    for name, (dtype, size, offsets) in expected.items():
        lead = tuple(dtype.names[:3])
        t = record_table(dtype, maps, lead)
        assert t.dtype == dtype and t.itemsize == size == dtype.itemsize and t.shape == (2,), name
        assert {n: t.dtype.fields[n][1] for n in t.dtype.names} == offsets, name
        assert t[lead[0]].tolist() == [4096, 8192] and t[lead[1]].tolist() == [3, 7] and t[lead[2]].tolist() == [5, 2], name
        assert all(not t[n].any() for n in dtype.names[3:]), name
    t = record_table(TILE_RECORD, maps, x1=[1, 2], y2=[9, 10])
    assert t["x1"].tolist() == [1, 2] and t["y2"].tolist() == [9, 10] and t["map"].tolist() == [4096, 8192]
    assert pp._TILE_RECORD is TILE_RECORD and pp._PAIR_RECORD is PAIR_RECORD and pp._GUIDED_RECORD is GUIDED_RECORD


@pytest.mark.parametrize("n, per_item, budget, cap, chunk", [(5, 10, 1, 65535, 1), (5, 10, 25, 65535, 2), (5, 10, 10 ** 9, 65535, 5),
                                                             (70000, 10, 10 ** 9, 65535, 65535), (5, 10, 10 ** 9, 3, 3)])
def test_scratch_chunk_rule(n, per_item, budget, cap, chunk):
    from muggled_dpt_amd.postprocess._common import scratch_chunk

    assert scratch_chunk(n, per_item, budget, "x", cap) == chunk == max(1, min(n, budget // per_item, cap))


def test_scratch_budget_must_be_positive():
    from muggled_dpt_amd.postprocess._common import scratch_chunk

    for bad in (0, -1):
        with pytest.raises(ValueError, match="x: max_scratch_bytes must be positive"):
            scratch_chunk(5, 10, bad, "x")


def test_prediction_count():
    import torch

    from muggled_dpt_amd.postprocess._common import prediction_count

    assert prediction_count(torch.zeros(4, 2, 3)) == 4 and prediction_count(torch.zeros(2, 3)) == -1
    assert prediction_count([1, 2, 3]) == 3 and prediction_count(()) == 0 and prediction_count(None) == -1 and prediction_count(np.zeros((2, 2, 2))) == -1


def test_ptr():
    import torch

    from muggled_dpt_amd.postprocess._common import ptr

    t = torch.zeros(3)
    assert ptr(None) is None and ptr(t) == t.data_ptr()


if __name__ == "__main__":
    with open(GOLDEN, "w") as fh:
        json.dump(surface(pp), fh, indent=1, sort_keys=True)
        fh.write("\n")
