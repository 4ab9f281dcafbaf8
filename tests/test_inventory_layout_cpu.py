"""The parameter inventory and the packed-weight / workspace layout of libmdpt, pinned against recorded values (no GPU, no compute calls).

tests/golden/inventory_layout.json was recorded with the library as it stood before the stage drivers switched from by-name lookups to typed
weight references: the order of mdpt_weight_name(i) (the .mdpt export and the strict-load messages depend on it), mdpt_packed_bytes (the order and
sizes of every packed matrix / vector, lo and fp8 planes included) and mdpt_workspace_bytes must not move when host code is reorganised.
Re-record (only with a change that is MEANT to move the layout): python -m tests.test_inventory_layout_cpu"""
import ctypes
import hashlib
import json
import os

import pytest

from muggled_dpt_amd import native
from muggled_dpt_amd.dpt_model import native_config
from muggled_dpt_amd.synthetic import BEIT_CONFIGS, STANDARD_CONFIGS, SWINV2_CONFIGS

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "inventory_layout.json")

# one toy of every family `synthetic` can build (config, family, a legal image size), plus the fp8-eligible toy of tests/test_gpu_f8_cross.py
# (every contraction length a multiple of 128: the mixed mode's fp8 weight planes exist) and the 96-wide first stage of swin2_tiny_256
F8_TOY = dict(features_per_token=128, num_heads=2, num_blocks=4, reassembly_features_list=[128, 128, 256, 256], base_patch_grid_hw=(5, 5),
              fusion_channels=256, patch_size_px=14)
CONFIGS = {
    "dav2_tiny": (STANDARD_CONFIGS["tiny"], "v2", 56),
    "dav1_tiny": (STANDARD_CONFIGS["tiny"], "v1", 56),
    "dav2_tiny_giant": (STANDARD_CONFIGS["tiny_giant"], "v2", 56),
    "dav2_f8_toy": (F8_TOY, "v2", 56),
    "beit_tiny": (BEIT_CONFIGS["beit_tiny"], "beit", 64),
    "swin2_tiny": (SWINV2_CONFIGS["swin2_tiny"], "swinv2", 64),
    "swin2_tiny_256": (SWINV2_CONFIGS["swin2_tiny_256"], "swinv2", 128),
}
HEAD = native.OP_CLASSES.index("head")
# (precision, call made on the fresh handle: both rebuild the inventory of a handle that already has one)
MODES = {
    "bf16": (native.PREC_BF16, None),
    "fp16": (native.PREC_FP16, None),
    "mixed": (native.PREC_MIXED, None),
    "bf16x3": (native.PREC_BF16X3, None),
    "mixed_head2": (native.PREC_MIXED, lambda lib, h: lib.mdpt_set_class_passes(h, HEAD, 2)),
    "mixed_nowrc": (native.PREC_MIXED, lambda lib, h: lib.mdpt_set_weight_rounding_compensation(h, 0)),
}
CASES = [f"{c}-{m}" for c in CONFIGS for m in MODES]


def measure(lib, case: str) -> dict:
    config, mode = case.split("-")
    cfg, family, size = CONFIGS[config]
    precision, after_create = MODES[mode]
    h = ctypes.c_void_p()
    assert lib.mdpt_create(ctypes.byref(native_config(cfg, family, precision)), ctypes.byref(h)) == 0, lib.mdpt_last_error()
    try:
        if after_create:
            assert after_create(lib, h) == 0, lib.mdpt_last_error()
        sha = hashlib.sha256()
        n = lib.mdpt_num_weights(h)
        ndim, shape = ctypes.c_int32(), (ctypes.c_int64 * 4)()
        for i in range(n):
            assert lib.mdpt_weight_shape(h, i, ctypes.byref(ndim), shape) == 0
            sha.update(repr((lib.mdpt_weight_name(h, i).decode(), list(shape)[: ndim.value])).encode())
        out = {"num_weights": n, "names_and_shapes_sha256": sha.hexdigest()}
        v = ctypes.c_size_t()
        assert lib.mdpt_packed_bytes(h, ctypes.byref(v)) == 0
        out["packed_bytes"] = v.value
        for batch in (1, 8):
            assert lib.mdpt_workspace_bytes(h, batch, size, size, ctypes.byref(v)) == 0, lib.mdpt_last_error()
            out[f"workspace_bytes_b{batch}"] = v.value
        return out
    finally:
        lib.mdpt_destroy(h)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


def test_golden_file_covers_exactly_the_cases(golden):
    assert sorted(golden) == sorted(CASES)


@pytest.mark.parametrize("case", CASES)
def test_inventory_and_layout_match_the_recorded_values(golden, case):
    assert measure(native.load(), case) == golden[case]


def test_rebuilt_inventories_differ_from_the_plain_mixed_one(golden):
    """the two calls that rebuild a handle's inventory really move the layout (so the cases above exercise the rebuild), and keep the names"""
    for config in CONFIGS:
        mixed, head2, nowrc = (golden[f"{config}-{m}"] for m in ("mixed", "mixed_head2", "mixed_nowrc"))
        assert head2["names_and_shapes_sha256"] == nowrc["names_and_shapes_sha256"] == mixed["names_and_shapes_sha256"]
        assert nowrc["packed_bytes"] < mixed["packed_bytes"], config  # no residue planes of the compensated encoder Linears
        # the head class of mixed runs three terms in the MiDaS families and where the fp8 forms exist (two already in the other toys: a no-op there)
        if CONFIGS[config][1] in ("beit", "swinv2") or config == "dav2_f8_toy":
            assert head2["packed_bytes"] < mixed["packed_bytes"], config  # head conv 1 loses its lo / fp8 weight planes


if __name__ == "__main__":
    lib = native.load()
    with open(GOLDEN, "w") as fh:
        json.dump({case: measure(lib, case) for case in CASES}, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(f"recorded {len(CASES)} cases to {GOLDEN}")
