"""Code-generation guard of the depth segmentation kernels (no GPU needed: hipcc cross-compiles gfx950), as tests/test_codegen_mask_cpu.py guards the
masking kernels: none of them may spill (ScratchSize == 0), and the cutout keeps its wide accesses (a dwordx3 BGR load, a dwordx4 BGRA store; flat-addressed, as the pointers are read from the device table). The
VGPR and LDS figures are recorded in profiles/segment_codegen.txt."""
import os
import re

from tests.test_codegen_cpu import REPO, _kernel_stats

KERNELS = ("minmax", "state", "tile", "merge", "flatten", "flag", "scan", "scatter", "relabel", "finish", "colors", "pick", "cutout")


def test_segment_kernels_do_not_spill(tmp_path):
    stats = {k: v for k, v in _kernel_stats("postprocess.hip", tmp_path).items() if re.search(r"segment_\w+_kernel", k)}
    assert sorted(re.search(r"segment_(\w+?)_kernel", k).group(1) for k in stats) == sorted(KERNELS), sorted(stats)
    for name, s in stats.items():
        assert s["ScratchSize"] == 0, f"{name} spills {s['ScratchSize']} bytes of scratch per lane ({s['NumVgprs']} VGPRs)"
        assert s["NumVgprs"] <= 64, (name, s)  # (the tile kernel runs 1024 threads a workgroup: 16 waves a CU need <= 128; the rest stay far below)


def test_segment_cutout_uses_wide_accesses(tmp_path):
    _kernel_stats("postprocess.hip", tmp_path)
    body, inside = [], False
    for line in open(tmp_path / "postprocess.hip.s"):
        if re.match(r"^_Z\S*segment_cutout_kernel\S*:", line):
            inside = True
        elif inside and line.startswith(".Lfunc_end"):
            break
        elif inside:
            body.append(line)
    text = "".join(body)
    # (the photo and output pointers come out of the device table, so the compiler addresses them as flat: the width is what is held here)
    assert re.search(r"(global|flat)_load_dwordx3", text) and re.search(r"(global|flat)_store_dwordx4", text)


def test_the_recorded_figures_name_every_kernel():
    text = open(os.path.join(REPO, "profiles", "segment_codegen.txt")).read()
    for k in KERNELS:
        assert f"segment_{k}_kernel" in text, k
