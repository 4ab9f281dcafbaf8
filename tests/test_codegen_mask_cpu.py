"""Code-generation guard of the depth masking kernels (no GPU needed: hipcc cross-compiles gfx950), as tests/test_codegen_cpu.py guards the hot
kernels: the cutout and display kernels must not spill (ScratchSize == 0), and the cutout keeps its wide accesses (a dwordx3 BGR load, a dwordx4
BGRA store)."""
import re

from tests.test_codegen_cpu import _kernel_stats


def test_mask_kernels_do_not_spill(tmp_path):
    stats = {k: v for k, v in _kernel_stats("postprocess.hip", tmp_path).items() if re.search(r"mask_(cutout|display)_kernel", k)}
    assert len(stats) == 2, sorted(stats)
    for name, s in stats.items():
        assert s["ScratchSize"] == 0, f"{name} spills {s['ScratchSize']} bytes of scratch per lane ({s['NumVgprs']} VGPRs)"
        assert s["NumVgprs"] <= 128


def test_cutout_uses_wide_accesses(tmp_path):
    _kernel_stats("postprocess.hip", tmp_path)
    body, inside = [], False
    for line in open(tmp_path / "postprocess.hip.s"):
        if re.match(r"^_Z\S*mask_cutout_kernel\S*:", line):
            inside = True
        elif inside and line.strip().startswith("s_endpgm"):
            break
        elif inside:
            body.append(line)
    text = "".join(body)
    assert "global_load_dwordx3" in text and "global_store_dwordx4" in text
