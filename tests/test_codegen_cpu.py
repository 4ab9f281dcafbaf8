"""Code-generation guard (no GPU needed: hipcc cross-compiles gfx950): the 8-phase GEMM main loop and the attention kernel run at the
256-VGPR occupancy limit, where a few extra live values turn into scratch spills inside the loop (measured: -6 % end to end, 2x on the
residual epilogue). Compile the kernels to ISA text and require ScratchSize == 0 for every hot kernel."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "muggled_dpt_amd", "csrc")


def _kernel_stats(src, tmp_path, extra=()):
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")
    if not hipcc:
        pytest.skip("hipcc not available")
    out = str(tmp_path / (src + ".s"))
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(REPO, "include"), "-I", CSRC, *extra, "-x", "hip",
                        "--cuda-device-only", "-S", os.path.join(CSRC, src), "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    stats, name = {}, None
    for line in open(out):
        m = re.match(r"^(_Z\S+):\s", line)
        if m:
            name = m.group(1)
        m = re.match(r"^; (NumVgprs|ScratchSize): (\d+)", line)
        if m and name:
            stats.setdefault(name, {})[m.group(1)] = int(m.group(2))
    return stats


# The instantiations that spill, by mangled template arguments <NQN, NP, SKIP, F32OUT, RELU, UP, BFOUT, UPIN, F8>, with the scratch bytes per lane
# read from the ISA of the commit that added conv3h.hip to this guard (an open item of DESIGN.md, not a budget: none may grow, no other may spill).
# Both are three-pass 256-channel forms with the skip add: conv3h_kernel<2, 3, true, true, true, true, true> and <2, 3, true, false, false, false, true>.
KNOWN_SPILLS = {
    ("conv3h.hip", "bf16"): {"conv3h_kernelILi2ELi3ELb1ELb1ELb1ELb1ELb1ELb0ELb0EE": 16, "conv3h_kernelILi2ELi3ELb1ELb0ELb0ELb0ELb1ELb0ELb0EE": 8},
    ("conv3h.hip", "fp16"): {"conv3h_kernelILi2ELi3ELb1ELb1ELb1ELb1ELb1ELb0ELb0EE": 16, "conv3h_kernelILi2ELi3ELb1ELb0ELb0ELb0ELb1ELb0ELb0EE": 16},
}


@pytest.mark.parametrize("operands", ["bf16", "fp16"])  # every kernel file exists once per MFMA operand format (csrc/op_types.h)
@pytest.mark.parametrize("src,pattern,at_least", [("gemm.hip", "gemm8_kernel", 6), ("attention.hip", "attn_kernel", 6),
                                                  ("head.hip", "head_tail_kernel", 2), ("conv3h.hip", "conv3h_kernel", 19)])
def test_hot_kernels_do_not_spill(tmp_path, src, pattern, at_least, operands):
    extra = ("-DMDPT_OP_F16",) if operands == "fp16" else ()
    stats = {k: v for k, v in _kernel_stats(src, tmp_path, extra).items() if pattern in k}
    assert len(stats) >= at_least, sorted(stats)
    known = KNOWN_SPILLS.get((src, operands), {})
    assert all(any(k in name for name in stats) for k in known), "a named exception no longer exists: remove it"
    for name, s in stats.items():
        allowed = max([b for k, b in known.items() if k in name], default=0)
        if allowed:
            assert s["ScratchSize"] <= allowed, f"{name} spills {s['ScratchSize']} bytes of scratch per lane, {allowed} when it was recorded"
            assert s["NumVgprs"] <= 256
            continue
        # (incl. the fp8 cross-term forms gemm8_kernel<..., true>, MDPT_PASSES_2F8 / _3F8: with four weight pointers instead of one they reloaded spilled
        #  pointer pairs inside the fp16 loop - a vmcnt(0) each, 370 us against 310 us for three fp16 passes on the 36x36 fusion convs)
        assert s["ScratchSize"] == 0, f"{name} spills {s['ScratchSize']} bytes of scratch per lane ({s['NumVgprs']} VGPRs)"
        assert s["NumVgprs"] <= 256
