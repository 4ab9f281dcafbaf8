"""Block norm capture and tiles, the parts that need no GPU: the C ABI surface (mdpt_encoder_block_norms, mdpt_post_block_norm_*), the argument
checks of DPTModel.block_norms / postprocess.block_norm_display that run before any device use, and the tool's option."""
import os
import re
import subprocess
import sys

import pytest
import torch

from muggled_dpt_amd import native
from muggled_dpt_amd import postprocess as pp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_new_entry_points_are_typed_exported_and_declared():
    header = open(os.path.join(REPO, "include", "mdpt.h")).read()
    declared = set(re.findall(r"\b(mdpt_[a-z0-9_]+)\s*\(", header))
    post = sorted(n for n in native.SYMBOLS if n.startswith("mdpt_post_block_norm_"))
    assert post, "no mdpt_post_block_norm_* entry point in native.SYMBOLS"
    lib = native.load()
    for name in ["mdpt_encoder_block_norms", *post]:
        assert name in native.SYMBOLS and name in declared and hasattr(lib, name), name
    assert sorted(n for n in declared if n.startswith("mdpt_post_block_norm_")) == post
    # additive: the ABI version did not move
    assert native.ABI_VERSION == 6 == lib.mdpt_abi_version()
    # the encoder entry names every argument the issue lists, the taps where mdpt_encoder_probe_blocks has them
    proto = re.search(r"int mdpt_encoder_block_norms\(([^;]*)\);", header).group(1)
    names = [a.split()[-1].split("[")[0].lstrip("*") for a in proto.replace("\n", " ").split(",")]
    assert names == ["h", "tokens_bnf", "B", "gh", "gw", "stage_out", "norm_out", "channel_index", "channel_out", "workspace", "workspace_bytes", "stream"]
    assert len(native.SYMBOLS["mdpt_encoder_block_norms"][1]) == len(names)


def test_display_rejects_host_tensors_and_non_whole_factors_before_the_device():
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        pp.block_norm_display([torch.zeros(2, 4, 6), torch.zeros(2, 2, 3)])
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        pp.block_norm_display(torch.zeros(3, 2, 4, 6))
    # 3x5 does not divide 6x9; checked on shapes alone (the tensors are on the host: a device check would have raised RuntimeError first)
    with pytest.raises(ValueError, match="whole factors"):
        pp.block_norm_display([torch.zeros(2, 6, 9), torch.zeros(2, 3, 5)])
    with pytest.raises(ValueError, match="whole factors"):
        pp.block_norm_display([torch.zeros(1, 6, 9)], max_token_hw=(9, 9))
    with pytest.raises(ValueError, match="batch size"):
        pp.block_norm_display([torch.zeros(2, 6, 9), torch.zeros(1, 6, 9)])
    with pytest.raises(ValueError):
        pp.block_norm_display([])
    with pytest.raises(RuntimeError):
        pp.block_norm_display([torch.zeros(6, 9)])


def _cpu_models():
    import muggled_dpt_amd as mda
    from muggled_dpt_amd.synthetic import make_synthetic_swinv2_state_dict
    from tests.helpers import synthetic_model
    osd, _, _ = synthetic_model("tiny", 0)
    _, vit = mda.make_depthanythingv2_dpt_from_original_state_dict(osd)
    _, swin = mda.make_swinv2_dpt_from_midas_v31_state_dict(make_synthetic_swinv2_state_dict("swin2_tiny", 1))
    return vit, swin


def test_channels_argument_is_checked_before_any_device_use():
    """The models live on the CPU: anything that reached the engine would raise RuntimeError ("MI355X GPUs only")."""
    vit, swin = _cpu_models()
    x = torch.zeros(1, 3, 56, 56)
    tokens = torch.zeros(1, 16, 64)
    for call in (lambda ch: vit.block_norms(x, channels=ch), lambda ch: vit.imgencoder.block_norms(tokens, (4, 4), channels=ch)):
        with pytest.raises(ValueError, match="4 blocks but 3"):
            call([0, 1, 2])
        with pytest.raises(ValueError, match="outside"):
            call(-1)
        with pytest.raises(ValueError, match="outside"):
            call([0, 0, 64, 0])  # F = 64
        with pytest.raises(TypeError):
            call([0, 0, 1.5, 0])
        with pytest.raises(TypeError):
            call("3")
        with pytest.raises(RuntimeError, match="MI355X"):  # a valid argument gets as far as the engine
            call([0, 1, 2, 63])
    # SwinV2: the bound is the width of the block's own stage (64, 128, 256, 512 over 2 + 2 + 4 + 2 blocks)
    assert swin.imgencoder._check_channels(63) == [63] * 10
    assert swin.imgencoder._check_channels([63, 63, 127, 127, 255, 255, 255, 255, 511, 511])[-1] == 511
    with pytest.raises(ValueError, match=r"block 0 is outside \[0, 64\)"):
        swin.imgencoder._check_channels(64)
    with pytest.raises(ValueError, match=r"block 3 is outside \[0, 128\)"):
        swin.imgencoder._check_channels([0, 0, 0, 128, 0, 0, 0, 0, 0, 0])
    assert vit.imgencoder._check_channels(None) is None


def test_run_image_tool_lists_the_block_norms_option():
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "mdpt_run_image.py"), "--help"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--block_norms" in r.stdout
