"""postprocess.fill_holes (mdpt_post_fill_holes, csrc/postprocess.hip fill_* kernels) against the numpy restatement of tests/fill_restate.py: on
the restatement's safe pixels the colour is equal byte for byte and the depth bit for bit - the definition uses correctly rounded fp64 + x / in a
fixed order, so a difference is a bug or a contraction, not a tolerance. tests/test_fill_cpu.py holds every case to at most 2 % unsafe pixels."""
import ctypes

import numpy as np
import pytest
import torch

from muggled_dpt_amd import native
from muggled_dpt_amd import postprocess as pp
from tests import fill_restate as fr

pytestmark = pytest.mark.gpu

RUNS = [(hw, family, band) for hw in fr.SIZES for family, band in fr.FAMILIES]


def device_case(hw, family):
    color, depth = fr.case(*hw, family)
    return torch.from_numpy(color.copy()).cuda(), torch.from_numpy(depth.copy()).cuda()


@pytest.mark.parametrize("hw, family, band", RUNS, ids=[f"{h}x{w}-{f}-{b}" for (h, w), f, b in RUNS])
def test_fill_matches_restatement(hw, family, band):
    color, depth = device_case(hw, family)
    out_c, out_d = pp.fill_holes(color, depth, band, return_depth=True)
    assert out_c.shape == color.shape and out_d.shape == depth.shape and (out_c.dtype, out_d.dtype) == (torch.uint8, torch.float32)
    got_c, got_d = out_c.cpu().numpy(), out_d.cpu().numpy()
    host_c, host_d = fr.case(*hw, family)
    for i, r in enumerate(fr.reference(*hw, family, band)):
        safe, where = r["safe"], (hw, family, band, i)
        diff_c = (got_c[i] != r["color"]).any(axis=-1)
        diff_d = got_d[i].view(np.uint32) != r["depth"].view(np.uint32)
        print(f"{where}: valid {r['valid'].mean():.3f} unsafe {(~safe).mean():.4f} colour differs on {int(diff_c[safe].sum())} depth on {int(diff_d[safe].sum())}"
              f" of {int(safe.sum())} safe pixels")
        assert (~safe).mean() <= 0.02, where
        assert not diff_c[safe].any() and not diff_d[safe].any(), where
        # what was valid is the input, byte for byte and bit for bit
        valid = r["valid"]
        assert (got_c[i][valid] == host_c[i][valid]).all() and (got_d[i].view(np.uint32)[valid] == host_d[i].view(np.uint32)[valid]).all(), where
    # the empty image is background, whatever its neighbours in the call hold
    assert (got_c[0] == 0).all() and np.isposinf(got_d[0]).all()
    assert (got_c[2][..., 3] == 255).all()
    # the colour alone is the same colour
    assert torch.equal(pp.fill_holes(color, depth, band), out_c)


@pytest.mark.parametrize("hw", [(70, 45), (9, 270)])
def test_deterministic_and_images_independent(hw):
    color, depth = device_case(hw, "cont")
    a = pp.fill_holes(color, depth, 0.1, return_depth=True)
    b = pp.fill_holes(color, depth, 0.1, return_depth=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    for i in range(3):
        one = pp.fill_holes(color[i], depth[i], 0.1, return_depth=True)
        assert one[0].shape == color.shape[1:] and one[1].shape == depth.shape[1:]
        assert torch.equal(one[0], a[0][i]) and torch.equal(one[1].view(torch.int32), a[1][i].view(torch.int32)), i
    # a scratch cap that one image alone exceeds: one image per call, the same bits
    small = pp.fill_holes(color, depth, 0.1, return_depth=True, max_scratch_bytes=1)
    assert all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(small, a))
    per = ctypes.c_size_t()
    lib = native.load()
    native.check(lib, lib.mdpt_post_fill_scratch_bytes(1, hw[0], hw[1], ctypes.byref(per)))
    two = pp.fill_holes(color, depth, 0.1, return_depth=True, max_scratch_bytes=2 * per.value)
    assert all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(two, a))


@pytest.mark.parametrize("hw", [(5, 3), (33, 17), (130, 67), (9, 270)])
def test_the_scratch_contents_before_do_not_matter(hw):
    color, depth = device_case(hw, "cont")
    want_c, want_d = pp.fill_holes(color, depth, 0.1, return_depth=True)
    lib = native.load()
    need = ctypes.c_size_t()
    native.check(lib, lib.mdpt_post_fill_scratch_bytes(3, hw[0], hw[1], ctypes.byref(need)))
    levels = fr.level_sizes(*hw)[1:]
    assert need.value == 3 * 16 * sum(h * w for h, w in levels)
    scratch = torch.full((need.value,), 0xFF, dtype=torch.uint8, device="cuda")
    out_c, out_d = torch.empty_like(color), torch.empty_like(depth)
    stream = torch.cuda.current_stream().cuda_stream
    native.check(lib, lib.mdpt_post_fill_holes(color.data_ptr(), depth.data_ptr(), 3, hw[0], hw[1], 0.1, out_c.data_ptr(), out_d.data_ptr(),
                                               scratch.data_ptr(), need.value, stream))
    assert torch.equal(out_c, want_c) and torch.equal(out_d.view(torch.int32), want_d.view(torch.int32))
    # no depth output asked for: the colour is the same
    out_c2 = torch.empty_like(color)
    native.check(lib, lib.mdpt_post_fill_holes(color.data_ptr(), depth.data_ptr(), 3, hw[0], hw[1], 0.1, out_c2.data_ptr(), None, scratch.data_ptr(),
                                               need.value, stream))
    assert torch.equal(out_c2, want_c)


def test_leading_dims_are_kept_and_inputs_untouched():
    color, depth = device_case((33, 17), "cont")
    c4 = torch.stack([color, color.flip(0)])  # [2,3,h,w,4]
    d4 = torch.stack([depth, depth.flip(0)])
    before = (c4.clone(), d4.clone())
    out_c, out_d = pp.fill_holes(c4, d4, 0.1, return_depth=True)
    assert out_c.shape == c4.shape and out_d.shape == d4.shape
    want = pp.fill_holes(color, depth, 0.1, return_depth=True)
    assert torch.equal(out_c[0], want[0]) and torch.equal(out_c[1], want[0].flip(0))
    assert torch.equal(out_d[0].view(torch.int32), want[1].view(torch.int32))
    assert torch.equal(c4, before[0]) and torch.equal(d4.view(torch.int32), before[1].view(torch.int32))
    # a strided view is copied, not misread
    wide = torch.cat([color, color], dim=2)[:, :, :17]
    assert torch.equal(pp.fill_holes(wide, depth, 0.1), want[0])


def test_bad_arguments_raise():
    color, depth = device_case((5, 3), "cont")
    with pytest.raises(TypeError, match="color must be a tensor"):
        pp.fill_holes(color.cpu().numpy(), depth)
    with pytest.raises(ValueError, match=r"color must be uint8 \[...,h,w,4\]"):
        pp.fill_holes(color.float(), depth)
    with pytest.raises(ValueError, match=r"color must be uint8 \[...,h,w,4\]"):
        pp.fill_holes(color[..., :3], depth)
    with pytest.raises(ValueError, match="depth must be float32"):
        pp.fill_holes(color, depth.double())
    with pytest.raises(ValueError, match="depth must be float32"):
        pp.fill_holes(color, depth[:2])
    for band in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match=r"band must be in \[0, 1\]"):
            pp.fill_holes(color, depth, band)
    with pytest.raises(TypeError, match="band must be a number"):
        pp.fill_holes(color, depth, "0.1")
    with pytest.raises(ValueError, match="max_scratch_bytes must be positive"):
        pp.fill_holes(color, depth, max_scratch_bytes=0)
    with pytest.raises(RuntimeError, match="expected a CUDA tensor"):
        pp.fill_holes(color.cpu(), depth.cpu())
    # the C entry points refuse what they cannot run, with a text
    lib = native.load()
    n = ctypes.c_size_t()
    scratch = torch.empty(4096, dtype=torch.uint8, device="cuda")
    out = torch.empty_like(color)
    args = dict(c=color.data_ptr(), d=depth.data_ptr(), n=3, h=5, w=3, band=0.1, o=out.data_ptr(), od=None, s=scratch.data_ptr(), sb=4096)

    def call(**kw):
        a = {**args, **kw}
        return lib.mdpt_post_fill_holes(a["c"], a["d"], a["n"], a["h"], a["w"], a["band"], a["o"], a["od"], a["s"], a["sb"], None)

    assert lib.mdpt_post_fill_scratch_bytes(3, 5, 3, None) != 0 and lib.mdpt_post_fill_scratch_bytes(0, 5, 3, ctypes.byref(n)) != 0
    assert lib.mdpt_post_fill_scratch_bytes(3, 5, 40000, ctypes.byref(n)) != 0
    for kw, text in ((dict(c=None), "null"), (dict(d=None), "null"), (dict(o=None), "null"), (dict(s=None), "null"), (dict(n=0), "image count"),
                     (dict(h=0), "image size"), (dict(w=-3), "image size"), (dict(band=-0.5), "band"), (dict(band=1.01), "band"),
                     (dict(band=float("nan")), "band"), (dict(sb=16), "scratch"), (dict(o=color.data_ptr()), "of their own")):
        assert call(**kw) != 0, kw
        assert text in lib.mdpt_last_error().decode(), (kw, lib.mdpt_last_error())
    assert call() == 0
    torch.cuda.synchronize()
