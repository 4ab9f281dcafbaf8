"""postprocess.block_norm_display (mdpt_post_block_norm_tiles): BlockData.__init__ of the reference's experiments/block_norm_visualization.py
(:137-147: each map normalised by its own min / max and rounded to uint8) and the nearest-neighbour enlargement of its tiles (:207-233), for
every block and image in one launch, against the same arithmetic in numpy float32 - byte for byte. The inputs are hand-made maps. `pytest -m gpu`."""
import numpy as np
import pytest
import torch

from muggled_dpt_amd import postprocess as pp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_native_lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from muggled_dpt_amd import native
    native.load()


def _numpy_tile(n: np.ndarray, hw) -> np.ndarray:
    """the reference's normalisation in float32 as numpy evaluates it, then np.repeat by the whole factors"""
    assert n.dtype == np.float32
    u8 = np.round(((n - n.min()) / (n.max() - n.min())) * 255).astype(np.uint8)
    return np.repeat(np.repeat(u8, hw[0] // n.shape[0], axis=0), hw[1] // n.shape[1], axis=1)


def _random_maps(sizes, b, seed):
    """seeded maps in the ranges block norms take: a positive bulk, a few large 'register token' cells, one map around zero (channel planes)"""
    rng = np.random.default_rng(seed)
    maps = []
    for l, (h, w) in enumerate(sizes):
        m = rng.gamma(4.0, 3.0, (b, h, w)).astype(np.float32)
        if l % 3 == 1:
            m = rng.standard_normal((b, h, w)).astype(np.float32) * np.float32(0.37)
        if l % 2 == 0:
            m[:, h // 2, w // 3] *= np.float32(37.0)
        maps.append(m)
    return maps


SIZES = [(24, 36), (24, 36), (12, 18), (12, 18), (6, 9), (3, 9)]  # L = 6: whole factors 1, 2, 4 and (8, 4) of the 24x36 tile


def test_tiles_and_minmax_are_numpys_byte_for_byte():
    b = 3
    maps = _random_maps(SIZES, b, 11)
    tiles, minmax = pp.block_norm_display([torch.from_numpy(m).cuda() for m in maps])
    assert tiles.dtype == torch.uint8 and tuple(tiles.shape) == (6, b, 24, 36)
    assert minmax.dtype == torch.float32 and tuple(minmax.shape) == (6, b, 2)
    tiles, minmax = tiles.cpu().numpy(), minmax.cpu().numpy()
    for l, m in enumerate(maps):
        for i in range(b):
            want = _numpy_tile(m[i], (24, 36))
            assert np.array_equal(tiles[l, i], want), f"map {l} image {i}: {int((tiles[l, i] != want).sum())} bytes differ"
            assert minmax[l, i, 0].tobytes() == m[i].min().tobytes() and minmax[l, i, 1].tobytes() == m[i].max().tobytes(), (l, i)
    # an explicit, larger tile size; and one [L, B, h, w] tensor instead of a list
    big, _ = pp.block_norm_display([torch.from_numpy(m).cuda() for m in maps], max_token_hw=(48, 72))
    assert tuple(big.shape) == (6, b, 48, 72)
    big = big.cpu().numpy()
    for l, m in enumerate(maps):
        for i in range(b):
            assert np.array_equal(big[l, i], _numpy_tile(m[i], (48, 72))), (l, i)
    stacked = torch.from_numpy(np.stack(maps[:2])).cuda()
    t2, mm2 = pp.block_norm_display(stacked)
    assert np.array_equal(t2.cpu().numpy(), tiles[:2]) and np.array_equal(mm2.cpu().numpy(), minmax[:2])


def test_more_maps_than_one_launch_holds_and_rounding_ties():
    """40 maps (two launches of the 32-map table); maps built so that many values land exactly on x.5 before rounding (ties go to even)."""
    b = 2
    maps = _random_maps([(6, 9)] * 39, b, 5)
    tie = np.zeros((b, 8, 64), dtype=np.float32)
    tie[:] = (np.arange(512, dtype=np.float32) * np.float32(0.5)).reshape(8, 64)  # 0, 0.5, ... 255.5: (n - 0) / 255.5 * 255
    tie[1] *= np.float32(2.0)
    tiles, minmax = pp.block_norm_display([torch.from_numpy(m).cuda() for m in maps])
    tiles = tiles.cpu().numpy()
    for l, m in enumerate(maps):
        for i in range(b):
            assert np.array_equal(tiles[l, i], _numpy_tile(m[i], (6, 9))), (l, i)
    tt, _ = pp.block_norm_display([torch.from_numpy(tie).cuda()])
    for i in range(b):
        assert np.array_equal(tt[0, i].cpu().numpy(), _numpy_tile(tie[i], (8, 64))), i
    half = np.array([[0.0, 0.5, 1.5, 2.5, 3.5, 127.5, 254.5, 255.0]], dtype=np.float32)[None]  # range 255: the values are their own tile values
    th, _ = pp.block_norm_display([torch.from_numpy(half).cuda()])
    assert th[0, 0, 0].cpu().tolist() == [0, 0, 2, 2, 4, 128, 254, 255] == _numpy_tile(half[0], (1, 8))[0].tolist()


def test_a_size_that_is_no_whole_factor_raises():
    maps = [torch.zeros(3, 24, 36, device="cuda"), torch.zeros(3, 3, 5, device="cuda")]
    with pytest.raises(ValueError, match="whole factors"):
        pp.block_norm_display(maps)
    with pytest.raises(ValueError, match="whole factors"):
        pp.block_norm_display(maps[:1], max_token_hw=(36, 36))
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        pp.block_norm_display([torch.zeros(3, 24, 36)])


def test_colormap_is_the_modules_colormap_path():
    b = 3
    maps = [torch.from_numpy(m).cuda() for m in _random_maps(SIZES, b, 23)]
    rng = np.random.default_rng(2)
    lut = rng.integers(0, 256, (1, 256, 3), dtype=np.uint8)
    gray, mm_gray = pp.block_norm_display(maps)
    color, mm = pp.block_norm_display(maps, lut=lut)
    assert color.dtype == torch.uint8 and tuple(color.shape) == (6, b, 24, 36, 3)
    for l in range(6):
        assert torch.equal(color[l], pp.apply_colormap(gray[l], lut)), l
    assert torch.equal(mm.view(torch.int32), mm_gray.view(torch.int32))
    # the LUT may be a device tensor too
    color2, _ = pp.block_norm_display(maps, lut=torch.from_numpy(lut).cuda())
    assert torch.equal(color2, color)


def test_constant_and_nan_maps_give_zero_tiles_and_leave_their_neighbours_alone():
    b = 3
    maps = _random_maps(SIZES, b, 31)
    clean = [m.copy() for m in maps]
    maps[1][2, :, :] = np.float32(4.25)          # a constant map: 0 / 0
    maps[2][0, 5, 7] = np.float32("nan")         # one NaN among 12 x 18 values
    maps[5][1, :, :] = np.float32(0.0)           # constant zero, in an enlarged map
    tiles, minmax = pp.block_norm_display([torch.from_numpy(m).cuda() for m in maps])
    tiles, minmax = tiles.cpu().numpy(), minmax.cpu().numpy()
    degenerate = {(1, 2), (2, 0), (5, 1)}
    for l in range(6):
        for i in range(b):
            if (l, i) in degenerate:
                assert not tiles[l, i].any(), (l, i)
            else:
                assert np.array_equal(tiles[l, i], _numpy_tile(clean[l][i], (24, 36))), (l, i)
                assert minmax[l, i].tolist() == [float(clean[l][i].min()), float(clean[l][i].max())]
    assert minmax[1, 2].tolist() == [4.25, 4.25] and minmax[5, 1].tolist() == [0.0, 0.0]
    assert np.isnan(minmax[2, 0]).all()  # min / max as numpy computes them for a map holding a NaN


def test_end_to_end_on_swin2_tiny():
    import muggled_dpt_amd as mda
    from muggled_dpt_amd.synthetic import make_synthetic_swinv2_state_dict
    from tests.helpers import seeded_input
    cfg, model = mda.make_swinv2_dpt_from_midas_v31_state_dict(make_synthetic_swinv2_state_dict("swin2_tiny", 5))
    model = model.to("cuda", torch.float32)
    x = seeded_input((2, 3, 64, 96), seed=13).cuda()
    norms, grid = model.block_norms(x)
    assert tuple(grid) == (16, 24)
    tiles, minmax = pp.block_norm_display(norms)
    n_blocks = sum(int(n) for n in cfg["layers_per_stage"])
    assert tuple(tiles.shape) == (n_blocks, 2, 16, 24) and tuple(minmax.shape) == (n_blocks, 2, 2)
    stage_of = [s for s, nl in enumerate(cfg["layers_per_stage"]) for _ in range(int(nl))]
    t = tiles.cpu().numpy()
    for l, s in enumerate(stage_of):
        f = 1 << s
        cells = t[l].reshape(2, 16 // f, f, 24 // f, f)
        assert (cells == cells[:, :, :1, :, :1]).all(), f"block {l} (stage {s}) is not constant over {f}x{f} cells"
        for i in range(2):  # and it is the numpy tile of that block's own norm map
            assert np.array_equal(t[l, i], np.repeat(np.repeat(_numpy_tile(norms[l][i].cpu().numpy(), norms[l][i].shape), f, 0), f, 1)), (l, i)
        assert t[l].max() == 255 and t[l].min() == 0
