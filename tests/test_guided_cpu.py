"""Photo-guided upsampling without a GPU: properties of the fp64 restatement tests/guided_restate.py that the GPU tests measure the kernels against
(radius 0 is the bilinear resize, a flat photo gives the window means, a map affine in the guide comes back at full resolution), and the argument
checks of postprocess.guided_upsample_images / the C entry points, which raise before anything touches a device."""
import ctypes

import numpy as np
import pytest
import torch

from muggled_dpt_amd import native
from muggled_dpt_amd import postprocess as pp
from tests import guided_restate as gr


def _case(map_hw, photo_hw, seed=0):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.0, 50.0, map_hw), rng.integers(0, 256, (*photo_hw, 3), dtype=np.uint8)


def test_cells_partition_the_photo_and_none_is_empty():
    for (h, w), (H, W) in (((5, 7), (13, 17)), ((16, 16), (16, 16)), ((37, 29), (300, 211)), ((1, 1), (9, 4))):
        _, photo = _case((h, w), (H, W))
        n, s = gr.cell_sums(photo, h, w)
        assert n.min() >= 1 and n.sum() == H * W
        assert np.array_equal(s.sum(axis=(0, 1)), photo.reshape(-1, 3).astype(np.int64).sum(axis=0))
        # the cell of a pixel, the other way round: cell c holds [ceil(c N / n), ceil((c + 1) N / n))
        starts = [-(-c * H // h) for c in range(h + 1)]
        assert all(((np.arange(starts[c], starts[c + 1]) * h) // H == c).all() for c in range(h)) and starts[h] == H


@pytest.mark.parametrize("map_hw,photo_hw", [((5, 7), (13, 17)), ((16, 16), (16, 16)), ((9, 6), (40, 31))])
def test_radius_zero_is_the_bilinear_resize(map_hw, photo_hw):
    p, photo = _case(map_hw, photo_hw, 1)
    q, mean, _ = gr.guided_upsample(p, photo, 0, 1e-4)
    assert np.array_equal(mean[..., :3], np.zeros((*map_hw, 3))) and np.array_equal(mean[..., 3], p)  # a = 0 exactly, b = p
    assert np.array_equal(q, gr.bilinear_resize(p, *photo_hw).astype(np.float32))


@pytest.mark.parametrize("radius", [1, 3, 9])
def test_a_flat_photo_gives_the_window_means(radius):
    p, _ = _case((5, 7), (13, 17), 2)
    photo = np.full((13, 17, 3), 77, dtype=np.uint8)
    _, mean, q = gr.guided_upsample(p, photo, radius, 1e-4)
    mp = gr.window_mean(p[..., None], radius)
    want = gr.bilinear_planes(gr.window_mean(mp, radius), 13, 17)[..., 0]
    # Sigma = eps I up to the rounding of g g - g g (g = 77 / 255 is not a binary fraction), so a is of the order 1e-16 * 50 / eps, not 0
    assert np.abs(mean[..., :3]).max() < 1e-9 and np.abs(q - want).max() < 1e-9
    if radius == 9:  # every window is the whole grid: one constant everywhere
        assert np.abs(q - p.mean()).max() < 1e-9


def test_a_map_affine_in_the_guide_comes_back_at_full_resolution():
    """p = alpha . g + beta at map resolution, with a guide that varies in all three channels: (a, b) = (alpha, beta) up to the eps bias in every window, so
    q is the same function of the full-resolution photo - edges inside a cell included. eps = 1e-9 keeps the bias (of the order eps / var) small."""
    rng = np.random.default_rng(3)
    h, w, H, W = 8, 9, 41, 52
    photo = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    alpha, beta = np.array([2.0, -1.0, 0.5]), 3.0
    g = gr.low_res_guide(photo, h, w)
    p = g @ alpha + beta
    q, mean, _ = gr.guided_upsample(p, photo, 2, 1e-9)
    ideal = (photo / 255.0) @ alpha + beta
    assert np.abs(mean[..., :3] - alpha).max() < 1e-4 and np.abs(mean[..., 3] - beta).max() < 1e-4
    assert np.abs(q - ideal).max() < 1e-4
    assert np.abs(gr.bilinear_resize(p, H, W) - ideal).max() > 0.1  # what the bilinear route makes of the same map


def test_longdouble_run_bounds_the_restatements_own_noise():
    """The yardstick of tests/test_gpu_guided.py, measured where it is cheap: fp64 against extended precision on one small shape."""
    p, photo = _case((5, 7), (13, 17), 4)
    q, mean, q64 = gr.guided_upsample(p, photo, 3, 1e-4)
    _, mean_ld, q_ld = gr.guided_upsample(p, photo, 3, 1e-4, np.longdouble)
    assert float(np.abs(mean - mean_ld).max()) < 1e-9
    assert float(np.abs(q64 - q_ld).max()) < 2.0 ** -23 * 50 * 1e-3


# ---- argument checks: nothing below reaches a device

def test_guided_upsample_images_checks_its_arguments_before_touching_a_device():
    maps = [torch.zeros(1, 4, 5), torch.zeros(1, 3, 3)]
    photos = [np.zeros((8, 10, 3), np.uint8), np.zeros((6, 7, 3), np.uint8)]
    for bad in (-1, 65, 2.0, True, None):
        with pytest.raises(ValueError, match="radius"):
            pp.guided_upsample_images(maps, photos, radius=bad)
    for bad in (0.0, -1e-4, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="eps"):
            pp.guided_upsample_images(maps, photos, eps=bad)
    with pytest.raises(ValueError, match="2 predictions but 1 images"):
        pp.guided_upsample_images(maps, photos[:1])
    with pytest.raises(ValueError, match="2 predictions but 1 images"):
        pp.guided_upsample_images(torch.zeros(2, 4, 5), photos[:1])
    for bad in (np.zeros((8, 10), np.uint8), np.zeros((8, 10, 1), np.uint8), np.zeros((8, 10, 4), np.uint8), np.zeros((8, 10, 3), np.float32),
                torch.zeros(8, 10, 3)):
        with pytest.raises(ValueError, match="BGR"):
            pp.guided_upsample_images(maps, [bad, photos[1]])
    with pytest.raises(ValueError, match="scale_prediction"):
        pp.guided_upsample_images(maps, [np.zeros((3, 10, 3), np.uint8), photos[1]])
    with pytest.raises(ValueError, match="scale_prediction"):
        pp.guided_upsample_images(maps, [photos[0], np.zeros((6, 2, 3), np.uint8)])
    with pytest.raises(RuntimeError, match="CUDA"):  # host tensors: there is no CPU implementation
        pp.guided_upsample_images(maps, photos)


def _table(rows):
    t = np.zeros(len(rows), dtype=pp._GUIDED_RECORD)
    for k, r in enumerate(rows):
        t[k] = r
    return t


A = 0x10000  # an aligned, non-null address that is never read


def _row(h=5, w=7, H=13, W=17, map_=A, photo=A + 1, pitch=None, out=A, off=0):
    return (map_, h, w, photo, 3 * W if pitch is None else pitch, H, W, out, off)


def test_scratch_bytes_is_monotone_in_cells_and_pairs():
    lib = native.load()
    need = ctypes.c_size_t()

    def size(rows):
        t = _table(rows)
        assert lib.mdpt_post_guided_scratch_bytes(t.ctypes.data, len(t), ctypes.byref(need)) == 0
        return need.value

    one = size([_row()])
    assert one >= 5 * 7 * 4 * 8 and one % 8 == 0  # at least the fp64 [h,w,4] coefficients
    sizes = [size([_row(h=h, w=w)]) for h, w in ((1, 1), (2, 3), (5, 7), (6, 6), (37, 29), (504, 504))]
    assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
    assert size([_row(h=6, w=6)]) == size([_row(h=4, w=9)])  # a function of h w
    counts = [size([_row()] * k) for k in (1, 2, 3, 32)]
    assert counts == [one * k for k in (1, 2, 3, 32)]
    t = _table([_row()])
    assert lib.mdpt_post_guided_scratch_bytes(None, 1, ctypes.byref(need)) == -1 and lib.mdpt_post_guided_scratch_bytes(t.ctypes.data, 1, None) == -1
    for P in (0, -1, 70000):
        assert lib.mdpt_post_guided_scratch_bytes(t.ctypes.data, P, ctypes.byref(need)) == -1
    for bad in (_row(h=0), _row(w=-1), _row(h=65536, w=65536)):
        assert lib.mdpt_post_guided_scratch_bytes(_table([bad]).ctypes.data, 1, ctypes.byref(need)) == -1 and lib.mdpt_last_error()


def test_c_entry_point_checks_on_the_host_and_launches_nothing():
    """Pointers are plain numbers here: a call that got past its checks would fault, so every call must return its error first."""
    lib = native.load()
    need = ctypes.c_size_t()
    one = _table([_row()])
    assert lib.mdpt_post_guided_scratch_bytes(one.ctypes.data, 1, ctypes.byref(need)) == 0
    per = need.value

    def rc(table, P=None, dt=native.DTYPE_F32, radius=2, eps=1e-4, scratch=A, nbytes=None, coeffs=None, tdev=A, host=True):
        return lib.mdpt_post_guided_upsample(table.ctypes.data if host else None, tdev, len(table) if P is None else P, dt, radius, eps, scratch,
                                             len(table) * per if nbytes is None else nbytes, coeffs, None)

    good = _table([_row(), _row(off=per)])
    for kw in (dict(host=False), dict(tdev=0), dict(scratch=0), dict(P=0), dict(P=-3), dict(P=70000), dict(dt=7), dict(radius=-1), dict(radius=65), dict(eps=0.0),
               dict(eps=-1.0), dict(eps=float("nan")), dict(eps=float("inf")), dict(nbytes=2 * per - 8), dict(nbytes=0), dict(tdev=A + 4), dict(scratch=A + 4),
               dict(coeffs=A + 4)):
        assert rc(good, **kw) == -1, kw
        assert lib.mdpt_last_error(), kw
    bad_rows = {
        "null": _row(map_=0), "null photo": _row(photo=0), "null output": _row(out=0), "map size": _row(h=0), "smaller": _row(H=4),
        "smaller than": _row(W=6, pitch=3 * 17), "pitch": _row(pitch=3 * 17 - 1), "misaligned": _row(map_=A + 2), "misaligned output": _row(out=A + 2),
        "scratch": _row(off=4), "negative": _row(off=-8), "outside": _row(off=8),
    }
    for word, row in bad_rows.items():
        assert rc(_table([row])) == -1, word
        assert lib.mdpt_last_error(), word
    assert rc(_table([_row(H=4)])) == -1 and b"smaller" in lib.mdpt_last_error()
    assert rc(_table([_row(pitch=50)])) == -1 and b"pitch" in lib.mdpt_last_error()
    assert rc(_table([_row(), _row(off=per - 8)]), nbytes=4 * per) == -1 and b"overlap" in lib.mdpt_last_error()
