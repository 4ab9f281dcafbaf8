"""Depth-banded push-pull hole filling (postprocess.fill_holes / mdpt_post_fill_holes) restated in numpy from its definition (include/mdpt.h): one
array per pyramid level, the contributors of a node taken in the definition's order, every sum and the one division in fp64, astype(float32) where
the definition rounds. It is not a port of the kernels: it knows nothing of blocks, launches or LDS.

It also returns the per-pixel `safe` mask. A selection comparison d_k >= (1 - band) dmax is UNSAFE where |d_k - (1 - band) dmax| <= 1e-6 dmax: there
an evaluation that rounds differently may decide differently. With band == 0 the threshold IS dmax (1.0 x dmax is exact), so d_k == dmax - the
farthest contributor itself and its exact ties, which the definition names as what band = 0 keeps - is decided exactly and is not unsafe; a d_k
within 1e-6 of dmax without being equal is. A node is unsafe if a comparison of its own is, or if any valid contributor it looked at is unsafe
(push: children, pull: parents, kept or not - an unsafe contributor's depth could have moved the threshold); a pixel that was valid in the input is
copied and always safe."""
import functools

import numpy as np

WEIGHTS_PUSH = (1.0, 1.0, 1.0, 1.0)  # the mean of the kept children: sum / count
WEIGHTS_PULL = (9.0 / 16.0, 3.0 / 16.0, 3.0 / 16.0, 1.0 / 16.0)
NEAR = 1e-6


def level_sizes(h: int, w: int) -> list:
    sizes = [(h, w)]
    while sizes[-1] != (1, 1):
        sizes.append(((sizes[-1][0] + 1) // 2, (sizes[-1][1] + 1) // 2))
    return sizes


def _mix(vals, unsafe, weights, band: float):
    """vals: four contributors, each fp32 [h,w,4] = {three channels, depth} (depth 0 = invalid), in the definition's order; unsafe: their flags
    [h,w] -> (fp64 [h,w,4] = sum w_k v_k / sum w_k over the kept ones, any [h,w] = some contributor is valid, unsafe [h,w])"""
    d = [v[..., 3] for v in vals]
    valid = [x > 0 for x in d]
    dd = [x.astype(np.float64) for x in d]
    dmax = np.zeros(d[0].shape, dtype=np.float64)
    for k in range(4):
        dmax = np.maximum(dmax, np.where(valid[k], dd[k], 0.0))
    thr = (1.0 - band) * dmax
    acc = np.zeros(vals[0].shape, dtype=np.float64)
    sw = np.zeros(d[0].shape, dtype=np.float64)
    bad = np.zeros(d[0].shape, dtype=bool)
    for k in range(4):
        keep = valid[k] & (dd[k] >= thr)
        acc = acc + np.where(keep[..., None], weights[k] * vals[k].astype(np.float64), 0.0)
        sw = sw + np.where(keep, weights[k], 0.0)
        near = valid[k] & (np.abs(dd[k] - thr) <= NEAR * dmax)
        if band == 0.0:
            near &= dd[k] != thr
        bad |= near | (valid[k] & unsafe[k])
    some = dmax > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        out = acc / sw[..., None]
    return out, some, bad & some


def fill(color: np.ndarray, depth: np.ndarray, band: float) -> dict:
    """color uint8 [h,w,4] BGRA, depth fp32 [h,w] -> dict(color uint8 [h,w,4], depth fp32 [h,w], safe bool [h,w], levels = the pyramid's depth
    planes after the pull, for the tests of the restatement itself)"""
    color, depth = np.asarray(color), np.asarray(depth, dtype=np.float32)
    h, w = depth.shape
    sizes = level_sizes(h, w)
    top = len(sizes) - 1
    with np.errstate(invalid="ignore"):
        valid0 = (color[..., 3] != 0) & (depth > 0) & (depth < np.inf)
    node0 = np.zeros((h, w, 4), dtype=np.float32)
    node0[..., :3] = color[..., :3]
    node0[..., 3] = np.where(valid0, depth, 0)
    node0[~valid0] = 0
    nodes, unsafe = [node0], [np.zeros((h, w), dtype=bool)]
    # push
    for l in range(top):
        hl, wl = sizes[l]
        h1, w1 = sizes[l + 1]
        # a child that does not exist contributes nothing: pad with invalid nodes
        padded = np.zeros((2 * h1, 2 * w1, 4), dtype=np.float32)
        padded[:hl, :wl] = nodes[l]
        flags = np.zeros((2 * h1, 2 * w1), dtype=bool)
        flags[:hl, :wl] = unsafe[l]
        order = ((0, 0), (0, 1), (1, 0), (1, 1))
        out, some, bad = _mix([padded[dy::2, dx::2] for dy, dx in order], [flags[dy::2, dx::2] for dy, dx in order], WEIGHTS_PUSH, band)
        node = np.zeros((h1, w1, 4), dtype=np.float32)
        node[some] = out[some].astype(np.float32)
        nodes.append(node)
        unsafe.append(bad)
    # pull
    filled0 = None
    for l in range(top - 1, -1, -1):
        hl, wl = sizes[l]
        h1, w1 = sizes[l + 1]
        y, x = np.arange(hl), np.arange(wl)
        ya, xa = y >> 1, x >> 1
        yb = np.clip(ya + np.where(y & 1, 1, -1), 0, h1 - 1)
        xb = np.clip(xa + np.where(x & 1, 1, -1), 0, w1 - 1)
        pairs = ((ya, xa), (ya, xb), (yb, xa), (yb, xb))
        out, some, bad = _mix([nodes[l + 1][py[:, None], px[None, :]] for py, px in pairs], [unsafe[l + 1][py[:, None], px[None, :]] for py, px in pairs],
                              WEIGHTS_PULL, band)
        take = ~(nodes[l][..., 3] > 0) & some
        if l > 0:
            nodes[l][take] = out[take].astype(np.float32)
        else:
            filled0 = take
            nodes[0][..., :3][take] = np.clip(np.floor(out[..., :3] + 0.5), 0.0, 255.0)[take].astype(np.float32)
            nodes[0][..., 3][take] = out[..., 3][take].astype(np.float32)
        unsafe[l] = np.where(take, bad, unsafe[l])
    if filled0 is None:
        filled0 = np.zeros((h, w), dtype=bool)
    out_color = np.zeros((h, w, 4), dtype=np.uint8)
    out_depth = np.full((h, w), np.inf, dtype=np.float32)
    out_color[filled0, :3] = nodes[0][..., :3][filled0].astype(np.uint8)
    out_color[filled0, 3] = 255
    out_depth[filled0] = nodes[0][..., 3][filled0]
    out_color[valid0] = color[valid0]
    out_depth[valid0] = depth[valid0]
    return dict(color=out_color, depth=out_depth, safe=~unsafe[0] | valid0, valid=valid0, levels=[n[..., 3] for n in nodes])


# ---- the cases the GPU tests fill and the CPU test checks the safe-mask cap for

# (h, w): 1x1: no level above the image; 1x7, 5x3: odd sizes, clamped parents, a single row; 33x17: just over the one-workgroup levels; 70x45:
# ragged blocks; 130x67: a three-level push launch with edges that are no multiple of its block; 9x270: two push launches (the second of one level)
SIZES = ((1, 1), (1, 7), (5, 3), (33, 17), (70, 45), (130, 67), (9, 270))
# (family, band): "pow2": depths from {1, 2, 4, 8} per 4 x 4 patch - with band 0.25 every kept set has equal depths, so every depth mean is exact
# and every comparison sits 25 % from its threshold: nothing is unsafe by construction; "cont": depths uniform in [1, 10]
FAMILIES = (("pow2", 0.25), ("cont", 0.0), ("cont", 0.1), ("cont", 1.0))


@functools.lru_cache(maxsize=None)
def case(h: int, w: int, family: str, seed: int = 7):
    """-> (color uint8 [3,h,w,4], depth fp32 [3,h,w]): image 0 all empty, image 1 all covered, image 2 mixed: random rectangular holes of sides 1
    to about a third of the image's, the first touching the border; holes are background as render_mesh leaves it, except the first (alpha 0 over
    a finite depth and a colour) and the second (alpha 255 over depth +inf): the validity rule's two halves"""
    rng = np.random.default_rng(seed + 1000 * h + w)
    color = rng.integers(0, 256, size=(3, h, w, 4)).astype(np.uint8)
    color[..., 3] = 255
    if family == "pow2":
        patches = rng.integers(0, 4, size=(3, (h + 3) // 4, (w + 3) // 4))
        depth = (2.0 ** np.repeat(np.repeat(patches, 4, axis=1), 4, axis=2)[:, :h, :w]).astype(np.float32)
    else:
        depth = rng.uniform(1.0, 10.0, size=(3, h, w)).astype(np.float32)
    color[0] = 0
    depth[0] = np.inf
    for k in range(min(6, max(1, h * w // 6))):  # (fewer on the smallest images: something valid has to remain)
        hh, ww = int(rng.integers(1, max(2, h // 3 + 1))), int(rng.integers(1, max(2, w // 3 + 1)))
        y0, x0 = (0, int(rng.integers(0, w - ww + 1))) if k == 0 else (int(rng.integers(0, h - hh + 1)), int(rng.integers(0, w - ww + 1)))
        box = (2, slice(y0, y0 + hh), slice(x0, x0 + ww))
        if k == 0:
            color[box][..., 3] = 0
        elif k == 1:
            depth[box] = np.inf
        else:
            color[box] = 0
            depth[box] = np.inf
    if h * w == 1:  # (a hole would leave the mixed image empty: keep its one pixel)
        color[2], depth[2] = color[1], depth[1]
    color.setflags(write=False)
    depth.setflags(write=False)
    return color, depth


@functools.lru_cache(maxsize=None)
def reference(h: int, w: int, family: str, band: float) -> tuple:
    color, depth = case(h, w, family)
    return tuple(fill(color[i], depth[i], band) for i in range(3))
