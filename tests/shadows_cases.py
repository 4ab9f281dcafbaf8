"""The scenes of tests/test_gpu_shadows.py and their restatement (tests/shadows_restate.py), computed once and shared read-only; tests/test_shadows_cpu.py
asserts on the CPU that every non-degenerate scene has nodes in shadow, lit nodes and occluded nodes, so that an all-lit scene cannot hide a broken march.

Shapes, the smallest at which the kernels can still go wrong: a 3 x 4 grid under a 5 x 7 photo (smaller than one tile); a 40 x 33 grid under a 33 x 65 photo
(2 x 2 grid tiles, marches that cross tile borders and use the whole halo) at reach 1, 5 and 32; a 33 x 40 grid given as grid_hw over a 9 x 12 map (the resized
grid); a 12 x 16 map under a 9 x 6 photo (a map larger than its photo); a 5 x 7 grid (odd both ways: the centre node has x0 = y0 = 0, so a light along the view
axis has gx = gy = 0 there)."""
import functools

import numpy as np
import torch

from tests import normals_restate as nr
from tests import shadows_restate as sr

TORCH = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16}
# towards the upper left; facing away (behind the surface); along the view axis (gx = gy = 0 where x0 = y0 = 0); grazing (Lz = 0); a low light from the right
UPPER_LEFT, AWAY, AXIS, GRAZING, LOW_RIGHT = (-1.0, 1.0, 1.0), (0.3, -0.2, -0.5), (0.0, 0.0, 1.0), (1.0, 0.5, 0.0), (1.0, -0.3, 0.35)
SHADING = dict(ambient=0.3, diffuse=0.8, specular=0.6, shininess_log2=3)

# map h x w, grid_hw, photo H x W, map dtype, what the map holds, lights, keywords of shade_images, degenerate (too small / flat for the coverage condition)
CASES = [
    dict(hw=(3, 4), grid=None, HW=(5, 7), dtype="float32", holds="plain", lights=[UPPER_LEFT], kw=dict(), degenerate=True),
    dict(hw=(40, 33), grid=None, HW=(33, 65), dtype="float32", holds="plain", lights=[UPPER_LEFT, AWAY, LOW_RIGHT], kw=dict(shadow_reach=1, ao_reach=1, ao_radius=0.6)),
    dict(hw=(40, 33), grid=None, HW=(33, 65), dtype="float16", holds="plain", lights=[UPPER_LEFT, AXIS, GRAZING], kw=dict(shadow_reach=5, ao_reach=8, ao_radius=0.6)),
    dict(hw=(40, 33), grid=None, HW=(33, 65), dtype="float32", holds="plain", lights=[UPPER_LEFT, AWAY, LOW_RIGHT],
         kw=dict(shadow_reach=32, ao_reach=32, ao_radius=0.8, shadow_thickness=0.3, **SHADING)),
    dict(hw=(9, 12), grid=(33, 40), HW=(33, 65), dtype="bfloat16", holds="plain", lights=[LOW_RIGHT], kw=dict(ao_radius=0.6, step=3)),
    dict(hw=(12, 16), grid=None, HW=(9, 6), dtype="float32", holds="plain", lights=[UPPER_LEFT, GRAZING, AXIS], kw=dict(ao_radius=0.6, min_depth=2.0, max_depth=9.0)),
    dict(hw=(40, 33), grid=None, HW=(33, 65), dtype="float32", holds="holes", lights=[UPPER_LEFT, LOW_RIGHT, AWAY],
         kw=dict(space="depth", ao_radius=0.6, shadow_thickness=0.5, edge_ratio=1.0, fov_deg=70.0)),
    dict(hw=(40, 33), grid=None, HW=(40, 33), dtype="bfloat16", holds="holes", lights=[UPPER_LEFT], kw=dict(ao_radius=0.6, edge_ratio=float("inf"), step=1)),
    dict(hw=(9, 12), grid=(33, 40), HW=(33, 65), dtype="float32", holds="flat", lights=[UPPER_LEFT, GRAZING, AXIS], kw=dict(), degenerate=True),
    dict(hw=(9, 12), grid=(5, 7), HW=(33, 65), dtype="float32", holds="plain", lights=[AXIS, UPPER_LEFT], kw=dict(space="depth"), degenerate=True),
]


def make_case(index: int):
    """-> (map fp32 holding values of the case's dtype, photo uint8), seeded by the index. A far background with a slight tilt and noise, and near blocks
    before it (inverse space: larger values; depth space: smaller depths) that cast shadows on it and on each other. "holes": NaN and +inf and, in depth
    space, zeros and negatives."""
    c = CASES[index]
    (h, w), (H, W) = c["hw"], c["HW"]
    rng = np.random.default_rng(900 + index)
    yy, xx = np.mgrid[0:h, 0:w]
    u, v = (xx + 0.5) / w, (yy + 0.5) / h
    blocks = ((u > 0.25) & (u < 0.5) & (v > 0.2) & (v < 0.55)) * 1.0 + ((u > 0.6) & (u < 0.85) & (v > 0.45) & (v < 0.9)) * 0.45 + ((u - 0.75) ** 2 + (v - 0.2) ** 2 < 0.01) * 0.7
    near = 0.1 + 0.1 * u + 0.05 * v + 0.01 * rng.standard_normal((h, w)) + blocks  # larger = nearer
    p = 10.0 - 4.0 * near if c["kw"].get("space") == "depth" else 2.0 + near
    if c["holds"] == "flat":
        p = np.full((h, w), 3.25)
    p = p.astype(np.float32)
    if c["holds"] == "holes":
        flat = p.reshape(-1)
        picks = rng.choice(p.size, 10, replace=False)
        flat[picks[:3]] = (np.nan, np.inf, np.nan)
        if c["kw"].get("space") == "depth":
            flat[picks[3:7]] = (0.0, -2.5, np.nan, 0.0)
    p = torch.from_numpy(p).to(TORCH[c["dtype"]]).to(torch.float32).numpy()
    return p, rng.integers(0, 256, (H, W, 3), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def restated(index: int):
    """the restatement of CASES[index], computed once and shared (read only) -> (map, photo, frames, ao, vis, valid nodes)"""
    c = CASES[index]
    p, photo = make_case(index)
    frames, ao, vis = sr.shade_images(p, photo, c["lights"], grid_hw=c["grid"], **c["kw"])
    camera = {k: v for k, v in c["kw"].items() if k in ("space", "fov_deg", "min_depth", "max_depth", "edge_ratio")}
    valid = sr.occlusion(p, photo.shape[0], photo.shape[1], None, c["grid"], **camera)[2]
    out = (p, photo, frames, ao, vis, valid)
    for a in out:
        a.setflags(write=False)
    return out


def coverage(index: int):
    """-> (per light the share of valid nodes in shadow - the others are lit -, the share with ao < 1)"""
    _, _, _, ao, vis, valid = restated(index)
    return [float((vis[v][valid] == 0.0).mean()) for v in range(vis.shape[0])], float((ao[valid] < 1.0).mean())


__all__ = ["CASES", "SHADING", "TORCH", "make_case", "restated", "coverage", "nr", "sr"]
