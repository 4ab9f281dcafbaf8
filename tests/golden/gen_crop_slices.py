#!/usr/bin/env python3
"""Fixtures of the crop rule, written to tests/golden/crop_slices.json.

Runs the reference's own make_crop_slices_from_xy1xy2_norm (demo_helpers/crop_ui.py) on about 200 (image shape, normalised box, minimum) cases and
records inputs and results only. The module imports its UI toolkit (and through it cv2) at the top: both are stubbed in memory, the function
itself needs numpy alone. Cases: shapes from 1x1 to 4032x3024, corners whose pixel product ends in .5 (np.round rounds half to even), reversed
corners, coordinates below 0 and above 1, and sides of 4, 5 and 6 px around the default minimum of 5.

usage: PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_crop_slices.py --reference PATH_TO_THE_REFERENCE_CHECKOUT
"""
from __future__ import annotations

import argparse
import importlib.util
import json
import os
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.dont_write_bytecode = True

SHAPES = [(1, 1), (3, 7), (5, 5), (6, 4), (10, 10), (61, 90), (217, 333), (333, 217), (480, 640), (720, 1280), (1080, 1920), (3024, 4032), (4032, 3024)]


def load_rule(reference: str):
    """the reference's function, from its file, with the UI imports of the module replaced by empty stand-ins"""
    class _Anything(types.ModuleType):
        def __getattr__(self, name):
            return type(name, (), {})

    pkg = types.ModuleType("demo_helpers")
    pkg.__path__ = []
    sys.modules["demo_helpers"] = pkg
    sys.modules["demo_helpers.toadui"] = _Anything("demo_helpers.toadui")
    sys.modules.setdefault("cv2", _Anything("cv2"))
    path = os.path.join(reference, "muggled_dpt", "demo_helpers", "crop_ui.py")
    if not os.path.exists(path):
        path = os.path.join(reference, "demo_helpers", "crop_ui.py")
    spec = importlib.util.spec_from_file_location("demo_helpers.crop_ui", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.make_crop_slices_from_xy1xy2_norm


def cases():
    rng = np.random.default_rng(2024)
    out = []
    for h, w in SHAPES:
        shape = [h, w, 3]
        out.append((shape, [[0.0, 0.0], [1.0, 1.0]], [5, 5]))
        out.append((shape, [[0.25, 0.1], [0.75, 0.9]], [5, 5]))
        # pixel products that end in .5: (k + 0.5) / side, rounded half to even
        for k in (0, 1, 2, 3):
            out.append((shape, [[(k + 0.5) / w, (k + 0.5) / h], [min(1.0, (k + 10.5) / w), min(1.0, (k + 11.5) / h)]], [5, 5]))
        # reversed corners, and coordinates outside 0..1 (clipped)
        out.append((shape, [[0.8, 0.9], [0.2, 0.1]], [5, 5]))
        out.append((shape, [[0.8, 0.1], [0.2, 0.9]], [5, 5]))
        out.append((shape, [[-0.3, -0.01], [1.2, 1.001]], [5, 5]))
        out.append((shape, [[-2.0, 0.5], [0.5, 3.0]], [5, 5]))
        # sides of 4, 5 and 6 px around the minimum, at an offset, in x, in y and in both
        for side in (4, 5, 6):
            x1, y1 = min(2, max(w - side, 0)), min(3, max(h - side, 0))
            out.append((shape, [[x1 / w, 0.0], [(x1 + side) / w, 1.0]], [5, 5]))
            out.append((shape, [[0.0, y1 / h], [1.0, (y1 + side) / h]], [5, 5]))
            out.append((shape, [[x1 / w, y1 / h], [(x1 + side) / w, (y1 + side) / h]], [5, 5]))
        # another minimum, and random boxes
        out.append((shape, [[0.1, 0.1], [0.12, 0.9]], [1, 1]))
        out.append((shape, [[0.1, 0.1], [0.6, 0.6]], [20, 40]))
        for _ in range(2):
            c = rng.uniform(-0.1, 1.1, 4)
            out.append((shape, [[float(c[0]), float(c[1])], [float(c[2]), float(c[3])]], [5, 5]))
    # 2-element shapes are accepted too (image_shape[0:2])
    out.append(([480, 640], [[0.1, 0.2], [0.3, 0.4]], [5, 5]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "crop_slices.json"))
    args = ap.parse_args()
    rule = load_rule(args.reference)
    records = []
    for shape, norm, minimum in cases():
        ys, xs = rule(tuple(shape), tuple(tuple(c) for c in norm), tuple(minimum))
        records.append({"shape": shape, "crop_xy1xy2_norm": norm, "minimum_crop_xy": minimum, "y": [ys.start, ys.stop], "x": [xs.start, xs.stop]})
    with open(args.out, "w") as fh:
        json.dump({"source": "demo_helpers/crop_ui.py: make_crop_slices_from_xy1xy2_norm", "cases": records}, fh, indent=0)
        fh.write("\n")
    print(f"wrote {len(records)} cases to {args.out}")


if __name__ == "__main__":
    main()
