"""tools/mdpt_run_image.py --render: a swing of PNGs from one image with synthetic weights, through the whole chain (a process of its own: the
tool is what the test is about)."""
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _decode_png(data: bytes) -> np.ndarray:
    """the writer's own subset: 8-bit RGBA, filter 0 on every row, one IDAT"""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    w, h, depth, kind = struct.unpack(">IIBB", data[16:26])
    assert (depth, kind) == (8, 6)
    at, idat = 8, b""
    while at < len(data):
        n, tag = struct.unpack(">I", data[at:at + 4])[0], data[at + 4:at + 8]
        if tag == b"IDAT":
            idat += data[at + 8:at + 8 + n]
        at += 12 + n
    rows = np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(h, 1 + 4 * w)
    assert (rows[:, 0] == 0).all()
    return rows[:, 1:].reshape(h, w, 4)


def test_render_writes_a_swing_of_pngs(tmp_path):
    img = np.random.default_rng(2).integers(0, 256, (90, 120, 3), dtype=np.uint8)
    np.save(tmp_path / "photo.npy", img)
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "mdpt_run_image.py"), "--synthetic", "tiny", "-i", str(tmp_path / "photo.npy"), "-s", "112",
                        "--render", str(tmp_path / "out"), "--render_views", "3", "--render_swing", "10", "5", "--render_wh", "96", "54", "--mesh_faces", "2000"],
                       capture_output=True, text=True, cwd=REPO, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    names = sorted(os.listdir(tmp_path / "out"))
    assert names == ["photo_view000.png", "photo_view001.png", "photo_view002.png"]
    views = [_decode_png((tmp_path / "out" / n).read_bytes()) for n in names]
    assert all(v.shape == (54, 96, 4) for v in views)
    assert all(set(np.unique(v[..., 3])) <= {0, 255} and (v[..., 3] == 255).mean() > 0.2 for v in views)
    assert all((v[v[..., 3] == 0] == 0).all() for v in views) and not np.array_equal(views[0], views[1])
