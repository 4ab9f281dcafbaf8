"""tools/mdpt_run_image.py --guided: the files it writes have each photo's shape and equal what the API returns for the same model and photos."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from muggled_dpt_amd import postprocess as pp

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_guided_flag_writes_a_map_of_each_photos_shape(tmp_path):
    from muggled_dpt_amd import make_depthanythingv2_dpt_from_original_state_dict as make
    from muggled_dpt_amd.synthetic import make_synthetic_original_state_dict
    rng = np.random.default_rng(7)
    photos = {"a": rng.integers(0, 256, (150, 130, 3), dtype=np.uint8), "b": rng.integers(0, 256, (113, 201, 3), dtype=np.uint8)}
    for k in photos:
        np.save(tmp_path / f"{k}.npy", photos[k])
    env = dict(os.environ, PYTHONPATH=REPO)
    cmd = [sys.executable, os.path.join(REPO, "tools", "mdpt_run_image.py"), "--synthetic", "tiny", "-s", "112", "-i", str(tmp_path / "a.npy"), "-i",
           str(tmp_path / "b.npy"), "--guided", "3", "1e-3"]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=tmp_path, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    model = make(make_synthetic_original_state_dict("tiny", 0))[1].to("cuda", torch.bfloat16)
    want = pp.guided_upsample_images(model.inference_images(list(photos.values()), 112, True, 32), list(photos.values()), 3, 1e-3)
    for k, name in enumerate(photos):
        got = np.load(tmp_path / f"{name}_guided.npy")
        assert got.dtype == np.float32 and got.shape == photos[name].shape[:2] and np.isfinite(got).all()
        assert np.array_equal(got.view(np.uint32), want[k][0].cpu().numpy().view(np.uint32))
