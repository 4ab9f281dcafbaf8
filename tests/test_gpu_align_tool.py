"""tools/mdpt_run_image.py --truth: the files it writes equal what the API returns for the same model, photos and measurements."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from muggled_dpt_amd import postprocess as pp

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_truth_flags_write_the_apis_results(tmp_path):
    from muggled_dpt_amd import make_depthanythingv2_dpt_from_original_state_dict as make
    from muggled_dpt_amd.synthetic import make_synthetic_original_state_dict
    rng = np.random.default_rng(5)
    photos = {"a": rng.integers(0, 256, (90, 130, 3), dtype=np.uint8), "b": rng.integers(0, 256, (64, 64, 3), dtype=np.uint8)}
    truths = {"a": rng.uniform(0.5, 6.0, (45, 70)).astype(np.float32), "b": rng.uniform(0.5, 6.0, (100, 80)).astype(np.float32)}
    truths["a"][rng.uniform(0, 1, (45, 70)) < 0.2] = 0.0
    truths["b"][rng.uniform(0, 1, (100, 80)) < 0.2] = np.nan
    os.makedirs(tmp_path / "lidar")
    for k in photos:
        np.save(tmp_path / f"{k}.npy", photos[k])
        np.save(tmp_path / "lidar" / f"{k}.npy", truths[k])
    env = dict(os.environ, PYTHONPATH=REPO)
    cmd = [sys.executable, os.path.join(REPO, "tools", "mdpt_run_image.py"), "--synthetic", "tiny", "-s", "112", "-i", str(tmp_path / "a.npy"), "-i",
           str(tmp_path / "b.npy"), "--truth", str(tmp_path / "lidar"), "--truth_method", "median", "--truth_range", "0.7", "5.5"]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=tmp_path, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    model = make(make_synthetic_original_state_dict("tiny", 0))[1].to("cuda", torch.bfloat16)
    preds = model.inference_images(list(photos.values()), 112, True, 32)
    fit = pp.fit_true_depth(preds, list(truths.values()), None, "inverse", "median", (0.7, 5.5))
    metrics = pp.depth_metrics(preds, list(truths.values()), fit, None, "inverse", (0.7, 5.5)).cpu().numpy()
    maps = pp.true_depth(preds, fit, [t.shape for t in truths.values()])
    for k, name in enumerate(photos):
        got = np.load(tmp_path / f"{name}_true.npy")
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), maps[k][0].cpu().numpy().view(np.uint32))
        rep = json.load(open(tmp_path / f"{name}_metrics.json"))
        assert rep["A"] == fit[k, 0].item() and rep["B"] == fit[k, 1].item() and rep["method"] == "median" and rep["space"] == "inverse"
        for c, key in enumerate(pp.DEPTH_METRIC_NAMES):
            assert rep[key] == metrics[k, c] or (np.isnan(rep[key]) and np.isnan(metrics[k, c])), key
        assert 0 < rep["n"] < truths[name].size
