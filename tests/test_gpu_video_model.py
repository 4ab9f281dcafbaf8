"""DPTModel.inference_video and tools/mdpt_run_image.py --stable on a tiny synthetic model: inference_video is inference_batch in chunks followed by
video.stabilize_video per chunk, bit for bit, whatever the chunk size; the tool writes those values."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from muggled_dpt_amd import mesh_io, video

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model():
    from muggled_dpt_amd import make_depthanythingv2_dpt_from_original_state_dict as make
    from muggled_dpt_amd.synthetic import make_synthetic_original_state_dict
    return make(make_synthetic_original_state_dict("tiny", 0))[1].to("cuda", torch.bfloat16)


def _frames(n=7, hw=(90, 120)):
    """a clip: one random photo under a brightness ramp that moves a little from frame to frame"""
    rng = np.random.default_rng(11)
    photo = rng.integers(0, 200, (*hw, 3)).astype(np.float64)
    ramp = np.linspace(0.0, 1.0, hw[1])[None, :, None]
    return [np.clip(photo + 40.0 * np.roll(ramp, 3 * t, axis=1) + rng.normal(0.0, 2.0, photo.shape), 0, 255).astype(np.uint8) for t in range(n)]


def test_inference_video_is_inference_batch_then_stabilize_video():
    model, frames = _model(), _frames()
    stable, table, state = model.inference_video(frames, batch_size=3, max_side_length=112)
    assert stable.dtype == torch.float32 and tuple(stable.shape) == (7, 112, 112) and tuple(table.shape) == (7, 4) and table.dtype == torch.float64
    st, want_s, want_t = None, [], []
    for at in (0, 3, 6):
        s, t, st = video.stabilize_video(model.inference_batch(frames[at:at + 3], 112), st)
        want_s.append(s)
        want_t.append(t)
    assert torch.equal(stable, torch.cat(want_s)) and torch.equal(table, torch.cat(want_t))
    assert all(torch.equal(getattr(state, k), getattr(st, k)) for k in ("raw", "out", "ab", "display_range", "started"))
    whole = model.inference_video(frames, batch_size=8, max_side_length=112)
    assert torch.equal(whole[0], stable) and torch.equal(whole[1], table) and torch.equal(whole[2].ab, state.ab)
    assert table[0].tolist() == [1.0, 0.0, 0.0, 1.0] and torch.isfinite(stable).all()
    # a second call goes on from the state; keywords reach stabilize_video
    more = model.inference_video(frames[:2], state, max_side_length=112, alpha=1.0)
    assert torch.equal(more[1], video.video_fit(model.inference_batch(frames[:2], 112), state))
    with pytest.raises(ValueError, match="batch_size"):
        model.inference_video(frames, batch_size=0)
    with pytest.raises(ValueError, match="no frames"):
        model.inference_video([])


def test_stable_flag_writes_the_clip(tmp_path):
    frames = _frames(4)
    cmd = [sys.executable, os.path.join(REPO, "tools", "mdpt_run_image.py"), "--synthetic", "tiny", "-s", "112", "-b", "3", "--stable", "0.5", "-o", str(tmp_path / "out")]
    for k, f in enumerate(frames):
        np.save(tmp_path / f"f{k}.npy", f)
        cmd += ["-i", str(tmp_path / f"f{k}.npy")]
    r = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=REPO), cwd=tmp_path, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    stable, table, _ = _model().inference_video(frames, batch_size=3, max_side_length=112, alpha=0.5)
    shown, _ = video.video_display(stable, table, None, (120, 90))
    for k in range(4):
        got = np.load(tmp_path / "out" / f"f{k}_stable.npy")
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), stable[k].cpu().numpy().view(np.uint32))
        with open(tmp_path / "out" / f"f{k}_stable.png", "rb") as fh:
            assert fh.read() == mesh_io.encode_png(shown[k].cpu().numpy())
