"""Data-parallel path on CPU: world_size-2 gloo run of the sharding + all-gather logic that bench.py uses on RCCL."""
import os
import socket
import sys

import pytest
import torch
import torch.multiprocessing as mp

from muggled_dpt_amd.parallel import shard_bounds

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shard_bounds_cover_the_batch_contiguously():
    for gb, world in ((256, 8), (32, 1), (10, 4), (3, 4)):
        spans = [shard_bounds(gb, r, world) for r in range(world)]
        assert spans[0][0] == 0 and spans[-1][1] == gb
        assert all(spans[i][1] == spans[i + 1][0] for i in range(world - 1))
        sizes = [e - s for s, e in spans]
        assert max(sizes) - min(sizes) <= 1


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _fake_depth(images):  # stand-in for model.forward: per-image independent, like the real path
    return images.mean(dim=1) * 2.0 + 1.0


def _worker(rank, world, port, global_batch, ret):
    sys.path.insert(0, REPO)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    from muggled_dpt_amd.parallel import DataParallelDepth, all_gather_ragged, init_distributed, shard_bounds as sb

    r, w, _ = init_distributed("gloo")
    assert (r, w) == (rank, world)
    full = torch.randn(global_batch, 3, 8, 8, generator=torch.Generator().manual_seed(0))
    s, e = sb(global_batch, rank, world)
    dp = DataParallelDepth(_fake_depth, rank, world)
    if global_batch % world == 0:
        out = dp.forward_shard(full[s:e])
    else:
        out = all_gather_ragged(_fake_depth(full[s:e]), global_batch, rank, world)
    ok = torch.equal(out, _fake_depth(full))  # gathered result == single-process result, bit for bit
    t = torch.tensor([1.0 + rank])
    dist.all_reduce(t, op=dist.ReduceOp.MAX)  # the bench's max-over-ranks timing reduction
    ret[rank] = bool(ok) and float(t) == float(world)
    dist.destroy_process_group()


@pytest.mark.parametrize("global_batch", [8, 7])
def test_two_rank_gloo_allgather_matches_single_process(global_batch):
    world = 2
    with mp.Manager() as mgr:
        ret = mgr.dict()
        mp.spawn(_worker, args=(world, _free_port(), global_batch, ret), nprocs=world, join=True)
        assert dict(ret) == {0: True, 1: True}


def test_bench_control_flow_at_world_size_2_on_gloo():
    """bench.py's N-rank control flow (barrier, timed region, max-over-ranks all_reduce right behind it, rank-0-only JSON line with
    cpu_baseline null, no rank left parked in a collective) under torch.distributed.run with a stand-in model on CPU / gloo - the
    driver runs the real thing ONCE on 8 GPUs with no retry."""
    import json, os, socket, subprocess, sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join(repo, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--fake-model", "--full"],
                       capture_output=True, text=True, timeout=600, cwd=repo, env={**os.environ, "OMP_NUM_THREADS": "1"})
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip().startswith("{")]
    assert len(lines) == 1, r.stdout  # rank 0 only
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["n_ranks_seen"] == 2 and d["steps"] == 3 and d["warmup"] == 1
    assert d["cpu_baseline"] is None and d["roofline"] is None and "secondary" not in d
    assert d["config"]["global_batch"] == 4 and d["config"]["parallelism"] == "dp2" and d["gathered_shape"] == [4, 16, 16]
    assert abs(d["value"] - 2 * 2 * 3 / (d["ms_per_step"] * 3 / 1e3)) / d["value"] < 1e-3
    # the one-shot 8-GPU line validates itself: the gathered tensor against a local recomputation of the last rank's shard, and every
    # rank's own clock (value is quoted on the slowest)
    assert d["gather_bitwise_ok"] is True
    assert 0 < d["per_rank_maps_per_s"]["min"] <= d["per_rank_maps_per_s"]["max"]
    assert abs(d["per_rank_maps_per_s"]["min"] * 2 - d["value"]) / d["value"] < 1e-3


def test_plain_bench_at_world_size_2_dumps_the_gathered_last_step(tmp_path):
    """Without --full the N-rank run skips the gather self-check, and --dump-outputs writes what rank 0 received in the last timed step:
    the gathered global batch, the concatenation of every rank's maps of its own seeded images (seed 1 + rank)."""
    import json, subprocess
    import numpy as np
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", str(_free_port()), os.path.join(REPO, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
                        "--fake-model", "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=600, cwd=REPO, env={**os.environ, "OMP_NUM_THREADS": "1"})
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip().startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["steps"] == 2 and d["gather_bitwise_ok"] is None and d["cpu_baseline"] is None and d["roofline"] is None
    y = np.load(tmp_path / "depth.npy")
    want = torch.cat([torch.randn(2, 3, 16, 16, generator=torch.Generator().manual_seed(1 + rank)).mean(dim=1) for rank in range(2)])
    assert y.dtype == np.float32 and np.array_equal(y, want.numpy())
