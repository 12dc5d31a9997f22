"""CPU: bench.py's command line and its --dump-outputs writer (the step itself runs on the GPU: test_gpu_multirank.py)."""
import os

import numpy as np
import pytest
import torch

import bench


def test_steps_and_warmup_are_validated():
    args = bench.parse_args(["--steps", "7", "--warmup", "0"])
    assert args.steps == 7 and args.warmup == 0 and args.dump_outputs is None
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse_args(["--warmup", "-1"])
    assert bench.parse_args(["--dump-outputs", "out"]).dump_outputs == "out"


def test_full_is_off_by_default():
    assert bench.parse_args(["--gpus", "1", "--steps", "3", "--warmup", "1"]).full is False
    assert bench.parse_args(["--full"]).full is True


def test_dump_writes_what_the_step_returns(tmp_path):
    gen = torch.Generator().manual_seed(0)
    pairs = torch.randint(0, 1000, (2, 500), generator=gen, dtype=torch.int64)
    scores = torch.rand(500, generator=gen).sort(descending=True).values
    info = bench.dump_outputs(str(tmp_path / "d"), pairs, scores, n_nodes=1000)
    p, s = np.load(tmp_path / "d" / "pairs.npy"), np.load(tmp_path / "d" / "scores.npy")
    assert p.dtype == np.float32 and s.dtype == np.float32
    assert np.array_equal(p, pairs.numpy().astype(np.float32)) and np.array_equal(s, scores.numpy())
    assert info["sampled_rows"] is None and info["rows"] == 500
    # ids of a graph above 2^24 nodes are not exact in float32
    big = pairs + (1 << 24)
    bench.dump_outputs(str(tmp_path / "w"), big, scores, n_nodes=(1 << 24) + 1000)
    pw = np.load(tmp_path / "w" / "pairs.npy")
    assert pw.dtype == np.float64 and np.array_equal(pw, big.numpy().astype(np.float64))


def test_dump_of_a_large_output_is_a_fixed_sample_under_the_cap(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 2 * 4096 + 12 * 100)     # room for 100 rows of 12 bytes
    pairs = torch.arange(2 * 1000, dtype=torch.int64).reshape(2, 1000)
    scores = torch.arange(1000, 0, -1, dtype=torch.float32)
    runs = []
    for name in ("a", "b"):
        info = bench.dump_outputs(str(tmp_path / name), pairs, scores, n_nodes=5000)
        assert info["sampled_rows"] == 100
        files = [tmp_path / name / f for f in ("pairs.npy", "scores.npy")]
        assert sum(os.path.getsize(f) for f in files) <= bench.DUMP_MAX_BYTES
        runs.append([np.load(f) for f in files])
    (p, s), (p2, s2) = runs
    assert np.array_equal(p, p2) and np.array_equal(s, s2)                # the same rows every time
    assert p.shape == (2, 100) and s.shape == (100,)
    idx = p[0].astype(np.int64)                                           # row j of pairs holds (j; 1000 + j), scores 1000 - j
    assert (np.diff(idx) > 0).all()
    assert np.array_equal(p[1], idx + 1000) and np.array_equal(s, 1000 - idx)
