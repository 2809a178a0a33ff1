"""bench.py's plain run and `--dump-outputs`: the plain line carries the headline
fields alone (everything else sits behind `--full`), `--steps` is the number of
timed steps, and the dumped arrays are float32, within the 64 MB budget and the
same frames from run to run."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def fake_run(bufs, kind="C2", rank=0, world=1):
    import torch
    run = types.SimpleNamespace(torch=torch, kind=kind, rank=rank, world=world)
    if kind == "C4":
        run.out = bufs[0]
    else:
        run.outs = bufs
    return run


def test_parse_defaults_are_the_plain_run():
    import bench
    args = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert args.full is False and args.dump_outputs is None
    assert (args.steps, args.warmup, args.workload) == (7, 2, "C2")
    assert bench.parse(["--full", "--dump-outputs", "d"]).full is True
    with pytest.raises(SystemExit):
        bench.parse(["--steps", "0"])


def test_dump_small_buffers_whole(tmp_path):
    import bench
    import torch
    g = torch.Generator().manual_seed(3)
    bufs = [torch.rand((1001, 2), generator=g), torch.rand((17, 2), generator=g)]
    written = bench.dump_outputs(fake_run(bufs), str(tmp_path / "d"))
    assert sorted(written) == ["out0", "out1"]
    for t, b in enumerate(bufs):
        a = np.load(tmp_path / "d" / f"out{t}.npy")
        assert a.dtype == np.float32 and np.array_equal(a, b.numpy())
        assert written[f"out{t}"] == {"frames": b.shape[0], "of": b.shape[0]}


def test_dump_samples_large_buffers_the_same_way_every_time(tmp_path, monkeypatch):
    import bench
    import torch
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 2 * 800)  # two buffers: 100 stereo f32 frames each
    big = torch.arange(2 * 5003, dtype=torch.float32).reshape(5003, 2)  # row r holds (2r, 2r + 1)
    small = torch.ones((100, 2))
    for d in ("a", "b"):
        written = bench.dump_outputs(fake_run([big, small]), str(tmp_path / d))
    a, b = np.load(tmp_path / "a" / "out0.npy"), np.load(tmp_path / "b" / "out0.npy")
    assert a.dtype == np.float32 and a.shape == (100, 2) and np.array_equal(a, b)
    assert written["out0"] == {"frames": 100, "of": 5003}
    rows = a[:, 0] / 2
    assert np.array_equal(a[:, 1], a[:, 0] + 1) and np.all(np.diff(rows) >= 0)  # whole frames, ascending
    assert rows.min() >= 0 and rows.max() < 5003 and len(np.unique(rows)) > 90  # spread over the buffer
    assert np.array_equal(np.load(tmp_path / "a" / "out1.npy"), small.numpy())  # within its share: whole
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 2 * 800 + 2 * 128  # the budget plus the .npy headers


def test_dump_names_carry_the_rank_when_there_are_several(tmp_path):
    import bench
    import torch
    written = bench.dump_outputs(fake_run([torch.zeros((5, 2))], kind="C4", rank=1, world=2), str(tmp_path))
    assert list(written) == ["rank1_out0"] and os.path.exists(tmp_path / "rank1_out0.npy")


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_its_outputs(tmp_path):
    """One plain run of the smallest workload (C1: a 30 s track): the line, the
    step count and the dump."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--workload", "C1", "--dump-outputs", str(tmp_path / "out")],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    (line,) = [json.loads(s) for s in p.stdout.splitlines() if s.strip()]
    assert all(k in line for k in HEADLINE)
    assert line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1
    frames = 30 * 44100
    assert line["value"] == pytest.approx(frames / (line["ms_per_step"] / 1e3), rel=1e-9)
    assert line["higher_is_better"] is True and line["unit"] == "stereo frames/s" and line["dtype"] == "f64"
    for moved in ("cpu_baseline", "chain"):  # behind --full
        assert moved not in line
    assert "dominant_kernel" not in line["roofline"]
    assert os.listdir(tmp_path / "out") == ["out0.npy"]
    a = np.load(tmp_path / "out" / "out0.npy")
    assert a.dtype == np.float32 and a.shape == (frames, 2) and line["dumped_outputs"]["out0"]["of"] == frames
    assert np.all(np.isfinite(a)) and 0.01 < np.abs(a).max() <= 1.0
