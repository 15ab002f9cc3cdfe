"""Host side of the pipelined self-play (no GPU): the split is checked before anything is
allocated, and bench.py pipelines every workload by default (measured gains); configs[2] keeps
its batch of 1,024 leaves per evaluation (1,024 games per pipeline)."""
import sys

import pytest

import bench


def test_pipelines_must_divide_the_games():
    from engine import PipelinedSelfPlay

    with pytest.raises(ValueError):
        PipelinedSelfPlay(None, {"num_simulations": 8}, 1023, pipelines=2)
    with pytest.raises(ValueError):
        PipelinedSelfPlay(None, {"num_simulations": 8}, 64, pipelines=0)


@pytest.mark.parametrize("argv,want", [([], 2), (["--workload", "c4"], 2),
                                       (["--workload", "c2"], 2), (["--workload", "c5"], 2),
                                       (["--pipelines", "2"], 2),
                                       (["--workload", "c5", "--games", "1023"], 1)])
def test_bench_pipeline_defaults(monkeypatch, argv, want):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    assert bench.parse().pipelines == want


@pytest.mark.parametrize("argv,games,pipes", [([], 2048, 2), (["--pipelines", "1"], 1024, 1),
                                              (["--pipelines", "4"], 4096, 4),
                                              (["--games", "1024"], 1024, 2)])
def test_bench_configs2_leaf_batch(monkeypatch, argv, games, pipes):
    """configs[2] ("batched leaf eval = 1024"): by default 1,024 games per pipeline."""
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    a = bench.parse()
    assert (a.games, a.pipelines) == (games, pipes)


def test_bench_window_protocol_defaults(monkeypatch):
    """The driver's command (--steps 20 --warmup 5) gets the sustained block and the settle
    windows between the warmup and the timed window."""
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "20", "--warmup", "5"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.settle, a.sustained_steps) == (20, 5, 3, 2000)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--settle", "0", "--sustained-steps", "0"])
    a = bench.parse()
    assert (a.settle, a.sustained_steps) == (0, 0)


@pytest.mark.parametrize("argv,skip_cpu,skip_kernel", [
    (["--gpus", "1", "--steps", "20", "--warmup", "5"], True, True),
    (["--skip-cpu"], True, True),
    (["--full"], False, False),
    (["--full", "--skip-cpu"], True, False),
    (["--full", "--skip-kernel"], False, True)])
def test_bench_plain_run_measures_the_headline_only(monkeypatch, argv, skip_cpu, skip_kernel):
    """The rooflines and the CPU baseline run under --full only; --skip-cpu / --skip-kernel
    take one of them out of a --full run."""
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    a = bench.parse()
    assert (a.skip_cpu, a.skip_kernel) == (skip_cpu, skip_kernel)
    assert a.dump_outputs is None


def test_bench_dump_arrays(monkeypatch, tmp_path):
    """--dump-outputs: float32 / float64 .npy files; above the byte limit the large arrays keep
    the same seeded row sample in every call, in row order, and the small ones stay whole."""
    import numpy as np

    monkeypatch.setattr(sys, "argv", ["bench.py", "--dump-outputs", str(tmp_path / "a")])
    assert bench.parse().dump_outputs == str(tmp_path / "a")
    assert bench.DUMP_MAX_BYTES == 64 << 20
    rng = np.random.default_rng(3)
    arrays = {"pi": rng.random((1000, 65)).astype(np.float32), "z": rng.random(1000),
              "slot": np.arange(1000, dtype=np.int32), "visits": rng.integers(0, 9, (7, 65)),
              "empty": np.zeros((0, 64), np.int8)}
    whole = bench.dump_arrays(str(tmp_path / "a"), arrays)
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == sorted(k + ".npy" for k in arrays)
    for k, v in arrays.items():
        got = np.load(tmp_path / "a" / (k + ".npy"))
        assert got.dtype == (np.float64 if v.dtype == np.float64 else np.float32)
        assert got.shape == v.shape and np.array_equal(got, v) and np.array_equal(got, whole[k])
    # a limit the 260,000-byte "pi" does not fit in (arrays of 1 MiB and more are sampled)
    big = {"pi": rng.random((20000, 65)).astype(np.float32), "z": arrays["z"]}
    limit = 2 << 20
    for d in ("b", "c"):
        bench.dump_arrays(str(tmp_path / d), big, max_bytes=limit)
    pi_b, pi_c = np.load(tmp_path / "b" / "pi.npy"), np.load(tmp_path / "c" / "pi.npy")
    assert np.array_equal(pi_b, pi_c) and np.array_equal(np.load(tmp_path / "b" / "z.npy"), big["z"])
    assert pi_b.nbytes + big["z"].nbytes <= limit and len(pi_b) > 0.9 * (limit - 8000) / 260
    # the kept rows are rows of the input, in its order
    keys = {r.tobytes(): i for i, r in enumerate(big["pi"])}
    idx = [keys[r.tobytes()] for r in pi_b]
    assert idx == sorted(idx) and len(set(idx)) == len(idx)
