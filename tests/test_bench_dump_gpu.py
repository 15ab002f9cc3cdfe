"""bench.py --dump-outputs on the device: a short run of the benchmark's own main() (configs[2]'s
two pipelines and net at 8 simulations per move, 128 games) writes what the timed window's last
step left -- float32 / float64 arrays consistent with each other and with the result line --
and a second run with the same arguments writes the same bytes (fixed seeds: the inputs are
identical from run to run)."""
import json
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

nat = pytest.importorskip("az_native")
import bench  # noqa: E402

STEPS, GAMES, SIMS = 48, 128, 8
ARGV = ["bench.py", "--gpus", "1", "--steps", str(STEPS), "--warmup", "0", "--sims", str(SIMS),
        "--games", str(GAMES), "--settle", "0", "--sustained-steps", "0"]
NAMES = ("leaf_planes", "priors", "values", "root_visits", "root_value", "sample_state",
         "sample_pi", "sample_z", "sample_player", "sample_slot", "counters")


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    out = []
    for tag in ("a", "b"):
        d = tmp_path_factory.mktemp("dump_" + tag)
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(sys, "argv", ARGV + ["--dump-outputs", str(d)])
            import contextlib
            import io

            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                bench.main()
        line = json.loads(buf.getvalue().strip().splitlines()[-1])
        out.append((line, {n: np.load(d / (n + ".npy")) for n in NAMES},
                    sorted(p.name for p in d.iterdir())))
    return out


def test_dump_holds_the_last_steps_outputs(runs):
    line, arr, files = runs[0]
    assert files == sorted(n + ".npy" for n in NAMES)
    assert line["steps"] == STEPS and line["ms_per_step"] > 0
    # a plain run: the headline only
    assert not {"roofline", "roofline_conv", "roofline_trunk", "cpu_baseline"} & set(line)
    for n, v in arr.items():
        assert v.dtype == (np.float64 if n in ("root_value", "sample_z", "counters")
                           else np.float32), n
        assert np.isfinite(v).all(), n
    assert sum(v.nbytes for v in arr.values()) <= bench.DUMP_MAX_BYTES
    assert arr["leaf_planes"].shape == (GAMES, 64) and arr["priors"].shape == (GAMES, 65)
    assert arr["values"].shape == (GAMES,) and arr["root_visits"].shape == (GAMES, 65)
    # the net's outputs for the packed leaves: a softmax and a tanh; planes in {-1, 0, 1}
    assert np.abs(arr["priors"].sum(1) - 1.0).max() < 1e-5 and (np.abs(arr["values"]) <= 1).all()
    assert np.isin(arr["leaf_planes"], (-1.0, 0.0, 1.0)).all()
    # the slots are searching: visit counts below their roots
    assert (arr["root_visits"] >= 0).all() and arr["root_visits"].sum() > 0
    # the window's sample rows: the count the line reports, ordered by slot, pi a distribution
    n = line["detail"]["allgather_rows"]
    assert n > 0 and all(len(arr[k]) == n for k in NAMES if k.startswith("sample_"))
    assert (np.diff(arr["sample_slot"]) >= 0).all() and arr["sample_slot"].max() < GAMES
    assert np.abs(arr["sample_pi"].sum(1) - 1.0).max() < 1e-5
    assert np.isin(arr["sample_state"], (-1.0, 0.0, 1.0)).all()
    assert (np.abs(arr["sample_z"]) <= 1.0).all() and np.isin(arr["sample_player"], (-1, 1)).all()
    assert arr["counters"][5] >= STEPS  # steps
    assert arr["counters"][3] == 0 and arr["counters"][4] == 0  # nothing dropped / overflowed


def test_same_arguments_same_outputs(runs):
    (_, a, _), (_, b, _) = runs
    for n in NAMES:
        assert a[n].shape == b[n].shape and np.array_equal(a[n], b[n]), n
