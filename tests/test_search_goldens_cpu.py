"""The tree searches' behaviour per position, pinned (tests/golden/search_goldens.npz, made
by tests/golden/make_search_goldens.py with the library of the revision recorded in the file,
before csrc/negamax.h took over the rules solve.h, search.h and solve_deep.h each kept a copy
of).  Every array the host entry points return is recomputed and must be equal element for
element: score / value, best and nodes of every root, so the same roots are skipped and the
same roots abort, with the same codes and the same node counts.

Positions (own = the side to move; each sample holds roots that pass, terminal roots, full
boards and overlapping boards, at least 12 / 10 / 12 / 12 of them, and solve and deep 12
roots above max_empties):
  oth_solve_cpu       3,208 with 1..10 empties (stride 2), max_empties 10, limits 2^31, 1000, 10
  oth_solve_deep_cpu  2,562 with 1..12 empties (stride 3), max_empties 12, windows (-65, 65),
                      (-1, 1), (-8, 3) x the same limits; 9 roots with 14..16 empties in (-1, 1)
  oth_search_cpu      961 of any empties (stride 40), depths 1, 2, 3, 6 x limits 2^31, 100;
                      6 roots at depth 10
  az_leaf_solve_cpu   the planes of the 2,562, max_empties 12, limits 2^31, 64: values, stats
About eight seconds on one host thread.  No GPU."""
import sys

import numpy as np
import pytest

from conftest import GOLDEN, load_golden

nat = pytest.importorskip("az_native")

sys.path.insert(0, GOLDEN)
import make_search_goldens as mk  # noqa: E402

COUNTS = {"solve": 3208, "deep": 2562, "search": 961, "late": 9, "search_deep": 6}


@pytest.fixture(scope="module")
def golden():
    return load_golden("search_goldens.npz")


@pytest.fixture(scope="module")
def sets(golden):
    """The samples, rebuilt from the corpus; they are the ones the file was made from."""
    s, counts = mk.samples()
    assert {k: len(v[0]) for k, v in s.items()} == COUNTS
    for name in ("solve", "deep", "search"):
        for kind in ("pass", "terminal", "full", "overlapping"):
            assert counts[name][kind] >= 10, (name, kind)
    assert counts["solve"]["above_cap"] == counts["deep"]["above_cap"] == 12
    for name, (o, p) in s.items():
        assert np.array_equal(o, golden[f"sample/{name}/own"]), name
        assert np.array_equal(p, golden[f"sample/{name}/opp"]), name
    return s


def test_every_result_array_equals_the_recorded_one(golden, sets):
    assert len(str(golden["revision"])) == 40 and len(str(golden["build_id"])) == 64
    got = mk.compute(nat, sets)
    want = {k: v for k, v in golden.items()
            if not k.startswith("sample/") and k not in ("revision", "build_id")}
    assert sorted(got) == sorted(want) and len(want) == 3 * (3 + 9 + 1 + 8 + 1) + 2 * 2
    bad = []
    for k in sorted(want):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        if not np.array_equal(got[k], want[k]):
            i = int(np.flatnonzero(got[k] != want[k])[0])
            bad.append((k, int((got[k] != want[k]).sum()), i, got[k][i], want[k][i]))
    assert not bad, bad


def test_the_sample_exercises_the_rules(golden, sets):
    """What the pins are worth: skipped roots, roots that pass, terminal roots and aborted
    roots are all there, in the numbers the generator printed."""
    sc, best, nd = (golden[f"solve/limit{mk.BIG}/{k}"] for k in ("score", "best", "nodes"))
    assert int((sc == nat.AZ_SOLVE_SKIPPED).sum()) == 12 + 12  # overlapping, above the cap
    skipped = sc == nat.AZ_SOLVE_SKIPPED
    assert (nd[skipped] == 0).all() and (best[skipped] == 255).all()
    assert int(((best == 64) & (nd == 1)).sum()) == 10 + 12  # terminal roots, full boards
    # roots that pass: the twelve picked for it and those the stride met itself
    assert int(((best == 64) & (nd > 1)).sum()) == mk.samples()[1]["solve"]["pass"] == 151
    aborted = {k: int((v == nat.AZ_SOLVE_ABORTED).sum()) for k, v in golden.items()
               if k.startswith(("solve/", "deep/")) and k.endswith("/score")}
    assert aborted["solve/limit1000/score"] == 882 and aborted["solve/limit10/score"] == 2320
    assert aborted["deep/window-1_1/limit1000/score"] == 267
    assert aborted["deep/window-8_3/limit10/score"] == 1699
    v = golden["search/depth6/limit100/value"]
    assert int((v == nat.AZ_SEARCH_ABORTED).sum()) == 835
    assert int((golden[f"search/depth6/limit{mk.BIG}/value"] == nat.AZ_SEARCH_SKIPPED).sum()) == 12
    for k, a in golden.items():
        if k.endswith("/best") and k.replace("/best", "/score") in aborted:
            s = golden[k.replace("/best", "/score")]
            assert (a[s == nat.AZ_SOLVE_ABORTED] == 255).all(), k
