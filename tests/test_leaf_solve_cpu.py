"""Exact leaf values, the host mirror (az_leaf_solve_cpu, csrc/leaf_solve.hip): which rows are
solved, what is written, what is left alone bit for bit, the node limit, the counters and
the argument checks.  The reference is endgame.solve_deep(window="wld") on the host, which
tests/test_solve_deep_cpu.py proves against the plain solver.  No GPU."""
import ctypes

import numpy as np
import pytest

import leaf_cases as lc

nat = pytest.importorskip("az_native")

EMPTIES = [1, 4, 8, 12]


def run_cpu(x, E, node_limit=1 << 31):
    v = lc.sentinels(len(x))
    stats = nat.leaf_solve_cpu(x, v, E, node_limit)
    return v, stats


def test_entry_points_are_declared_and_abi_is_1():
    assert nat.lib.az_abi_version() == 1
    for name in ("az_leaf_solve_cpu", "az_leaf_solve_gpu", "az_leaf_solve_stats_gpu"):
        assert name in nat.SIGNATURES


@pytest.mark.parametrize("E", EMPTIES)
def test_solved_rows_hold_the_sign_of_the_score(E):
    import endgame

    r = lc.rows()
    got, _ = run_cpu(r["x"], E)
    m = (r["emp"] >= 1) & (r["emp"] <= E)
    assert m.sum() == E * lc.PER_DEPTH
    score = endgame.solve_deep(r["own"][m], r["opp"][m], E, window="wld", device="cpu")[0]
    assert (score > nat.AZ_SOLVE_ABORTED).all()
    want = np.sign(score.astype(np.int64)).astype(np.float32)
    assert np.array_equal(got[m], want)
    assert set(np.unique(want)) <= {-1.0, 0.0, 1.0} and len(np.unique(want)) >= 2


@pytest.mark.parametrize("E", EMPTIES)
def test_other_rows_keep_their_value_bit_for_bit(E):
    r = lc.rows()
    got, _ = run_cpu(r["x"], E)
    m = (r["emp"] >= 1) & (r["emp"] <= E)
    keep = ~m
    # all three kinds are there: no leaf, a full board, more empties than E
    assert (r["emp"][keep] == 64).any() and (r["emp"][keep] == 0).any()
    assert (r["emp"][keep] == E + 1).any()
    assert np.array_equal(got.view(np.uint32)[keep], lc.sentinels(len(got)).view(np.uint32)[keep])
    # and the whole result is what the shared expectation says (the GPU tests compare with it)
    want, _ = lc.expected(E)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_symmetric_images_get_the_same_value():
    r = lc.rows()
    m = (r["emp"] >= 1) & (r["emp"] <= 8)
    own, opp = r["own"][m], r["opp"][m]
    base, _ = run_cpu(lc.planes(own, opp), 8)
    assert not np.array_equal(base, lc.sentinels(len(base)))
    for sym in range(1, 8):
        x = lc.planes(nat.d4_cpu(own, sym), nat.d4_cpu(opp, sym))
        got, _ = run_cpu(x, 8)
        assert np.array_equal(got, base), sym


def test_node_limit_leaves_the_net_value():
    r = lc.rows()
    _, nodes = lc.solved()
    got, stats = run_cpu(r["x"], 8, 64)
    task = (r["emp"] >= 1) & (r["emp"] <= 8)
    within = task & (nodes <= 64)
    over = task & (nodes > 64)
    assert within[r["emp"] == 8].any() and over[r["emp"] == 8].any()
    sent = lc.sentinels(len(got))
    written = got.view(np.uint32) != sent.view(np.uint32)
    assert np.array_equal(written, within)
    score, _ = lc.solved()
    assert np.array_equal(got[within], np.sign(score[within]).astype(np.float32))
    assert stats["solved"] == within.sum() and stats["limited"] == over.sum()
    want, want_stats = lc.expected(8, 64)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and stats == want_stats


@pytest.mark.parametrize("E", EMPTIES)
def test_counters_are_the_host_solver_s(E):
    r = lc.rows()
    _, stats = run_cpu(r["x"], E)
    _, nodes = lc.solved()
    task = (r["emp"] >= 1) & (r["emp"] <= E)
    assert stats == {"solved": int(task.sum()), "limited": 0, "nodes": int(nodes[task].sum())}


@pytest.mark.parametrize("E,limit", [(0, 256), (13, 256), (-1, 256), (6, 0)])
def test_argument_errors(E, limit):
    r = lc.rows()
    v = lc.sentinels(8)
    x = np.ascontiguousarray(r["x"][:8])
    rc = nat.lib.az_leaf_solve_cpu(nat.ptr(x), nat.ptr(v), 8, E, limit, None)
    assert rc == nat.AZ_ERR_ARG and nat.last_error()
    assert np.array_equal(v, lc.sentinels(8))
    # the device entry point checks the same before it touches anything (the size query)
    need = ctypes.c_size_t(0)
    rc = nat.lib.az_leaf_solve_gpu(None, None, 8, E, limit, None, ctypes.byref(need), None)
    assert rc == nat.AZ_ERR_ARG


def test_workspace_size_query_and_empty_call():
    need = ctypes.c_size_t(0)
    assert nat.lib.az_leaf_solve_gpu(None, None, 1000, 6, 256, None, ctypes.byref(need),
                                     None) == nat.AZ_OK
    assert need.value >= 256 + 1000 * 20 and need.value % 8 == 0
    assert nat.lib.az_leaf_solve_cpu(None, None, 0, 6, 256, None) == nat.AZ_OK


def test_args_keys():
    import engine

    assert engine.leaf_solve_args({}) == (0, engine.LEAF_SOLVE_NODES)
    assert engine.leaf_solve_args({"leaf_solve_empties": 6, "leaf_solve_nodes": 64}) == (6, 64)
    for bad in ({"leaf_solve_empties": 13}, {"leaf_solve_empties": -1},
                {"leaf_solve_empties": 4, "leaf_solve_nodes": 0}):
        with pytest.raises(ValueError):
            engine.leaf_solve_args(bad)
