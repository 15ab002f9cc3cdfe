"""Whole MCTS trees of the GPU engine against the oracle (oracle/mcts.py SeqMCTS), node for
node: every node's boards, legal mask, N, W, prior, action, flags and terminal value, and
the parent / first / nchild links, after every search and every re-root -- three re-roots
per tree, so the comparison sees the second arena half and the first one again.  The other
parity tests read root-level data only.

The cases are tests/tree_cases.py's (tests/test_oracle_capacity_cpu.py shows on the CPU that
they reach terminal nodes, pass nodes, overflowing arenas and re-chosen overflowed leaves):

  * roomy arenas through az_make_move, through the arena's batched az_reroot_slots /
    az_root_stats, and through the fused az_select_expand launch;
  * a 128-node arena (the smallest the engine accepts) that overflows, against the oracle's
    node_capacity rule -- a leaf whose children do not fit is evaluated and backed up, gets
    no children and is counted once -- with roomy neighbours on both sides whose trees must
    be untouched; the per-slot and the engine-wide overflow counters equal the oracle's;
  * the guards that turn a non-zero counter into an error (engine.check_complete through
    BatchedSelfPlay.play_games, arena.BatchedArena).

Left out: the second source of the overflow counter, a descent deeper than kMaxPath = 64
nodes; no Othello search of these sizes gets 64 plies below its root.
"""
import functools

import numpy as np
import pytest

import tree_cases as tc
from mock_policy import MockNet, mock_eval_torch, sharp_eval_torch

pytestmark = pytest.mark.gpu

nat = pytest.importorskip("az_native")
from engine import BatchedSelfPlay, Engine  # noqa: E402


def step_plain(e, evaluate=mock_eval_torch):
    e.select()
    pr, va = evaluate(e.nn_in)
    e.priors.copy_(pr)
    e.values.copy_(va)
    e.expand()
    e.play()


def step_fused(e, evaluate=mock_eval_torch):
    """The drop-in MCTS's fused iteration: the last select's leaves, then this one's descents."""
    e.select_expand()
    pr, va = evaluate(e.nn_in)
    e.priors.copy_(pr)
    e.values.copy_(va)


def run_search(e, step, max_steps=2000):
    for _ in range(max_steps):
        step(e)
        if (e.game_info()["status"] != nat.AZ_GAME_ACTIVE).all():
            return
    raise AssertionError("search did not finish")


def replay(e, script, step, batched=False, stray=None):
    """Run the script's searches and re-roots on engine `e` (slot g = script[g]) and compare
    every slot's whole tree with the oracle's after each of them; a slot whose script has
    ended must keep its last tree.  batched: begin and re-root through the arena's batched
    calls, with `stray` = {slot: action} sent along with every re-root (a negative or a
    non-child action: not found, tree unchanged), and az_root_stats read after every search.
    Returns the largest n_nodes seen per slot."""
    G = len(script)
    assert G == e.G
    biggest = np.zeros(G, np.int64)
    for i in range(max(len(s) for s in script)):
        live = [g for g in range(G) if i < len(script[g])]
        kind = script[live[0]][i].kind
        assert all(script[g][i].kind == kind for g in live)
        if kind == "search":
            if batched:
                for sims in sorted({script[g][i].arg for g in live}):
                    e.begin_search_slots([g for g in live if script[g][i].arg == sims], sims)
            else:
                for g in live:
                    e.begin_search(g, script[g][i].arg)
            run_search(e, step)
        elif batched:
            actions = np.full(G, -1, np.int32)
            for g in live:
                actions[g] = script[g][i].arg
            for g, a in (stray or {}).items():
                actions[g] = a
            found = e.reroot_slots(actions)
            assert (found[live] >= 1).all(), found
            assert all(found[g] == -1 for g in range(G) if g not in live), found
        else:
            for g in live:
                e.make_move(g, script[g][i].arg)
        info = e.game_info()
        if batched and kind == "search":
            counts, vroot = e.root_stats()
        for g in range(G):
            s = script[g][min(i, len(script[g]) - 1)]
            where = f"slot {g} after step {i} ({kind} {s.arg})"
            n = tc.assert_same_tree(e.export_tree(g), s.tree, where)
            assert info["n_nodes"][g] == n, where
            assert info["overflow"][g] == s.overflows, \
                f"{where}: {info['overflow'][g]} overflows counted, the oracle has {s.overflows}"
            biggest[g] = max(biggest[g], n)
            if batched and kind == "search":
                assert (counts[g] == s.tree.counts()).all(), where
                assert vroot[g] == s.tree.vroot(), where
    return biggest


def roomy_engine(K, c_puct, eps, extra=0):
    roots = tc.roomy_roots() + [tc.roomy_roots()[0]] * extra
    e = Engine(len(roots), 120, c_puct=c_puct, dirichlet_alpha=1.0, dirichlet_epsilon=eps,
               injected_rng=True, auto_play=False, inj_noise_slots=tc.NOISE_SLOTS,
               leaves_per_step=K)
    for g, (own, opp, player) in enumerate(roots):
        e.set_root(g, own, opp, player)
    # an extra slot repeats slot 0's root and therefore gets slot 0's noise
    e.inject(noise=np.stack([tc.noise_vectors(g if g < 3 else 0) for g in range(len(roots))]))
    return e


@pytest.mark.parametrize("K,c_puct,eps", tc.ROOMY_PARAMS)
def test_whole_trees_match_oracle(K, c_puct, eps):
    e = roomy_engine(K, c_puct, eps)
    replay(e, tc.roomy_script(K, c_puct, eps), step_plain)
    c = e.counters()
    assert c["arena_overflows"] == 0 and c["simulations"] == 3 * sum(tc.ROOMY_SCHEDULE)


@pytest.mark.parametrize("K,c_puct,eps", tc.ROOMY_PARAMS)
def test_whole_trees_match_oracle_batched_control(K, c_puct, eps):
    """az_begin_search_slots / az_reroot_slots / az_root_stats.  Slots 3 and 4 hold slot 0's
    first tree; every re-root sends slot 3 action -1 and slot 4 a corner square, which is no
    child of the opening position's root: found = -1 for both, trees unchanged node for node."""
    script = tc.roomy_script(K, c_puct, eps)
    e = roomy_engine(K, c_puct, eps, extra=2)
    replay(e, script + [script[0][:1]] * 2, step_plain, batched=True, stray={3: -1, 4: 0})
    assert e.counters()["arena_overflows"] == 0


@pytest.mark.parametrize("K,c_puct,eps", tc.ROOMY_PARAMS)
def test_whole_trees_match_oracle_fused_select_expand(K, c_puct, eps):
    e = roomy_engine(K, c_puct, eps)
    replay(e, tc.roomy_script(K, c_puct, eps), step_fused)
    c = e.counters()
    assert c["arena_overflows"] == 0 and c["simulations"] == 3 * sum(tc.ROOMY_SCHEDULE)


def overflow_engine(K, sims):
    e = Engine(3, sims, c_puct=2.0, auto_play=False, node_capacity=tc.CAPACITY,
               leaves_per_step=K)
    assert e.C == tc.CAPACITY
    for g in range(3):
        e.set_root(g, tc.INIT_OWN, tc.INIT_OPP, 1)
    return e


def check_overflow_case(K, sims, step, script=None):
    script = script or tc.overflow_script(K, sims)
    e = overflow_engine(K, sims)
    biggest = replay(e, script, step)
    assert (biggest <= tc.CAPACITY).all() and biggest[1] > tc.CAPACITY - 33
    c = e.counters()
    assert c["arena_overflows"] == sum(s[-1].overflows for s in script) > 0
    assert c["simulations"] == 2 * (sims + 2 * tc.NEIGHBOUR_SIMS)


@pytest.mark.parametrize("K,sims", tc.OVERFLOW_PARAMS)
def test_arena_overflow_follows_the_capacity_rule(K, sims):
    """Slot 1 overflows its 128-node arena; its tree, both neighbours' trees and every
    counter are the oracle's, after the first search, the re-root and the second search."""
    check_overflow_case(K, sims, step_plain)


@pytest.mark.parametrize("sims", [s for K, s in tc.OVERFLOW_PARAMS if K == 1])
def test_arena_overflow_fused_select_expand(sims):
    check_overflow_case(1, sims, step_fused)


# ---- the sharp policy ---------------------------------------------------------------
# mock_policy.sharp_eval: priors of exactly 0, of 2^-44 and equal powers of two, values of
# exactly +-1 and 0 (tests/test_sharp_cpu.py counts what that reaches in a search).  Whole
# trees, so a sibling group left unnormalised or a tie taken at another child shows at the
# node where it happened and not only in the root's counts.

step_plain_sharp = functools.partial(step_plain, evaluate=sharp_eval_torch)
step_fused_sharp = functools.partial(step_fused, evaluate=sharp_eval_torch)


@pytest.mark.parametrize("K,c_puct,eps", tc.ROOMY_PARAMS)
def test_whole_trees_match_oracle_sharp(K, c_puct, eps):
    e = roomy_engine(K, c_puct, eps)
    replay(e, tc.roomy_script_sharp(K, c_puct, eps), step_plain_sharp)
    c = e.counters()
    assert c["arena_overflows"] == 0 and c["simulations"] == 3 * sum(tc.ROOMY_SCHEDULE)


@pytest.mark.parametrize("K,c_puct,eps", tc.ROOMY_PARAMS)
def test_whole_trees_match_oracle_fused_select_expand_sharp(K, c_puct, eps):
    e = roomy_engine(K, c_puct, eps)
    replay(e, tc.roomy_script_sharp(K, c_puct, eps), step_fused_sharp)
    c = e.counters()
    assert c["arena_overflows"] == 0 and c["simulations"] == 3 * sum(tc.ROOMY_SCHEDULE)


@pytest.mark.parametrize("K,sims", tc.OVERFLOW_PARAMS_SHARP)
def test_arena_overflow_follows_the_capacity_rule_sharp(K, sims):
    check_overflow_case(K, sims, step_plain_sharp, tc.overflow_script_sharp(K, sims))


# ---- the guards -------------------------------------------------------------------

SP_ARGS = {"c_puct": 2.0, "num_simulations": 60, "dirichlet_alpha": 1.0,
           "dirichlet_epsilon": 0.25, "mcts_temperature": 1.0, "num_exploratory_moves": 10,
           "lambda": 0.98}


def test_play_games_raises_on_arena_overflow():
    sp = BatchedSelfPlay(MockNet(), SP_ARGS, 8, seed=3, fold=False, node_capacity=tc.CAPACITY)
    with pytest.raises(RuntimeError, match="node_capacity"):
        sp.play_games(8)
    c = sp.counters()
    # the searches all finished all the same: the guard is what stops their use
    assert c["games_finished"] == 8 and c["arena_overflows"] > 0
    assert c["simulations"] == SP_ARGS["num_simulations"] * c["moves"]
    assert (sp.engine.game_info()["n_nodes"] <= tc.CAPACITY).all()


def test_play_games_returns_with_the_default_capacity():
    sp = BatchedSelfPlay(MockNet(), SP_ARGS, 8, seed=3, fold=False)
    tuples = sp.play_games(8)
    c = sp.counters()
    assert c["games_finished"] == 8 and c["arena_overflows"] == 0
    assert len(tuples) == c["samples"] >= 8 * 9


def test_batched_arena_raises_on_arena_overflow():
    from arena import BatchedArena, tie_break_lowest

    arena = BatchedArena(MockNet(1).cuda(), MockNet(2).cuda(),
                         {"c_puct": 2.0, "num_simulations": 60}, n_slots=2,
                         tie_break=tie_break_lowest, node_capacity=tc.CAPACITY)
    with pytest.raises(RuntimeError, match="node_capacity"):
        arena.play(2)
