"""The oracle's node-capacity rule (oracle/mcts.py, node_capacity) and, on the oracle alone,
proof that the cases of tests/test_engine_tree_gpu.py reach what they are meant to reach:
overflowing arenas that end nearly full, roomy ones that never overflow, terminal nodes that
were visited, pass nodes, and an overflowed leaf that a later descent chose again.  Also the
comparison helper itself: it accepts an oracle tree laid out as the engine exports one and
rejects single-field and single-link damage."""
import numpy as np
import pytest

import tree_cases as tc
from oracle.mcts import SeqMCTS


def trees(script):
    return [s.tree for steps in script for s in steps]


def is_pass_node(t, i):
    return len(t.kids[i]) == 1 and t.action[t.kids[i][0]] == 64


@pytest.mark.parametrize("K,sims", tc.OVERFLOW_PARAMS)
def test_overflow_cases_overflow_and_end_nearly_full(K, sims):
    near, full, _ = tc.overflow_script(K, sims)
    assert [s.kind for s in full] == ["search", "move", "search"]
    first, _, second = full
    assert first.overflows >= 1 and second.overflows > first.overflows
    # full: the next expansion of any node (at most 33 children in Othello) may not fit
    for s in (first, second):
        assert tc.CAPACITY - 33 < len(s.tree.own) <= tc.CAPACITY
    # every simulation still ran: the root counts one visit per simulation (+ its own
    # expansion's backup, first search only)
    assert first.tree.N[0] == sims + 1
    # the neighbours always have room for one more expansion, so the unbounded oracle is theirs
    assert all(s.overflows == 0 and len(s.tree.own) <= tc.CAPACITY - 33 for s in near)
    assert near[0].tree.N[0] == tc.NEIGHBOUR_SIMS + 1


@pytest.mark.parametrize("K,c_puct,eps", tc.ROOMY_PARAMS)
def test_roomy_cases_never_overflow_and_run_their_whole_schedule(K, c_puct, eps):
    script = tc.roomy_script(K, c_puct, eps)
    for steps in script:
        assert [s.kind for s in steps] == ["search", "move", "search", "move", "search", "move",
                                           "search"]
        assert all(s.overflows == 0 for s in steps)
        assert not any(s.tree.term[s.tree.root] for s in steps)  # never moved onto a terminal
        # a re-root keeps a proper subtree, the next search grows it again
        assert all(len(m.tree.own) < len(b.tree.own) for b, m in zip(steps, steps[1:])
                   if m.kind == "move")
    # the noised cases consumed their injected vectors (at least the first root expansion's)
    noised = [t for t in trees(script) if t.kids[0] and isinstance(t.prior[t.kids[0][0]], np.float64)]
    assert bool(noised) == (eps > 0)


def test_roomy_cases_differ_from_each_other():
    """The parameters are not decorative: K, c_puct and the noise each change the trees."""
    sig = {p: tuple(tuple(t.N) for t in trees(tc.roomy_script(*p))) for p in tc.ROOMY_PARAMS}
    assert len(set(sig.values())) == len(sig)


def test_late_root_trees_hold_visited_terminal_nodes_and_pass_nodes():
    own, opp, _ = tc.corpus_root(*tc.LATE_ROOT)
    assert 8 <= 64 - bin(own | opp).count("1") <= 12
    for p in tc.ROOMY_PARAMS:
        late = [s.tree for s in tc.roomy_script(*p)[2]]
        assert any(t.term[i] and t.N[i] > 0 for t in late for i in range(len(t.own))), p
        # a pass node: one child, action 64 -- and the pass was walked through
        assert any(is_pass_node(t, i) and t.N[t.kids[i][0]] > 0
                   for t in late for i in range(len(t.own))), p


@pytest.mark.parametrize("sims", [40, 120, 300])
def test_an_overflowed_leaf_is_chosen_again(sims):
    """K = 1: a non-terminal node without children and with N >= 2 was reached by two
    descents, and the first of them must have overflowed (it would have children otherwise)."""
    for s in tc.overflow_script(1, sims)[1]:
        if s.kind == "search":
            t = s.tree
            assert any(not t.kids[i] and not t.term[i] and t.N[i] >= 2
                       for i in range(1, len(t.own)))


def test_repeated_leaf_of_one_batch_counts_once():
    """K > 1: the descents of one batch that wait on the same overflowing leaf cost one
    evaluation and one overflow, and each backs the value up (the engine's `repeat`)."""
    calls = []

    def ev(own, opp, player):
        calls.append((own, opp))
        return tc.evaluate(own, opp, player)

    o = SeqMCTS(2.0, 0, ev, leaves_per_step=4, node_capacity=tc.CAPACITY)
    o.search(tc.INIT_OWN, tc.INIT_OPP, 1)  # the root's expansion alone
    seen_repeat = False
    for _ in range(80):
        before = (o.overflows, len(calls), o.N[0], len(o.own))
        done = o.simulate_batch(4)
        assert o.N[0] - before[2] == done
        skipped = o.overflows - before[0]
        evals = len(calls) - before[1]
        assert skipped <= evals <= done
        if len(o.own) == before[3] and skipped and evals < done:
            seen_repeat = True  # fewer evaluations than backups, nothing expanded
            assert skipped == evals
    assert seen_repeat and o.overflows > 0


def test_capacity_none_is_the_reference_tree():
    a = tc.run_schedule(SeqMCTS(2.0, 0, tc.evaluate), (tc.INIT_OWN, tc.INIT_OPP, 1), (40,))
    b = tc.run_schedule(SeqMCTS(2.0, 0, tc.evaluate, node_capacity=10 ** 6),
                        (tc.INIT_OWN, tc.INIT_OPP, 1), (40,))
    assert a[0].tree.N == b[0].tree.N and a[0].tree.W == b[0].tree.W
    assert a[0].overflows == b[0].overflows == 0
    assert len(a[0].tree.own) > tc.CAPACITY  # the 40-simulation case is past the limit


def test_capacity_rule_is_exactly_nodes_plus_children():
    """The boundary: an expansion that fills the arena to the last node is made, one more
    child than room is skipped (engine.hip: fc + nc <= C)."""
    plain = SeqMCTS(2.0, 0, tc.evaluate)
    plain.search(tc.INIT_OWN, tc.INIT_OPP, 1)
    sizes = [len(plain.own)]  # after the root's expansion, then after each simulation
    for _ in range(6):
        plain.simulate()
        sizes.append(len(plain.own))
    n = max(i for i in range(1, 7) if sizes[i] > sizes[i - 1])  # the last one that expanded
    before, after = sizes[n - 1], sizes[n]
    for cap, want_overflow in ((after, 0), (after - 1, 1)):
        o = SeqMCTS(2.0, 0, tc.evaluate, node_capacity=cap)
        o.search(tc.INIT_OWN, tc.INIT_OPP, 1)
        for _ in range(n):
            o.simulate()
        assert o.overflows == want_overflow
        assert len(o.own) == (before if want_overflow else after)
        assert o.N[0] == n + 1  # backed up either way


# ---- the comparison helper ---------------------------------------------------------

def _late_tree():
    return tc.roomy_script(1, 2.0, 0.25)[2][2].tree  # re-rooted once, searched again


def test_helper_accepts_the_oracle_tree_in_export_layout():
    for p in (tc.ROOMY_PARAMS[1], tc.ROOMY_PARAMS[4]):
        for steps in tc.roomy_script(*p):
            for s in steps:
                assert tc.assert_same_tree(tc.export_of(s.tree), s.tree) == len(s.tree.own)
    for s in tc.overflow_script(4, 120)[1]:
        tc.assert_same_tree(tc.export_of(s.tree), s.tree)


def _inner(t):
    """An expanded node below the root's children."""
    return next(i for i in range(1, len(t.own)) if t.kids[i] and i not in t.kids[0])


@pytest.mark.parametrize("field,change", [
    ("W", lambda x: np.nextafter(x, np.inf)), ("N", lambda x: x + 1),
    ("prior", lambda x: np.nextafter(x, 0.0)), ("own", lambda x: x ^ np.uint64(1)),
    ("opp", lambda x: x ^ np.uint64(1 << 63)), ("legal", lambda x: x ^ np.uint64(2)),
    ("tval", lambda x: x + 1), ("action", lambda x: x + 1),
    ("flags", lambda x: x ^ 1), ("flags", lambda x: x ^ 2), ("flags", lambda x: x ^ 4),
    ("flags", lambda x: x | 8), ("nchild", lambda x: x - 1), ("first", lambda x: x + 1),
    ("parent", lambda x: x + 1)])
def test_helper_rejects_one_damaged_inner_node(field, change):
    o = _late_tree()
    t = tc.export_of(o)
    i = _inner(o)
    if field == "parent":
        i = o.kids[i][0]
    t[field][i] = change(t[field][i])
    with pytest.raises(AssertionError):
        tc.assert_same_tree(t, o)


def test_helper_rejects_garbage_and_lost_nodes():
    o = _late_tree()
    t = tc.export_of(o)
    t["n_nodes"] += 1  # one node more in the arena than the tree reaches
    with pytest.raises(AssertionError):
        tc.assert_same_tree(t, o)
    t = tc.export_of(o)
    leaf = next(i for i in range(len(o.own) - 1, 0, -1) if o.kids[i])
    t["flags"][leaf] &= 0xFE  # a subtree cut off: its nodes are no longer reached
    t["nchild"][leaf] = 0
    with pytest.raises(AssertionError):
        tc.assert_same_tree(t, o)
    # the root's own prior, action and parent are not compared
    t = tc.export_of(o)
    t["prior"][0], t["action"][0], t["parent"][0] = 0.5, 7, 3
    tc.assert_same_tree(t, o)
