"""Depth-limited alpha-beta on the host (oth_eval_cpu / oth_search_cpu, csrc/search.h) and the
Python surface on top of it (alphabeta.py, the arena's alpha-beta side), without a GPU.

The independent restatement is NumPy: the oracle's verified batched legal / step build the
tree, a literal copy of the square table W and of the constants below evaluates the leaves,
and an unpruned level-by-level minimax backs the values up with the key
(32768 - child value) * 256 + 255 - action (the lowest action among the best).  Depths 1..5
are compared with it directly; depths 6..10 follow by induction: V(root, d) and best must be
the backup of the native search of the children at d - 1."""
import numpy as np
import pytest

from conftest import load_golden
from oracle import board as ob

nat = pytest.importorskip("az_native")

_SH = np.arange(64, dtype=np.uint64)
W = np.array([[100, -20, 10, 5, 5, 10, -20, 100],
              [-20, -50, -2, -2, -2, -2, -50, -20],
              [10, -2, -1, -1, -1, -1, -2, 10],
              [5, -2, -1, -1, -1, -1, -2, 5],
              [5, -2, -1, -1, -1, -1, -2, 5],
              [10, -2, -1, -1, -1, -1, -2, 10],
              [-20, -50, -2, -2, -2, -2, -50, -20],
              [100, -20, 10, 5, 5, 10, -20, 100]], np.int64).reshape(64)
MOBILITY, WIN, PER_DISC = 12, 10000, 100
SKIPPED, ABORTED, LIMIT = -32768, -32767, 1 << 31


def popc(x):
    x = np.ascontiguousarray(x, np.uint64)
    return np.unpackbits(x.view(np.uint8).reshape(-1, 8), axis=1).sum(axis=1).astype(np.int64)


def bits(x):
    return ((np.ascontiguousarray(x, np.uint64)[:, None] >> _SH) & np.uint64(1)).astype(np.int64)


def terminal_value(d):
    return np.sign(d) * (WIN + PER_DISC * np.abs(d))


def heuristic(own, opp, lg, lg2):
    out = np.empty(len(own), np.int64)
    for a in range(0, len(own), 1 << 17):  # bounded temporaries
        s = slice(a, a + (1 << 17))
        out[s] = (bits(own[s]) - bits(opp[s])) @ W
    return out + MOBILITY * (popc(lg) - popc(lg2))


def static_eval(own, opp):
    lg, lg2 = ob.legal_batch(own, opp), ob.legal_batch(opp, own)
    term = (lg == 0) & (lg2 == 0)
    return np.where(term, terminal_value(popc(own) - popc(opp)), heuristic(own, opp, lg, lg2))


def expand(own, opp, depth):
    """One level of the tree: per node its kind (terminal / horizon leaf / interior) and
    static value, and the children of the interior nodes: the placements with one ply less,
    or the single pass with the same depth."""
    lg, lg2 = ob.legal_batch(own, opp), ob.legal_batch(opp, own)
    term = (lg == 0) & (lg2 == 0)
    leaf = ~term & (depth == 0)
    inner = ~term & ~leaf
    passer = inner & (lg == 0)
    static = np.where(term, terminal_value(popc(own) - popc(opp)), 0)
    if leaf.any():
        static[leaf] = heuristic(own[leaf], opp[leaf], lg[leaf], lg2[leaf])
    par, act = np.nonzero(bits(lg).astype(bool) & inner[:, None])
    pidx = np.flatnonzero(passer)
    cdepth = np.concatenate([depth[par] - 1, depth[pidx]])
    par = np.concatenate([par, pidx])
    act = np.concatenate([act, np.full(len(pidx), 64)]).astype(np.uint8)
    co, cp, _, _, bad = ob.step_batch(own[par], opp[par], act)
    assert bad == -1
    return {"n": len(own), "inner": inner, "static": static, "par": par, "act": act,
            "passes": int(passer.sum()), "early_ends": int((term & (depth > 0)).sum())}, \
        co, cp, cdepth


def back_up(n, inner, static, par, act, child_value):
    key = np.full(n, -1, np.int64)
    if len(par):
        np.maximum.at(key, par, (32768 - child_value) * 256 + 255 - act.astype(np.int64))
    assert (~inner | (key >= 0)).all()
    return np.where(inner, key // 256 - 32768, static), np.where(inner, 255 - key % 256, 64)


def minimax(own, opp, depth):
    """Unpruned minimax of every root to `depth`: (value, best, interior passes, terminal
    nodes above the horizon), the last two counted below the roots."""
    levels = []
    o, p, d = own, opp, np.full(len(own), depth, np.int64)
    while len(o):
        lv, o, p, d = expand(o, p, d)
        levels.append(lv)
    value = best = None
    for lv in reversed(levels):
        value, best = back_up(lv["n"], lv["inner"], lv["static"], lv["par"], lv["act"], value)
    return (value, best, sum(lv["passes"] for lv in levels[1:]),
            sum(lv["early_ends"] for lv in levels[1:]))


@pytest.fixture(scope="module")
def corpus():
    d = load_golden("board_corpus.npz")
    own = np.where(d["player"] == 1, d["pos"], d["neg"]).astype(np.uint64)
    opp = np.where(d["player"] == 1, d["neg"], d["pos"]).astype(np.uint64)
    end = d["term_next"] == 1
    town = np.where(d["player"] == 1, d["nneg"], d["npos"])[end].astype(np.uint64)
    topp = np.where(d["player"] == 1, d["npos"], d["nneg"])[end].astype(np.uint64)
    return {"own": own, "opp": opp, "emp": 64 - popc(own | opp), "town": town, "topp": topp}


def sample(corpus, per_class, lo=1, hi=60):
    """The first per_class of default_rng(0).permutation of every empties class lo..hi."""
    idx = []
    for e in range(lo, hi + 1):
        cls = np.flatnonzero(corpus["emp"] == e)
        idx.append(cls[np.random.default_rng(0).permutation(len(cls))[:per_class]])
    idx = np.concatenate(idx)
    return corpus["own"][idx], corpus["opp"][idx]


def test_eval(corpus):
    own, opp = corpus["own"], corpus["opp"]
    assert len(own) == 36565
    lg, lg2 = ob.legal_batch(own, opp), ob.legal_batch(opp, own)
    assert ((lg == 0) & (lg2 != 0)).sum() == 275 and not ((lg == 0) & (lg2 == 0)).any()
    got = nat.eval_cpu(own, opp)
    assert got.dtype == np.int16
    want = heuristic(own, opp, lg, lg2)
    assert (got == want).all()
    assert want.min() == -658 and want.max() == 705
    # the corpus games' final positions: decided games outrank every heuristic value
    town, topp = corpus["town"], corpus["topp"]
    assert len(town) >= 600
    d = popc(town) - popc(topp)
    got = nat.eval_cpu(town, topp).astype(np.int64)
    assert (got == terminal_value(d)).all() and (got == static_eval(town, topp)).all()
    assert (np.abs(got[d != 0]) > 10000).all() and (got[d == 0] == 0).all()
    assert len(nat.eval_cpu(np.zeros(0, np.uint64), np.zeros(0, np.uint64))) == 0


def check_depth(own, opp, depth, need_coverage=True):
    want_v, want_b, passes, ends = minimax(own, opp, depth)
    print(f"depth {depth}: {len(own)} roots, {passes} interior passes, {ends} early ends")
    if need_coverage:
        assert passes >= 1 and ends >= 1
    v, b, nodes = nat.search_cpu(own, opp, depth)
    assert (v == want_v).all()
    assert (b == want_b).all()
    assert (nodes >= 1).all()


def test_depth_1_whole_corpus(corpus):
    # depth 1 has no interior node below the root, so no coverage condition
    check_depth(corpus["own"], corpus["opp"], 1, need_coverage=False)


@pytest.mark.parametrize("depth,per_class", [
    (2, 20), (3, 8), (4, 2), pytest.param(4, 4, marks=pytest.mark.slow),
    pytest.param(5, 1, marks=pytest.mark.slow)])
def test_brute_force(corpus, depth, per_class):
    own, opp = sample(corpus, per_class)
    check_depth(own, opp, depth, need_coverage=depth <= 4)


def one_ply(own, opp, depth):
    """Value and best at `depth` from the native search of the children at depth - 1; a
    pass-only root is the negation of the position after the pass (test_solve_cpu.one_ply)."""
    lg, lg2 = ob.legal_batch(own, opp), ob.legal_batch(opp, own)
    assert ((lg != 0) | (lg2 != 0)).all()
    passer = lg == 0
    o, p = np.where(passer, opp, own), np.where(passer, own, opp)
    par, act = np.nonzero(bits(ob.legal_batch(o, p)).astype(bool))
    co, cp, _, _, bad = ob.step_batch(o[par], p[par], act.astype(np.uint8))
    assert bad == -1
    import alphabeta

    cv, _, _ = alphabeta.search(co, cp, depth - 1, device="cpu", node_limit=LIMIT)
    assert (cv > ABORTED).all()
    v, b = back_up(len(o), np.ones(len(o), bool), np.zeros(len(o), np.int64), par, act,
                   cv.astype(np.int64))
    return np.where(passer, -v, v), np.where(passer, 64, b)


@pytest.mark.parametrize("depth", [6, 7, 8, pytest.param(9, marks=pytest.mark.slow),
                                   pytest.param(10, marks=pytest.mark.slow)])
def test_one_ply_induction(corpus, depth):
    import alphabeta

    cls = np.flatnonzero((corpus["emp"] >= 20) & (corpus["emp"] <= 40))
    idx = cls[np.random.default_rng(0).permutation(len(cls))[:64]]
    own, opp = corpus["own"][idx], corpus["opp"][idx]
    v, b, _ = alphabeta.search(own, opp, depth, device="cpu", node_limit=LIMIT)
    want_v, want_b = one_ply(own, opp, depth)
    assert (v == want_v).all()
    assert (b == want_b).all()


def test_d4_invariance(corpus):
    own, opp = sample(corpus, 8)
    base, _, _ = nat.search_cpu(own, opp, 3)
    for sym in range(1, 8):
        so, sp = nat.d4_cpu(own, sym), nat.d4_cpu(opp, sym)
        v, b, _ = nat.search_cpu(so, sp, 3)
        assert (v == base).all()
        # best is a legal move that achieves the value
        lg = nat.legal_cpu(so, sp)
        assert (np.where(b == 64, lg == 0, ((lg >> (b & 63).astype(np.uint64)) & np.uint64(1)) == 1)).all()
        m = b < 64
        co, cp = nat.make_move_cpu(so[m], sp[m], b[m])
        assert (-nat.search_cpu(co, cp, 2)[0].astype(np.int64) == v[m]).all()


def test_conventions(corpus):
    own, opp, emp = corpus["own"], corpus["opp"], corpus["emp"]
    i30 = np.flatnonzero(emp == 30)[:5]
    # overlapping boards are skipped, no work
    v, b, n = nat.search_cpu(own[i30] | opp[i30], opp[i30], 3)
    assert (v == SKIPPED).all() and (b == 255).all() and (n == 0).all()
    # terminal roots: T(d), best 64, one node, at any depth
    town, topp = corpus["town"], corpus["topp"]
    for depth in (1, 10):
        v, b, n = nat.search_cpu(town, topp, depth)
        assert (v == terminal_value(popc(town) - popc(topp))).all()
        assert (b == 64).all() and (n == 1).all()
    # pass-only roots
    lg, lg2 = nat.legal_cpu(own, opp), nat.legal_cpu(opp, own)
    passer = np.flatnonzero((lg == 0) & (lg2 != 0))
    v, b, n = nat.search_cpu(own[passer], opp[passer], 2)
    assert (b == 64).all() and (v > ABORTED).all() and (n >= 3).all()
    # the node limit
    v, b, n = nat.search_cpu(own[i30], opp[i30], 4, node_limit=10)
    assert (v == ABORTED).all() and (b == 255).all()
    v, b, n = nat.search_cpu(np.concatenate([own[i30], town[:3]]),
                             np.concatenate([opp[i30], topp[:3]]), 4, node_limit=1)
    assert (v[:5] == ABORTED).all() and (b[:5] == 255).all()
    assert (v[5:] > ABORTED).all() and (b[5:] == 64).all()  # a terminal root is one node
    full = nat.search_cpu(own[i30], opp[i30], 4)
    again = nat.search_cpu(own[i30], opp[i30], 4, node_limit=int(full[2].max()))
    assert (again[0] == full[0]).all() and (again[2] == full[2]).all()
    assert (full[2] >= 1).all()
    # n = 0, NULL nodes, depth outside 1..10
    v, b, n = nat.search_cpu(np.zeros(0, np.uint64), np.zeros(0, np.uint64), 3)
    assert len(v) == 0 and v.dtype == np.int16 and b.dtype == np.uint8 and n.dtype == np.uint64
    assert nat.lib.oth_search_cpu(None, None, 0, 3, 100, None, None, None) == nat.AZ_OK
    o16, ou = np.zeros(1, np.int16), np.zeros(1, np.uint8)
    assert nat.lib.oth_search_cpu(nat.ptr(own[i30]), nat.ptr(opp[i30]), 1, 4, LIMIT, nat.ptr(o16),
                                  nat.ptr(ou), None) == nat.AZ_OK
    assert o16[0] == full[0][0] and ou[0] == full[1][0]
    for depth in (0, 11, -1):
        with pytest.raises(RuntimeError, match="depth"):
            nat.search_cpu(own[i30], opp[i30], depth)
        assert nat.lib.oth_search_cpu(nat.ptr(own[i30]), nat.ptr(opp[i30]), 1, depth, 100,
                                      nat.ptr(o16), nat.ptr(ou), None) == nat.AZ_ERR_ARG
    assert (nat.AZ_SEARCH_SKIPPED, nat.AZ_SEARCH_ABORTED, nat.AZ_SEARCH_MAX_DEPTH) == \
        (SKIPPED, ABORTED, 10)


def test_python_surface_threads_match_single_call(corpus):
    import alphabeta
    import torch

    own, opp = sample(corpus, 20)
    v, b, n = alphabeta.search(own, opp, 3, device="cpu")
    v1, b1, n1 = nat.search_cpu(own, opp, 3)
    assert v.dtype == np.int16 and b.dtype == np.uint8 and n.dtype == np.uint64
    assert (v == v1).all() and (b == b1).all() and (n == n1).all()
    assert (alphabeta.evaluate(own, opp, device="cpu") == nat.eval_cpu(own, opp)).all()
    tv, tb, tn = alphabeta.search(torch.from_numpy(own.view(np.int64)),
                                  torch.from_numpy(opp.view(np.int64)), 3, device="cpu")
    assert tv.dtype == torch.int16 and (tv.numpy() == v1).all() and (tb.numpy() == b1).all()
    with pytest.raises(RuntimeError, match="depth"):
        alphabeta.search(own, opp, 11, device="cpu")


def test_openings():
    import alphabeta

    for plies, n in ((2, 12), (4, 100), (6, 64), (8, 1024)):
        own, opp, player = alphabeta.openings(n, plies, 0)
        assert len(own) == len(opp) == len(player) == n
        assert own.dtype == np.uint64 and (player == 1).all()
        assert len({(int(o), int(p)) for o, p in zip(own, opp)}) == n  # distinct
        assert ((own & opp) == 0).all() and (popc(own | opp) == 4 + plies).all()
        assert (ob.legal_batch(own, opp) != 0).all()
        again = alphabeta.openings(n, plies, 0)
        assert (again[0] == own).all() and (again[1] == opp).all()
    other = alphabeta.openings(1024, 8, 1)
    assert (other[0] != own).any()
    # two plies reach 4 * 3 = 12 positions, every one distinct as a raw bitboard pair
    assert len(alphabeta.reachable(2)[0]) == 12
    with pytest.raises(ValueError):
        alphabeta.openings(13, 2, 0)
    with pytest.raises(ValueError):
        alphabeta.openings(10, 0, 0)
    with pytest.raises(ValueError):
        alphabeta.openings(4, 3, 0)
    with pytest.raises(ValueError):
        alphabeta.openings(4, 10, 0)


def replay(rec, side_move):
    """Replay one recorded match with the host step: every action goes through
    side_move(side, own, opp, action) (side 0 = A, 1 = B); returns (plies, result for A)."""
    own = np.array([rec["own"]], np.uint64)
    opp = np.array([rec["opp"]], np.uint64)
    player, first = rec["player"], rec["player"]
    for i, a in enumerate(rec["actions"]):
        side = 0 if (player == first) == rec["a_first"] else 1
        side_move(side, own, opp, a)
        own, opp, _, st = nat.step_cpu(own, opp, np.array([a], np.uint8))
        player = -player
        term = bool(nat.status_flags(st)[0] & nat.AZ_FLAG_TERMINAL)
        assert term == (i == len(rec["actions"]) - 1)
    # own is the side to move after the last action: `player`
    d = int(popc(own)[0] - popc(opp)[0])
    a_colour = first if rec["a_first"] else -first
    d_a = d if player == a_colour else -d
    return len(rec["actions"]), int(np.sign(d_a))


def expect_alphabeta_move(depth, exact_empties):
    def check(own, opp, a):
        e = 64 - int(popc(own | opp)[0])
        if 1 <= e <= exact_empties:
            want = nat.solve_cpu(own, opp, exact_empties)[1][0]
        else:
            want = nat.search_cpu(own, opp, depth)[1][0]
        assert a == want
    return check


def test_arena_two_alphabeta_players_on_the_host():
    import alphabeta
    from arena import BatchedArena

    a = alphabeta.AlphaBetaPlayer(2, exact_empties=4, device="cpu")
    b = alphabeta.AlphaBetaPlayer(1, exact_empties=0, device="cpu")
    ops = alphabeta.openings(8, 6, 0)
    arena = BatchedArena(a, b, {"num_simulations": 1, "c_puct": 2.0}, 16)
    wa, wb, dr, plies, recs = arena.play(16, openings=ops, record=True)
    assert wa + wb + dr == 16 and len(plies) == len(recs) == 16
    checks = [expect_alphabeta_move(2, 4), expect_alphabeta_move(1, 0)]
    results = []
    for g, rec in enumerate(recs):
        assert rec["a_first"] == (g % 2 == 0)  # colours alternate by match index
        assert (rec["own"], rec["opp"], rec["player"]) == \
            (int(ops[0][g // 2]), int(ops[1][g // 2]), int(ops[2][g // 2]))
        n, res = replay(rec, lambda side, o, p, act: checks[side](o, p, act))
        assert n == plies[g] and res == rec["result"]
        results.append(res)
    assert (wa, wb, dr) == (results.count(1), results.count(-1), results.count(0))
    # too few openings
    with pytest.raises(ValueError):
        arena.play(18, openings=ops)
    # levels
    lv = alphabeta.AlphaBetaPlayer.level(3)
    assert (lv.depth, lv.exact_empties) == (3, 6)
    assert alphabeta.AlphaBetaPlayer.level(8).exact_empties == 12
    for bad in (0, 9):
        with pytest.raises(ValueError):
            alphabeta.AlphaBetaPlayer.level(bad)
    with pytest.raises(ValueError):
        alphabeta.AlphaBetaPlayer(3, exact_empties=13)
    with pytest.raises(ValueError):
        alphabeta.AlphaBetaPlayer(11)


def test_player_raises_on_aborted_search(corpus, monkeypatch):
    import alphabeta

    i = np.flatnonzero(corpus["emp"] == 30)[:4]
    real = alphabeta.search
    monkeypatch.setattr(alphabeta, "search",
                        lambda o, p, d, device=None: real(o, p, d, device=device, node_limit=5))
    with pytest.raises(RuntimeError, match="node limit"):
        alphabeta.AlphaBetaPlayer(3, device="cpu").moves(corpus["own"][i], corpus["opp"][i])
