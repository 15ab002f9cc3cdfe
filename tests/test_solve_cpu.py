"""Exact endgame solver on the host (oth_solve_cpu, csrc/solve.h) and the Python surface on
top of it (endgame.py, OthelloGameNew.solve, collect_self_play_games' exact_endgame).

Exactness is proved by induction over the empties count: every corpus position with 1..6
empties is compared with an unpruned minimax built from the oracle's verified batched step,
and for 7..10 empties a position's score must be the best of its children's scores, the
children made by the oracle and solved at one empty fewer.  No GPU."""
import numpy as np
import pytest

from conftest import load_golden
from oracle import board as ob

nat = pytest.importorskip("az_native")

_SH = np.arange(64, dtype=np.uint64)


def popc(x):
    x = np.ascontiguousarray(x, np.uint64)
    return np.unpackbits(x.view(np.uint8).reshape(-1, 8), axis=1).sum(axis=1).astype(np.int64)


@pytest.fixture(scope="module")
def corpus():
    d = load_golden("board_corpus.npz")
    own = np.where(d["player"] == 1, d["pos"], d["neg"]).astype(np.uint64)
    opp = np.where(d["player"] == 1, d["neg"], d["pos"]).astype(np.uint64)
    return own, opp, 64 - popc(own | opp)


def children(own, opp):
    """Every child of every position through the oracle: (parent index, action, child own,
    child opp) with the placements of a position, or its single pass when it has none but
    the opponent has; and the terminal mask of the positions."""
    lg, lg2 = ob.legal_batch(own, opp), ob.legal_batch(opp, own)
    term = (lg == 0) & (lg2 == 0)
    par, act = np.nonzero(((lg[:, None] >> _SH) & np.uint64(1)).astype(bool))
    passers = np.flatnonzero((lg == 0) & ~term)
    par = np.concatenate([par, passers])
    act = np.concatenate([act, np.full(len(passers), 64)]).astype(np.uint8)
    co, cp, _, _, bad = ob.step_batch(own[par], opp[par], act)
    assert bad == -1
    return par, act, co, cp, term


def back_up(n, term, diff, par, act, child_value):
    """Negamax backup with the lowest-index argmax: key = (value + 64) * 256 + 255 - action."""
    key = np.full(n, -1, np.int64)
    if len(par):
        np.maximum.at(key, par, (64 - child_value) * 256 + 255 - act.astype(np.int64))
    assert (term | (key >= 0)).all()
    return np.where(term, diff, key // 256 - 64), np.where(term, 64, 255 - key % 256)


def brute_force(own, opp):
    """Unpruned level-by-level minimax to the end of every game."""
    levels = []
    o, p = own, opp
    while len(o):
        par, act, co, cp, term = children(o, p)
        levels.append((len(o), term, popc(o) - popc(p), par, act))
        o, p = co, cp
    value = best = None
    for n, term, diff, par, act in reversed(levels):
        value, best = back_up(n, term, diff, par, act, value)
    return value, best


def test_brute_force_1_to_6_empties(corpus):
    own, opp, emp = corpus
    m = (emp >= 1) & (emp <= 6)
    assert m.sum() == 3875
    own, opp = own[m], opp[m]
    lg = ob.legal_batch(own, opp)
    assert ((lg == 0) & (ob.legal_batch(opp, own) != 0)).sum() > 0  # pass-only roots included
    want_v, want_b = brute_force(own, opp)
    score, best, nodes = nat.solve_cpu(own, opp, 6)
    assert (score == want_v).all()
    assert (best == want_b).all()
    assert (nodes >= 1).all()


def one_ply(own, opp, e):
    """Score and best of positions with e empties from their children's solved scores; the
    children of a placement have e - 1 empties.  A pass-only position is the negation of the
    position after the pass, which has placements."""
    lg, lg2 = ob.legal_batch(own, opp), ob.legal_batch(opp, own)
    passer = (lg == 0) & (lg2 != 0)
    o = np.where(passer, opp, own)
    p = np.where(passer, own, opp)
    par, act, co, cp, term = children(o, p)
    assert (act < 64).all()
    cs, _, _ = nat.solve_cpu(co, cp, e - 1)
    assert (cs > -127).all()
    v, b = back_up(len(o), term, popc(o) - popc(p), par, act, cs.astype(np.int64))
    return np.where(passer, -v, v), np.where(passer, 64, b)


@pytest.mark.parametrize("e", [7, 8, 9, pytest.param(10, marks=pytest.mark.slow)])
def test_one_ply_consistency(corpus, e):
    own, opp, emp = corpus
    m = emp == e
    assert m.sum() >= 600
    own, opp = own[m], opp[m]
    score, best, _ = nat.solve_cpu(own, opp, e)
    want_v, want_b = one_ply(own, opp, e)
    assert (score == want_v).all()
    assert (best == want_b).all()


def test_d4_invariance(corpus):
    own, opp, emp = corpus
    m = emp == 8
    own, opp = own[m], opp[m]
    base, _, _ = nat.solve_cpu(own, opp, 8)
    for sym in range(1, 8):
        s, b, _ = nat.solve_cpu(nat.d4_cpu(own, sym), nat.d4_cpu(opp, sym), 8)
        assert (s == base).all()
        lg = nat.legal_cpu(nat.d4_cpu(own, sym), nat.d4_cpu(opp, sym))
        ok = np.where(b == 64, lg == 0, ((lg >> (b & 63).astype(np.uint64)) & np.uint64(1)) == 1)
        assert ok.all()


def test_conventions(corpus):
    own, opp, emp = corpus
    lg, lg2 = nat.legal_cpu(own, opp), nat.legal_cpu(opp, own)
    late = emp <= 10
    passer = np.flatnonzero(late & (lg == 0) & (lg2 != 0))
    assert len(passer)
    # terminal roots: the corpus games' final positions (the side that would move next)
    d = load_golden("board_corpus.npz")
    end = d["term_next"] == 1
    town = np.where(d["player"] == 1, d["nneg"], d["npos"])[end].astype(np.uint64)
    topp = np.where(d["player"] == 1, d["npos"], d["nneg"])[end].astype(np.uint64)
    assert len(town) >= 600 and (64 - popc(town | topp)).max() > 0
    s, b, n = nat.solve_cpu(town, topp, 14)
    assert (s == popc(town) - popc(topp)).all() and (b == 64).all() and (n == 1).all()
    s, b, _ = nat.solve_cpu(own[passer], opp[passer], 10)
    assert (b == 64).all() and (s > -127).all()
    # more empties than max_empties, overlapping boards: skipped, no work
    i8 = np.flatnonzero(emp == 8)[:5]
    s, b, n = nat.solve_cpu(own[i8], opp[i8], 7)
    assert (s == -128).all() and (b == 255).all() and (n == 0).all()
    s, b, n = nat.solve_cpu(own[i8] | opp[i8], opp[i8], 14)
    assert (s == -128).all() and (b == 255).all()
    # a mixed batch reads back as a mask
    i3 = np.flatnonzero(emp == 3)[:5]
    s, _, _ = nat.solve_cpu(np.concatenate([own[i8], own[i3]]), np.concatenate([opp[i8], opp[i3]]), 4)
    assert ((s == -128) == np.array([True] * 5 + [False] * 5)).all()
    # the hard cap
    with pytest.raises(RuntimeError, match="max_empties"):
        nat.solve_cpu(own[i8], opp[i8], 15)
    buf = np.zeros(1, np.uint64)
    out8, outu = np.zeros(1, np.int8), np.zeros(1, np.uint8)
    assert nat.lib.oth_solve_cpu(nat.ptr(buf), nat.ptr(buf), 1, 15, 100, nat.ptr(out8),
                                 nat.ptr(outu), None) == nat.AZ_ERR_ARG
    # the node limit
    s, b, n = nat.solve_cpu(own[i8], opp[i8], 8, node_limit=10)
    assert (s == -127).all()
    # n = 0, and nodes_o = NULL
    s, b, n = nat.solve_cpu(np.zeros(0, np.uint64), np.zeros(0, np.uint64), 12)
    assert len(s) == 0
    assert nat.lib.oth_solve_cpu(None, None, 0, 12, 100, None, None, None) == nat.AZ_OK
    assert nat.lib.oth_solve_cpu(nat.ptr(own[i3]), nat.ptr(opp[i3]), 1, 12, 1 << 20,
                                 nat.ptr(out8), nat.ptr(outu), None) == nat.AZ_OK
    assert out8[0] == nat.solve_cpu(own[i3[:1]], opp[i3[:1]], 12)[0][0]


def make_rows(corpus, seed=0):
    """Synthetic engine sample rows: every corpus position with 1..6 empties that has a
    placement, mixed with earlier positions, one-hot pi on the solver's best move."""
    own, opp, emp = corpus
    lg = nat.legal_cpu(own, opp)
    late = np.flatnonzero((emp >= 1) & (emp <= 6) & (lg != 0))
    early = np.flatnonzero(emp >= 20)[:300]
    idx = np.random.default_rng(seed).permutation(np.concatenate([late, early]))
    o, p = own[idx], opp[idx]
    score, best, _ = nat.solve_cpu(o, p, 6)
    pi = np.zeros((len(idx), 65), np.float32)
    solved = score > -127
    pi[np.flatnonzero(solved), best[solved]] = 1.0
    pi[~solved, 64] = 1.0
    z = np.random.default_rng(seed + 1).uniform(-1, 1, len(idx))
    rows = {"own": o, "opp": p, "pi": pi, "z": z, "player": np.ones(len(idx), np.int8)}
    return rows, score, solved


def test_relabel_rows(corpus):
    import endgame

    rows, score, solved = make_rows(corpus)
    z0 = rows["z"].copy()
    out, mask = endgame.relabel_rows(rows, 6, device="cpu")
    assert (mask == solved).all() and mask.sum() > 3000 and (~mask).sum() == 300
    assert (out["z"][mask] == np.sign(score[mask].astype(np.int64))).all()
    assert set(np.unique(out["z"][mask])) <= {-1.0, 0.0, 1.0}
    assert (out["z"][~mask] == z0[~mask]).all()
    assert (rows["z"] == z0).all()  # the input rows are not written
    for k in ("own", "opp", "pi", "player"):
        assert out[k] is rows[k]
    # a smaller bound relabels fewer rows
    _, mask3 = endgame.relabel_rows(rows, 3, device="cpu")
    assert 0 < mask3.sum() < mask.sum() and (mask3 <= mask).all()


def test_move_report(corpus):
    import endgame

    rows, score, solved = make_rows(corpus)
    rep = endgame.move_report(rows, 6, device="cpu")
    assert rep["total"]["n"] == solved.sum()
    assert sum(v["n"] for v in rep["by_empties"].values()) == solved.sum()
    assert sorted(rep["by_empties"]) == [1, 2, 3, 4, 5, 6]
    for st in [rep["total"]] + list(rep["by_empties"].values()):
        assert st["optimal_frac"] == 1.0 and st["wld_kept_frac"] == 1.0
        assert st["mean_disc_loss"] == 0.0
    # one-hot pi on the worst placement of every late row
    o, p = rows["own"][solved], rows["opp"][solved]
    par, act, co, cp, term = children(o, p)
    assert not term.any() and (act < 64).all()
    cs = nat.solve_cpu(co, cp, 6)[0].astype(np.int64)
    key = np.full(len(o), 1 << 20, np.int64)
    np.minimum.at(key, par, (64 - cs) * 256 + act)
    worst_v, worst_a = key // 256 - 64, key % 256
    pi = np.zeros((len(o), 65), np.float32)
    pi[np.arange(len(o)), worst_a] = 1.0
    bad = {"own": o, "opp": p, "pi": pi, "z": np.zeros(len(o)), "player": np.ones(len(o), np.int8)}
    rep = endgame.move_report(bad, 6, device="cpu")
    loss = score[solved].astype(np.int64) - worst_v
    assert (loss >= 0).all() and loss.max() > 0
    assert rep["total"]["mean_disc_loss"] == pytest.approx(loss.mean(), abs=1e-12)
    assert rep["total"]["optimal_frac"] == pytest.approx((loss == 0).mean(), abs=1e-12)
    assert rep["total"]["wld_kept_frac"] == pytest.approx(
        (np.sign(worst_v) == np.sign(score[solved])).mean(), abs=1e-12)


def test_endgame_solve_threads_match_single_call(corpus):
    import endgame

    own, opp, emp = corpus
    m = emp <= 8
    s, b, n = endgame.solve(own[m], opp[m], 8, device="cpu")
    s1, b1, n1 = nat.solve_cpu(own[m], opp[m], 8)
    assert s.dtype == np.int8 and b.dtype == np.uint8 and n.dtype == np.uint64
    assert (s == s1).all() and (b == b1).all() and (n == n1).all()


def test_game_solve(corpus):
    from envs.othello import OthelloGameNew

    g = OthelloGameNew(8)
    own, opp, emp = corpus
    idx = np.flatnonzero((emp >= 1) & (emp <= 8))[::97]
    score, best, _ = nat.solve_cpu(own[idx], opp[idx], 8)
    for i, sc, b in zip(idx, score, best):
        for player in (1, -1):
            state = nat.unpack_np(own[i:i + 1], opp[i:i + 1], player)[0]
            assert g.solve(state, player, max_empties=8) == (int(sc), int(b))
            assert g.solve(state, -player, max_empties=8)[0] == \
                int(nat.solve_cpu(opp[i:i + 1], own[i:i + 1], 8)[0][0])
    with pytest.raises(ValueError):
        g.solve(g.get_initial_state(), 1)


def test_collect_self_play_games_exact_endgame(corpus, monkeypatch):
    """exact_endgame = 0 is today's path; E > 0 changes only z of the rows with 1..E empties."""
    import self_play_worker as spw

    rows, score, solved = make_rows(corpus, seed=3)
    monkeypatch.setattr(spw, "_local_rows", lambda *a, **k: {k_: v.copy() for k_, v in rows.items()})
    base = spw.collect_self_play_games(None, {"num_simulations": 4}, 5)
    off = spw.collect_self_play_games(None, {"num_simulations": 4}, 5, exact_endgame=0)
    on = spw.collect_self_play_games(None, {"num_simulations": 4}, 5, exact_endgame=6)
    assert len(base) == len(off) == len(on) == len(rows["z"])
    for i, (a, b, c) in enumerate(zip(base, off, on)):
        assert (a[0] == b[0]).all() and (a[1] == b[1]).all() and a[2] == b[2] == rows["z"][i]
        assert (a[0] == c[0]).all() and (a[1] == c[1]).all()
        assert c[2] == (float(np.sign(int(score[i]))) if solved[i] else rows["z"][i])
