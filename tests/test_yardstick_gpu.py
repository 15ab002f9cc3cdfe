"""The arena against the alpha-beta yardstick on the device: one side is an MCTS engine (rollout
or net evaluation), the other an AlphaBetaPlayer; every recorded match is replayed on the
host, where each alpha-beta action must be the host search's or solver's move and each
engine action a legal one."""
import numpy as np
import pytest

from test_search_cpu import expect_alphabeta_move, replay

nat = pytest.importorskip("az_native")
pytestmark = pytest.mark.gpu

ARGS = {"c_puct": 2.0, "num_simulations": 16}


def legal_move(own, opp, a):
    lg = int(nat.legal_cpu(own, opp)[0])
    assert (lg >> a) & 1 if a < 64 else lg == 0


def check_records(arena, out, ops, ab_side):
    wa, wb, dr, plies, recs = out
    assert wa + wb + dr == 16 and len(plies) == len(recs) == 16
    checks = [legal_move, legal_move]
    checks[ab_side] = expect_alphabeta_move(2, 6)
    results = []
    for g, rec in enumerate(recs):
        assert rec["a_first"] == (g % 2 == 0)
        assert (rec["own"], rec["opp"], rec["player"]) == \
            (int(ops[0][g // 2]), int(ops[1][g // 2]), int(ops[2][g // 2]))
        n, res = replay(rec, lambda side, o, p, act: checks[side](o, p, act))
        assert n == plies[g] and res == rec["result"]
        results.append(res)
    assert (wa, wb, dr) == (results.count(1), results.count(-1), results.count(0))
    assert arena.eng[ab_side] is None
    assert arena.eng[1 - ab_side].counters()["arena_overflows"] == 0


@pytest.mark.parametrize("ab_side", [1, 0])
def test_arena_against_the_search(ab_side):
    import alphabeta
    from arena import BatchedArena

    ops = alphabeta.openings(8, 6, 0)
    sides = [None, None]  # the net side is the rollout engine
    sides[ab_side] = alphabeta.AlphaBetaPlayer(2, exact_empties=6)
    arena = BatchedArena(sides[0], sides[1], dict(ARGS), 16)
    check_records(arena, arena.play(16, openings=ops, record=True), ops, ab_side)


def test_ladder_on_a_random_net():
    from arena import ladder
    from Models import FastOthelloNet

    out = ladder(FastOthelloNet(8, 65).eval(), dict(ARGS), (1, 2), 8, plies=6, n_slots=8)
    assert sorted(out) == [1, 2]
    for r in out.values():
        assert r["wins"] + r["draws"] + r["losses"] == 8
        assert 0.0 <= r["score"] <= 1.0
        assert r["score"] == (r["wins"] + 0.5 * r["draws"]) / 8


def test_default_path_keeps_its_shape():
    from arena import BatchedArena

    out = BatchedArena(None, None, dict(ARGS), 4).play(4)
    assert len(out) == 4
    wa, wb, dr, plies = out
    assert wa + wb + dr == 4 and len(plies) == 4 and all(isinstance(p, int) for p in plies)
    # record alone: the initial position, no openings
    out = BatchedArena(None, None, dict(ARGS), 4).play(2, record=True)
    assert len(out) == 5 and [r["player"] for r in out[4]] == [1, 1]
    assert all(r["own"] == 0x0000000810000000 and len(r["actions"]) == p
               for r, p in zip(out[4], out[3]))
