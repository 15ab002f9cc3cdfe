"""Windowed, move-ordered endgame solver on the host (oth_solve_deep_cpu, csrc/solve_deep.h)
and the Python surface on top of it (endgame.solve_deep, relabel_rows(wld=True), move_report
and collect_self_play_games beyond 14 empties).

The reference is oth_solve_cpu, which tests/test_solve_cpu.py proves exact; beyond its cap the
win / draw / loss of a position must be the best of its oracle-made children's.  No GPU."""
import numpy as np
import pytest

from test_solve_cpu import children, popc
from conftest import load_golden

nat = pytest.importorskip("az_native")

WINDOWS = [(-1, 1), (0, 1), (-64, -63)]


@pytest.fixture(scope="module")
def corpus():
    d = load_golden("board_corpus.npz")
    own = np.where(d["player"] == 1, d["pos"], d["neg"]).astype(np.uint64)
    opp = np.where(d["player"] == 1, d["neg"], d["pos"]).astype(np.uint64)
    return own, opp, 64 - popc(own | opp)


@pytest.fixture(scope="module")
def late(corpus):
    """Every corpus position with 1..10 empties, the proven solver's results, every child of
    every position with its exact score, and the deep solver's full-window results."""
    import endgame

    own, opp, emp = corpus
    m = (emp >= 1) & (emp <= 10)
    own, opp = own[m], opp[m]
    assert 6000 < len(own) < 6600
    s, b, nd = endgame.solve(own, opp, 10, device="cpu")
    par, act, co, cp, term = children(own, opp)
    cs = endgame.solve(co, cp, 10, device="cpu")[0].astype(np.int64)
    ds, db, dn = nat.solve_deep_cpu(own, opp, 10)
    return {"own": own, "opp": opp, "emp": emp[m], "score": s.astype(np.int64), "best": b,
            "nodes": nd, "par": par, "act": act, "child_score": cs, "term": term,
            "lg": nat.legal_cpu(own, opp), "deep": (ds, db, dn)}


def child_value(late, best):
    """Exact value (the root's view) of action best[i] at root i; None-free: roots whose best
    is not one of their children's actions fail the assertion."""
    n = len(late["own"])
    table = np.full((n, 65), 1000, np.int64)
    table[late["par"], late["act"]] = -late["child_score"]
    v = table[np.arange(n), np.minimum(best, 64)]
    return v


def check_contract(v, s, alpha, beta):
    """The three cases of the window contract, v and s int64 arrays, alpha / beta arrays or
    scalars."""
    v, s = np.asarray(v, np.int64), np.asarray(s, np.int64)
    inside = (alpha < s) & (s < beta)
    high = s >= beta
    low = s <= alpha
    assert (v[inside] == s[inside]).all()
    assert ((np.broadcast_to(beta, s.shape)[high] <= v[high]) & (v[high] <= s[high])).all()
    assert ((s[low] <= v[low]) & (v[low] <= np.broadcast_to(alpha, s.shape)[low])).all()


def test_full_window_scores_1_to_10(late):
    ds, db, dn = late["deep"]
    assert (ds == late["score"]).all()
    assert (dn >= 1).all()


def test_full_window_scores_12(corpus):
    import endgame

    own, opp, emp = corpus
    i = np.flatnonzero(emp == 12)[:64]
    want = endgame.solve(own[i], opp[i], 12, device="cpu")[0]
    got = endgame.solve_deep(own[i], opp[i], 12, device="cpu")[0]
    assert (want > -127).all() and (got == want).all()


@pytest.mark.slow
def test_full_window_scores_14(corpus):
    import endgame

    own, opp, emp = corpus
    i = np.flatnonzero(emp == 14)[:8]
    want = endgame.solve(own[i], opp[i], 14, device="cpu")[0]
    got = endgame.solve_deep(own[i], opp[i], 14, device="cpu")[0]
    assert (want > -127).all() and (got == want).all()
    wld = endgame.solve_deep(own[i], opp[i], 14, window="wld", device="cpu")[0]
    assert (np.sign(wld.astype(np.int64)) == np.sign(want.astype(np.int64))).all()


def test_best_is_optimal(late):
    ds, db, dn = late["deep"]
    has = late["lg"] != 0
    assert (db[~has] == 64).all() and (~has).sum() > 0
    assert (db[has] < 64).all()
    assert (((late["lg"][has] >> db[has].astype(np.uint64)) & np.uint64(1)) == 1).all()
    assert (child_value(late, db)[has] == late["score"][has]).all()


def windowed(late, alpha, beta):
    """solve_deep_cpu with one window per position (grouped by window)."""
    n = len(late["own"])
    alpha = np.broadcast_to(alpha, n)
    beta = np.broadcast_to(beta, n)
    v = np.empty(n, np.int8)
    b = np.empty(n, np.uint8)
    code = (alpha + 65) * 256 + (beta + 65)
    for c in np.unique(code):
        m = code == c
        a0, b0 = int(alpha[m][0]), int(beta[m][0])
        v[m], b[m], _ = nat.solve_deep_cpu(late["own"][m], late["opp"][m], 10, a0, b0)
    return v.astype(np.int64), b


def check_window(late, alpha, beta):
    v, b = windowed(late, alpha, beta)
    s = late["score"]
    check_contract(v, s, alpha, beta)
    has = late["lg"] != 0
    assert (b[~has] == 64).all()
    assert (((late["lg"][has] >> (b[has] & 63).astype(np.uint64)) & np.uint64(1)) == 1).all()
    assert (b[has] < 64).all()
    cv = child_value(late, b)
    high = has & (v >= beta)
    assert (cv[high] >= np.broadcast_to(beta, len(s))[high]).all()
    exact = has & (alpha < v) & (v < beta)
    assert (cv[exact] == s[exact]).all()
    return v


def test_window_contract_random(late):
    rng = np.random.default_rng(2024)
    n = len(late["own"])
    alpha = rng.integers(-64, 64, n)          # -64..63
    beta = alpha + 1 + rng.integers(0, 8, n)  # narrow windows near alpha, ...
    wide = rng.random(n) < 0.5
    beta = np.where(wide, rng.integers(alpha + 1, 65), beta)  # ... and any beta up to 64
    beta = np.minimum(beta, 64)
    assert (alpha < beta).all() and alpha.min() == -64 and beta.max() == 64
    v = check_window(late, alpha, beta)
    s = late["score"]
    assert ((s >= beta).sum() > 100) and ((s <= alpha).sum() > 100)
    assert (((alpha < s) & (s < beta)).sum() > 100)
    assert (v != s).any()  # fail-soft bounds that are not the score do occur


@pytest.mark.parametrize("window", WINDOWS)
def test_window_contract_fixed(late, window):
    check_window(late, *window)


def test_wld_sign(late, corpus):
    import endgame

    v, _ = windowed(late, -1, 1)
    assert (np.sign(v) == np.sign(late["score"])).all()
    assert {-1, 0, 1} <= set(np.sign(v))
    own, opp, emp = corpus
    i = np.flatnonzero(emp == 12)[:64]
    want = endgame.solve(own[i], opp[i], 12, device="cpu")[0].astype(np.int64)
    got = endgame.solve_deep(own[i], opp[i], 12, window="wld", device="cpu")[0].astype(np.int64)
    assert (np.sign(got) == np.sign(want)).all()


@pytest.mark.parametrize("e", [15, 16])
def test_one_ply_induction_beyond_old_cap(corpus, e):
    """sign(root) in win / draw / loss mode = max over the oracle-made children of
    -sign(child), the children solved at one empty fewer; a pass-only root is the negation
    of the position after the pass (as in test_solve_cpu.one_ply)."""
    import endgame
    from oracle import board as ob

    own, opp, emp = corpus
    idx = np.flatnonzero(emp == e)
    i = idx[::max(1, len(idx) // 16)][:16]
    assert len(i) == 16
    own, opp = own[i], opp[i]
    root = endgame.solve_deep(own, opp, e, window="wld", device="cpu")[0].astype(np.int64)
    assert (root > -127).all()
    lg, lg2 = ob.legal_batch(own, opp), ob.legal_batch(opp, own)
    passer = (lg == 0) & (lg2 != 0)
    o, p = np.where(passer, opp, own), np.where(passer, own, opp)
    par, act, co, cp, term = children(o, p)
    assert (act < 64).all() and not term.any()
    cs = endgame.solve_deep(co, cp, e - 1, window="wld", device="cpu")[0].astype(np.int64)
    assert (cs > -127).all()
    want = np.full(len(o), -2, np.int64)
    np.maximum.at(want, par, -np.sign(cs))
    want = np.where(passer, -want, want)
    assert (np.sign(root) == want).all()


def test_d4_invariance(corpus):
    own, opp, emp = corpus
    m = emp == 10
    own, opp = own[m], opp[m]
    base, _, _ = nat.solve_deep_cpu(own, opp, 10)
    for sym in range(1, 8):
        so, sp = nat.d4_cpu(own, sym), nat.d4_cpu(opp, sym)
        s, b, _ = nat.solve_deep_cpu(so, sp, 10)
        assert (s == base).all()
        lg = nat.legal_cpu(so, sp)
        ok = np.where(b == 64, lg == 0, ((lg >> (b & 63).astype(np.uint64)) & np.uint64(1)) == 1)
        assert ok.all()


def test_node_reduction_at_12_empties(corpus):
    """Deterministic: total nodes over all 605 corpus positions with 12 empties against the
    parent's solver in the same test.  Full window <= 1/3, win / draw / loss <= 1/10."""
    import endgame

    own, opp, emp = corpus
    m = emp == 12
    assert m.sum() == 605
    s0, _, n0 = endgame.solve(own[m], opp[m], 12, device="cpu")
    s1, _, n1 = endgame.solve_deep(own[m], opp[m], 12, device="cpu")
    s2, _, n2 = endgame.solve_deep(own[m], opp[m], 12, window="wld", device="cpu")
    assert (s1 == s0).all()
    assert (np.sign(s2.astype(np.int64)) == np.sign(s0.astype(np.int64))).all()
    t0, t1, t2 = int(n0.sum()), int(n1.sum()), int(n2.sum())
    print(f"12 empties, 605 positions: solve {t0} nodes, solve_deep full window {t1} "
          f"(1/{t0 / t1:.1f}), wld {t2} (1/{t0 / t2:.1f})")
    assert 3 * t1 <= t0
    assert 10 * t2 <= t0


def test_conventions(corpus):
    own, opp, emp = corpus
    lg, lg2 = nat.legal_cpu(own, opp), nat.legal_cpu(opp, own)
    passer = np.flatnonzero((emp <= 10) & (lg == 0) & (lg2 != 0))
    assert len(passer)
    d = load_golden("board_corpus.npz")
    end = d["term_next"] == 1
    town = np.where(d["player"] == 1, d["nneg"], d["npos"])[end].astype(np.uint64)
    topp = np.where(d["player"] == 1, d["npos"], d["nneg"])[end].astype(np.uint64)
    for window in [(-65, 65), (-1, 1)]:
        s, b, n = nat.solve_deep_cpu(town, topp, 20, *window)
        assert (s == popc(town) - popc(topp)).all() and (b == 64).all() and (n == 1).all()
        s, b, _ = nat.solve_deep_cpu(own[passer], opp[passer], 10, *window)
        assert (b == 64).all() and (s > -127).all()
    want = nat.solve_cpu(own[passer], opp[passer], 10)[0]
    assert (nat.solve_deep_cpu(own[passer], opp[passer], 10)[0] == want).all()
    # more empties than max_empties, overlapping boards: skipped, no work
    i8 = np.flatnonzero(emp == 8)[:5]
    s, b, n = nat.solve_deep_cpu(own[i8], opp[i8], 7)
    assert (s == -128).all() and (b == 255).all() and (n == 0).all()
    s, b, n = nat.solve_deep_cpu(own[i8] | opp[i8], opp[i8], 20)
    assert (s == -128).all() and (b == 255).all()
    # a mixed batch reads back as a mask
    i3 = np.flatnonzero(emp == 3)[:5]
    s, _, _ = nat.solve_deep_cpu(np.concatenate([own[i8], own[i3]]),
                                 np.concatenate([opp[i8], opp[i3]]), 4)
    assert ((s == -128) == np.array([True] * 5 + [False] * 5)).all()
    # the node limit
    s, b, n = nat.solve_deep_cpu(own[i8], opp[i8], 8, node_limit=10)
    assert (s == -127).all() and (b == 255).all()
    # n = 0, and nodes_o = NULL
    s, b, n = nat.solve_deep_cpu(np.zeros(0, np.uint64), np.zeros(0, np.uint64), 12)
    assert len(s) == 0
    f = nat.lib.oth_solve_deep_cpu
    assert f(None, None, 0, 12, -65, 65, 100, None, None, None) == nat.AZ_OK
    out8, outu = np.zeros(1, np.int8), np.zeros(1, np.uint8)
    assert f(nat.ptr(own[i3]), nat.ptr(opp[i3]), 1, 12, -65, 65, 1 << 20, nat.ptr(out8),
             nat.ptr(outu), None) == nat.AZ_OK
    assert out8[0] == nat.solve_cpu(own[i3[:1]], opp[i3[:1]], 12)[0][0]
    # bad arguments
    buf = np.zeros(1, np.uint64)
    q = lambda me, a, b: f(nat.ptr(buf), nat.ptr(buf), 1, me, a, b, 100, nat.ptr(out8),
                           nat.ptr(outu), None)
    assert q(20, -65, 65) == nat.AZ_OK
    assert q(21, -65, 65) == nat.AZ_ERR_ARG
    assert q(-1, -65, 65) == nat.AZ_ERR_ARG
    assert q(12, 0, 0) == nat.AZ_ERR_ARG
    assert q(12, 1, -1) == nat.AZ_ERR_ARG
    assert q(12, -66, 0) == nat.AZ_ERR_ARG
    assert q(12, 0, 66) == nat.AZ_ERR_ARG
    assert f(nat.ptr(buf), nat.ptr(buf), -1, 12, -65, 65, 100, nat.ptr(out8), nat.ptr(outu),
             None) == nat.AZ_ERR_ARG
    with pytest.raises(RuntimeError, match="max_empties"):
        nat.solve_deep_cpu(own[i8], opp[i8], 21)
    with pytest.raises(RuntimeError, match="window"):
        nat.solve_deep_cpu(own[i8], opp[i8], 12, 3, 3)


def test_solve_deep_threads_match_single_call(late):
    import endgame

    for window, ab in [(None, (-65, 65)), ("wld", (-1, 1)), ((-3, 5), (-3, 5))]:
        s, b, n = endgame.solve_deep(late["own"], late["opp"], 10, window=window, device="cpu")
        s1, b1, n1 = nat.solve_deep_cpu(late["own"], late["opp"], 10, *ab)
        assert s.dtype == np.int8 and b.dtype == np.uint8 and n.dtype == np.uint64
        assert (s == s1).all() and (b == b1).all() and (n == n1).all()
    with pytest.raises(ValueError):
        endgame.solve_deep(late["own"], late["opp"], 10, window="exact", device="cpu")
    with pytest.raises(RuntimeError, match="window"):
        endgame.solve_deep(late["own"], late["opp"], 10, window=(2, 2), device="cpu")
    import torch

    o_t = torch.from_numpy(late["own"][:50].view(np.int64))
    p_t = torch.from_numpy(late["opp"][:50].view(np.int64))
    st, bt, nt = endgame.solve_deep(o_t, p_t, 10, device="cpu")
    assert st.dtype == torch.int8 and (st.numpy() == late["deep"][0][:50]).all()
    assert (nt.numpy().view(np.uint64) == late["deep"][2][:50]).all()


def deep_rows(corpus):
    """make_rows-style rows up to 10 empties plus eight rows each at 15 and 16 empties."""
    own, opp, emp = corpus
    lg = nat.legal_cpu(own, opp)
    late = np.flatnonzero((emp >= 1) & (emp <= 10) & (lg != 0))[::3]
    deep = np.concatenate([np.flatnonzero((emp == e) & (lg != 0))[:8] for e in (15, 16)])
    early = np.flatnonzero(emp >= 20)[:100]
    idx = np.random.default_rng(5).permutation(np.concatenate([late, deep, early]))
    pi = np.zeros((len(idx), 65), np.float32)
    pi[:, 64] = 1.0
    z = np.random.default_rng(6).uniform(-1, 1, len(idx))
    return {"own": own[idx], "opp": opp[idx], "pi": pi, "z": z,
            "player": np.ones(len(idx), np.int8)}, emp[idx]


def test_relabel_rows_wld(corpus):
    import endgame

    rows, emp = deep_rows(corpus)
    z0 = rows["z"].copy()
    a, ma = endgame.relabel_rows(rows, 10, device="cpu")
    b, mb = endgame.relabel_rows(rows, 10, device="cpu", wld=True)
    assert (ma == mb).all() and ma.sum() > 1000 and (a["z"] == b["z"]).all()
    assert (ma == ((emp >= 1) & (emp <= 10))).all()
    c, mc = endgame.relabel_rows(rows, 16, device="cpu", wld=True)
    assert (mc == ((emp >= 1) & (emp <= 16))).all() and (mc & ~ma).sum() == 16
    assert (c["z"][ma] == a["z"][ma]).all()
    extra = mc & ~ma
    s, _, _ = endgame.solve_deep(rows["own"][extra], rows["opp"][extra], 16, device="cpu")
    assert (c["z"][extra] == np.sign(s.astype(np.int64))).all()
    assert (c["z"][~mc] == z0[~mc]).all() and (rows["z"] == z0).all()
    for k in ("own", "opp", "pi", "player"):
        assert c[k] is rows[k]
    with pytest.raises(RuntimeError, match="max_empties"):
        endgame.relabel_rows(rows, 16, device="cpu")  # the exact path keeps its cap


def test_collect_self_play_games_exact_endgame_16(corpus, monkeypatch):
    import endgame
    import self_play_worker as spw

    rows, emp = deep_rows(corpus)
    monkeypatch.setattr(spw, "_local_rows",
                        lambda *a, **k: {k_: v.copy() for k_, v in rows.items()})
    base = spw.collect_self_play_games(None, {"num_simulations": 4}, 5)
    on6 = spw.collect_self_play_games(None, {"num_simulations": 4}, 5, exact_endgame=6)
    on16 = spw.collect_self_play_games(None, {"num_simulations": 4}, 5, exact_endgame=16)
    want6 = endgame.relabel_rows(rows, 6, device="cpu")[0]["z"]
    m16 = (emp >= 1) & (emp <= 16)
    s16 = endgame.solve_deep(rows["own"][m16], rows["opp"][m16], 16, device="cpu")[0]
    want16 = rows["z"].copy()
    want16[m16] = np.sign(s16.astype(np.int64))
    assert len(base) == len(on6) == len(on16) == len(emp)
    assert (emp == 16).sum() == 8 and (want16 != rows["z"]).sum() > (want6 != rows["z"]).sum()
    for i, (a, b, c) in enumerate(zip(base, on6, on16)):
        assert (a[0] == b[0]).all() and (a[1] == b[1]).all() and a[2] == rows["z"][i]
        assert (a[0] == c[0]).all() and (a[1] == c[1]).all()
        assert b[2] == want6[i] and c[2] == want16[i]


def test_move_report_16(corpus):
    import endgame

    own, opp, emp = corpus
    lg = nat.legal_cpu(own, opp)
    idx = np.concatenate([np.flatnonzero((emp == e) & (lg != 0))[:n]
                          for e, n in ((3, 20), (9, 20), (15, 4), (16, 4))])
    o, p = own[idx], opp[idx]
    score, best, _ = endgame.solve_deep(o, p, 16, device="cpu")
    pi = np.zeros((len(idx), 65), np.float32)
    pi[np.arange(len(idx)), best] = 1.0
    rows = {"own": o, "opp": p, "pi": pi, "z": np.zeros(len(idx)),
            "player": np.ones(len(idx), np.int8)}
    rep = endgame.move_report(rows, 16, device="cpu")
    assert rep["total"]["n"] == len(idx) and rep["by_empties"][16]["n"] == 4
    assert sorted(rep["by_empties"]) == list(range(1, 17))
    assert rep["total"]["optimal_frac"] == 1.0 and rep["total"]["mean_disc_loss"] == 0.0
