"""The exact value of every move on the host (oth_solve_moves_cpu, csrc/solve_moves.hip) and
the Python surface on top of it: endgame.solve_moves / exact_policy / relabel_rows(policy=True)
/ policy_report, collect_self_play_games(exact_policy=True), OthelloGameNew.solve_moves.

The reference is an independent composition: the legal mask, the batched board step and the
first solver (endgame.solve, proven exact by tests/test_solve_cpu.py) on every child.  Node
counts are pinned to the windowed solver's own per-search counts.  No GPU."""
import numpy as np
import pytest

from conftest import load_golden

nat = pytest.importorskip("az_native")

NONE = -128
SCORES, WLD, OPTIMAL = 0, 1, 2
_SH = np.arange(64, dtype=np.uint64)


def popc(x):
    x = np.ascontiguousarray(x, np.uint64)
    return np.unpackbits(x.view(np.uint8).reshape(-1, 8), axis=1).sum(axis=1).astype(np.int64)


@pytest.fixture(scope="module")
def corpus():
    d = load_golden("board_corpus.npz")
    own = np.where(d["player"] == 1, d["pos"], d["neg"]).astype(np.uint64)
    opp = np.where(d["player"] == 1, d["neg"], d["pos"]).astype(np.uint64)
    end = d["term_next"] == 1
    town = np.where(d["player"] == 1, d["nneg"], d["npos"])[end].astype(np.uint64)
    topp = np.where(d["player"] == 1, d["npos"], d["nneg"])[end].astype(np.uint64)
    return {"own": own, "opp": opp, "emp": 64 - popc(own | opp), "town": town, "topp": topp}


def compose(own, opp):
    """(parent, action, child own, child opp) of every available action, by the legal mask and
    the batched board step."""
    lg = nat.legal_cpu(own, opp)
    passer = (lg == 0) & (nat.legal_cpu(opp, own) != 0)
    par, act = np.nonzero(((lg[:, None] >> _SH) & np.uint64(1)).astype(bool))
    par = np.concatenate([par, np.flatnonzero(passer)])
    act = np.concatenate([act, np.full(passer.sum(), 64)]).astype(np.uint8)
    co, cp, _, _ = nat.step_cpu(own[par], opp[par], act)
    return par, act, co, cp, passer


def windowed_nodes(co, cp, alpha, beta):
    """solve_deep_cpu's (score, nodes) per position with one window each (grouped by window)."""
    alpha, beta = np.broadcast_to(alpha, len(co)), np.broadcast_to(beta, len(co))
    v, nd = np.empty(len(co), np.int64), np.empty(len(co), np.uint64)
    code = (alpha + 65) * 256 + (beta + 65)
    for c in np.unique(code):
        m = code == c
        s, _, k = nat.solve_deep_cpu(co[m], cp[m], 20, int(alpha[m][0]), int(beta[m][0]))
        v[m], nd[m] = s, k
    return v, nd


@pytest.fixture(scope="module")
def late(corpus):
    """Every corpus position with 1..10 empties, the composed table of true move values, the
    first solver's root scores, and the three modes' host results."""
    import endgame

    m = (corpus["emp"] >= 1) & (corpus["emp"] <= 10)
    own, opp = corpus["own"][m], corpus["opp"][m]
    n = len(own)
    assert 6000 < n < 6600
    par, act, co, cp, passer = compose(own, opp)
    assert 200 < passer.sum() < 320
    cs = endgame.solve(co, cp, 10, device="cpu")[0].astype(np.int64)
    assert (cs > -127).all()
    table = np.full((n, 65), NONE, np.int64)
    table[par, act] = -cs
    score = endgame.solve(own, opp, 10, device="cpu")[0].astype(np.int64)
    got = {mode: nat.solve_moves_cpu(own, opp, 10, mode) for mode in (SCORES, WLD, OPTIMAL)}
    return {"own": own, "opp": opp, "emp": corpus["emp"][m], "par": par, "act": act, "co": co,
            "cp": cp, "table": table, "score": score, "got": got,
            "has": (table != NONE).any(axis=1)}


def sum_by_parent(n, par, x):
    out = np.zeros(n, np.uint64)
    np.add.at(out, par, x.astype(np.uint64))
    return out


def test_scores_against_composition(late):
    v, s, nd = late["got"][SCORES]
    assert v.dtype == np.int8 and v.shape == (len(late["own"]), 65) and s.dtype == np.int8
    assert nd.dtype == np.uint64
    assert (v.astype(np.int64) == late["table"]).all()
    has = late["has"]
    assert (~has).sum() < 40  # the few roots of the set at which the game is over
    assert (s[has] == late["score"][has]).all()
    _, cn = windowed_nodes(late["co"], late["cp"], -65, 65)
    assert (nd == 1 + sum_by_parent(len(s), late["par"], cn)).all()


def test_wld_is_the_sign_table(late):
    v, s, nd = late["got"][WLD]
    t = late["table"]
    assert (v.astype(np.int64) == np.where(t == NONE, NONE, np.sign(t))).all()
    has = late["has"]
    assert (s[has] == np.sign(late["score"][has])).all()
    assert {-1, 0, 1} <= set(s[has].tolist())
    _, cn = windowed_nodes(late["co"], late["cp"], -1, 1)
    assert (nd == 1 + sum_by_parent(len(s), late["par"], cn)).all()
    assert nd.sum() < late["got"][SCORES][2].sum()


def test_optimal_marks_exactly_the_optimal_moves(late):
    v, s, nd = late["got"][OPTIMAL]
    v, t, has = v.astype(np.int64), late["table"], late["has"]
    sc = late["score"]
    assert (s[has] == sc[has]).all()
    assert ((v == NONE) == (t == NONE)).all()
    avail = t != NONE
    best = avail & (t == sc[:, None])
    assert (best.sum(axis=1)[has] >= 1).all() and (best.sum(axis=1) > 1).mean() > 0.05
    assert (v[best] == np.broadcast_to(sc[:, None], v.shape)[best]).all()
    rest = avail & ~best
    bound = np.broadcast_to(sc[:, None] - 1, v.shape)
    assert ((t[rest] <= v[rest]) & (v[rest] <= bound[rest])).all()
    assert (v[rest] != t[rest]).any()  # bounds that are not the move's value do occur
    # nodes: 1 + the root search + every child in its window
    _, rn = nat.solve_deep_cpu(late["own"], late["opp"], 20)[::2]
    cw = sc[late["par"]]
    _, cn = windowed_nodes(late["co"], late["cp"], -cw - 1, -cw + 1)
    want = 1 + np.where(has, rn, 0).astype(np.uint64) + sum_by_parent(len(s), late["par"], cn)
    assert (nd == want).all()
    assert nd[has].sum() < late["got"][SCORES][2][has].sum()


def test_edge_roots(corpus, late):
    town, topp = corpus["town"], corpus["topp"]
    assert len(town) > 10
    for mode in (SCORES, WLD, OPTIMAL):
        v, s, nd = nat.solve_moves_cpu(town, topp, 20, mode)
        assert (v == NONE).all() and (s == popc(town) - popc(topp)).all() and (nd == 1).all()
        # more empties than max_empties, overlapping boards: skipped, no work
        i8 = np.flatnonzero(late["emp"] == 8)[:5]
        o, p = late["own"][i8], late["opp"][i8]
        v, s, nd = nat.solve_moves_cpu(o, p, 7, mode)
        assert (v == NONE).all() and (s == -128).all() and (nd == 0).all()
        v, s, nd = nat.solve_moves_cpu(o | p, p, 20, mode)
        assert (v == NONE).all() and (s == -128).all() and (nd == 0).all()
        # a mixed batch: only the rows within the bound are filled, and with the same bytes
        i3 = np.flatnonzero(late["emp"] == 3)[:5]
        v, s, nd = nat.solve_moves_cpu(np.concatenate([o, late["own"][i3]]),
                                       np.concatenate([p, late["opp"][i3]]), 4, mode)
        assert (s[:5] == -128).all() and (v[:5] == NONE).all()
        assert (v[5:] == late["got"][mode][0][i3]).all()
        assert (s[5:] == late["got"][mode][1][i3]).all()
        assert (nd[5:] == late["got"][mode][2][i3]).all()
        v, s, nd = nat.solve_moves_cpu(np.zeros(0, np.uint64), np.zeros(0, np.uint64), 12, mode)
        assert v.shape == (0, 65) and len(s) == 0 and len(nd) == 0
    f = nat.lib.oth_solve_moves_cpu
    assert f(None, None, 0, 12, SCORES, 100, None, None, None) == nat.AZ_OK
    # nodes_o = NULL
    i = np.flatnonzero(late["emp"] == 5)[:1]
    v, s = np.zeros((1, 65), np.int8), np.zeros(1, np.int8)
    assert f(nat.ptr(late["own"][i]), nat.ptr(late["opp"][i]), 1, 12, SCORES, 1 << 20, nat.ptr(v),
             nat.ptr(s), None) == nat.AZ_OK
    assert (v == late["got"][SCORES][0][i]).all() and s[0] == late["got"][SCORES][1][i[0]]


def limited_set(late):
    m = late["emp"] <= 8
    return m, late["own"][m], late["opp"][m]


@pytest.mark.parametrize("mode", [SCORES, WLD, OPTIMAL])
def test_node_limit(late, mode):
    """10 nodes per search at 1..8 empties: some roots abort, some finish."""
    m, own, opp = limited_set(late)
    v, s, nd = nat.solve_moves_cpu(own, opp, 8, mode, node_limit=10)
    ab = s == -127
    print(f"mode {mode}: {int(ab.sum())} of {len(s)} roots aborted at 10 nodes per search")
    assert 0 < ab.sum() < len(s)
    assert (v[ab] == NONE).all()
    fv, fs, fn = (x[m] for x in late["got"][mode])
    assert (v[~ab] == fv[~ab]).all() and (s[~ab] == fs[~ab]).all() and (nd[~ab] == fn[~ab]).all()
    assert (nd[ab] > 10).all()
    # the same bytes on a second run, and from the thread pool
    import endgame

    name = {SCORES: "scores", WLD: "wld", OPTIMAL: "optimal"}[mode]
    v2, s2, n2 = endgame.solve_moves(own, opp, 8, mode=name, device="cpu", node_limit=10)
    assert (v2 == v).all() and (s2 == s).all() and (n2 == nd).all()


def test_d4_symmetry(corpus):
    from train_gpu import pi_source_tables

    src = pi_source_tables()
    idx = np.flatnonzero((corpus["emp"] >= 1) & (corpus["emp"] <= 9))[::7]
    own, opp = corpus["own"][idx], corpus["opp"][idx]
    base = {mode: nat.solve_moves_cpu(own, opp, 9, mode) for mode in (SCORES, WLD, OPTIMAL)}
    for sym in range(1, 8):
        so, sp = nat.d4_cpu(own, sym), nat.d4_cpu(opp, sym)
        for mode in (SCORES, WLD):
            v, s, _ = nat.solve_moves_cpu(so, sp, 9, mode)
            assert (v == base[mode][0][:, src[sym]]).all() and (s == base[mode][1]).all()
        # "optimal": the bounds of the other moves depend on the move order; the optimal set
        # and the score do not
        v, s, _ = nat.solve_moves_cpu(so, sp, 9, OPTIMAL)
        bv, bs, _ = base[OPTIMAL]
        assert (s == bs).all()
        assert ((v == s[:, None]) == (bv == bs[:, None])[:, src[sym]]).all()
        assert ((v == NONE) == (bv == NONE)[:, src[sym]]).all()


def test_exact_policy(late):
    import endgame
    import torch

    for mode in (SCORES, WLD, OPTIMAL):
        v = late["got"][mode][0]
        pi = endgame.exact_policy(v)
        assert pi.dtype == np.float32 and pi.shape == v.shape
        has = late["has"]
        assert np.allclose(pi[has].sum(axis=1), 1.0, atol=1e-6) and (pi[~has] == 0).all()
        top = v.astype(np.int64).max(axis=1, keepdims=True)
        support = (v == top) & (v != NONE)
        assert ((pi > 0) == support).all()
        k = support.sum(axis=1, keepdims=True)
        assert (pi[support] == (1.0 / np.maximum(k, 1)).astype(np.float32).repeat(65, 1)[support]).all()
    # the optimal set is the same from "scores" and from "optimal"
    assert (endgame.exact_policy(late["got"][SCORES][0]) ==
            endgame.exact_policy(late["got"][OPTIMAL][0])).all()
    t = endgame.exact_policy(torch.from_numpy(late["got"][SCORES][0][:50]))
    assert t.dtype == torch.float32 and (t.numpy() == endgame.exact_policy(
        late["got"][SCORES][0][:50])).all()


def test_endgame_solve_moves_surface(late):
    import endgame
    import torch

    for name, mode in (("scores", SCORES), ("wld", WLD), ("optimal", OPTIMAL)):
        v, s, nd = endgame.solve_moves(late["own"], late["opp"], 10, mode=name, device="cpu")
        gv, gs, gn = late["got"][mode]
        assert v.dtype == np.int8 and s.dtype == np.int8 and nd.dtype == np.uint64
        assert (v == gv).all() and (s == gs).all() and (nd == gn).all()
    o_t = torch.from_numpy(late["own"][:50].view(np.int64))
    p_t = torch.from_numpy(late["opp"][:50].view(np.int64))
    v, s, nd = endgame.solve_moves(o_t, p_t, 10, device="cpu")
    assert v.dtype == torch.int8 and tuple(v.shape) == (50, 65)
    assert (v.numpy() == late["got"][SCORES][0][:50]).all()
    assert (nd.numpy().view(np.uint64) == late["got"][SCORES][2][:50]).all()
    with pytest.raises(ValueError, match="mode"):
        endgame.solve_moves(late["own"], late["opp"], 10, mode="best", device="cpu")
    with pytest.raises(RuntimeError, match="max_empties"):
        endgame.solve_moves(late["own"], late["opp"], 21, device="cpu")


def make_rows(corpus, late):
    """Engine-style rows: every third late position, 12 rows at 15 and 16 empties, 100 early
    ones and the corpus's finished games' last positions, shuffled; a searched-looking pi."""
    emp = corpus["emp"]
    lt = np.flatnonzero((emp >= 1) & (emp <= 10))[::3]
    deep = np.concatenate([np.flatnonzero(emp == e)[:6] for e in (15, 16)])
    early = np.flatnonzero(emp >= 20)[:100]
    own = np.concatenate([corpus["own"][np.concatenate([lt, deep, early])], corpus["town"]])
    opp = np.concatenate([corpus["opp"][np.concatenate([lt, deep, early])], corpus["topp"]])
    idx = np.random.default_rng(11).permutation(len(own))
    own, opp = own[idx], opp[idx]
    pi = np.random.default_rng(12).random((len(idx), 65)).astype(np.float32)
    pi /= pi.sum(axis=1, keepdims=True)
    z = np.random.default_rng(13).uniform(-1, 1, len(idx))
    rows = {"own": own, "opp": opp, "pi": pi, "z": z, "player": np.ones(len(idx), np.int8)}
    return rows, 64 - popc(own | opp)


@pytest.mark.parametrize("wld", [False, True])
def test_relabel_rows_policy(corpus, late, wld):
    import endgame

    rows, emp = make_rows(corpus, late)
    pi0, z0 = rows["pi"].copy(), rows["z"].copy()
    plain, pm = endgame.relabel_rows(rows, 10, device="cpu", wld=wld)
    assert plain["pi"] is rows["pi"]  # policy=False: today's path
    off, om = endgame.relabel_rows(rows, 10, device="cpu", wld=wld, policy=False)
    assert off["pi"] is rows["pi"] and (off["z"] == plain["z"]).all() and (om == pm).all()
    out, mask = endgame.relabel_rows(rows, 10, device="cpu", wld=wld, policy=True)
    assert (mask == pm).all() and (mask == ((emp >= 1) & (emp <= 10))).all()
    assert (out["z"] == plain["z"]).all()
    for k in ("own", "opp", "player"):
        assert out[k] is rows[k]
    assert out["pi"] is not rows["pi"] and out["pi"].dtype == pi0.dtype
    assert out["pi"].shape == pi0.shape
    assert (rows["pi"] == pi0).all() and (rows["z"] == z0).all()  # the input is not written
    assert (out["pi"][~mask] == pi0[~mask]).all()
    v, s, _ = nat.solve_moves_cpu(rows["own"][mask], rows["opp"][mask], 10, SCORES)
    v = v.astype(np.int64)
    has = (v != NONE).any(axis=1)
    assert 0 < (~has).sum() < 200  # rows at which the game is over keep their pi
    assert (out["pi"][mask][~has] == pi0[mask][~has]).all()
    good = np.sign(v) == np.sign(s.astype(np.int64))[:, None] if wld else v == s[:, None]
    good &= v != NONE
    want = (good / np.maximum(good.sum(axis=1, keepdims=True), 1)).astype(np.float32)
    assert (out["pi"][mask][has] == want[has]).all()
    # up to 20 empties in both settings
    out16, m16 = endgame.relabel_rows(rows, 16, device="cpu", wld=wld, policy=True)
    extra = m16 & ~mask
    assert extra.sum() == 12
    assert (out16["pi"][mask] == out["pi"][mask]).all() and (out16["z"][mask] == out["z"][mask]).all()
    sd = endgame.solve_deep(rows["own"][extra], rows["opp"][extra], 16, window="wld",
                            device="cpu")[0]
    assert (out16["z"][extra] == np.sign(sd.astype(np.int64))).all()
    assert np.allclose(out16["pi"][extra].sum(axis=1), 1.0, atol=1e-6)
    lg = nat.legal_cpu(rows["own"][extra], rows["opp"][extra])
    on = out16["pi"][extra][:, :64] > 0
    assert (on <= ((lg[:, None] >> _SH) & np.uint64(1)).astype(bool)).all()


def test_collect_self_play_games_exact_policy(corpus, late, monkeypatch):
    """exact_policy changes only pi and z of the rows with 1..E empties."""
    import endgame
    import self_play_worker as spw

    rows, emp = make_rows(corpus, late)
    monkeypatch.setattr(spw, "_local_rows", lambda *a, **k: {k_: v.copy() for k_, v in rows.items()})
    base = spw.collect_self_play_games(None, {"num_simulations": 4}, 5)
    off = spw.collect_self_play_games(None, {"num_simulations": 4}, 5, exact_endgame=6,
                                      exact_policy=False)
    on = spw.collect_self_play_games(None, {"num_simulations": 4}, 5, exact_endgame=6,
                                     exact_policy=True)
    want, mask = endgame.relabel_rows(rows, 6, device="cpu", policy=True)
    assert len(base) == len(off) == len(on) == len(emp)
    assert (mask == ((emp >= 1) & (emp <= 6))).all() and mask.sum() > 500
    changed = 0
    for i, (a, b, c) in enumerate(zip(base, off, on)):
        assert (a[0] == b[0]).all() and (a[0] == c[0]).all()  # the state planes
        assert (a[1] == b[1]).all()                           # exact_policy=False: pi as searched
        assert b[2] == c[2] == want["z"][i]
        assert (c[1] == want["pi"][i]).all()
        if not mask[i]:
            assert (c[1] == a[1]).all() and c[2] == a[2]
        changed += int((c[1] != a[1]).any())
    assert changed > 500
    with pytest.raises(ValueError, match="exact_endgame"):
        spw.collect_self_play_games(None, {"num_simulations": 4}, 5, exact_policy=True)
    with pytest.raises(ValueError, match="exact_endgame"):
        spw.collect_self_play_games(None, {"num_simulations": 4}, 5, exact_endgame=0,
                                    exact_policy=True)


def test_policy_report(late):
    import endgame

    m = late["has"] & (late["emp"] <= 8)
    own, opp, t, sc = late["own"][m], late["opp"][m], late["table"][m], late["score"][m]
    n = len(own)
    avail = t != NONE
    best = np.where(avail, t, -1000).argmax(axis=1)
    worst = np.where(avail, t, 1000).argmin(axis=1)
    rows = lambda a: {"own": own, "opp": opp, "z": np.zeros(n), "player": np.ones(n, np.int8),
                      "pi": np.eye(65, dtype=np.float32)[a]}
    rep = endgame.policy_report(rows(best), 8, device="cpu")
    assert rep["total"] == {"n": n, "optimal_mass": 1.0, "wld_kept_mass": 1.0}
    assert sorted(rep["by_empties"]) == list(range(1, 9))
    assert sum(v["n"] for v in rep["by_empties"].values()) == n
    rep = endgame.policy_report(rows(worst), 8, device="cpu")
    wv = t[np.arange(n), worst]
    assert rep["total"]["optimal_mass"] == pytest.approx((wv == sc).mean(), abs=1e-12)
    assert rep["total"]["wld_kept_mass"] == pytest.approx((np.sign(wv) == np.sign(sc)).mean(),
                                                         abs=1e-12)
    # one-hot on a move that loses a won or drawn position: no mass on either set
    lose = np.flatnonzero((np.sign(wv) < np.sign(sc)))
    assert len(lose) > 100
    r = rows(worst)
    r = {k: v[lose] for k, v in r.items()}
    rep = endgame.policy_report(r, 8, device="cpu")
    assert rep["total"] == {"n": len(lose), "optimal_mass": 0.0, "wld_kept_mass": 0.0}
    # the exact policy has all its mass on optimal moves; a uniform pi over the legal moves
    # has the optimal moves' share
    r = rows(best)
    r["pi"] = endgame.exact_policy(late["got"][OPTIMAL][0][m])
    assert endgame.policy_report(r, 8, device="cpu")["total"]["optimal_mass"] == \
        pytest.approx(1.0, abs=1e-6)
    r["pi"] = (avail / avail.sum(axis=1, keepdims=True)).astype(np.float32)
    share = ((avail & (t == sc[:, None])).sum(axis=1) / avail.sum(axis=1)).mean()
    assert endgame.policy_report(r, 8, device="cpu")["total"]["optimal_mass"] == \
        pytest.approx(share, abs=1e-6)
    assert endgame.policy_report({k: v[:0] for k, v in r.items()}, 8, device="cpu")["total"] == \
        {"n": 0, "optimal_mass": None, "wld_kept_mass": None}


def test_game_solve_moves(late):
    from envs.othello import OthelloGameNew

    g = OthelloGameNew(8)
    idx = np.flatnonzero(late["emp"] <= 8)[::97]
    seen_pass = False
    for i in np.concatenate([idx, np.flatnonzero(late["table"][:, 64] != NONE)[:3]]):
        row = late["table"][i]
        want = {int(a): int(row[a]) for a in np.flatnonzero(row != NONE)}
        for player in (1, -1):
            state = nat.unpack_np(late["own"][i:i + 1], late["opp"][i:i + 1], player)[0]
            assert g.solve_moves(state, player, max_empties=10) == want
            if want:
                assert max(want.values()) == g.solve(state, player, max_empties=10)[0]
        seen_pass |= 64 in want
    assert seen_pass
    with pytest.raises(ValueError):
        g.solve_moves(g.get_initial_state(), 1)


def test_argument_errors(late):
    f = nat.lib.oth_solve_moves_cpu
    buf = np.zeros(1, np.uint64)
    v, s = np.zeros((1, 65), np.int8), np.zeros(1, np.int8)
    q = lambda n=1, me=12, mode=SCORES: f(nat.ptr(buf), nat.ptr(buf), n, me, mode, 100, nat.ptr(v),
                                          nat.ptr(s), None)
    assert q() == nat.AZ_OK and q(me=0) == nat.AZ_OK and q(me=20) == nat.AZ_OK
    assert q(me=21) == nat.AZ_ERR_ARG and "max_empties" in nat.last_error()
    assert q(me=-1) == nat.AZ_ERR_ARG
    assert q(mode=3) == nat.AZ_ERR_ARG and "mode" in nat.last_error()
    assert q(mode=-1) == nat.AZ_ERR_ARG
    assert q(n=-1) == nat.AZ_ERR_ARG
    assert f(None, None, 1, 12, SCORES, 100, nat.ptr(v), nat.ptr(s), None) == nat.AZ_ERR_ARG
    assert f(nat.ptr(buf), nat.ptr(buf), 1, 12, SCORES, 100, None, nat.ptr(s), None) == \
        nat.AZ_ERR_ARG
    assert f(nat.ptr(buf), nat.ptr(buf), 1, 12, SCORES, 100, nat.ptr(v), None, None) == \
        nat.AZ_ERR_ARG and "null" in nat.last_error()
    with pytest.raises(RuntimeError, match="max_empties"):
        nat.solve_moves_cpu(late["own"][:4], late["opp"][:4], 21)
    with pytest.raises(RuntimeError, match="mode"):
        nat.solve_moves_cpu(late["own"][:4], late["opp"][:4], 12, 7)
    assert nat.AZ_MOVES_NONE == NONE
    assert (nat.AZ_MOVES_SCORES, nat.AZ_MOVES_WLD, nat.AZ_MOVES_OPTIMAL) == (0, 1, 2)
    assert nat.lib.az_abi_version() == 1
