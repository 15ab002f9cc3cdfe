"""The GPU engine on sharp net outputs: priors of exactly 0, of 2^-44 (a legal row sums to a
non-zero value below the 1e-12 renormalisation threshold, so it stays unnormalised) and equal
powers of two (exact PUCT ties, taken in action order), values of exactly +-1 and 0 --
tests/mock_policy.py sharp_eval.  The expected results are the reference's own, recorded by
tests/golden/make_sharp_goldens.py; tests/test_sharp_cpu.py shows on the CPU that the oracle
replays them and counts how often each of these situations occurs in them.

  * host-driven searches (mcts_sharp_cases.npz: one leaf per step; mcts_sharp_vl_cases.npz:
    four, under virtual loss) through az_select + az_expand_backup and through the fused
    az_select_expand: counts, root value, pi and root N bit-exact;
  * complete self-play games (selfplay_sharp.npz) on device through BatchedSelfPlay with the
    recorded streams injected, in the default step shape (deferred moves, fused expansion,
    graphs) and in eager mode: every canonical board, pi and z bit-identical.
"""
import functools

import numpy as np
import pytest

from conftest import load_golden
from mock_policy import SharpNet, sharp_eval_torch
from replay_rng import case_log, engine_streams
from test_engine_tree_gpu import run_search, step_fused, step_plain

pytestmark = pytest.mark.gpu

nat = pytest.importorskip("az_native")
from engine import BatchedSelfPlay, Engine  # noqa: E402

STEPS = {"plain": functools.partial(step_plain, evaluate=sharp_eval_torch),
         "fused": functools.partial(step_fused, evaluate=sharp_eval_torch)}
# ARGS of test_bench_path_gpu.py: what the self-play fixtures were recorded with
ARGS = {"c_puct": 2.0, "dirichlet_alpha": 1.0, "dirichlet_epsilon": 0.3,
        "mcts_temperature": 1.0, "num_exploratory_moves": 35, "lambda": 0.98}


def own_opp(pos, neg, player):
    return (int(pos), int(neg)) if player == 1 else (int(neg), int(pos))


def _groups(name):
    d = load_golden(name)
    return sorted({(float(c), float(e)) for c, e in zip(d["c_puct"], d["eps"])})


def _run_cases(name, K, group, step):
    """Every case of fixture `name` with (c_puct, eps) = group, one engine slot each."""
    d = load_golden(name)
    single = "log_kind" in d  # mcts_cases schema: choice draws and temperatures recorded
    cases = [c for c in range(int(d["n_cases"]))
             if (float(d["c_puct"][d["log_case"] == c][0]),
                 float(d["eps"][d["log_case"] == c][0])) == group]
    G = len(cases)
    assert G >= 7
    e = Engine(G, 1, c_puct=group[0], dirichlet_alpha=1.0, dirichlet_epsilon=group[1],
               injected_rng=True, auto_play=False, inj_noise_slots=2, inj_uniform_slots=4,
               leaves_per_step=K)
    noise = np.zeros((G, 2, 65))
    rows, ties = [], []
    for s, c in enumerate(cases):
        nz = d["noise"][int(d["noise_offsets"][c]):int(d["noise_offsets"][c + 1])]
        noise[s, :len(nz)] = nz
        if single:
            kinds, a, b, _ = case_log(d, c)
            ties.append([(int(x), int(y)) for k, x, y in zip(kinds, a, b) if k == 1])
        r = np.nonzero(d["log_case"] == c)[0]
        rows.append(r)
        if not single:
            assert (d["k"][r] == K).all()
        own, opp = own_opp(d["pos"][r[0]], d["neg"][r[0]], d["player"][r[0]])
        e.set_root(s, own, opp, int(d["player"][r[0]]))
    e.inject(noise=noise)
    for mv in range(max(len(r) for r in rows)):
        live = [s for s in range(G) if mv < len(rows[s])]
        for s in live:
            e.begin_search(s, int(d["sims"][rows[s][mv]]))
        run_search(e, step)
        for s in live:
            r = rows[s][mv]
            temp = float(d["temp"][r]) if single else 1.0
            u_tie = 0.0
            if abs(temp) < 0.1:
                k, j = ties[s].pop(0)
                u_tie = (j + 0.5) / k
            pi, counts, vroot = e.root_policy(s, temp, u_tie)
            where = f"case {cases[s]} move {mv}"
            assert (counts == d["counts"][r]).all(), where
            assert vroot == d["root_value"][r], where
            assert (pi == d["probs"][r]).all(), where
            assert e.export_tree(s, max_nodes=1)["N"][0] == d["root_n"][r], where
            if mv + 1 < len(rows[s]):
                e.make_move(s, int(np.argmax(d["counts"][r])))
    assert e.counters()["arena_overflows"] == 0


@pytest.mark.parametrize("step", sorted(STEPS))
@pytest.mark.parametrize("group", _groups("mcts_sharp_cases.npz"))
def test_sharp_searches_match_reference(group, step):
    _run_cases("mcts_sharp_cases.npz", 1, group, STEPS[step])


@pytest.mark.parametrize("step", sorted(STEPS))
@pytest.mark.parametrize("group", _groups("mcts_sharp_vl_cases.npz"))
def test_sharp_virtual_loss_searches_match_reference(group, step):
    _run_cases("mcts_sharp_vl_cases.npz", 4, group, STEPS[step])


# ---- complete games ----------------------------------------------------------------------

NG = 4  # reference games queued per slot (its injected streams, back to back)


def _play(games, S, K, G, use_graph):
    """test_bench_path_gpu.py's _play at a few slots: slot s plays games[(s + i) % n],
    i = 0, 1, ..., with unlimited refill and staggered starts until every slot has completed
    two games."""
    d = load_golden("selfplay_sharp.npz")
    n = len(games)
    queues = [[games[(s + i) % n] for i in range(NG)] for s in range(G)]
    streams = {g: engine_streams(*case_log(d, g)) for g in games}
    NU = max(sum(len(streams[g][1]) for g in q) for q in queues)
    noise = np.zeros((G, NG, 65))
    uni = np.zeros((G, NU))
    for s, q in enumerate(queues):
        u = 0
        for i, g in enumerate(q):
            nz, us = streams[g]
            assert len(nz) == 1  # one Dirichlet vector per game: the ply-0 root
            noise[s, i] = nz[0]
            uni[s, u:u + len(us)] = us
            u += len(us)
    sp = BatchedSelfPlay(SharpNet(), dict(ARGS, num_simulations=S), G, fold=False,
                         use_graph=use_graph, require_graph=use_graph, leaves_per_step=K,
                         injected_rng=True, inj_noise_slots=NG, inj_uniform_slots=NU,
                         sample_capacity=G * NG * 70)
    # a game is at most 64 plies of ceil(S / K) + 1 steps, + 1 per ply sitting out; the starts
    # are spread over 16 moves, so the slots of a wave are at different plies and end apart
    per_game = 64 * (-(-S // K) + 2)
    stagger = (-(-S // K) + 1) * 16
    sp.reset(start_budget=-1, stagger_steps=stagger)
    sp.inject(noise=noise, uniforms=uni)
    total = stagger + 2 * per_game + 64
    done = 0
    while done < total:
        sp.step(min(1024, total - done))
        done += min(1024, total - done)
    c = sp.engine.counters()
    assert (sp.graph is not None) == use_graph and sp.graph_error is None
    assert c["arena_overflows"] == 0 and c["samples_dropped"] == 0
    smp = sp.engine.samples()
    order = np.argsort(smp["slot"], kind="stable")  # a slot's rows in the order its games ended
    smp = {k: v[order] for k, v in smp.items()}
    rows = {g: {"own": d["pos"][d["game"] == g], "opp": d["neg"][d["game"] == g],
                "pi": d["pi"][d["game"] == g], "z": d["z"][d["game"] == g]} for g in games}
    return sp, smp, [[rows[g] for g in q] for q in queues]


def _check(smp, want):
    """Every slot's rows are its queue's first m >= 2 games, bit for bit."""
    bounds = np.searchsorted(smp["slot"], np.arange(len(want) + 1))
    for s, q in enumerate(want):
        lo, hi = bounds[s], bounds[s + 1]
        m, rows = 0, 0
        while m < len(q) and rows + len(q[m]["z"]) <= hi - lo:
            rows += len(q[m]["z"])
            m += 1
        assert rows == hi - lo and 2 <= m < len(q), f"slot {s}: {hi - lo} rows, {m} games"
        for k in ("own", "opp", "pi", "z"):
            w = np.concatenate([g[k] for g in q[:m]])
            assert np.array_equal(smp[k][lo:hi], w), (s, k)


def _games(K, S):
    d = load_golden("selfplay_sharp.npz")
    return [g for g, m in enumerate(d["meta"]) if int(m[3]) == K and int(m[0]) == S]


@pytest.mark.parametrize("S,K,G", [(25, 1, 64), (100, 1, 64), (25, 4, 16)])
@pytest.mark.parametrize("use_graph", [True, False])
def test_sharp_selfplay_games_on_device(S, K, G, use_graph):
    games = _games(K, S)
    assert games, (S, K)
    sp, smp, want = _play(games, S, K, G, use_graph)
    assert sp.defer_moves and sp.fuse_expand  # the default step shape
    assert sp.engine.nn_in.shape == (G * K, 64)
    _check(smp, want)
