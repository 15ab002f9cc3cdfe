"""Exact leaf values on the device (az_leaf_solve_gpu, csrc/leaf_solve.hip) and through every
caller that takes args["leaf_solve_empties"].

  * the kernels against the host mirror az_leaf_solve_cpu, bit for bit with the counters: row
    counts around the wave and block sizes, unaligned row slices of larger buffers, repeated
    calls on one workspace, the node limit, and a captured graph replayed on fresh values;
  * whole MCTS trees of the host-driven engine, node for node, against the oracle with an
    evaluator that swaps the solved sign in (tests/leaf_cases.py exact_evaluate), and a
    control that the comparison fails against the plain evaluator;
  * BatchedSelfPlay's default (benchmarked) step playing whole games, row for row the
    oracle's, K = 1 and 4, graphs and eager, and two pipelines against the same games;
  * the arena and the drop-in MCTS against the oracle; off means off.
"""
import functools

import numpy as np
import pytest

import leaf_cases as lc
import tree_cases as tc
from conftest import load_golden
from mock_policy import MockNet, MockPolicy, mock_eval, mock_eval_torch
from replay_rng import engine_streams

pytestmark = pytest.mark.gpu

nat = pytest.importorskip("az_native")
import torch  # noqa: E402

from engine import BatchedSelfPlay, Engine, PipelinedSelfPlay  # noqa: E402
from oracle import board as ob  # noqa: E402
from oracle.mcts import SeqMCTS  # noqa: E402
from oracle.selfplay import play_game  # noqa: E402

OFFSET = 3  # rows: the slices start here, 768 bytes into nn_in and 12 into values


# ---- the kernels against the host mirror -----------------------------------------------

@functools.lru_cache(maxsize=None)
def device_rows():
    return torch.from_numpy(lc.rows()["x"].copy()).cuda()


def host_mirror(R, E, limit):
    x = lc.rows()["x"][OFFSET:OFFSET + R]
    v = lc.sentinels(len(lc.rows()["x"]))[OFFSET:OFFSET + R].copy()
    stats = nat.leaf_solve_cpu(x, v, E, limit)
    return v, stats


def fresh_values():
    return torch.from_numpy(lc.sentinels(len(lc.rows()["x"]))).cuda()


def check_slice(values, want, R):
    """Rows [OFFSET, OFFSET + R) hold `want`, the rows around them their sentinels."""
    got = values.cpu().numpy()
    sent = lc.sentinels(len(got))
    assert np.array_equal(got[OFFSET:OFFSET + R].view(np.uint32), want.view(np.uint32))
    sent[OFFSET:OFFSET + R] = want
    assert np.array_equal(got.view(np.uint32), sent.view(np.uint32))


@pytest.mark.parametrize("E", [4, 12])
@pytest.mark.parametrize("R", [1, 63, 64, 65, 1000])
def test_device_equals_host_mirror(R, E):
    x, values = device_rows(), fresh_values()
    ws = nat.leaf_solve_workspace(R, x.device)
    nat.leaf_solve_gpu(x[OFFSET:OFFSET + R], values[OFFSET:OFFSET + R], E, 1 << 31, ws)
    want, stats = host_mirror(R, E, 1 << 31)
    check_slice(values, want, R)
    assert nat.leaf_solve_stats_gpu(ws) == stats
    if R >= 63:
        assert stats["solved"] > 0


def test_repeated_calls_rearm_the_queue_and_accumulate():
    R, E = 1000, 8
    x = device_rows()
    ws = nat.leaf_solve_workspace(R, x.device)
    want, stats = host_mirror(R, E, 1 << 31)
    for call in (1, 2):
        values = fresh_values()
        nat.leaf_solve_gpu(x[OFFSET:OFFSET + R], values[OFFSET:OFFSET + R], E, 1 << 31, ws)
        check_slice(values, want, R)
        assert nat.leaf_solve_stats_gpu(ws) == {k: call * v for k, v in stats.items()}
    # a shorter call on the same workspace: the task list of the longer one is not reused
    want65, stats65 = host_mirror(65, E, 1 << 31)
    values = fresh_values()
    nat.leaf_solve_gpu(x[OFFSET:OFFSET + 65], values[OFFSET:OFFSET + 65], E, 1 << 31, ws)
    check_slice(values, want65, 65)
    assert nat.leaf_solve_stats_gpu(ws) == {k: 2 * v + stats65[k] for k, v in stats.items()}


def test_node_limit_rows_are_the_host_s():
    R, E, limit = 1000, 8, 64
    x, values = device_rows(), fresh_values()
    ws = nat.leaf_solve_workspace(R, x.device)
    nat.leaf_solve_gpu(x[OFFSET:OFFSET + R], values[OFFSET:OFFSET + R], E, limit, ws)
    want, stats = host_mirror(R, E, limit)
    assert stats["limited"] > 0 and stats["solved"] > 0
    exp, exp_stats = lc.expected(E, limit, n=R, start=OFFSET)
    assert np.array_equal(want.view(np.uint32), exp.view(np.uint32)) and stats == exp_stats
    check_slice(values, want, R)
    assert nat.leaf_solve_stats_gpu(ws) == stats


def test_captured_graph_replays():
    R, E = 1000, 6
    x, values = device_rows(), fresh_values()
    ws = nat.leaf_solve_workspace(R, x.device)
    want, stats = host_mirror(R, E, 256)
    sent = fresh_values()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # once eagerly, as every captured step here is warmed
        nat.leaf_solve_gpu(x[OFFSET:OFFSET + R], values[OFFSET:OFFSET + R], E, 256, ws)
    torch.cuda.current_stream().wait_stream(s)
    check_slice(values, want, R)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        nat.leaf_solve_gpu(x[OFFSET:OFFSET + R], values[OFFSET:OFFSET + R], E, 256, ws)
    for replay in (1, 2, 3):
        values.copy_(sent)
        g.replay()
        check_slice(values, want, R)
        assert nat.leaf_solve_stats_gpu(ws) == {k: (1 + replay) * v for k, v in stats.items()}


# ---- whole trees through the host-driven engine ---------------------------------------

E_TREE = 6
TREE_SCHEDULE = (120, 60, 60)
TREE_PARAMS = [(K, eps) for K in (1, 4) for eps in (0.0, 0.25)]


@functools.lru_cache(maxsize=None)
def tree_roots():
    """Corpus roots with 8, 10 and 12 empties (the first position of each depth; 10: the late
    root of tests/tree_cases.py, whose tree holds terminal and pass nodes)."""
    d = load_golden("board_corpus.npz")
    emp = 64 - lc.popc(d["pos"] | d["neg"])
    out = []
    for e in (8, 10, 12):
        i = int(np.flatnonzero(emp == e)[0])
        out.append(tc.LATE_ROOT if e == 10 else (int(d["game"][i]), int(d["ply"][i])))
    roots = [tc.corpus_root(*gp) for gp in out]
    assert [64 - bin(o | p).count("1") for o, p, _ in roots] == [8, 10, 12]
    return roots


@functools.lru_cache(maxsize=None)
def tree_script(K, eps, exact=True):
    ev = lc.exact_evaluate(tc.evaluate, E_TREE) if exact else tc.evaluate
    out = []
    for slot, root in enumerate(tree_roots()):
        o = SeqMCTS(2.0, 0, ev, dirichlet_alpha=1.0, dirichlet_epsilon=eps,
                    rng=tc.NoiseRng(tc.noise_vectors(slot)), leaves_per_step=K)
        out.append(tc.run_schedule(o, root, TREE_SCHEDULE))
    return out


def step_exact(e):
    e.select()
    pr, va = mock_eval_torch(e.nn_in)
    e.priors.copy_(pr)
    e.values.copy_(va)
    e.leaf_solve()
    e.expand()
    e.play()


def tree_engine(K, eps):
    roots = tree_roots()
    e = Engine(len(roots), 120, c_puct=2.0, dirichlet_alpha=1.0, dirichlet_epsilon=eps,
               injected_rng=True, auto_play=False, inj_noise_slots=tc.NOISE_SLOTS,
               leaves_per_step=K, leaf_solve_empties=E_TREE)
    for g, (own, opp, player) in enumerate(roots):
        e.set_root(g, own, opp, player)
    e.inject(noise=np.stack([tc.noise_vectors(g) for g in range(len(roots))]))
    return e


@pytest.mark.parametrize("K,eps", TREE_PARAMS)
def test_whole_trees_match_the_exact_oracle(K, eps):
    from test_engine_tree_gpu import replay

    e = tree_engine(K, eps)
    replay(e, tree_script(K, eps), step_exact)
    assert e.counters()["arena_overflows"] == 0
    st = e.leaf_solve_stats()
    assert st["solved"] > 0


def test_whole_trees_differ_from_the_plain_oracle():
    """The control: against the oracle with the unwrapped evaluator the same comparison fails,
    so it sees the override."""
    from test_engine_tree_gpu import replay

    e = tree_engine(1, 0.0)
    with pytest.raises(AssertionError):
        replay(e, tree_script(1, 0.0, exact=False), step_exact)


# ---- the bench path: whole games ------------------------------------------------------

SP_ARGS = {"c_puct": 2.0, "num_simulations": 25, "dirichlet_alpha": 1.0,
           "dirichlet_epsilon": 0.3, "mcts_temperature": 1.0, "num_exploratory_moves": 35,
           "lambda": 0.98, "leaf_solve_empties": 6}
N_GAMES = 8


class RecordingRng:
    """Seeded draws for the oracle, logged in tests/golden/make_goldens.py's form (kind 0 a
    Dirichlet vector, 1 a tie break among a choices taking b, 2 an action sample with the
    uniform a), which replay_rng.engine_streams turns into the engine's injected streams."""

    def __init__(self, seed):
        self.g = np.random.default_rng(seed)
        self.kinds, self.a, self.b, self.noise = [], [], [], []

    def _log(self, kind, a, b=0):
        self.kinds.append(kind)
        self.a.append(a)
        self.b.append(b)

    def dirichlet(self, alpha, n):
        v = self.g.dirichlet([alpha] * n)
        self._log(0, len(self.noise))
        self.noise.append(v)
        return v

    def choice_tie(self, best):
        j = int(self.g.integers(len(best)))
        self._log(1, len(best), j)
        return best[j]

    def choice_p(self, n, p):
        u = float(self.g.random())
        self._log(2, u)
        cdf = np.asarray(p, np.float64).cumsum()
        cdf /= cdf[-1]
        return int(cdf.searchsorted(u, side="right"))


def oracle_eval(salt=0):
    def f(own, opp, player):
        st = ob.to_state(own, opp, player)
        p, v = mock_eval((player * st).reshape(-1), salt)
        return p.astype(np.float32), float(v)
    return f


@functools.lru_cache(maxsize=None)
def oracle_games(K):
    """N_GAMES oracle self-play games with exact late values: per game its sample rows and its
    injected streams (Dirichlet vectors, uniforms)."""
    ev = lc.exact_evaluate(oracle_eval(), SP_ARGS["leaf_solve_empties"])
    games = []
    for g in range(N_GAMES):
        rng = RecordingRng(100 * K + g)
        samples, _ = play_game(SP_ARGS, ev, rng=rng, leaves_per_step=K)
        own, opp = nat.pack_np(np.stack([s[0] for s in samples]), 1)
        rows = {"own": own, "opp": opp, "pi": np.stack([s[1] for s in samples]),
                "z": np.array([s[2] for s in samples], np.float64)}
        games.append((rows, engine_streams(rng.kinds, rng.a, rng.b, rng.noise)))
    return games


def injection(games):
    nz = max(len(s[0]) for _, s in games)
    nu = max(len(s[1]) for _, s in games)
    noise = np.zeros((len(games), nz, 65))
    uni = np.zeros((len(games), nu))
    for g, (_, (n, u)) in enumerate(games):
        noise[g, :len(n)] = n
        uni[g, :len(u)] = u
    return noise, uni


def check_rows(engine, games):
    c = engine.counters()
    assert c["games_finished"] == len(games)
    assert c["arena_overflows"] == 0 and c["samples_dropped"] == 0
    smp = engine.samples()
    order = np.argsort(smp["slot"], kind="stable")
    smp = {k: v[order] for k, v in smp.items()}
    bounds = np.searchsorted(smp["slot"], np.arange(len(games) + 1))
    for g, (rows, _) in enumerate(games):
        lo, hi = bounds[g], bounds[g + 1]
        assert hi - lo == len(rows["z"]), g
        for k in ("own", "opp", "pi", "z"):
            assert np.array_equal(smp[k][lo:hi], rows[k]), (g, k)


def run_until_finished(sp, n_games, K):
    per_game = 64 * (-(-SP_ARGS["num_simulations"] // K) + 2)
    done = 0
    while done < 2 * per_game and sp.counters()["games_finished"] < n_games:
        sp.step(256)
        done += 256


@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("K", [1, 4])
def test_bench_path_plays_the_exact_oracle_games(K, use_graph):
    games = oracle_games(K)
    noise, uni = injection(games)
    sp = BatchedSelfPlay(MockNet(), SP_ARGS, N_GAMES, fold=False, use_graph=use_graph,
                         require_graph=use_graph, leaves_per_step=K, injected_rng=True,
                         inj_noise_slots=noise.shape[1], inj_uniform_slots=uni.shape[1],
                         sample_capacity=N_GAMES * 70)
    assert sp.defer_moves and sp.fuse_expand  # the bench's default step
    sp.reset(start_budget=N_GAMES)
    sp.inject(noise=noise, uniforms=uni)
    run_until_finished(sp, N_GAMES, K)
    assert (sp.graph is not None) == use_graph and sp.graph_error is None
    check_rows(sp.engine, games)
    st = sp.engine.leaf_solve_stats()
    assert st["solved"] > 0


@pytest.mark.parametrize("defer_moves,fuse_expand", [(False, False), (True, False)])
def test_other_step_shapes_play_the_same_games(defer_moves, fuse_expand):
    """The plain step (select, net, expand, play) and deferred moves without the fused
    expansion: the same games."""
    games = oracle_games(1)
    noise, uni = injection(games)
    sp = BatchedSelfPlay(MockNet(), SP_ARGS, N_GAMES, fold=False, use_graph=False,
                         injected_rng=True, inj_noise_slots=noise.shape[1],
                         inj_uniform_slots=uni.shape[1], sample_capacity=N_GAMES * 70,
                         defer_moves=defer_moves, fuse_expand=fuse_expand)
    assert sp.defer_moves == defer_moves and not sp.fuse_expand
    sp.reset(start_budget=N_GAMES)
    sp.inject(noise=noise, uniforms=uni)
    run_until_finished(sp, N_GAMES, 1)
    check_rows(sp.engine, games)
    assert sp.engine.leaf_solve_stats()["solved"] > 0


def test_two_pipelines_equal_their_parts():
    """PipelinedSelfPlay, 16 slots in two pipelines on two streams, each with its own
    workspace: both parts play the games a single BatchedSelfPlay of 8 slots plays."""
    games = oracle_games(1)
    noise, uni = injection(games)
    sp = PipelinedSelfPlay(MockNet(), SP_ARGS, 2 * N_GAMES, pipelines=2, fold=False,
                           use_graph=True, require_graph=True, injected_rng=True,
                           inj_noise_slots=noise.shape[1], inj_uniform_slots=uni.shape[1],
                           sample_capacity=N_GAMES * 70)
    ws = [p.engine.leaf_ws for p in sp.parts]
    assert ws[0] is not None and ws[1] is not None and ws[0].data_ptr() != ws[1].data_ptr()
    sp.reset(start_budget=2 * N_GAMES)
    for p in sp.parts:
        p.inject(noise=noise, uniforms=uni)
    run_until_finished(sp, 2 * N_GAMES, 1)
    for p in sp.parts:
        check_rows(p.engine, games)
    stats = [p.engine.leaf_solve_stats() for p in sp.parts]
    assert stats[0] == stats[1] and stats[0]["solved"] > 0


# ---- arena and drop-in ----------------------------------------------------------------

ARENA_ARGS = {"c_puct": 2.0, "num_simulations": 16, "leaf_solve_empties": 6}


class LowestTie:
    def choice_tie(self, best):
        return best[0]


def oracle_match(first_salt, second_salt, args):
    """eval.py's play_match on the oracle with exact late values: (result from the first
    player's side, the actions)."""
    K = args.get("num_threads", 4)
    E = args["leaf_solve_empties"]
    trees = {1: SeqMCTS(args["c_puct"], args["num_simulations"],
                        lc.exact_evaluate(oracle_eval(first_salt), E), rng=LowestTie(),
                        leaves_per_step=K),
             -1: SeqMCTS(args["c_puct"], args["num_simulations"],
                         lc.exact_evaluate(oracle_eval(second_salt), E), rng=LowestTie(),
                         leaves_per_step=K)}
    game = ob.OracleGame()
    state, player, actions = game.get_initial_state(), 1, []
    while True:
        own, opp = ob.to_bitboards(state, player)
        probs = trees[player].search(own, opp, player, 0.0)
        action = int(np.argmax(probs))
        actions.append(action)
        state = game.get_next_state(state, action, player)
        reward, done = game.get_value_and_terminated(state, action, player)
        if done:
            if reward == 0:
                return 0, actions
            return (1 if (reward == 1) == (player == 1) else -1), actions
        for t in trees.values():
            if t.root >= 0:
                t.make_move(action)
        player = -player


def test_arena_matches_the_exact_oracle():
    from arena import BatchedArena, tie_break_lowest

    arena = BatchedArena(MockNet(1).cuda(), MockNet(2).cuda(), ARENA_ARGS, n_slots=4,
                         tie_break=tie_break_lowest)
    assert arena.use_graph
    _, _, _, _, records = arena.play(4, record=True)
    for m, rec in enumerate(records):
        a_first = m % 2 == 0
        r, actions = oracle_match(1 if a_first else 2, 2 if a_first else 1, ARENA_ARGS)
        assert rec["a_first"] == a_first
        assert rec["actions"] == actions, m
        assert rec["result"] == (r if a_first else -r), m
    assert sum(e.leaf_solve_stats()["solved"] for e in arena.eng) > 0


def test_dropin_mcts_search_equals_the_exact_oracle():
    from MCTS_model import MCTS
    from envs.othello import OthelloGameNew

    own, opp, player = tc.corpus_root(*tc.LATE_ROOT)  # 10 empties
    args = {"c_puct": 2.0, "num_simulations": 60, "leaf_solve_empties": 6}
    state = ob.to_state(own, opp, player)
    mcts = MCTS(OthelloGameNew(8), args, MockPolicy())
    pi = mcts.policy_improve_step(np.array(state), player, temp=1.0)
    ref = SeqMCTS(2.0, 60, lc.exact_evaluate(oracle_eval(), 6), leaves_per_step=4)
    want = ref.search(own, opp, player, 1.0)
    assert np.array_equal(np.asarray(pi, np.float32), np.asarray(want, np.float32))
    plain = SeqMCTS(2.0, 60, oracle_eval(), leaves_per_step=4).search(own, opp, player, 1.0)
    assert not np.array_equal(np.asarray(plain), np.asarray(want))  # the key changes the search
    assert mcts._impl.engine.leaf_solve_stats()["solved"] > 0


# ---- off means off, and the combinations that cannot work --------------------------------

@pytest.mark.parametrize("key", [None, 0])
def test_off_means_off(key):
    args = {k: v for k, v in SP_ARGS.items() if k != "leaf_solve_empties"}
    if key is not None:
        args["leaf_solve_empties"] = key
    sp = BatchedSelfPlay(MockNet(), args, N_GAMES, fold=False, seed=1)
    assert sp.engine.leaf_empties == 0 and sp.engine.leaf_ws is None
    sp.reset()
    sp.step(64)
    assert sp.engine.leaf_solve_stats() == {"solved": 0, "limited": 0, "nodes": 0}
    with pytest.raises(RuntimeError, match="off"):
        sp.engine.leaf_solve()


def test_rollout_evaluation_refuses_the_key():
    with pytest.raises(ValueError, match="rollout"):
        BatchedSelfPlay(None, SP_ARGS, N_GAMES)
    with pytest.raises(ValueError):
        BatchedSelfPlay(MockNet(), dict(SP_ARGS, leaf_solve_empties=13), N_GAMES, fold=False)
