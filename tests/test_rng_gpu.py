"""The AZ_RNG_DEVICE draws of the self-play engine (csrc/philox.h, engine.hip), which every
production run uses and every bit-exact engine test replaces with injected ones.

The sampler: the device's uniforms equal the host's bit for bit; gamma_draw is Gamma(alpha, 1)
by a Kolmogorov-Smirnov test against scipy's CDF in both branches; the 65-way normalisation
is the kernel's butterfly sum, exactly, and its components are Beta(alpha, 64 alpha);
neighbouring slots, events and streams are uncorrelated.

The schedule: an injected_rng engine fed the probe's draws at the (event, sub) each draw
kind is documented to use ("The device draws' counters") must play exactly what
the device-mode engine plays, so a draw that moved to another counter, or two kinds that
came to share one, changes a result here.

The KS bound sqrt(N) D <= 2.25 is Kolmogorov's tail 2 exp(-2 c^2) = 8e-5 per test at
c = 2.25 (about 2e-3 over the file for a correct sampler).  On the host,
numpy.random.Generator.gamma at N = 16,384 * 65 gives 0.56 .. 0.88 for the four alphas and
4.0 .. 7.9 when drawn at 1.01 alpha against alpha's CDF: the bound passes a correct sampler
and resolves a 1 % error in alpha.  A test that lands in the tail is not loosened and no seed
is hunted: it is rerun once at seed 20261020 with n = 65,536, which a real defect fails too.
"""
import math

import numpy as np
import pytest
import torch

from conftest import load_golden
from mock_policy import MockNet, mock_eval_torch

pytestmark = pytest.mark.gpu

nat = pytest.importorskip("az_native")
st = pytest.importorskip("scipy.stats")
from engine import BatchedSelfPlay, Engine, PipelinedSelfPlay  # noqa: E402

from test_rng_cpu import TUPLES  # noqa: E402

SEED, N_SLOTS = 20261019, 16384
ALPHAS = (0.03, 0.3, 1.0, 3.0)
KS_BOUND = 2.25
INIT_OWN, INIT_OPP = 0x0000000810000000, 0x0000001008000000
W64 = np.uint64(1) << np.arange(64, dtype=np.uint64)


def ks_stat(x, cdf):
    """sqrt(N) * D_N of a one-sample Kolmogorov-Smirnov test."""
    x = np.sort(np.asarray(x, np.float64).ravel())
    n = len(x)
    c = cdf(x)
    i = np.arange(1, n + 1, dtype=np.float64)
    return math.sqrt(n) * max(float((i / n - c).max()), float((c - (i - 1) / n).max()))


_DIR = {}


def dirichlet(alpha, seed=SEED, stream=0, slot0=0, n=N_SLOTS, event=0):
    """(gammas, noise) of the probe as numpy arrays, computed once per argument tuple."""
    key = (alpha, seed, stream, slot0, n, event)
    if key not in _DIR:
        g, z = nat.rng_dirichlet_gpu(seed, stream, slot0, n, event, alpha)
        _DIR[key] = (g.cpu().numpy(), z.cpu().numpy())
    return _DIR[key]


# ---------------------------------------------------------------------------------------
# the sampler

@pytest.mark.parametrize("seed,stream,slot0,event,sub", TUPLES)
def test_device_uniforms_equal_the_hosts(seed, stream, slot0, event, sub):
    n = 65537  # one past a multiple of the kernel's block
    got = nat.rng_uniform_gpu(seed, stream, slot0, n, event, sub).cpu().numpy()
    assert np.array_equal(got, nat.rng_uniform_cpu(seed, stream, slot0, n, event, sub))


@pytest.mark.parametrize("alpha", ALPHAS)
def test_gamma_law(alpha):
    """sqrt(N) D on an MI355X at seed 20261019, n = 16,384 (N = 1,064,960): 0.667, 0.828,
    1.459 and 1.246 for alpha = 0.03, 0.3, 1.0 and 3.0, so no rerun was needed; at four and
    sixteen times the N (other seeds) alpha = 1.0 gave 1.008 and 1.071, alpha = 3.0 1.050 and
    0.867: the statistic does not grow with N, as a bias would make it."""
    g, _ = dirichlet(alpha)
    assert g.shape == (N_SLOTS, 65) and np.isfinite(g).all() and (g > 0).all()
    d = ks_stat(g, st.gamma(alpha).cdf)
    print(f"gamma alpha={alpha}: sqrt(N) D = {d:.4f}")
    if d > KS_BOUND:  # the documented single rerun; a real defect fails both
        g2, _ = dirichlet(alpha, seed=SEED + 1, n=65536)
        d2 = ks_stat(g2, st.gamma(alpha).cdf)
        print(f"gamma alpha={alpha}: rerun sqrt(N) D = {d2:.4f}")
        assert d2 <= KS_BOUND, (alpha, d, d2)


@pytest.mark.parametrize("alpha", ALPHAS)
def test_normalisation_is_the_kernels_sum_exactly(alpha):
    g, z = dirichlet(alpha)
    s = g[:, :64].copy()
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):  # s += __shfl_xor(s, off): every lane ends with one sum
        s = s + s[:, lanes ^ off]
    assert (s == s[:, :1]).all()
    s = s[:, :1] + g[:, 64:65]
    assert np.array_equal(z, g / s)
    # each component is within half an ulp of g / s and s within 7 roundings of the true
    # sum: the row sums sit a few ulp from 1, far inside 65
    rows = np.array([math.fsum(r) for r in z])
    assert (np.abs(rows - 1.0) <= 65 * 2.0 ** -52).all()
    assert (z >= 0).all() and (z <= 1).all()


@pytest.mark.parametrize("alpha", ALPHAS)
def test_dirichlet_marginals(alpha):
    """Component j of Dirichlet(alpha x 65) is Beta(alpha, 64 alpha); 64 is the component
    every lane draws redundantly.  Largest sqrt(N) D over the four components on an MI355X:
    1.241, 1.078, 1.181 and 1.014 for alpha = 0.03, 0.3, 1.0 and 3.0 (no rerun needed)."""
    _, z = dirichlet(alpha)
    cdf = st.beta(alpha, 64 * alpha).cdf
    worst = {}
    for j in (0, 31, 63, 64):
        d = ks_stat(z[:, j], cdf)
        if d > KS_BOUND:  # the documented single rerun
            d = ks_stat(dirichlet(alpha, seed=SEED + 1, n=65536)[1][:, j], cdf)
        worst[j] = d
    print(f"beta alpha={alpha}: sqrt(N) D = {worst}")
    assert max(worst.values()) <= KS_BOUND, worst


def test_neighbouring_counters_draw_separately():
    """The vectors of (slot, event), (slot + 1, event), (slot, event + 1) and (slot, event) on
    stream 1: no value in common slot by slot, and no correlation over the slots."""
    a = 1.0
    sets = [dirichlet(a), dirichlet(a, slot0=1), dirichlet(a, event=1), dirichlet(a, stream=1)]
    raw = np.sort(np.concatenate([g for g, _ in sets], 1), 1)  # [n, 260]
    assert (np.diff(raw, axis=1) != 0).all()
    bound = 4.5 / math.sqrt(N_SLOTS)
    zs = [(z - z.mean(0)) / z.std(0) for _, z in sets]
    for i in range(4):
        for j in range(i + 1, 4):
            r = (zs[i] * zs[j]).mean(0)  # per component, over the slots
            assert (np.abs(r) <= bound).all(), (i, j, float(np.abs(r).max()))


def test_probe_rejects_a_stream_that_aliases():
    g = torch.empty(65, dtype=torch.float64, device="cuda")
    rc = nat.lib.az_rng_dirichlet_gpu(1, 1 << 31, 0, 1, 0, 1.0, nat.ptr(g), nat.ptr(g), None)
    assert rc == nat.AZ_ERR_ARG and "0x80000000" in nat.last_error()
    assert nat.lib.az_rng_dirichlet_gpu(1, 0, 0, 1, 0, 0.0, nat.ptr(g), nat.ptr(g),
                                        None) == nat.AZ_ERR_ARG


# ---------------------------------------------------------------------------------------
# az_engine_create and the stream id

def test_engine_rejects_stream_ids_that_alias():
    """gamma_draw's second pair of uniforms comes from stream ^ 0x80000000 and the counter
    holds 32 bits of the id: 2^31 and above would share draws with a lower id."""
    for bad in (1 << 31, (1 << 31) + 7, 1 << 32, (1 << 63) + 1):
        with pytest.raises(RuntimeError, match="0x80000000"):
            Engine(1, 1, stream_id=bad)
    Engine(1, 1, stream_id=(1 << 31) - 1).close()


# ---------------------------------------------------------------------------------------
# the engine's schedule

def step_mock(e):
    e.select()
    pr, va = mock_eval_torch(e.nn_in)
    e.priors.copy_(pr)
    e.values.copy_(va)
    e.expand()
    e.play()


def play_two_plies(e, sims):
    e_steps = 0
    while e.game_info()["ply"].min() < 2:
        for _ in range(sims + 1):
            step_mock(e)
        e_steps += sims + 1
        assert e_steps <= 8 * (sims + 1), "the slots did not move"


SCHEDULE = [  # (num_exploratory_moves, simulations, seed, stream)
    (35, 16, SEED, 0),
    (0, 16, SEED, 0),
    (35, 16, (0xDEADBEEF << 32) | SEED, 5),
    (0, 16, (0xDEADBEEF << 32) | SEED, 5),
    # 16 simulations leave the root's top visit count untied (9 against 7 in every slot), so
    # there the tie-break draw decides nothing; 4 simulations tie it (2 against 2)
    (0, 4, SEED, 0),
]


@pytest.mark.parametrize("explore,sims,seed,stream", SCHEDULE)
def test_root_noise_and_first_move_use_their_counters(explore, sims, seed, stream):
    """Event 0 is the root's Dirichlet vector.  With temperature 1 the action sample is
    event 1 at sub 0x2000; at temperature 0 the tie break is event 1 at sub 0x1000 and the
    action sample event 2 at sub 0x2000.  The comparison can tell: fed the same draws with
    the two subs exchanged, the injected engine plays something else."""
    G, alpha = 1024, 1.0
    kw = dict(c_puct=2.0, dirichlet_alpha=alpha, dirichlet_epsilon=0.3, temperature=1.0,
              num_exploratory_moves=explore, lambd=0.98)
    noise = nat.rng_dirichlet_gpu(seed, stream, 0, G, 0, alpha)[1].cpu().numpy()

    def uniforms(draws):
        return np.stack([nat.rng_uniform_gpu(seed, stream, 0, G, ev, sub).cpu().numpy()[:, 0]
                         for ev, sub in draws], 1)

    if explore:
        uni, wrong = uniforms([(1, 0x2000)]), uniforms([(1, 0x1000)])
    else:
        uni = uniforms([(1, 0x1000), (2, 0x2000)])
        wrong = uniforms([(1, 0x2000), (2, 0x1000)])

    # auto-play: ply 0's pi and root value, and the board the sampled move leads to
    def first_move(u):
        e = Engine(G, sims, injected_rng=u is not None, auto_play=True, refill=False, seed=seed,
                   stream_id=stream, inj_noise_slots=1, inj_uniform_slots=uni.shape[1], **kw)
        e.reset_all()
        if u is not None:
            e.inject(noise=noise.reshape(G, 1, 65), uniforms=u)
        play_two_plies(e, sims)
        assert e.counters()["arena_overflows"] == 0
        t = [e.export_trajectory(g) for g in range(G)]
        e.close()
        assert all(x["own"][0] == INIT_OWN and x["opp"][0] == INIT_OPP for x in t)
        return t

    def differing(ta, tb):
        return [g for g, (a, b) in enumerate(zip(ta, tb))
                if not (np.array_equal(a["pi"][0], b["pi"][0]) and a["vroot"][0] == b["vroot"][0]
                        and a["own"][1] == b["own"][1] and a["opp"][1] == b["opp"][1])]

    dev = first_move(None)
    assert differing(dev, first_move(uni)) == []
    if explore or sims == 4:
        n_diff = len(differing(dev, first_move(wrong)))
        print(f"explore={explore} sims={sims}: {n_diff} of {G} slots tell the subs apart")
        assert n_diff > 0

    # host-driven: the root children's priors right after the first expansion
    trees = []
    slots = np.arange(G, dtype=np.int32)
    for injected in (False, True):
        e = Engine(G, sims, injected_rng=injected, auto_play=False, seed=seed, stream_id=stream,
                   inj_noise_slots=1, **kw)
        e.set_roots(slots, np.full(G, INIT_OWN, np.uint64), np.full(G, INIT_OPP, np.uint64),
                    np.ones(G, np.int32))
        if injected:
            e.inject(noise=noise.reshape(G, 1, 65))
        e.begin_search_slots(slots, sims)
        step_mock(e)
        trees.append([e.export_tree(g) for g in range(G)])
        e.close()
    distinct = set()
    for dev, inj in zip(*trees):
        assert dev["n_nodes"] == inj["n_nodes"] == 5 and dev["nchild"][0] == 4
        assert np.array_equal(dev["prior"], inj["prior"])
        assert np.array_equal(dev["action"], inj["action"])
        distinct.add(dev["prior"][1:5].tobytes())
    assert len(distinct) == len(trees[0])  # the noise reached the priors: no two slots agree


def asymmetric_root():
    c = load_golden("board_corpus.npz")
    i = np.nonzero((c["game"] == 1) & (c["ply"] == 11))[0][0]
    player = int(c["player"][i])
    pos, neg = int(c["pos"][i]), int(c["neg"][i])
    own, opp = (pos, neg) if player == 1 else (neg, pos)
    images = {(int(nat.d4_cpu([own], s)[0]), int(nat.d4_cpu([opp], s)[0])) for s in range(8)}
    assert len(images) == 8  # no symmetry: the transform shows in the packed row
    return own, opp, player


def planes_of(own, opp, sym):
    """The canonical planes of boards (own to move) seen through D4 element sym, per row."""
    p, n = nat.d4_cpu(own, sym), nat.d4_cpu(opp, sym)
    return (((p[:, None] & W64) != 0).astype(np.float32)
            - ((n[:, None] & W64) != 0).astype(np.float32))


@pytest.mark.parametrize("K", [1, 4])
def test_d4_draw_uses_its_counter(K):
    """Each packed leaf is seen through sym = floor(8 u), u the slot's draw at sub 0x5000 of
    its next event: event 0 for the root; the root's expansion then takes event 1 for its
    noise, and the next select's leaves take events 2, 3, ... in row order."""
    G, seed, stream, alpha = 1024, SEED, 3, 1.0
    own, opp, player = asymmetric_root()
    e = Engine(G, 16, c_puct=2.0, dirichlet_alpha=alpha, dirichlet_epsilon=0.3, d4_augment=True,
               auto_play=False, seed=seed, stream_id=stream, leaves_per_step=K)
    slots = np.arange(G, dtype=np.int32)
    e.set_roots(slots, np.full(G, own, np.uint64), np.full(G, opp, np.uint64),
                np.full(G, player, np.int32))
    e.begin_search_slots(slots, 16)

    def sym_at(event):
        u = nat.rng_uniform_gpu(seed, stream, 0, G, event, 0x5000).cpu().numpy()[:, 0]
        return np.floor(8.0 * u).astype(np.uint8)

    e.select()
    rows = e.nn_in.cpu().numpy().reshape(G, K, 64)
    leaf = e.leaf.cpu().numpy().reshape(G, K)
    sym0 = sym_at(0)
    assert (leaf[:, 0] == 0).all() and (leaf[:, 1:] == -1).all()
    assert np.array_equal(rows[:, 0], planes_of(np.full(G, own, np.uint64),
                                                np.full(G, opp, np.uint64), sym0))
    assert (rows[:, 1:] == 0).all()
    # |z| <= 4.5 per category against 1/8, as tests/test_rollout_gpu.py tests its categories
    for s in range(8):
        z = ((sym0 == s).mean() - 0.125) / math.sqrt(0.125 * 0.875 / G)
        assert abs(z) <= 4.5, (s, z)

    pr, va = mock_eval_torch(e.nn_in)
    e.priors.copy_(pr)
    e.values.copy_(va)
    e.expand()
    e.play()
    e.select()
    rows = e.nn_in.cpu().numpy().reshape(G, K, 64)
    leaf = e.leaf.cpu().numpy().reshape(G, K)
    legal = int(nat.legal_cpu([own], [opp])[0])
    acts = np.array([a for a in range(64) if (legal >> a) & 1], np.uint8)
    assert len(acts) >= 4
    c_own, c_opp, _, _ = nat.step_cpu(np.full(len(acts), own, np.uint64),
                                      np.full(len(acts), opp, np.uint64), acts)
    # the root's children are nodes 1 .. in ascending action order, none terminal here
    assert (leaf >= 1).all() and (leaf <= len(acts)).all()
    for j in range(K):
        child = leaf[:, j] - 1
        assert np.array_equal(rows[:, j], planes_of(c_own[child], c_opp[child], sym_at(2 + j))), j
    e.close()


def game_keys(s):
    """One key per finished game: the game's board sequence (which the move sequence
    determines).  Rows of a game are contiguous in the sample buffer and start at the
    initial position, which occurs nowhere else in a game."""
    start = np.flatnonzero((s["own"] == np.uint64(INIT_OWN)) & (s["opp"] == np.uint64(INIT_OPP)))
    assert len(start) and start[0] == 0
    end = np.r_[start[1:], len(s["own"])]
    keys = []
    for a, b in zip(start, end):
        assert (s["slot"][a:b] == s["slot"][a]).all() and b - a >= 9
        keys.append((int(s["slot"][a]), s["own"][a:b].tobytes() + s["opp"][a:b].tobytes()))
    return keys


SP_ARGS = {"c_puct": 2.0, "num_simulations": 8, "dirichlet_alpha": 1.0, "dirichlet_epsilon": 0.3,
           "mcts_temperature": 1.0, "num_exploratory_moves": 35, "lambda": 0.98}


def test_no_game_is_played_twice():
    """512 finished games on 256 refilled slots: all different (a slot's consecutive games
    included: a restart must not rewind the slot's event counter), none shared between
    streams 0 and 1, between the two pipelines of a PipelinedSelfPlay, or between those and
    pipeline 0 of the next stream id."""
    G, n_games = 256, 512
    games = {}
    for stream in (0, 1):
        sp = BatchedSelfPlay(MockNet(), SP_ARGS, G, seed=SEED, stream_id=stream, fold=False,
                             sample_capacity=n_games * 96)
        sp.play_games(n_games)
        keys = game_keys(sp.engine.samples())
        assert len(keys) == n_games
        assert max(np.bincount([k[0] for k in keys], minlength=G)) >= 2  # slots were refilled
        games[stream] = {k[1] for k in keys}
        assert len(games[stream]) == n_games
        sp.engine.close()
    assert not games[0] & games[1]

    pipes = {}
    for stream in (0, 1):
        pp = PipelinedSelfPlay(MockNet(), SP_ARGS, 2 * G, pipelines=2, seed=SEED,
                               stream_id=stream, fold=False, sample_capacity=n_games * 96)
        rows = pp.play_games(2 * n_games, tuples=False)
        for i in range(2):
            part = {k: v[(rows["slot"] // G) == i] for k, v in rows.items()}
            keys = game_keys(part)
            assert len(keys) == n_games
            pipes[stream, i] = {k[1] for k in keys}
            assert len(pipes[stream, i]) == n_games
        for p in pp.parts:
            p.engine.close()
    assert not pipes[0, 0] & pipes[0, 1]
    assert not (pipes[0, 0] | pipes[0, 1]) & pipes[1, 0]
