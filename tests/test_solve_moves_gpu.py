"""The exact value of every move on the device (endgame.solve_moves on cuda: composed from
oth_legal_gpu, oth_step_gpu and oth_solve_deep_gpu) against the host's oth_solve_moves_cpu
(tests/test_solve_moves_cpu.py checks that one against an independent composition): the same
searches run on both sides, so values, scores and node counts are equal bit for bit.  Every
call passes a node limit, so a runaway search ends as AZ_SOLVE_ABORTED and a failed assertion
within seconds."""
import numpy as np
import pytest
import torch

from conftest import load_golden

nat = pytest.importorskip("az_native")
pytestmark = pytest.mark.gpu

LIMIT = 1 << 24
NONE = -128
SCORES, WLD, OPTIMAL = 0, 1, 2
MODES = [SCORES, WLD, OPTIMAL]


def popc(x):
    x = np.ascontiguousarray(x, np.uint64)
    return np.unpackbits(x.view(np.uint8).reshape(-1, 8), axis=1).sum(axis=1).astype(np.int64)


def dev_i64(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).cuda()


def gpu_moves(own, opp, max_empties, mode, limit=LIMIT):
    import endgame

    v, s, nd = endgame.solve_moves_gpu_tensors(dev_i64(own), dev_i64(opp), max_empties, mode,
                                               limit)
    torch.cuda.synchronize()
    return v.cpu().numpy(), s.cpu().numpy(), nd.cpu().numpy().view(np.uint64)


def same(got, want):
    return all((a == b).all() for a, b in zip(got, want))


@pytest.fixture(scope="module")
def corpus():
    d = load_golden("board_corpus.npz")
    own = np.where(d["player"] == 1, d["pos"], d["neg"]).astype(np.uint64)
    opp = np.where(d["player"] == 1, d["neg"], d["pos"]).astype(np.uint64)
    end = d["term_next"] == 1
    town = np.where(d["player"] == 1, d["nneg"], d["npos"])[end].astype(np.uint64)
    topp = np.where(d["player"] == 1, d["npos"], d["nneg"])[end].astype(np.uint64)
    return {"own": own, "opp": opp, "emp": 64 - popc(own | opp), "town": town, "topp": topp}


@pytest.fixture(scope="module")
def late(corpus):
    """Every corpus position with 1..10 empties with the host's results in the three modes."""
    import endgame

    m = (corpus["emp"] >= 1) & (corpus["emp"] <= 10)
    own, opp = corpus["own"][m], corpus["opp"][m]
    assert 6000 < len(own) < 6600
    names = {SCORES: "scores", WLD: "wld", OPTIMAL: "optimal"}
    host = {mode: endgame.solve_moves(own, opp, 10, mode=names[mode], device="cpu",
                                      node_limit=LIMIT) for mode in MODES}
    assert (host[SCORES][1] > -127).all()
    return {"own": own, "opp": opp, "emp": corpus["emp"][m], "host": host}


def mixed_batch(corpus, n):
    """n roots cycling through skipped (many empties, overlapping), terminal, pass-only and
    1..9-empties positions."""
    own, opp, emp = corpus["own"], corpus["opp"], corpus["emp"]
    lg, lg2 = nat.legal_cpu(own, opp), nat.legal_cpu(opp, own)
    kinds = [np.flatnonzero(emp >= 21), np.flatnonzero(emp == 9),
             np.flatnonzero((emp <= 9) & (lg == 0) & (lg2 != 0)), np.flatnonzero(emp == 1),
             None, np.flatnonzero(emp == 5), np.flatnonzero(emp == 7), np.flatnonzero(emp == 3)]
    o, p = [], []
    for i in range(n):
        k = kinds[i % len(kinds)]
        if k is None:  # a terminal position; every other one with overlapping boards instead
            j = (i // len(kinds)) % len(corpus["town"])
            to, tp = corpus["town"][j], corpus["topp"][j]
            o.append(to | (tp if (i // len(kinds)) % 2 else np.uint64(0)))
            p.append(tp)
        else:
            j = k[(i // len(kinds)) % len(k)]
            o.append(own[j])
            p.append(opp[j])
    return np.array(o, np.uint64), np.array(p, np.uint64)


@pytest.mark.parametrize("mode", MODES)
def test_parity_with_host(late, mode):
    got = gpu_moves(late["own"], late["opp"], 10, mode)
    assert same(got, late["host"][mode])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_batch_sizes(corpus, n, mode):
    own, opp = mixed_batch(corpus, max(n, 2))
    if n == 1:  # the 9-empties position alone
        own, opp = own[1:], opp[1:]
    want = nat.solve_moves_cpu(own, opp, 9, mode, node_limit=LIMIT)
    if n > 8:
        assert (want[1] == -128).sum() >= n // 8 and (want[0][:, 64] != NONE).sum() >= n // 9
    assert same(gpu_moves(own, opp, 9, mode), want)


@pytest.mark.parametrize("mode", MODES)
def test_node_limit_parity(late, mode):
    m = late["emp"] <= 8
    own, opp = late["own"][m], late["opp"][m]
    want = nat.solve_moves_cpu(own, opp, 8, mode, node_limit=10)
    ab = want[1] == -127
    assert 0 < ab.sum() < len(ab)
    got = gpu_moves(own, opp, 8, mode, limit=10)
    assert same(got, want)
    assert (got[0][ab] == NONE).all()
    assert same(gpu_moves(own, opp, 8, mode, limit=10), got)  # the same bits on a second run


@pytest.fixture(scope="module")
def deep_sets(corpus):
    """16 corpus roots at 14 empties and 8 at 16 empties (a fixed stride)."""
    out = {}
    for e, k in ((14, 16), (16, 8)):
        idx = np.flatnonzero(corpus["emp"] == e)
        i = idx[::len(idx) // k][:k]
        assert len(i) == k
        out[e] = (corpus["own"][i], corpus["opp"][i])
    return out


@pytest.mark.parametrize("e,mode", [(14, SCORES), (14, WLD), (14, OPTIMAL), (16, WLD)])
def test_deeper_roots(deep_sets, e, mode):
    import endgame

    own, opp = deep_sets[e]
    name = {SCORES: "scores", WLD: "wld", OPTIMAL: "optimal"}[mode]
    want = endgame.solve_moves(own, opp, e, mode=name, device="cpu", node_limit=1 << 22)
    print(f"{e} empties, {name}: host nodes {int(want[2].sum())}, hardest root "
          f"{int(want[2].max())}, {int((want[1] == -127).sum())} of {len(own)} aborted")
    assert (want[1] > -127).sum() >= len(own) // 2
    assert same(gpu_moves(own, opp, e, mode, limit=1 << 22), want)


def test_tensor_round_trip(late):
    import endgame

    m = late["emp"] <= 9
    own, opp = late["own"][m][:500], late["opp"][m][:500]
    want = nat.solve_moves_cpu(own, opp, 9, SCORES, node_limit=LIMIT)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        o_t, p_t = dev_i64(own), dev_i64(opp)
        v, s, nd = endgame.solve_moves(o_t, p_t, 9, node_limit=LIMIT)
        pi = endgame.exact_policy(v)
    stream.synchronize()
    assert v.is_cuda and v.dtype == torch.int8 and tuple(v.shape) == (500, 65)
    assert s.dtype == torch.int8 and nd.dtype == torch.int64
    assert same((v.cpu().numpy(), s.cpu().numpy(), nd.cpu().numpy().view(np.uint64)), want)
    assert pi.is_cuda and (pi.cpu().numpy() == endgame.exact_policy(want[0])).all()
    # numpy in, numpy out on the device
    v, s, nd = endgame.solve_moves(own, opp, 9, mode="optimal", node_limit=LIMIT)
    assert isinstance(v, np.ndarray) and nd.dtype == np.uint64
    assert same((v, s, nd), nat.solve_moves_cpu(own, opp, 9, OPTIMAL, node_limit=LIMIT))
    e = torch.empty(0, dtype=torch.int64, device="cuda")
    v, s, nd = endgame.solve_moves(e, e, 12)
    assert tuple(v.shape) == (0, 65) and s.numel() == 0 and nd.numel() == 0
    with pytest.raises(RuntimeError, match="max_empties"):
        endgame.solve_moves(o_t, p_t, 21)
    with pytest.raises(ValueError, match="mode"):
        endgame.solve_moves(o_t, p_t, 9, mode="best")


@pytest.mark.parametrize("wld", [False, True])
def test_relabel_rows_policy_on_device(late, wld):
    import endgame

    own, opp = late["own"][::4], late["opp"][::4]
    pi = np.random.default_rng(3).random((len(own), 65)).astype(np.float32)
    rows = {"own": own, "opp": opp, "pi": pi, "z": np.linspace(-1, 1, len(own)),
            "player": np.ones(len(own), np.int8)}
    g_rows, g_mask = endgame.relabel_rows(rows, 10, device="cuda", wld=wld, policy=True)
    c_rows, c_mask = endgame.relabel_rows(rows, 10, device="cpu", wld=wld, policy=True)
    assert g_mask.all() and (g_mask == c_mask).all()
    assert (g_rows["z"] == c_rows["z"]).all() and (g_rows["pi"] == c_rows["pi"]).all()
    assert (g_rows["pi"] != pi).any() and g_rows["pi"] is not rows["pi"]
    assert (g_rows["z"] == endgame.relabel_rows(rows, 10, device="cuda", wld=wld)[0]["z"]).all()
    rep_g = endgame.policy_report(rows, 10, device="cuda")
    assert rep_g == endgame.policy_report(rows, 10, device="cpu")


def test_self_play_exact_policy():
    """8 games on 8 slots: only the late rows' pi and z differ from the plain run."""
    import endgame
    import self_play_worker as spw
    from test_solve_gpu import _IntMockNet

    args = {"c_puct": 2.0, "num_simulations": 25, "dirichlet_alpha": 1.0,
            "dirichlet_epsilon": 0.3, "mcts_temperature": 1.0, "num_exploratory_moves": 10,
            "lambda": 0.98, "num_threads": 1}
    net = _IntMockNet()
    plain = spw.collect_self_play_games(net, args, 8, n_slots=8, seed=11, exact_endgame=0)
    exact = spw.collect_self_play_games(net, args, 8, n_slots=8, seed=11, exact_endgame=6,
                                        exact_policy=True)
    assert len(plain) == len(exact) > 8 * 50

    def split(rows):
        states = np.stack([t[0] for t in rows]).reshape(-1, 64)
        own, opp = nat.pack_np(states, 1)
        emp = 64 - popc(own | opp)
        late = (emp >= 1) & (emp <= 6)
        return own, opp, late

    key = lambda t: (t[0].tobytes(), t[1].tobytes(), t[2])
    po, pp, pl = split(plain)
    eo, ep, el = split(exact)
    assert pl.sum() == el.sum() >= 8 * 4
    # the other rows: the same multiset of (state, pi, z)
    assert sorted(key(t) for t, l in zip(plain, pl) if not l) == \
        sorted(key(t) for t, l in zip(exact, el) if not l)
    # the late rows: the same positions, with the exact targets
    assert sorted(zip(po[pl].tolist(), pp[pl].tolist())) == \
        sorted(zip(eo[el].tolist(), ep[el].tolist()))
    v, s, _ = nat.solve_moves_cpu(eo[el], ep[el], 6, SCORES)
    want_pi = endgame.exact_policy(v)
    has = (v != NONE).any(axis=1)
    assert has.any()
    got_pi = np.stack([t[1] for t, l in zip(exact, el) if l])
    got_z = np.array([t[2] for t, l in zip(exact, el) if l])
    assert (got_pi[has] == want_pi[has]).all()
    assert (got_z == np.sign(s.astype(np.int64))).all()
    plain_pi = {t[0].tobytes(): t[1] for t, l in zip(plain, pl) if l}
    differs = sum(int((t[1] != plain_pi[t[0].tobytes()]).any()) for t, l in zip(exact, el) if l)
    assert differs > 0
