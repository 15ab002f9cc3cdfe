"""Exact endgame solver on the device (oth_solve_gpu, csrc/solve.hip) against the host
solver, which tests/test_solve_cpu.py proves exact: the same search code runs on both, so
with split_plies = 0 even the node counts are equal; the split front end must give the same
scores and best moves.  Every call passes node_limit = 2^24 (the hardest 10-empties corpus
position needs under 10^6 nodes), so a runaway search ends as AZ_SOLVE_ABORTED and a failed
assertion within seconds."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_golden

nat = pytest.importorskip("az_native")
pytestmark = pytest.mark.gpu

LIMIT = 1 << 24


def popc(x):
    x = np.ascontiguousarray(x, np.uint64)
    return np.unpackbits(x.view(np.uint8).reshape(-1, 8), axis=1).sum(axis=1).astype(np.int64)


def dev_i64(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).cuda()


def raw_solve(own_t, opp_t, max_empties, limit, split, score_t, best_t, nodes_t):
    """oth_solve_gpu on the given device tensors (any element offset), current stream."""
    n = own_t.numel()
    need = ctypes.c_size_t(0)
    nat.check(nat.lib.oth_solve_gpu(None, None, n, max_empties, limit, split, None, None, None,
                                    None, ctypes.byref(need), None), "oth_solve_gpu")
    ws = torch.empty(max(need.value, 8), dtype=torch.uint8, device="cuda")
    nat.check(nat.lib.oth_solve_gpu(nat.ptr(own_t), nat.ptr(opp_t), n, max_empties, limit, split,
                                    nat.ptr(score_t), nat.ptr(best_t), nat.ptr(nodes_t),
                                    nat.ptr(ws), ctypes.byref(need), nat.stream_ptr()),
              "oth_solve_gpu")
    torch.cuda.synchronize()


def gpu_solve(own, opp, max_empties, limit=LIMIT, split=0):
    n = len(own)
    s = torch.full((n,), 99, dtype=torch.int8, device="cuda")
    b = torch.full((n,), 99, dtype=torch.uint8, device="cuda")
    nd = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    raw_solve(dev_i64(own), dev_i64(opp), max_empties, limit, split, s, b, nd)
    return s.cpu().numpy(), b.cpu().numpy(), nd.cpu().numpy().view(np.uint64)


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
    """Every corpus position with 1..10 empties and the host solver's results (computed once)."""
    import endgame

    m = (corpus["emp"] >= 1) & (corpus["emp"] <= 10)
    own, opp = corpus["own"][m], corpus["opp"][m]
    assert 6000 < len(own) < 6600
    s, b, nd = endgame.solve(own, opp, 10, device="cpu", node_limit=LIMIT)
    assert (s > -127).all()
    return {"own": own, "opp": opp, "emp": corpus["emp"][m], "score": s, "best": b, "nodes": nd}


def test_parity_with_cpu_one_call(late):
    s, b, nd = gpu_solve(late["own"], late["opp"], 10, split=0)
    assert (s == late["score"]).all()
    assert (b == late["best"]).all()
    assert (nd == late["nodes"]).all()


@pytest.mark.parametrize("split", [1, 2])
def test_split_parity_with_cpu(late, split):
    s, b, nd = gpu_solve(late["own"], late["opp"], 10, split=split)
    assert (s == late["score"]).all()
    assert (b == late["best"]).all()
    # unsplit roots are the same single search; a split root's count covers its whole tree
    small = late["emp"] < 9
    assert (nd[small] == late["nodes"][small]).all()
    assert (nd[~small] > 1).all()


def mixed_batch(corpus, n):
    """n positions cycling through skipped (many empties, overlapping), terminal, pass-only
    and 1..8-empties positions, so neighbouring lanes finish at very different times."""
    own, opp, emp = corpus["own"], corpus["opp"], corpus["emp"]
    lg, lg2 = nat.legal_cpu(own, opp), nat.legal_cpu(opp, own)
    kinds = [np.flatnonzero(emp >= 20), np.flatnonzero(emp == 8),
             np.flatnonzero((emp <= 8) & (lg == 0) & (lg2 != 0)), np.flatnonzero(emp == 1),
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


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("split", [0, 2])
def test_awkward_batch_sizes(corpus, n, split):
    own, opp = mixed_batch(corpus, n)
    ws, wb, wn = nat.solve_cpu(own, opp, 8, node_limit=LIMIT)
    if n >= 63:
        assert (ws == -128).sum() >= n // 8 and (wb == 64).sum() >= n // 8
    s, b, nd = gpu_solve(own, opp, 8, split=split)
    assert (s == ws).all() and (b == wb).all()
    if split == 0:
        assert (nd == wn).all()


def test_one_hard_position_among_trivial_ones(corpus, late):
    hard = int(np.argmax(np.where(late["emp"] == 10, late["nodes"], 0)))
    ones = np.flatnonzero(corpus["emp"] == 1)[:63]
    own = np.concatenate([corpus["own"][ones[:20]], late["own"][hard:hard + 1],
                          corpus["own"][ones[20:]]])
    opp = np.concatenate([corpus["opp"][ones[:20]], late["opp"][hard:hard + 1],
                          corpus["opp"][ones[20:]]])
    assert len(own) == 64
    ws, wb, wn = nat.solve_cpu(own, opp, 10, node_limit=LIMIT)
    assert wn[20] == late["nodes"][hard] and wn[20] > 1000 * wn[0]
    for split in (0, 1, 2):
        s, b, nd = gpu_solve(own, opp, 10, split=split)
        assert (s == ws).all() and (b == wb).all()
        if split == 0:
            assert (nd == wn).all()


@pytest.mark.parametrize("split", [0, 1])
def test_unaligned_buffers(corpus, split):
    own, opp = mixed_batch(corpus, 130)
    ws, wb, wn = nat.solve_cpu(own, opp, 8, node_limit=LIMIT)
    n = len(own)
    pad = np.zeros(1, np.uint64)
    own_t = dev_i64(np.concatenate([pad, own]))[1:]
    opp_t = dev_i64(np.concatenate([pad, opp]))[1:]
    s = torch.full((n + 2,), 99, dtype=torch.int8, device="cuda")
    b = torch.full((n + 2,), 99, dtype=torch.uint8, device="cuda")
    nd = torch.full((n + 2,), -1, dtype=torch.int64, device="cuda")
    raw_solve(own_t, opp_t, 8, LIMIT, split, s[1:n + 1], b[1:n + 1], nd[1:n + 1])
    assert own_t.data_ptr() % 16 == 8 and s[1:].data_ptr() % 2 == 1
    s, b, nd = s.cpu().numpy(), b.cpu().numpy(), nd.cpu().numpy()
    assert (s[1:n + 1] == ws).all() and (b[1:n + 1] == wb).all()
    if split == 0:
        assert (nd[1:n + 1].view(np.uint64) == wn).all()
    # nothing outside the n results was written
    assert s[0] == 99 and s[n + 1] == 99 and b[0] == 99 and b[n + 1] == 99
    assert nd[0] == -1 and nd[n + 1] == -1


def test_abort_code_matches_cpu(late):
    m = late["emp"] <= 8
    own, opp = late["own"][m], late["opp"][m]
    ws, wb, wn = nat.solve_cpu(own, opp, 8, node_limit=10)
    assert 0 < (ws == -127).sum() < len(ws)
    s, b, nd = gpu_solve(own, opp, 8, limit=10, split=0)
    assert ((s == -127) == (ws == -127)).all()
    assert (s == ws).all() and (b == wb).all() and (nd == wn).all()
    # a split root with an aborted leaf is aborted; roots that finish keep their result
    s2, b2, _ = gpu_solve(late["own"], late["opp"], 10, limit=10, split=2)
    done = s2 != -127
    assert (~done).any() and done.any()
    assert (s2[done] == late["score"][done]).all() and (b2[done] == late["best"][done]).all()
    assert (b2[~done] == 255).all()


def test_argument_errors():
    need = ctypes.c_size_t(0)
    q = lambda **k: nat.lib.oth_solve_gpu(None, None, k.get("n", 4), k.get("me", 12), 100,
                                          k.get("split", 0), None, None, None, None,
                                          ctypes.byref(need), None)
    assert q() == nat.AZ_OK and need.value > 0
    assert q(me=15) == nat.AZ_ERR_ARG
    assert q(split=3) == nat.AZ_ERR_ARG
    assert q(n=-1) == nat.AZ_ERR_ARG
    assert q(n=1 << 20, me=14, split=2) == nat.AZ_OK
    bounded = need.value
    assert q(n=1 << 24, me=14, split=2) == nat.AZ_OK and need.value == bounded  # chunked


def test_python_surface_on_device(late):
    import endgame

    m = late["emp"] <= 8
    own, opp = late["own"][m], late["opp"][m]
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        o_t, p_t = dev_i64(own), dev_i64(opp)
        s, b, nd = endgame.solve(o_t, p_t, 8, node_limit=LIMIT)
    stream.synchronize()
    assert s.is_cuda and s.dtype == torch.int8 and b.dtype == torch.uint8
    assert (s.cpu().numpy() == late["score"][m]).all()
    assert (b.cpu().numpy() == late["best"][m]).all()
    # numpy in, numpy out, the default split
    s, b, nd = endgame.solve(own, opp, 8, node_limit=LIMIT)
    assert isinstance(s, np.ndarray) and nd.dtype == np.uint64
    assert (s == late["score"][m]).all() and (b == late["best"][m]).all()
    s0 = endgame.solve(own, opp, 8, node_limit=LIMIT, split_plies=0)
    assert (s0[2] == late["nodes"][m]).all()
    # rows: late positions with a placement mixed with early ones, pi on a fixed legal move
    lg = nat.legal_cpu(own, opp)
    keep = lg != 0
    ro, rp, lg = own[keep][:1500], opp[keep][:1500], lg[keep][:1500]
    hi = np.array([int(x).bit_length() - 1 for x in lg])
    pi = np.zeros((len(ro), 65), np.float32)
    pi[np.arange(len(ro)), hi] = 1.0
    rows = {"own": ro, "opp": rp, "pi": pi, "z": np.linspace(-1, 1, len(ro)),
            "player": np.ones(len(ro), np.int8)}
    g_rows, g_mask = endgame.relabel_rows(rows, 8, device="cuda")
    c_rows, c_mask = endgame.relabel_rows(rows, 8, device="cpu")
    assert g_mask.all() and (g_mask == c_mask).all() and (g_rows["z"] == c_rows["z"]).all()
    assert (g_rows["z"] == np.sign(late["score"][m][keep][:1500].astype(np.int64))).all()
    g_rep = endgame.move_report(rows, 8, device="cuda")
    c_rep = endgame.move_report(rows, 8, device="cpu")
    assert g_rep == c_rep and g_rep["total"]["n"] == len(ro)
    assert 0.0 < g_rep["total"]["optimal_frac"] < 1.0 and g_rep["total"]["mean_disc_loss"] > 0


class _IntMockNet(torch.nn.Module):
    """tests/mock_policy.py's closed-form policy as a module collect_self_play_games can copy
    for inference: the matrices are integer buffers, which the copy's cast to float32 leaves
    alone (MockNet's float64 buffers would be narrowed)."""

    def __init__(self):
        super().__init__()
        from mock_policy import A, B

        self.register_buffer("At", torch.as_tensor(A.T.copy(), dtype=torch.int64))
        self.register_buffer("Bt", torch.as_tensor(B.copy(), dtype=torch.int64))

    def evaluate_into(self, planes, priors, values):
        x = torch.round(planes.double()) + 1.0
        h = torch.remainder(x @ self.At.double(), 1021.0) + 1.0
        k = torch.remainder(x @ self.Bt.double(), 2001.0)
        priors.copy_((h / 1024.0).float())
        values.copy_(((k - 1000.0) / 1024.0).float())


def test_self_play_exact_endgame():
    import self_play_worker as spw

    args = {"c_puct": 2.0, "num_simulations": 25, "dirichlet_alpha": 1.0,
            "dirichlet_epsilon": 0.3, "mcts_temperature": 1.0, "num_exploratory_moves": 10,
            "lambda": 0.98, "num_threads": 1}
    net = _IntMockNet()
    plain = spw.collect_self_play_games(net, args, 8, n_slots=8, seed=11, exact_endgame=0)
    exact = spw.collect_self_play_games(net, args, 8, n_slots=8, seed=11, exact_endgame=6)
    assert len(plain) == len(exact) > 8 * 50
    # the same games both times; rows of games that end in the same step may swap places.
    # Rows with equal state and pi (the first plies of two games) are ordered by z: early rows
    # keep their z in both calls, and late rows with equal state get equal exact z
    by_row = lambda t: (t[0].tobytes() + t[1].tobytes(), t[2])
    plain, exact = sorted(plain, key=by_row), sorted(exact, key=by_row)
    states = np.stack([t[0] for t in exact]).reshape(-1, 64)
    assert (states == np.stack([t[0] for t in plain]).reshape(-1, 64)).all()
    own, opp = nat.pack_np(states, 1)
    emp = 64 - popc(own | opp)
    late = (emp >= 1) & (emp <= 6)
    assert late.sum() >= 8 * 4
    score, _, _ = nat.solve_cpu(own[late], opp[late], 6)
    z_exact = np.array([t[2] for t in exact])
    z_plain = np.array([t[2] for t in plain])
    assert (z_exact[late] == np.sign(score.astype(np.int64))).all()
    assert set(np.unique(z_exact[late])) <= {-1.0, 0.0, 1.0}
    assert (z_exact[~late] == z_plain[~late]).all()
    for a, b in zip(plain, exact):
        assert (a[1] == b[1]).all()
