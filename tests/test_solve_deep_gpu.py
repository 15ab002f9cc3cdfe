"""Windowed, move-ordered endgame solver on the device (oth_solve_deep_gpu,
csrc/solve_deep.hip) against the host's (tests/test_solve_deep_cpu.py checks that one against
the proven solver): the same search code runs on both, so with split_plies = 0 score, best
and node counts are equal; the split front end must stay within the window contract.  Every
call passes a node limit, so a runaway search ends as AZ_SOLVE_ABORTED and a failed assertion
within seconds."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_golden

nat = pytest.importorskip("az_native")
pytestmark = pytest.mark.gpu

LIMIT = 1 << 24
FULL, WLD = (-65, 65), (-1, 1)


def popc(x):
    x = np.ascontiguousarray(x, np.uint64)
    return np.unpackbits(x.view(np.uint8).reshape(-1, 8), axis=1).sum(axis=1).astype(np.int64)


def dev_i64(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).cuda()


def raw_solve(own_t, opp_t, max_empties, window, limit, split, score_t, best_t, nodes_t,
              stream=None):
    """oth_solve_deep_gpu on the given device tensors (any element offset)."""
    n = own_t.numel()
    need = ctypes.c_size_t(0)
    f = nat.lib.oth_solve_deep_gpu
    nat.check(f(None, None, n, max_empties, *window, limit, split, None, None, None, None,
                ctypes.byref(need), None), "oth_solve_deep_gpu")
    ws = torch.empty(max(need.value, 8), dtype=torch.uint8, device="cuda")
    nat.check(f(nat.ptr(own_t), nat.ptr(opp_t), n, max_empties, *window, limit, split,
                nat.ptr(score_t), nat.ptr(best_t), nat.ptr(nodes_t), nat.ptr(ws),
                ctypes.byref(need), nat.stream_ptr(stream)), "oth_solve_deep_gpu")
    torch.cuda.synchronize()


def gpu_solve(own, opp, max_empties, window=FULL, limit=LIMIT, split=0):
    n = len(own)
    s = torch.full((n,), 99, dtype=torch.int8, device="cuda")
    b = torch.full((n,), 99, dtype=torch.uint8, device="cuda")
    nd = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    raw_solve(dev_i64(own), dev_i64(opp), max_empties, window, limit, split, s, b, nd)
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
    """Every corpus position with 1..10 empties with the host's results in both windows, and
    the exact value of every action at every root (1000 where the action is no child)."""
    import endgame

    m = (corpus["emp"] >= 1) & (corpus["emp"] <= 10)
    own, opp = corpus["own"][m], corpus["opp"][m]
    n = len(own)
    assert 6000 < n < 6600
    host = {w: endgame.solve_deep(own, opp, 10, window=w, device="cpu", node_limit=LIMIT)
            for w in (FULL, WLD)}
    assert (host[FULL][0] > -127).all()
    lg = nat.legal_cpu(own, opp)
    passer = (lg == 0) & (nat.legal_cpu(opp, own) != 0)
    par, act = np.nonzero(((lg[:, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1))
                          .astype(bool))
    par = np.concatenate([par, np.flatnonzero(passer)])
    act = np.concatenate([act, np.full(passer.sum(), 64)]).astype(np.uint8)
    co, cp, _, _ = nat.step_cpu(own[par], opp[par], act)
    cs = endgame.solve_deep(co, cp, 10, device="cpu", node_limit=LIMIT)[0].astype(np.int64)
    value = np.full((n, 65), 1000, np.int64)
    value[par, act] = -cs
    return {"own": own, "opp": opp, "emp": corpus["emp"][m], "host": host, "lg": lg,
            "value": value, "score": host[FULL][0].astype(np.int64)}


@pytest.mark.parametrize("window", [FULL, WLD])
def test_parity_with_host_split_0(late, window):
    s, b, nd = gpu_solve(late["own"], late["opp"], 10, window, split=0)
    hs, hb, hn = late["host"][window]
    assert (s == hs).all()
    assert (b == hb).all()
    assert (nd == hn).all()


def check_contract(late, s, b, window, done=None):
    """Window contract of scores against the host's exact ones, and best by its exact value."""
    alpha, beta = window
    done = np.ones(len(s), bool) if done is None else done
    v, t = s.astype(np.int64)[done], late["score"][done]
    inside, high, low = (alpha < t) & (t < beta), t >= beta, t <= alpha
    assert (v[inside] == t[inside]).all()
    assert ((beta <= v[high]) & (v[high] <= t[high])).all()
    assert ((t[low] <= v[low]) & (v[low] <= alpha)).all()
    lg, bb = late["lg"][done], b[done]
    has = lg != 0
    assert (bb[~has] == 64).all() and (bb[has] < 64).all()
    assert (((lg[has] >> bb[has].astype(np.uint64)) & np.uint64(1)) == 1).all()
    bv = late["value"][done][np.arange(done.sum()), np.minimum(bb, 64)]
    exact = has & (alpha < v) & (v < beta)
    assert (bv[exact] == t[exact]).all()
    assert (bv[has & (v >= beta)] >= beta).all()


@pytest.mark.parametrize("window", [FULL, WLD, (2, 9)])
@pytest.mark.parametrize("split", [1, 2])
def test_splits_keep_the_window_contract(late, split, window):
    s, b, nd = gpu_solve(late["own"], late["opp"], 10, window, split=split)
    assert (s > -127).all()
    check_contract(late, s, b, window)
    if window == FULL:
        assert (s == late["host"][FULL][0]).all()
    if window == WLD:
        assert (np.sign(s) == np.sign(late["score"])).all()
    # unsplit roots are the same single search; a split root's count covers its whole tree
    if window in late["host"]:
        small = late["emp"] < 9
        assert (nd[small] == late["host"][window][2][small]).all()
        assert (nd[~small] > 1).all()


def test_abort_code(late):
    m = late["emp"] <= 8
    own, opp = late["own"][m], late["opp"][m]
    ws, wb, wn = nat.solve_deep_cpu(own, opp, 8, node_limit=10)
    assert 0 < (ws == -127).sum() < len(ws)
    s, b, nd = gpu_solve(own, opp, 8, limit=10, split=0)
    assert (s == ws).all() and (b == wb).all() and (nd == wn).all()
    # a split root with an aborted leaf is aborted; roots that finish keep the contract
    for window in (FULL, WLD):
        s2, b2, _ = gpu_solve(late["own"], late["opp"], 10, window, limit=10, split=2)
        done = s2 != -127
        assert (~done).any() and done.any()
        assert (b2[~done] == 255).all()
        check_contract(late, s2, b2, window, done)


@pytest.fixture(scope="module")
def deep_sets(corpus):
    """32 corpus positions each at 14 and 16 empties (a fixed stride) with the host's win /
    draw / loss results at node_limit 2^22."""
    import endgame

    out = {}
    for e in (14, 16):
        idx = np.flatnonzero(corpus["emp"] == e)
        i = idx[::len(idx) // 32][:32]
        assert len(i) == 32
        own, opp = corpus["own"][i], corpus["opp"][i]
        s, b, nd = endgame.solve_deep(own, opp, e, window="wld", device="cpu", node_limit=1 << 22)
        out[e] = (own, opp, s, b, nd)
    return out


@pytest.mark.parametrize("e", [14, 16])
def test_beyond_the_old_cap(deep_sets, e):
    import endgame

    own, opp, hs, hb, hn = deep_sets[e]
    take = (hs > -127) & (hn <= (1 << 21))
    print(f"{e} empties: host nodes max {int(hn.max())}, mean {float(hn.mean()):.0f}, "
          f"{int((~take).sum())} of 32 excluded")
    assert (~take).sum() <= 8
    own, opp, hs, hb, hn = own[take], opp[take], hs[take], hb[take], hn[take]
    s, b, nd = gpu_solve(own, opp, e, WLD, limit=1 << 22, split=0)
    assert (s == hs).all() and (b == hb).all() and (nd == hn).all()
    # the default split: every participating root is solved, with the host's sign
    s, b, nd = gpu_solve(own, opp, e, WLD, limit=1 << 22, split=endgame.DEFAULT_DEEP_SPLIT_PLIES)
    assert (s > -127).all()
    assert (np.sign(s) == np.sign(hs)).all()
    lg = nat.legal_cpu(own, opp)
    ok = np.where(b == 64, lg == 0, ((lg >> (b & 63).astype(np.uint64)) & np.uint64(1)) == 1)
    assert ok.all()


def mixed_batch(corpus, n):
    """n positions cycling through skipped (many empties, overlapping), terminal, pass-only
    and 1..9-empties positions, so neighbouring lanes finish at very different times."""
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


@pytest.mark.parametrize("n", [1, 129])
@pytest.mark.parametrize("split", [0, 1, 2])
def test_batch_sizes(corpus, n, split):
    own, opp = mixed_batch(corpus, max(n, 2))
    if n == 1:  # the 9-empties position alone
        own, opp = own[1:], opp[1:]
    ws, wb, wn = nat.solve_deep_cpu(own, opp, 9, node_limit=LIMIT)
    if n > 1:
        assert (ws == -128).sum() >= n // 8 and (wb == 64).sum() >= n // 8
    s, b, nd = gpu_solve(own, opp, 9, split=split)
    assert (s == ws).all()
    if split == 0:
        assert (b == wb).all() and (nd == wn).all()
    else:  # the lowest action among the best: same score through either, both legal
        assert ((b == 255) == (wb == 255)).all() and ((b == 64) == (wb == 64)).all()


def test_n_zero():
    need = ctypes.c_size_t(0)
    f = nat.lib.oth_solve_deep_gpu
    for split in (0, 1, 2):
        assert f(None, None, 0, 12, -65, 65, 100, split, None, None, None, None,
                 ctypes.byref(need), None) == nat.AZ_OK
        ws = torch.empty(max(need.value, 8), dtype=torch.uint8, device="cuda")
        assert f(None, None, 0, 12, -65, 65, 100, split, None, None, None, nat.ptr(ws),
                 ctypes.byref(need), None) == nat.AZ_OK
    e = torch.empty(0, dtype=torch.int64, device="cuda")
    s, b, nd = nat.solve_deep_gpu(e, e, 12)
    assert s.numel() == 0 and b.numel() == 0 and nd.numel() == 0


def test_just_above_one_chunk_split_1(corpus):
    """16384 roots are one chunk of the one-ply split: 16384 + 3 take a second pass through
    the workspace."""
    m = np.flatnonzero((corpus["emp"] >= 1) & (corpus["emp"] <= 9))
    i = np.resize(m, 16384 + 3)
    own, opp = corpus["own"][i], corpus["opp"][i]
    ws, wb, wn = nat.solve_deep_cpu(own[:len(m)], opp[:len(m)], 9, node_limit=LIMIT)
    s, b, nd = gpu_solve(own, opp, 9, split=1)
    k = np.arange(len(i)) % len(m)
    assert (s == ws[k]).all()
    assert (s[-3:] == ws[k[-3:]]).all() and (b[-3:] != 99).all()


@pytest.mark.parametrize("split", [0, 1])
def test_unaligned_buffers_and_stream(corpus, split):
    own, opp = mixed_batch(corpus, 130)
    ws, wb, wn = nat.solve_deep_cpu(own, opp, 9, -1, 1, node_limit=LIMIT)
    n = len(own)
    pad = np.zeros(1, np.uint64)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        own_t = dev_i64(np.concatenate([pad, own]))[1:]
        opp_t = dev_i64(np.concatenate([pad, opp]))[1:]
        s = torch.full((n + 2,), 99, dtype=torch.int8, device="cuda")
        b = torch.full((n + 2,), 99, dtype=torch.uint8, device="cuda")
        nd = torch.full((n + 2,), -1, dtype=torch.int64, device="cuda")
        raw_solve(own_t, opp_t, 9, WLD, LIMIT, split, s[1:n + 1], b[1:n + 1], nd[1:n + 1],
                  stream=stream)
    assert own_t.data_ptr() % 16 == 8 and s[1:].data_ptr() % 2 == 1
    s, b, nd = s.cpu().numpy(), b.cpu().numpy(), nd.cpu().numpy()
    assert (np.sign(s[1:n + 1][ws > -127]) == np.sign(ws[ws > -127])).all()
    assert ((s[1:n + 1] == -128) == (ws == -128)).all()
    if split == 0:
        assert (s[1:n + 1] == ws).all() and (b[1:n + 1] == wb).all()
        assert (nd[1:n + 1].view(np.uint64) == wn).all()
    # nothing outside the n results was written
    assert s[0] == 99 and s[n + 1] == 99 and b[0] == 99 and b[n + 1] == 99
    assert nd[0] == -1 and nd[n + 1] == -1


def test_argument_errors():
    need = ctypes.c_size_t(0)
    q = lambda **k: nat.lib.oth_solve_deep_gpu(
        None, None, k.get("n", 4), k.get("me", 12), k.get("a", -65), k.get("b", 65), 100,
        k.get("split", 0), None, None, None, None, ctypes.byref(need), None)
    assert q() == nat.AZ_OK and need.value > 0
    assert q(me=20) == nat.AZ_OK
    assert q(me=21) == nat.AZ_ERR_ARG
    assert q(split=3) == nat.AZ_ERR_ARG
    assert q(n=-1) == nat.AZ_ERR_ARG
    assert q(a=0, b=0) == nat.AZ_ERR_ARG
    assert q(a=-66) == nat.AZ_ERR_ARG
    assert q(b=66) == nat.AZ_ERR_ARG
    assert q(n=1 << 20, me=20, split=2) == nat.AZ_OK
    bounded = need.value
    assert q(n=1 << 24, me=20, split=2) == nat.AZ_OK and need.value == bounded  # chunked
    # a workspace one byte short
    assert q(n=64, split=1) == nat.AZ_OK
    short = ctypes.c_size_t(need.value - 1)
    ws = torch.empty(need.value, dtype=torch.uint8, device="cuda")
    x = torch.zeros(64, dtype=torch.int64, device="cuda")
    s = torch.zeros(64, dtype=torch.int8, device="cuda")
    b = torch.zeros(64, dtype=torch.uint8, device="cuda")
    assert nat.lib.oth_solve_deep_gpu(nat.ptr(x), nat.ptr(x), 64, 12, -65, 65, 100, 1,
                                      nat.ptr(s), nat.ptr(b), None, nat.ptr(ws),
                                      ctypes.byref(short), None) == nat.AZ_ERR_ARG


def test_python_surface_on_device(late):
    import endgame

    m = late["emp"] <= 9
    own, opp = late["own"][m], late["opp"][m]
    hs = late["host"][FULL][0][m]
    o_t, p_t = dev_i64(own), dev_i64(opp)
    s, b, nd = endgame.solve_deep(o_t, p_t, 9, node_limit=LIMIT)
    assert s.is_cuda and s.dtype == torch.int8 and b.dtype == torch.uint8
    assert (s.cpu().numpy() == hs).all()
    # numpy in, numpy out; split 0 reproduces the host's node counts
    s, b, nd = endgame.solve_deep(own, opp, 9, window="wld", node_limit=LIMIT, split_plies=0)
    assert isinstance(s, np.ndarray) and nd.dtype == np.uint64
    assert (s == late["host"][WLD][0][m]).all() and (nd == late["host"][WLD][2][m]).all()
    s, b, nd = endgame.solve_deep(own, opp, 9, window=(-3, 4), node_limit=LIMIT)
    inside = (hs > -3) & (hs < 4)
    assert (s[inside] == hs[inside]).all() and (s[hs >= 4] >= 4).all() and (s[hs <= -3] <= -3).all()
    ro, rp = own[::4], opp[::4]
    pi = np.zeros((len(ro), 65), np.float32)
    pi[:, 64] = 1.0
    rows = {"own": ro, "opp": rp, "pi": pi, "z": np.linspace(-1, 1, len(ro)),
            "player": np.ones(len(ro), np.int8)}
    g_rows, g_mask = endgame.relabel_rows(rows, 9, device="cuda", wld=True)
    c_rows, c_mask = endgame.relabel_rows(rows, 9, device="cpu", wld=True)
    x_rows, x_mask = endgame.relabel_rows(rows, 9, device="cuda")
    assert g_mask.all() and (g_mask == c_mask).all() and (g_rows["z"] == c_rows["z"]).all()
    assert (g_rows["z"] == x_rows["z"]).all()
    assert (g_rows["z"] == np.sign(hs[::4].astype(np.int64))).all()
