"""Depth-limited alpha-beta on the device (oth_eval_gpu / oth_search_gpu, csrc/search.hip)
against the host search, which tests/test_search_cpu.py checks against an unpruned minimax:
the same search code runs on both, so with split_plies = 0 even the node counts are equal;
the split front end must give the same values and best moves.  Every call passes
node_limit = 2^24, so a runaway search ends as AZ_SEARCH_ABORTED and a failed assertion
within seconds."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_golden

nat = pytest.importorskip("az_native")
pytestmark = pytest.mark.gpu

LIMIT = 1 << 24
SKIPPED, ABORTED = -32768, -32767


def popc(x):
    x = np.ascontiguousarray(x, np.uint64)
    return np.unpackbits(x.view(np.uint8).reshape(-1, 8), axis=1).sum(axis=1).astype(np.int64)


def dev_i64(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).cuda()


def raw_search(own_t, opp_t, depth, limit, split, value_t, best_t, nodes_t):
    """oth_search_gpu on the given device tensors (any element offset), current stream."""
    n = own_t.numel()
    need = ctypes.c_size_t(0)
    nat.check(nat.lib.oth_search_gpu(None, None, n, depth, limit, split, None, None, None, None,
                                     ctypes.byref(need), None), "oth_search_gpu")
    ws = torch.empty(max(need.value, 8), dtype=torch.uint8, device="cuda")
    nat.check(nat.lib.oth_search_gpu(nat.ptr(own_t), nat.ptr(opp_t), n, depth, limit, split,
                                     nat.ptr(value_t), nat.ptr(best_t), nat.ptr(nodes_t),
                                     nat.ptr(ws), ctypes.byref(need), nat.stream_ptr()),
              "oth_search_gpu")
    torch.cuda.synchronize()


def gpu_search(own, opp, depth, limit=LIMIT, split=0):
    n = len(own)
    v = torch.full((n,), 99, dtype=torch.int16, device="cuda")
    b = torch.full((n,), 99, dtype=torch.uint8, device="cuda")
    nd = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    raw_search(dev_i64(own), dev_i64(opp), depth, limit, split, v, b, nd)
    return v.cpu().numpy(), b.cpu().numpy(), nd.cpu().numpy().view(np.uint64)


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
def spread(corpus):
    """About 2,000 corpus positions over all empties counts (every 18th in corpus order, the
    pass-only positions among them) and the host's results at every depth used below
    (computed once, read only)."""
    import alphabeta

    idx = np.arange(0, len(corpus["own"]), 18)
    own, opp = corpus["own"][idx], corpus["opp"][idx]
    assert 2000 <= len(own) <= 2100 and len(np.unique(corpus["emp"][idx])) == 60
    host = {d: alphabeta.search(own, opp, d, device="cpu", node_limit=LIMIT) for d in (1, 2, 3, 6)}
    for v, _, _ in host.values():
        assert (v > ABORTED).all()
    return {"own": own, "opp": opp, "host": host}


@pytest.mark.parametrize("depth", [1, 3, 6])
def test_parity_with_cpu_unsplit(spread, depth):
    wv, wb, wn = spread["host"][depth]
    v, b, nd = gpu_search(spread["own"], spread["opp"], depth, split=0)
    assert (v == wv).all()
    assert (b == wb).all()
    assert (nd == wn).all()


@pytest.mark.parametrize("split", [1, 2])
@pytest.mark.parametrize("depth", [1, 2, 3, 6])
def test_split_parity_with_cpu(spread, depth, split):
    wv, wb, wn = spread["host"][depth]
    v, b, nd = gpu_search(spread["own"], spread["opp"], depth, split=split)
    assert (v == wv).all()
    assert (b == wb).all()
    if depth <= split:  # nothing below the split: the same single search
        assert (nd == wn).all()
    else:
        assert (nd > 1).all()


def mixed_batch(corpus, n):
    """n positions cycling through overlapping, terminal, pass-only, 1-empty and 30-empties
    positions, so that neighbouring lanes finish far apart."""
    own, opp, emp = corpus["own"], corpus["opp"], corpus["emp"]
    lg, lg2 = nat.legal_cpu(own, opp), nat.legal_cpu(opp, own)
    kinds = [np.flatnonzero(emp == 30), "overlap", np.flatnonzero((lg == 0) & (lg2 != 0)),
             np.flatnonzero(emp == 1), "terminal", np.flatnonzero(emp == 30)[::-1]]
    o, p = [], []
    for i in range(n):
        k, r = kinds[i % len(kinds)], i // len(kinds)
        if isinstance(k, str):
            j = r % len(corpus["town"])
            to, tp = corpus["town"][j], corpus["topp"][j]
            o.append(to | tp if k == "overlap" else to)
            p.append(tp)
        else:
            o.append(own[k[r % len(k)]])
            p.append(opp[k[r % len(k)]])
    return np.array(o, np.uint64), np.array(p, np.uint64)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
@pytest.mark.parametrize("split", [0, 1, 2])
def test_awkward_batch_sizes_mixed(corpus, n, split):
    own, opp = mixed_batch(corpus, n)
    wv, wb, wn = nat.search_cpu(own, opp, 4, node_limit=LIMIT)
    if n >= 63:
        assert (wv == SKIPPED).sum() >= n // 6 and (wb == 64).sum() >= n // 3
    v, b, nd = gpu_search(own, opp, 4, split=split)
    assert (v == wv).all() and (b == wb).all()
    if split == 0:
        assert (nd == wn).all()


@pytest.mark.parametrize("split", [0, 1, 2])
def test_batch_across_a_split_chunk(corpus, split):
    """16,385 roots at depth 2: one more than the 16,384 roots of a one-ply chunk (and 17
    two-ply chunks, searched unsplit at this depth)."""
    import alphabeta

    n = 16385
    own, opp = corpus["own"][-n:], corpus["opp"][-n:]
    wv, wb, wn = alphabeta.search(own, opp, 2, device="cpu", node_limit=LIMIT)
    v, b, nd = gpu_search(own, opp, 2, split=split)
    assert (v == wv).all() and (b == wb).all()
    if split != 1:
        assert (nd == wn).all()
    # three plies: the two-ply front end really splits, over 17 chunks
    if split == 2:
        wv, wb, _ = alphabeta.search(own, opp, 3, device="cpu", node_limit=LIMIT)
        v, b, nd = gpu_search(own, opp, 3, split=2)
        assert (v == wv).all() and (b == wb).all() and (nd > 1).all()


@pytest.mark.parametrize("split", [0, 1, 2])
def test_unaligned_buffers_and_untouched_memory(corpus, split):
    own, opp = mixed_batch(corpus, 130)
    wv, wb, wn = nat.search_cpu(own, opp, 4, node_limit=LIMIT)
    n = len(own)
    pad = np.zeros(1, np.uint64)
    own_t = dev_i64(np.concatenate([pad, own]))[1:]
    opp_t = dev_i64(np.concatenate([pad, opp]))[1:]
    v = torch.full((n + 2,), 99, dtype=torch.int16, device="cuda")
    b = torch.full((n + 2,), 99, dtype=torch.uint8, device="cuda")
    nd = torch.full((n + 2,), -1, dtype=torch.int64, device="cuda")
    raw_search(own_t, opp_t, 4, LIMIT, split, v[1:n + 1], b[1:n + 1], nd[1:n + 1])
    assert own_t.data_ptr() % 16 == 8 and v[1:].data_ptr() % 4 == 2 and b[1:].data_ptr() % 2 == 1
    v, b, nd = v.cpu().numpy(), b.cpu().numpy(), nd.cpu().numpy()
    assert (v[1:n + 1] == wv).all() and (b[1:n + 1] == wb).all()
    if split == 0:
        assert (nd[1:n + 1].view(np.uint64) == wn).all()
    # nothing outside the n results was written
    assert v[0] == 99 and v[n + 1] == 99 and b[0] == 99 and b[n + 1] == 99
    assert nd[0] == -1 and nd[n + 1] == -1


def test_abort_code_matches_cpu(spread):
    own, opp = spread["own"], spread["opp"]
    full_v, full_b, _ = spread["host"][3]
    wv, wb, wn = nat.search_cpu(own, opp, 3, node_limit=40)
    assert 0 < (wv == ABORTED).sum() < len(wv)
    v, b, nd = gpu_search(own, opp, 3, limit=40, split=0)
    assert (v == wv).all() and (b == wb).all() and (nd == wn).all()
    assert (b[v == ABORTED] == 255).all()
    # a split root with an aborted leaf is aborted; roots that finish keep their result
    for split in (1, 2):
        v2, b2, _ = gpu_search(own, opp, 3, limit=8, split=split)
        done = v2 != ABORTED
        assert (~done).any() and done.any()
        assert (v2[done] == full_v[done]).all() and (b2[done] == full_b[done]).all()
        assert (b2[~done] == 255).all()


def test_a_level_that_overruns_aborts_its_root_and_leaves_nothing_behind(corpus):
    """An unreachable board with 34 placements, one more than a level holds per root: alone
    in its chunk it overruns level 1, a handled path with a defined result."""
    own = np.array([0x0a11640000b40402], np.uint64)
    opp = np.array([0x006602647002ba00], np.uint64)
    assert (own & opp)[0] == 0 and popc(nat.legal_cpu(own, opp))[0] == 34
    wv, wb, _ = nat.search_cpu(own, opp, 3, node_limit=LIMIT)
    assert wv[0] > ABORTED and wb[0] < 64
    need = ctypes.c_size_t(0)
    nat.check(nat.lib.oth_search_gpu(None, None, 64, 3, LIMIT, 1, None, None, None, None,
                                     ctypes.byref(need), None), "oth_search_gpu")
    size1 = need.value
    nat.check(nat.lib.oth_search_gpu(None, None, 1, 3, LIMIT, 2, None, None, None, None,
                                     ctypes.byref(need), None), "oth_search_gpu")
    ws = torch.empty(max(size1, need.value), dtype=torch.uint8, device="cuda")

    def run(o, p, split):
        n = len(o)
        o_t, p_t = dev_i64(o), dev_i64(p)
        v = torch.full((n + 2,), 99, dtype=torch.int16, device="cuda")
        b = torch.full((n + 2,), 99, dtype=torch.uint8, device="cuda")
        nd = torch.full((n + 2,), -1, dtype=torch.int64, device="cuda")
        nat.check(nat.lib.oth_search_gpu(
            nat.ptr(o_t), nat.ptr(p_t), n, 3, LIMIT, split, nat.ptr(v[1:]), nat.ptr(b[1:]),
            nat.ptr(nd[1:]), nat.ptr(ws), ctypes.byref(ctypes.c_size_t(ws.numel())),
            nat.stream_ptr()), "oth_search_gpu")
        torch.cuda.synchronize()
        v, b, nd = v.cpu().numpy(), b.cpu().numpy(), nd.cpu().numpy()
        # the sentinels around the n results are untouched
        assert v[0] == 99 and v[-1] == 99 and b[0] == 99 and b[-1] == 99
        assert nd[0] == -1 and nd[-1] == -1
        return v[1:-1], b[1:-1]

    for split in (1, 2):
        v, b = run(own, opp, split)
        assert v[0] == ABORTED and b[0] == 255
    # the same workspace, next call: 64 roots, nothing of the overrun is left
    o64, p64 = corpus["own"][::577][:64], corpus["opp"][::577][:64]
    assert len(o64) == 64
    hv, hb, _ = nat.search_cpu(o64, p64, 3, node_limit=LIMIT)
    v, b = run(o64, p64, 1)
    assert (v == hv).all() and (b == hb).all()
    # unsplit, and as one of two roots (the level holds 66 nodes: it fits), it is searched
    v, b = run(own, opp, 0)
    assert v[0] == wv[0] and b[0] == wb[0]
    o2, p2 = np.concatenate([own, o64[:1]]), np.concatenate([opp, p64[:1]])
    assert popc(nat.legal_cpu(o2, p2)).sum() <= 66
    v, b = run(o2, p2, 1)
    assert v[0] == wv[0] and b[0] == wb[0] and v[1] == hv[0] and b[1] == hb[0]


def test_eval_whole_corpus(corpus):
    own = np.concatenate([corpus["own"], corpus["town"]])
    opp = np.concatenate([corpus["opp"], corpus["topp"]])
    want = nat.eval_cpu(own, opp)
    out = torch.full((len(own) + 2,), 99, dtype=torch.int16, device="cuda")
    own_t, opp_t = dev_i64(own), dev_i64(opp)
    nat.check(nat.lib.oth_eval_gpu(nat.ptr(own_t), nat.ptr(opp_t), len(own), nat.ptr(out[1:]),
                                   nat.stream_ptr()), "oth_eval_gpu")
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert (out[1:-1] == want).all() and out[0] == 99 and out[-1] == 99
    assert nat.lib.oth_eval_gpu(None, None, 0, None, None) == nat.AZ_OK
    assert nat.lib.oth_eval_gpu(None, None, -1, None, None) == nat.AZ_ERR_ARG


def test_workspace_protocol(corpus):
    need = ctypes.c_size_t(0)
    q = lambda **k: nat.lib.oth_search_gpu(None, None, k.get("n", 4), k.get("depth", 6), 100,
                                           k.get("split", 0), None, None, None, None,
                                           ctypes.byref(need), None)
    assert q() == nat.AZ_OK and need.value > 0
    assert q(depth=0) == nat.AZ_ERR_ARG and q(depth=11) == nat.AZ_ERR_ARG
    assert q(split=3) == nat.AZ_ERR_ARG and q(split=-1) == nat.AZ_ERR_ARG
    assert q(n=-1) == nat.AZ_ERR_ARG
    # a function of (n, depth, split): grows with n up to a chunk, then stays; a depth at or
    # below the split needs only the unsplit workspace
    sizes = {}
    for split in (0, 1, 2):
        for n in (4, 1024, 1 << 20, 1 << 24):
            assert q(n=n, split=split) == nat.AZ_OK
            sizes[(n, split)] = need.value
    assert sizes[(4, 1)] < sizes[(1024, 1)] < sizes[(1 << 20, 1)] == sizes[(1 << 24, 1)]
    assert sizes[(4, 2)] < sizes[(1024, 2)] == sizes[(1 << 24, 2)] < 1 << 27
    assert q(n=1024, split=2, depth=2) == nat.AZ_OK and need.value == sizes[(1024, 0)]
    # too small, misaligned
    own_t, opp_t = dev_i64(corpus["own"][:64]), dev_i64(corpus["opp"][:64])
    v = torch.full((64,), 99, dtype=torch.int16, device="cuda")
    b = torch.full((64,), 99, dtype=torch.uint8, device="cuda")
    assert q(n=64, split=1) == nat.AZ_OK
    ws = torch.empty(need.value + 8, dtype=torch.uint8, device="cuda")
    call = lambda w, size: nat.lib.oth_search_gpu(
        nat.ptr(own_t), nat.ptr(opp_t), 64, 6, 100, 1, nat.ptr(v), nat.ptr(b), None, nat.ptr(w),
        ctypes.byref(ctypes.c_size_t(size)), nat.stream_ptr())
    assert call(ws, need.value - 1) == nat.AZ_ERR_ARG
    assert call(ws[4:], need.value) == nat.AZ_ERR_ARG
    torch.cuda.synchronize()
    assert (v == 99).all() and (b == 99).all()  # a rejected call writes nothing


def test_python_surface_on_device(spread):
    import alphabeta

    own, opp = spread["own"], spread["opp"]
    wv, wb, wn = spread["host"][3]
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        o_t, p_t = dev_i64(own), dev_i64(opp)
        v, b, nd = alphabeta.search(o_t, p_t, 3, node_limit=LIMIT)
        e = alphabeta.evaluate(o_t, p_t)
    stream.synchronize()
    assert v.is_cuda and v.dtype == torch.int16 and b.dtype == torch.uint8
    assert (v.cpu().numpy() == wv).all() and (b.cpu().numpy() == wb).all()
    assert e.is_cuda and (e.cpu().numpy() == nat.eval_cpu(own, opp)).all()
    # numpy in, numpy out, the default split; split 0 reproduces the host's node counts
    v, b, nd = alphabeta.search(own, opp, 3, node_limit=LIMIT)
    assert isinstance(v, np.ndarray) and nd.dtype == np.uint64
    assert (v == wv).all() and (b == wb).all()
    assert (alphabeta.search(own, opp, 3, node_limit=LIMIT, split_plies=0)[2] == wn).all()
    assert (alphabeta.evaluate(own, opp) == nat.eval_cpu(own, opp)).all()


def test_player_moves_straddling_the_exact_range(corpus):
    import alphabeta

    m = (corpus["emp"] >= 5) & (corpus["emp"] <= 11)
    own, opp, emp = corpus["own"][m][::4], corpus["opp"][m][::4], corpus["emp"][m][::4]
    assert (emp <= 8).sum() > 100 and (emp > 8).sum() > 100
    got = alphabeta.AlphaBetaPlayer(3, exact_empties=8, device="cuda").moves(own, opp)
    want = np.where(emp <= 8, nat.solve_cpu(own, opp, 8)[1], nat.search_cpu(own, opp, 3)[1])
    assert got.dtype == np.uint8 and (got == want).all()
    assert (got == alphabeta.AlphaBetaPlayer(3, exact_empties=8, device="cpu").moves(own, opp)).all()
    # the two rules differ somewhere in the exact range, so the switch is observable
    assert (nat.solve_cpu(own, opp, 8)[1] != nat.search_cpu(own, opp, 3)[1])[emp <= 8].any()
