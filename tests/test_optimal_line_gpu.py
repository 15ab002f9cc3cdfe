"""endgame.optimal_line on the device against the host, bit for bit (rows, off, score), at 1, 63,
64, 65 and 1,000 roots with 0..10 empties on unaligned slices; and oth_line_step_gpu alone
against its host mirror oth_line_step_cpu on seeded tables (finished roots, skipped / aborted
codes and full row buffers among them)."""
import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

nat = pytest.importorskip("az_native")

FIELDS = ("own", "opp", "pi", "act", "z")
E = 10
N = 1000


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
    return own, opp, town, topp


@pytest.fixture(scope="module")
def roots(corpus):
    """1,001 roots in a fixed shuffle: 0..10 empties evenly, passes as the corpus has them,
    terminal roots, roots above E (11 empties) and overlapping boards.  Entry 0 only shifts the
    slices off 16-byte alignment."""
    own, opp, town, topp = corpus
    emp = 64 - popc(own | opp)
    late, above = np.flatnonzero(emp <= E), np.flatnonzero(emp == E + 1)
    pick = late[np.linspace(0, len(late) - 1, N - 57).astype(int)].tolist()
    pick += above[np.linspace(0, len(above) - 1, 20).astype(int)].tolist()
    o = np.concatenate([own[pick], town[:30]])
    p = np.concatenate([opp[pick], topp[:30]])
    assert len(o) == N + 1 - 8 and len(set(emp[pick].tolist())) >= E + 1
    o = np.concatenate([o, o[:8] | (p[:8] & (~p[:8] + np.uint64(1)))])  # overlapping boards
    p = np.concatenate([p, p[:8]])
    assert len(o) == N + 1
    order = np.random.RandomState(7).permutation(N + 1)
    return np.ascontiguousarray(o[order]), np.ascontiguousarray(p[order])


@pytest.fixture(scope="module")
def host(roots):
    """The host's lines of roots 1..1000, computed once."""
    import endgame

    o, p = roots
    ref = endgame.optimal_line(o[1:], p[1:], E, device="cpu")
    emp = 64 - popc(o[1:] | p[1:])
    skipped = ref["score"] == nat.AZ_SOLVE_SKIPPED
    assert 20 <= skipped.sum() <= 40 and (ref["score"] != nat.AZ_SOLVE_ABORTED).all()
    assert ((emp > E) | ((o[1:] & p[1:]) != 0) == skipped).all()
    assert (ref["act"] == 64).sum() > 50 and (np.diff(ref["off"]) == 0).sum() > 30
    return ref


@pytest.mark.parametrize("n", [1, 63, 64, 65, N])
def test_device_equals_host(roots, host, n):
    import endgame

    o, p = roots
    dev_o = torch.from_numpy(o.view(np.int64)).cuda()
    dev_p = torch.from_numpy(p.view(np.int64)).cuda()
    a, b = dev_o[1:1 + n], dev_p[1:1 + n]  # 8 bytes past a 16-byte boundary
    assert a.data_ptr() % 16 == 8
    got = endgame.optimal_line(a, b, E)
    assert all(v.is_cuda for v in got.values())
    assert torch.equal(dev_o, torch.from_numpy(o.view(np.int64)).cuda())  # inputs untouched
    rows = int(host["off"][n])
    assert got["off"].cpu().numpy().tobytes() == host["off"][:n + 1].tobytes()
    assert got["score"].cpu().numpy().tobytes() == host["score"][:n].tobytes()
    for k in FIELDS:
        want = np.ascontiguousarray(host[k][:rows])
        assert got[k].cpu().numpy().tobytes() == want.tobytes(), k
    # numpy in, numpy out, through the device
    if n == 65:
        again = endgame.optimal_line(o[1:1 + n], p[1:1 + n], E, device="cuda")
        assert again["own"].dtype == np.uint64
        for k in FIELDS + ("off", "score"):
            assert np.ascontiguousarray(again[k]).tobytes() == \
                np.ascontiguousarray(got[k].cpu().numpy()).tobytes(), k


def _state(own, opp, n, stride, seed):
    """A seeded call of the step: tables over each root's available actions with random values,
    scores with the solvers' codes mixed in, finished roots, counts up to a full buffer."""
    r = np.random.RandomState(seed)
    lg = nat.legal_cpu(own, opp)
    passer = (lg == 0) & (nat.legal_cpu(opp, own) != 0)
    avail = ((lg[:, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool)
    avail = np.concatenate([avail, passer[:, None]], axis=1)
    values = np.where(avail, r.randint(-3, 4, (n, 65)), -128).astype(np.int8)
    score = r.randint(-64, 65, n).astype(np.int8)
    code = r.randint(0, 12, n)
    score[code == 0] = nat.AZ_SOLVE_SKIPPED
    score[code == 1] = nat.AZ_SOLVE_ABORTED
    values[code <= 1] = -128
    return {"own": own.copy(), "opp": opp.copy(), "values": values, "score": score,
            "count": r.randint(0, stride + 1, n).astype(np.int32),
            "done": (r.randint(0, 5, n) == 0).astype(np.uint8),
            "root_score": r.randint(-64, 65, n).astype(np.int8),
            "row_own": r.randint(0, 1 << 62, n * stride).astype(np.uint64),
            "row_opp": r.randint(0, 1 << 62, n * stride).astype(np.uint64),
            "row_pi": r.rand(n * stride, 65).astype(np.float32),
            "row_act": r.randint(0, 65, n * stride).astype(np.uint8),
            "row_z": r.rand(n * stride).astype(np.float32)}


ORDER = ("own", "opp", "values", "score", "count", "done", "root_score", "row_own", "row_opp",
         "row_pi", "row_act", "row_z")


def _padded(v):
    """The array on the device behind one zero element."""
    t = torch.from_numpy(v.view(np.int64) if v.dtype == np.uint64 else v).reshape(-1)
    return torch.cat([torch.zeros(1, dtype=t.dtype), t]).cuda()


def _call(fn, s, n, stride, first, live, *tail):
    a = [nat.ptr(s[k]) for k in ORDER]
    return fn(a[0], a[1], a[2], a[3], n, stride, first, *a[4:], nat.ptr(live), *tail)


@pytest.mark.parametrize("n,stride,first", [(1, 4, 1), (65, 6, 0), (N, 20, 1), (N, 3, 0)])
def test_line_step_kernel_equals_host_mirror(roots, n, stride, first):
    o, p = roots
    o, p = o[1:1 + n], p[1:1 + n]
    h = _state(o, p, n, stride, seed=n + stride)
    # device copies at an odd element offset (unaligned for every element size above one byte)
    pad = {k: _padded(v) for k, v in h.items()}
    d = {k: t[1:] for k, t in pad.items()}
    live_h, live_d = np.full(1, -5, np.int32), torch.full((1,), -5, dtype=torch.int32).cuda()
    before = {k: v.copy() for k, v in h.items()}
    assert _call(nat.lib.oth_line_step_cpu, h, n, stride, first, live_h) == nat.AZ_OK
    assert _call(nat.lib.oth_line_step_gpu, d, n, stride, first, live_d,
                 nat.stream_ptr()) == nat.AZ_OK
    torch.cuda.synchronize()
    assert int(live_d.item()) == int(live_h[0]) == int((h["done"] == 0).sum())
    for k in ORDER:
        got = d[k].cpu().numpy()
        want = h[k].view(np.int64) if h[k].dtype == np.uint64 else h[k]
        assert got.tobytes() == np.ascontiguousarray(want).reshape(-1).tobytes(), k
        assert pad[k][0].item() == 0  # nothing written in front of the arrays
    # the call did something of every kind
    wrote = h["count"] > before["count"]
    assert (h["count"][~wrote] <= before["count"][~wrote]).all()
    if n == N:
        assert wrote.sum() > n // 4 and (before["done"] == 1).sum() > n // 10
        full = (before["done"] == 0) & (before["count"] >= stride) & (before["score"] > -127) \
            & (before["values"] != -128).any(axis=1)
        assert full.sum() > 5 and (h["root_score"][full] == nat.AZ_SOLVE_ABORTED).all()
        assert (h["count"][full] == 0).all()
        fin = before["done"] == 1
        for k in ("own", "opp", "count", "root_score"):
            assert (h[k][fin] == before[k][fin]).all()
