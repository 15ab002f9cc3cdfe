"""Positions up to the eight symmetries of the square on the GPU: oth_canon_gpu,
az_rows_d4_gpu and az_rows_symmetrise_gpu against their host twins bit for bit, and the
flags that carry them through replay.aggregate_rows and records.dedup."""
import numpy as np
import pytest
import torch

import canon_reference as ref
from conftest import load_golden

pytestmark = pytest.mark.gpu

nat = pytest.importorskip("az_native")
import records  # noqa: E402
import replay  # noqa: E402
import symmetry  # noqa: E402

DEV = "cuda"
N_MAX = 4099


def dev(a, dt=None):
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(DEV)
    return t if dt is None else t.to(dt)


def host(t):
    a = t.cpu().numpy()
    return a.view(np.uint64) if a.dtype == np.int64 else a


@pytest.fixture(scope="module")
def base():
    """N_MAX + 1 rows (one spare for the odd-offset slices): playout positions, symmetric and
    single-stone boards, two error rows; random pi, actions over 0..64; and the host results."""
    own, opp, act, _ = ref.playout_rows(80, seed=21)
    single = np.uint64(1) << np.arange(64, dtype=np.uint64)
    extra_own = np.concatenate([np.array([0, 2**64 - 1, ref.INIT_OWN, 3], np.uint64), single])
    extra_opp = np.concatenate([np.array([0, 0, ref.INIT_OPP, 1], np.uint64), 0 * single])
    n = N_MAX + 1
    own = np.concatenate([extra_own, own])[:n]
    opp = np.concatenate([extra_opp, opp])[:n]
    assert len(own) == n
    rng = np.random.default_rng(22)
    pi = rng.random((n, 65)).astype(np.float32)
    act = rng.integers(0, 65, n).astype(np.uint8)
    c = symmetry.canon_cpu(own, opp)
    sym = c[2].copy()
    sym[5] = 9  # one row with a symmetry out of range (row 3 has overlapping boards)
    rows = symmetry.rows_d4_cpu(pi, act, sym, c[3])
    sm = symmetry.symmetrise_cpu(pi, c[3])
    return {"own": own, "opp": opp, "pi": pi, "act": act, "sym": sym, "canon": c, "rows": rows,
            "symmetrised": sm,
            "d": {k: dev(v) for k, v in (("own", own), ("opp", opp), ("pi", pi), ("act", act),
                                         ("sym", sym), ("stab", c[3]))}}


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.float32:
        a, b = a.view(np.uint32), b.view(np.uint32)
    return a.shape == b.shape and np.array_equal(a, b)


@pytest.mark.parametrize("first", [0, 1])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000, N_MAX])
def test_device_equals_host(base, n, first):
    """first = 1: slices that start at an odd element, so the board arrays are not 16-byte
    aligned (the one-position kernel) and the pi rows start at an odd float."""
    d, sl = base["d"], slice(first, first + n)
    got = symmetry.canon_gpu(d["own"][sl], d["opp"][sl])
    for g, w in zip(got, base["canon"]):
        assert same_bits(host(g), w[sl])
    pi_o, act_o = symmetry.rows_d4_gpu(d["pi"][sl], d["act"][sl], d["sym"][sl], d["stab"][sl])
    assert same_bits(host(pi_o), base["rows"][0][sl])
    assert same_bits(host(act_o), base["rows"][1][sl])
    sm = symmetry.symmetrise_gpu(d["pi"][sl], d["stab"][sl])
    assert same_bits(host(sm), base["symmetrised"][sl])


def test_device_payloads_alone_and_conventions(base):
    d, sl = base["d"], slice(0, 65)
    pi_o, none = symmetry.rows_d4_gpu(d["pi"][sl], None, d["sym"][sl], None)
    assert none is None and same_bits(host(pi_o), base["rows"][0][sl])
    none, act_o = symmetry.rows_d4_gpu(None, d["act"][sl], d["sym"][sl], None)
    want = symmetry.rows_d4_cpu(None, base["act"][sl], base["sym"][sl], None)[1]
    assert none is None and same_bits(host(act_o), want)
    lib, p, s = nat.lib, nat.ptr, nat.stream_ptr()
    assert lib.oth_canon_gpu(None, None, 0, None, None, None, None, s) == nat.AZ_OK
    assert lib.az_rows_d4_gpu(None, None, None, None, 0, None, None, s) == nat.AZ_OK
    assert lib.az_rows_symmetrise_gpu(None, None, 0, None, s) == nat.AZ_OK
    assert lib.az_rows_d4_gpu(p(d["pi"]), None, p(d["sym"]), None, 4, p(d["pi"]), None,
                              s) == nat.AZ_ERR_ARG
    assert lib.az_rows_symmetrise_gpu(p(d["pi"]), p(d["stab"]), 4, p(d["pi"]), s) == nat.AZ_ERR_ARG
    assert lib.oth_canon_gpu(None, None, 4, None, None, None, None, s) == nat.AZ_ERR_ARG
    # NumPy in, NumPy out through the GPU; tensors in, tensors out
    via = symmetry.canon(base["own"][:100], base["opp"][:100], device=DEV)
    assert all(isinstance(x, np.ndarray) for x in via)
    assert all(same_bits(g, w[:100]) for g, w in zip(via, base["canon"]))
    assert all(x.is_cuda for x in symmetry.canon(d["own"][:100], d["opp"][:100]))


# ---- aggregation ------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fixture_rows():
    d = load_golden("replay_aggregate.npz")
    return d["in_pos"], d["in_neg"], d["in_ver"], d["in_pi"], d["in_v"]


def aggregate(own, opp, ver, pi, v, symmetry):
    res = replay.aggregate_rows(dev(own), dev(opp), dev(ver), dev(pi), dev(v), symmetry=symmetry)
    return {k: host(t) for k, t in res.items()}


@pytest.fixture(scope="module")
def merged(fixture_rows):
    return aggregate(*fixture_rows, symmetry=True)


def numpy_path(own, opp, ver, pi, v):
    """The same result from the parts: rows made canonical in NumPy, the aggregation as it
    was, the NumPy symmetrise of its output.

    A canonical row's pi is averaged over the stabiliser of its board before the aggregation:
    two images of a symmetric position can reach the canonical board through symmetries that
    differ by a member of the stabiliser, so their transformed pi differ by that permutation,
    and a float mean of differently permuted rows, symmetrised afterwards, equals the other
    image's only up to rounding -- not bit for bit, which
    test_aggregate_under_random_symmetries asks for.  Symmetrised first, the rows are bit-equal
    whichever image was stored; the aggregation's per-entry sums keep an orbit's entries
    bit-equal, so the symmetrise of its output here changes no bit."""
    co, cp, sym, stab = ref.canon(own, opp)
    rows = ref.symmetrise(ref.transform_pi(pi, sym), stab)
    res = aggregate(co, cp, ver, rows, v, symmetry=False)
    res["pi"] = ref.symmetrise(res["pi"], ref.canon(res["own"], res["opp"])[3])
    return res


def test_aggregate_fixture_merges_to_755(fixture_rows, merged):
    assert len(merged["own"]) == 755
    assert len(aggregate(*fixture_rows, symmetry=False)["own"]) == 766
    assert int(merged["count"].sum()) == 4000
    c = ref.canon(merged["own"], merged["opp"])
    assert same_bits(c[0], merged["own"]) and same_bits(c[1], merged["opp"])
    for t in range(1, 8):  # every output row is exactly symmetric under its own stabiliser
        rows = ((c[3] >> t) & 1) == 1
        moved = ref.transform_pi(merged["pi"][rows], np.full(int(rows.sum()), t))
        assert same_bits(moved, merged["pi"][rows]), t
    assert ((c[3] != 1).sum()) > 0
    want = numpy_path(*fixture_rows)
    assert merged.keys() == want.keys()
    for k in want:
        assert same_bits(merged[k], want[k]), k


def test_aggregate_under_random_symmetries(fixture_rows, merged):
    own, opp, ver, pi, v = fixture_rows
    s = np.random.default_rng(31).integers(0, 8, len(own))
    t_own, t_opp = own.copy(), opp.copy()
    for k in range(8):
        m = s == k
        t_own[m], t_opp[m] = ref.image(own[m], k), ref.image(opp[m], k)
    t_pi = ref.transform_pi(pi, s)
    turned = aggregate(t_own, t_opp, ver, t_pi, v, symmetry=True)
    assert len(turned["own"]) == 755
    want = numpy_path(t_own, t_opp, ver, t_pi, v)
    for k in merged:
        assert same_bits(turned[k], merged[k]), k
        assert same_bits(turned[k], want[k]), k


def test_initial_position_collapses_to_one_symmetric_row():
    rng = np.random.default_rng(32)
    s = np.arange(16) % 8
    own = np.concatenate([ref.image(ref.INIT_OWN, int(k)) for k in s])
    opp = np.concatenate([ref.image(ref.INIT_OPP, int(k)) for k in s])
    assert len(set(zip(own.tolist(), opp.tolist()))) == 2   # the position and its mirror image
    pi = rng.random((16, 65)).astype(np.float32)
    pi /= pi.sum(1, keepdims=True)
    res = aggregate(own, opp, np.zeros(16, np.int32), pi, rng.uniform(-1, 1, 16), symmetry=True)
    assert len(res["own"]) == 1 and res["count"].tolist() == [16]
    c = ref.canon(ref.INIT_OWN, ref.INIT_OPP)
    assert res["own"][0] == c[0][0] and res["opp"][0] == c[1][0]
    four = res["pi"][0, [19, 26, 37, 44]].view(np.uint32)
    assert (four == four[0]).all()
    for t in (2, 5, 7):
        assert same_bits(ref.transform_pi(res["pi"], [t]), res["pi"])


def test_aggregate_duplicates_takes_the_flag(fixture_rows, merged):
    own, opp, ver, pi, v = fixture_rows
    n = 600
    states = nat.unpack_np(own[:n], opp[:n], np.ones(n, np.int8))
    buf = [(states[i], pi[i], float(v[i]), int(ver[i])) for i in range(n)]
    st, ps, vs = replay.aggregate_duplicates(buf, symmetry=True)
    want = aggregate(own[:n], opp[:n], ver[:n], pi[:n], v[:n], symmetry=True)
    o, p = nat.pack_np(np.stack(st), np.ones(len(st), np.int8))
    assert same_bits(o, want["own"]) and same_bits(p, want["opp"])
    assert same_bits(np.stack(ps), want["pi"]) and same_bits(np.array(vs, np.float32), want["v"])
    plain = replay.aggregate_duplicates(buf)
    assert len(plain[0]) == len(aggregate(own[:n], opp[:n], ver[:n], pi[:n], v[:n], False)["own"])


# ---- records ----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def turned_rows():
    own, opp, act, z = ref.playout_rows(48, seed=11)
    s = np.random.default_rng(12).integers(0, 8, len(own))
    t_own, t_opp = own.copy(), opp.copy()
    for k in range(8):
        m = s == k
        t_own[m], t_opp[m] = ref.image(own[m], k), ref.image(opp[m], k)
    return t_own, t_opp, ref.transform_act(act, s), z


@pytest.mark.parametrize("how", ["vote", "mean", None])
def test_records_dedup_on_device_equals_host(turned_rows, how):
    own, opp, act, z = turned_rows
    want = records.dedup(own, opp, act, z, how=how, symmetry=True, device="cpu")
    got = records.dedup(own, opp, act, z, how=how, symmetry=True, device=DEV)
    assert got.keys() == want.keys()
    for k in want:
        if how == "mean" and k == "pi":
            # the device renormalises the float32 shares by their float32 sum, with or without
            # the flag (tests/test_records_gpu.py derives the 6.5 eps)
            assert np.abs(got[k] - want[k]).max() <= 6.5 * np.finfo(np.float32).eps
        else:
            assert same_bits(got[k], want[k]), k
    # and bit for bit what the device gives for rows canonicalised in NumPy
    co, cp, sym, stab = ref.canon(own, opp)
    plain = records.dedup(co, cp, ref.transform_act(act, sym, stab), z, how=how, device=DEV)
    for k in plain:
        assert same_bits(got[k], plain[k]), k
    # tensors in, tensors out
    t = records.dedup(dev(own), dev(opp), dev(act), dev(z), how=how, symmetry=True)
    assert all(x.is_cuda for x in t.values())
    assert same_bits(host(t["own"]), got["own"]) and same_bits(host(t["count"]), got["count"])
