"""Positions up to the eight symmetries of the square, host side: oth_canon_cpu,
az_rows_d4_cpu and az_rows_symmetrise_cpu (csrc/canon.hip) through symmetry.py against a
NumPy reference on unpacked 8 x 8 arrays (tests/canon_reference.py), and the flags that
carry the canonical form into alphabeta.reachable / openings and records.dedup.

The order of symmetrise's sum.  A plain left-to-right float32 sum over a stabiliser of four
or eight symmetries is not the same on all squares of an orbit: on square 19 of the initial
position it adds pi[19], pi[44], pi[37], pi[26] in that order, on square 26 pi[26], pi[37],
pi[44], pi[19], and float addition is not associative
(test_symmetrise_plain_order_is_not_invariant shows a row where the two differ).  The entry
points therefore add the same terms, still in ascending t, inside a fixed tree of cosets
(include/az_othello.h), which is exactly invariant and equals the plain sum for one or two
terms; the reference here restates that tree in NumPy float32."""
import numpy as np
import pytest

import canon_reference as ref
from conftest import load_golden

nat = pytest.importorskip("az_native")
import alphabeta  # noqa: E402
import records  # noqa: E402
import symmetry  # noqa: E402
from train_gpu import pi_source_tables  # noqa: E402

SINGLE = np.uint64(1) << np.arange(64, dtype=np.uint64)
ZERO64 = np.zeros(64, np.uint64)


@pytest.fixture(scope="module")
def inputs():
    """(own, opp): the corpus, 4,096 random disjoint pairs, the empty, full and initial boards,
    every single stone as own and as opp."""
    d = load_golden("board_corpus.npz")
    rng = np.random.default_rng(2024)
    a = rng.integers(0, 2**64, 4096, dtype=np.uint64)
    b = rng.integers(0, 2**64, 4096, dtype=np.uint64) & ~a
    full = 2**64 - 1
    own = np.concatenate([d["pos"], a, np.array([0, full, 0, ref.INIT_OWN], np.uint64), SINGLE,
                          ZERO64])
    opp = np.concatenate([d["neg"], b, np.array([0, 0, full, ref.INIT_OPP], np.uint64), ZERO64,
                          SINGLE])
    assert own.dtype == opp.dtype == np.uint64 and not (own & opp).any()
    return own, opp


@pytest.fixture(scope="module")
def expected(inputs):
    return ref.canon(*inputs)


@pytest.fixture(scope="module")
def got(inputs):
    return symmetry.canon(*inputs)


def test_reference_tables_are_the_loaders():
    assert np.array_equal(ref.source_tables(), pi_source_tables())


def test_canon_matches_reference(got, expected):
    for g, e, name in zip(got, expected, ("own", "opp", "sym", "stab")):
        assert g.dtype == e.dtype and np.array_equal(g, e), name
    assert (got[3] & 1).all()


def test_canon_sym_reaches_the_canonical_pair(inputs, got):
    own, opp = inputs
    assert np.array_equal(nat.d4_cpu(own, got[2]), got[0])
    assert np.array_equal(nat.d4_cpu(opp, got[2]), got[1])


def test_canon_is_idempotent(got):
    again = symmetry.canon(got[0], got[1])
    assert np.array_equal(again[0], got[0]) and np.array_equal(again[1], got[1])
    assert not again[2].any()
    assert np.array_equal(again[3], got[3])


@pytest.mark.parametrize("s", range(8))
def test_canon_of_every_image_is_the_same(inputs, got, s):
    own, opp = inputs
    img = symmetry.canon(ref.image(own, s), ref.image(opp, s))
    assert np.array_equal(img[0], got[0]) and np.array_equal(img[1], got[1])
    assert np.array_equal(img[3], got[3])


def test_canon_known_values():
    o, p, sym, stab = symmetry.canon(np.array([ref.INIT_OWN, 1], np.uint64),
                                     np.array([ref.INIT_OPP, 0], np.uint64))
    assert stab.tolist() == [0xA5, 0x81]
    # checked in NumPy: the initial position is fixed by the half turn and both diagonal flips
    fixed = [t for t in range(8) if ref.image(ref.INIT_OWN, t)[0] == ref.INIT_OWN
             and ref.image(ref.INIT_OPP, t)[0] == ref.INIT_OPP]
    assert fixed == [0, 2, 5, 7]


def test_canon_overlapping_boards_are_reported():
    o, p, sym, stab = symmetry.canon(np.array([3, 1], np.uint64), np.array([1, 2], np.uint64))
    assert (int(o[0]), int(p[0]), int(sym[0]), int(stab[0])) == (3, 1, nat.AZ_CANON_BAD, 0)
    assert sym[1] != nat.AZ_CANON_BAD and stab[1] & 1


def test_transform_rows_pi_is_the_table_gather():
    rng = np.random.default_rng(5)
    pi = rng.random((8 * 300, 65)).astype(np.float32)
    sym = np.repeat(np.arange(8, dtype=np.uint8), 300)
    out, none = symmetry.transform_rows(pi=pi, sym=sym)
    assert none is None
    assert np.array_equal(out, np.take_along_axis(pi, pi_source_tables()[sym], axis=1))
    for s in range(8):
        assert np.array_equal(out[s * 300:(s + 1) * 300],
                              np.take(pi[s * 300:(s + 1) * 300], pi_source_tables()[s], axis=1))


def test_transform_rows_act_is_the_inverse_table():
    src = pi_source_tables()
    act = np.tile(np.arange(65, dtype=np.uint8), 8)
    sym = np.repeat(np.arange(8, dtype=np.uint8), 65)
    none, out = symmetry.transform_rows(act=act, sym=sym)
    assert none is None
    assert (src[sym, out.astype(np.int64)] == act).all()     # out is where act's stone lands
    assert (out[act == 64] == 64).all()
    assert np.array_equal(out, ref.transform_act(act, sym))


def test_transform_rows_orbit_minimum(inputs, got):
    own, opp = inputs
    rng = np.random.default_rng(6)
    act = rng.integers(0, 65, len(own)).astype(np.uint8)
    _, out = symmetry.transform_rows(act=act, sym=got[2], stab=got[3])
    assert np.array_equal(out, ref.transform_act(act, got[2], got[3]))
    # the four opening moves d3, c4, f5, e6 are one move of the initial position
    first = np.array([19, 26, 37, 44, 64], np.uint8)
    _, o = symmetry.transform_rows(act=first, sym=np.zeros(5, np.uint8),
                                   stab=np.full(5, 0xA5, np.uint8))
    assert o.tolist() == [19, 19, 19, 19, 64]


def test_transform_rows_bad_rows_are_reported():
    pi = np.ones((2, 65), np.float32)
    out, act = symmetry.transform_rows(pi=pi, act=np.array([3, 65], np.uint8),
                                       sym=np.array([8, 0], np.uint8))
    assert np.isnan(out[0]).all() and np.array_equal(out[1], pi[1])
    assert act.tolist() == [nat.AZ_CANON_BAD, nat.AZ_CANON_BAD]


@pytest.fixture(scope="module")
def sym_rows():
    """Random rows under every subgroup of the square's symmetries."""
    groups = [0x01, 0x05, 0x11, 0x21, 0x41, 0x81, 0x0F, 0x55, 0xA5, 0xFF]
    rng = np.random.default_rng(7)
    stab = np.repeat(np.array(groups, np.uint8), 64)
    pi = rng.random((len(stab), 65)).astype(np.float32)
    pi /= pi.sum(1, keepdims=True)
    return pi, stab


def test_symmetrise_matches_numpy(sym_rows):
    pi, stab = sym_rows
    out = symmetry.symmetrise(pi, stab)
    assert out.dtype == np.float32
    assert np.array_equal(out.view(np.uint32), ref.symmetrise(pi, stab).view(np.uint32))
    small = np.array([bin(int(s)).count("1") <= 2 for s in stab])
    assert np.array_equal(out[small].view(np.uint32),
                          ref.ascending_sum(pi[small], stab[small]).view(np.uint32))
    # the plain order differs from the tree by rounding only: every entry is below 2^-4, so a
    # partial sum of up to eight is below 2^-1 and each of the seven additions of either
    # order errs by at most half an ulp of that, 2^-26; 14 * 2^-26 / 4 < 2^-24 after the
    # division by four or eight
    assert pi.max() < 2.0 ** -4
    assert np.allclose(out, ref.ascending_sum(pi, stab), rtol=0, atol=2.0 ** -24)


def test_symmetrise_is_exactly_invariant(sym_rows):
    pi, stab = sym_rows
    out = symmetry.symmetrise(pi, stab)
    for t in range(8):
        rows = ((stab >> t) & 1) == 1
        moved = ref.transform_pi(out[rows], np.full(int(rows.sum()), t))
        assert np.array_equal(moved.view(np.uint32), out[rows].view(np.uint32)), t
    assert np.array_equal(out[stab == 1].view(np.uint32), pi[stab == 1].view(np.uint32))
    assert np.array_equal(out[:, 64], pi[:, 64])


def test_symmetrise_plain_order_is_not_invariant(sym_rows):
    """Why the sum is a tree: the left-to-right sum in ascending t is not the same on the
    squares of an orbit."""
    pi, stab = sym_rows
    rows = stab == 0xA5
    plain = ref.ascending_sum(pi[rows], stab[rows])
    moved = ref.transform_pi(plain, np.full(int(rows.sum()), 7))
    assert not np.array_equal(moved.view(np.uint32), plain.view(np.uint32))


@pytest.mark.parametrize("plies,classes", [(2, 3), (3, 14), (4, 60), (5, 322), (6, 1773)])
def test_reachable_up_to_symmetry(plies, classes):
    own, opp = alphabeta.reachable(plies, symmetry=True)
    assert len(own) == classes
    assert len(set(zip(own.tolist(), opp.tolist()))) == classes
    c = ref.canon(own, opp)
    assert np.array_equal(c[0], own) and np.array_equal(c[1], opp)
    # and they are the classes of the plain enumeration
    full = ref.canon(*alphabeta.reachable(plies))
    assert set(zip(full[0].tolist(), full[1].tolist())) == set(zip(own.tolist(), opp.tolist()))


def test_reachable_default_is_unchanged():
    assert [len(alphabeta.reachable(p)[0]) for p in (2, 4, 6)] == [12, 236, 7092]
    for a, b in zip(alphabeta.reachable(4), alphabeta.reachable(4, symmetry=False)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("seed", [0, 3])
def test_openings_up_to_symmetry(seed):
    own, opp, player = alphabeta.openings(60, 4, seed, symmetry=True)
    assert len(own) == 60 and (player == 1).all()
    c = ref.canon(own, opp)
    assert np.array_equal(c[0], own) and np.array_equal(c[1], opp)
    assert len(set(zip(own.tolist(), opp.tolist()))) == 60       # pairwise inequivalent
    with pytest.raises(ValueError):
        alphabeta.openings(61, 4, 0, symmetry=True)


@pytest.mark.parametrize("n,plies,seed", [(12, 2, 0), (40, 4, 1), (236, 4, 2), (64, 8, 3)])
def test_openings_default_is_unchanged(n, plies, seed):
    a = alphabeta.openings(n, plies, seed)
    b = alphabeta.openings(n, plies, seed, symmetry=False)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    assert len(set(zip(a[0].tolist(), a[1].tolist()))) == n
    if plies <= 4:
        with pytest.raises(ValueError):
            alphabeta.openings({2: 13, 4: 237}[plies], plies, seed)


@pytest.fixture(scope="module")
def turned_rows():
    """Playout rows, each board and move under a seeded random symmetry (in NumPy)."""
    own, opp, act, z = ref.playout_rows(48, seed=11)
    rng = np.random.default_rng(12)
    s = rng.integers(0, 8, len(own))
    t_own, t_opp = own.copy(), opp.copy()
    for k in range(8):
        m = s == k
        t_own[m], t_opp[m] = ref.image(own[m], k), ref.image(opp[m], k)
    return t_own, t_opp, ref.transform_act(act, s), z


def numpy_canonical_rows(own, opp, act):
    co, cp, sym, stab = ref.canon(own, opp)
    return co, cp, ref.transform_act(act, sym, stab)


@pytest.mark.parametrize("how", ["vote", "mean", None])
def test_records_dedup_up_to_symmetry_on_the_host(turned_rows, how):
    own, opp, act, z = turned_rows
    got_rows = records.dedup(own, opp, act, z, how=how, symmetry=True, device="cpu")
    co, cp, ca = numpy_canonical_rows(own, opp, act)
    want = records.dedup(co, cp, ca, z, how=how, symmetry=False, device="cpu")
    assert got_rows.keys() == want.keys()
    for k in want:
        assert np.array_equal(np.asarray(got_rows[k]), np.asarray(want[k])), k
    if how is not None:  # the turned rows merge at least as far as the games' own rows do
        plain = records.dedup(own, opp, act, z, how=how, device="cpu")
        assert len(got_rows["own"]) < len(plain["own"])


def test_host_mirrors_take_the_flag(turned_rows):
    own, opp, act, z = turned_rows
    co, cp, ca = numpy_canonical_rows(own, opp, act)
    for g, w in zip(records.vote_numpy(own, opp, act, z, symmetry=True),
                    records.vote_numpy(co, cp, ca, z)):
        assert np.array_equal(g, w)
    g, w = records.mean_numpy(own, opp, act, z, symmetry=True), records.mean_numpy(co, cp, ca, z)
    for k in w:
        assert np.array_equal(g[k], w[k]), k


def test_ladder_passes_the_flag_on(monkeypatch):
    import arena

    seen = []

    class Stop(Exception):
        pass

    def fake(n, plies, seed, symmetry=False):
        seen.append((n, plies, seed, symmetry))
        raise Stop

    monkeypatch.setattr(arena, "make_openings", fake)
    for kw, want in (({}, False), ({"symmetry": True}, True)):
        with pytest.raises(Stop):
            arena.ladder(None, {}, (1,), 7, plies=4, seed=5, **kw)
        assert seen[-1] == (4, 4, 5, want)


def test_argument_conventions():
    lib = nat.lib
    assert lib.az_abi_version() == 1
    assert lib.oth_canon_cpu(None, None, 0, None, None, None, None) == nat.AZ_OK
    assert lib.az_rows_d4_cpu(None, None, None, None, 0, None, None) == nat.AZ_OK
    assert lib.az_rows_symmetrise_cpu(None, None, 0, None) == nat.AZ_OK
    for out in symmetry.canon(np.zeros(0, np.uint64), np.zeros(0, np.uint64)):
        assert out.shape == (0,)
    pi = np.ones((2, 65), np.float32)
    pi_o = np.empty_like(pi)
    sym, stab = np.zeros(2, np.uint8), np.ones(2, np.uint8)
    act, act_o = np.array([5, 64], np.uint8), np.empty(2, np.uint8)
    p = nat.ptr
    # either payload alone
    assert lib.az_rows_d4_cpu(p(pi), None, p(sym), None, 2, p(pi_o), None) == nat.AZ_OK
    assert lib.az_rows_d4_cpu(None, p(act), p(sym), p(stab), 2, None, p(act_o)) == nat.AZ_OK
    assert act_o.tolist() == [5, 64]
    # in place, a payload without its output, negative n, null buffers
    assert lib.az_rows_d4_cpu(p(pi), None, p(sym), None, 2, p(pi), None) == nat.AZ_ERR_ARG
    assert "pi_o" in nat.last_error()
    assert lib.az_rows_symmetrise_cpu(p(pi), p(stab), 2, p(pi)) == nat.AZ_ERR_ARG
    assert lib.az_rows_d4_cpu(p(pi), None, p(sym), None, 2, None, None) == nat.AZ_ERR_ARG
    assert lib.az_rows_d4_cpu(p(pi), None, None, None, 2, p(pi_o), None) == nat.AZ_ERR_ARG
    assert lib.oth_canon_cpu(None, None, -1, None, None, None, None) == nat.AZ_ERR_ARG
    assert lib.oth_canon_cpu(None, None, 2, None, None, None, None) == nat.AZ_ERR_ARG
    assert lib.az_rows_symmetrise_cpu(None, p(stab), 2, p(pi_o)) == nat.AZ_ERR_ARG
    with pytest.raises(RuntimeError):
        nat.check(lib.oth_canon_cpu(None, None, 2, None, None, None, None), "oth_canon_cpu")
