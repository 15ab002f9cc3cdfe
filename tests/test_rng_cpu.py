"""The engine's counter-based generator (csrc/philox.h) on the host: azr::uniform2 through
az_rng_uniform_cpu against the published Philox4x32-10 known answers and against a
restatement of the algorithm in numpy uint64 arithmetic written here, exactly.  A draw's
counter is (slot, event, sub, stream), its key the seed's low and high 32-bit words, and the
two doubles are the first and the last 64 output bits, each >> 11, / 2^53."""
import numpy as np
import pytest

nat = pytest.importorskip("az_native")

M32 = np.uint64(0xFFFFFFFF)
# Random123's known-answer vectors for philox4x32, 10 rounds: counter, key, result
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]

# (seed, stream, slot0, event, sub): the extremes of every counter word, a seed with a high
# word, slots that wrap past 2^32, and the sub-draw bases the engine uses
TUPLES = [
    (0, 0, 0, 0, 0),
    (20261019, 0, 0, 0xFFFFFFFF, 0xFFFFFFFF),
    (0x9E3779B97F4A7C15, 3, 0xFFFFFFFF - 1000, 7, 0x2000),
    (0xFFFFFFFF00000001, 0x7FFFFFFF, 0xFFFF8000, 1, 0x5000),
    (1234, 0x80000005, 12345, 0xFFFFFFFF, 0x6000 + 59),
    (0xFFFFFFFFFFFFFFFF, 0xFFFFFFFF, 0x80000000, 0x80000000, 64 * 64 + 63),
]
N = 1 << 16


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon, Moraes, Dror, Shaw 2011) on uint64 arrays holding 32-bit words:
    ten rounds of two 32x32 -> 64 multiplies by the constants M0 / M1, the key bumped by the
    Weyl constants W0 / W1 between rounds."""
    c0, c1, c2, c3, k0, k1 = (np.asarray(x, np.uint64) for x in (c0, c1, c2, c3, k0, k1))
    M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    s32 = np.uint64(32)
    for _ in range(10):
        p0 = M0 * c0  # both factors below 2^32: the product fits 64 bits
        p1 = M1 * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & M32, (p0 >> s32) ^ c3 ^ k1, p0 & M32
        k0 = (k0 + W0) & M32
        k1 = (k1 + W1) & M32
    return c0, c1, c2, c3


def to_unit(hi, lo):
    """53 bits of (hi << 32 | lo) as a double in [0, 1): exact in float64."""
    x = (np.asarray(hi, np.uint64) << np.uint64(32)) | np.asarray(lo, np.uint64)
    return (x >> np.uint64(11)).astype(np.float64) / 9007199254740992.0


def uniform2_numpy(seed, stream, slot0, n, event, sub):
    slot = (np.uint64(slot0) + np.arange(n, dtype=np.uint64)) & M32
    full = lambda v: np.full(n, v, np.uint64)  # noqa: E731
    r = philox4x32_10(slot, full(event), full(sub), full(stream), full(seed & 0xFFFFFFFF),
                      full(seed >> 32))
    return np.stack([to_unit(r[0], r[1]), to_unit(r[2], r[3])], 1)


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_known_answers(ctr, key, want):
    seed = key[0] | (key[1] << 32)
    out = nat.rng_uniform_cpu(seed, ctr[3], ctr[0], 1, ctr[1], ctr[2])
    a = ((want[0] << 32) | want[1]) >> 11
    b = ((want[2] << 32) | want[3]) >> 11
    # an integer below 2^53 over 2^53: the division is exact, so equality is the full check
    assert out[0, 0] == a / 2.0**53 and out[0, 1] == b / 2.0**53
    # and the restatement below reproduces the published words themselves
    got = philox4x32_10(*ctr, *key)
    assert tuple(int(x) for x in got) == want


@pytest.mark.parametrize("seed,stream,slot0,event,sub", TUPLES)
def test_entry_point_equals_numpy_restatement(seed, stream, slot0, event, sub):
    got = nat.rng_uniform_cpu(seed, stream, slot0, N, event, sub)
    want = uniform2_numpy(seed, stream, slot0, N, event, sub)
    assert got.shape == (N, 2) and np.array_equal(got, want)
    assert (got >= 0.0).all() and (got < 1.0).all()
    # 2^17 draws of 53 bits: a repeat means a counter collapsed (chance 2^-20 otherwise)
    assert len(np.unique(got)) == 2 * N


def test_counter_words_are_not_interchangeable():
    """Each of slot, event, sub, stream and the two key words lands in its own place: moving
    a 1 from one word to another gives another draw."""
    base = dict(seed=0, stream=0, slot0=0, event=0, sub=0)
    seen = set()
    for k, v in (("seed", 1), ("seed", 1 << 32), ("stream", 1), ("slot0", 1), ("event", 1),
                 ("sub", 1), ("sub", 0)):
        a = dict(base, **{k: v})
        out = nat.rng_uniform_cpu(a["seed"], a["stream"], a["slot0"], 1, a["event"], a["sub"])
        seen.add((out[0, 0], out[0, 1]))
    assert len(seen) == 7


def test_n_zero_and_bad_arguments():
    assert nat.rng_uniform_cpu(1, 2, 3, 0, 4, 5).shape == (0, 2)
    assert nat.lib.az_rng_uniform_cpu(1, 2, 3, -1, 4, 5, None) == nat.AZ_ERR_ARG
    assert nat.lib.az_rng_uniform_cpu(1, 2, 3, 1, 4, 5, None) == nat.AZ_ERR_ARG
