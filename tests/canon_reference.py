"""NumPy reference for the canon tests: the eight symmetries as np.rot90 / np.flip over
unpacked 8 x 8 arrays (the definition csrc/bitboard.h's d4 cites), never the library's own
transforms.  sym = k + 4 * flip: rot90 k times, then fliplr."""
import numpy as np

SH = np.arange(64, dtype=np.uint64)
INIT_OWN, INIT_OPP = np.uint64(0x0000000810000000), np.uint64(0x0000001008000000)


def unpack(x):
    x = np.asarray(x, np.uint64).reshape(-1)
    return ((x[:, None] >> SH) & np.uint64(1)).astype(np.uint8).reshape(-1, 8, 8)


def pack(b):
    return (b.reshape(-1, 64).astype(np.uint64) << SH).sum(axis=1, dtype=np.uint64)


def image(x, s):
    b = np.rot90(unpack(x), s & 3, axes=(1, 2))
    return pack(np.flip(b, axis=2) if s & 4 else b)


def canon(own, opp):
    """(own, opp, sym, stab) by definition: the smallest image pair as unsigned words, own
    first; the smallest symmetry that attains it; the symmetries that fix the result."""
    own, opp = np.asarray(own, np.uint64).reshape(-1), np.asarray(opp, np.uint64).reshape(-1)
    co, cp, sym = own.copy(), opp.copy(), np.zeros(len(own), np.uint8)
    for s in range(1, 8):
        a, b = image(own, s), image(opp, s)
        lt = (a < co) | ((a == co) & (b < cp))
        co, cp, sym = np.where(lt, a, co), np.where(lt, b, cp), np.where(lt, s, sym)
    stab = np.zeros(len(own), np.uint8)
    for t in range(8):
        fixed = (image(co, t) == co) & (image(cp, t) == cp)
        stab |= (fixed.astype(np.uint8) << np.uint8(t)).astype(np.uint8)
    return co, cp, sym.astype(np.uint8), stab


def square_tables():
    """int64 [8, 64]: dst[s, j] = the square the stone of square j lands on under s."""
    dst = np.empty((8, 64), np.int64)
    for s in range(8):
        moved = image(np.uint64(1) << SH, s)
        dst[s] = [int(m).bit_length() - 1 for m in moved]
    return dst


def source_tables():
    """int64 [8, 65]: out[i] = in[src[s, i]], the pass (64) to itself."""
    dst = square_tables()
    src = np.full((8, 65), 64, np.int64)
    for s in range(8):
        src[s, dst[s]] = np.arange(64)
    return src


def transform_pi(pi, sym):
    return np.take_along_axis(pi, source_tables()[np.asarray(sym, np.int64)], axis=1)


def transform_act(act, sym, stab=None):
    """act under sym; with stab, then the smallest square of its orbit; the pass stays."""
    dst = square_tables()
    act, sym = np.asarray(act, np.int64), np.asarray(sym, np.int64)
    place = act < 64
    a = np.where(place, dst[sym, np.minimum(act, 63)], act)
    if stab is not None:
        best = a.copy()
        for t in range(8):
            on = place & (((np.asarray(stab, np.int64) >> t) & 1) == 1)
            best = np.where(on, np.minimum(best, dst[t, np.minimum(a, 63)]), best)
        a = best
    return a.astype(np.uint8)


def symmetrise(pi, stab):
    """float32 average of every row over its stabiliser.  The terms pi[src_t(j)] are added in
    ascending t inside the fixed tree ((t0 + t2) + (t1 + t3)) + ((t4 + t6) + (t5 + t7)), absent
    terms left out -- for one or two terms the plain ascending sum -- then multiplied by the
    exact 1 / popcount(stab)."""
    pi = np.asarray(pi, np.float32)
    stab = np.asarray(stab, np.int64)
    src = source_tables()
    term = [pi[:, src[t]] for t in range(8)]                       # [n, 65] each
    has = [np.broadcast_to((((stab >> t) & 1) == 1)[:, None], pi.shape) for t in range(8)]

    def add(x, hx, y, hy):
        return np.where(hx & hy, x + y, np.where(hx, x, y)).astype(np.float32), hx | hy

    p02, p13 = add(term[0], has[0], term[2], has[2]), add(term[1], has[1], term[3], has[3])
    p46, p57 = add(term[4], has[4], term[6], has[6]), add(term[5], has[5], term[7], has[7])
    total, _ = add(*add(*p02, *p13), *add(*p46, *p57))
    k = np.array([bin(int(s)).count("1") for s in stab], np.float32)[:, None]
    out = np.where(k > 1, total * (np.float32(1) / np.maximum(k, 1)), total).astype(np.float32)
    out[:, 64] = pi[:, 64]
    return out


def ascending_sum(pi, stab):
    """The plain left-to-right float32 sum over the set bits of stab in ascending t, times
    1 / popcount(stab)."""
    pi = np.asarray(pi, np.float32)
    src = source_tables()
    out = np.empty_like(pi)
    for i, s in enumerate(np.asarray(stab, np.int64)):
        ts = [t for t in range(8) if (s >> t) & 1]
        acc = pi[i, src[ts[0]]].copy()
        for t in ts[1:]:
            acc = (acc + pi[i, src[t]]).astype(np.float32)
        out[i] = acc * (np.float32(1) / np.float32(len(ts))) if len(ts) > 1 else acc
        out[i, 64] = pi[i, 64]
    return out


def playout_rows(n_games, seed):
    """(own, opp, act, z) of seeded uniformly random games through the library's host replay."""
    import records

    acts = records.random_playouts(n_games, seed=seed)
    own, opp, act, z, _, _, _ = records.replay(acts, device="cpu")
    return own, opp, act, z
