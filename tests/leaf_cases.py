"""Rows for the leaf-solve tests (tests/test_leaf_solve_cpu.py, test_leaf_solve_gpu.py) and
the oracle evaluator with exact late values.

The rows are board_corpus.npz positions with 0..14 empties, PER_DEPTH of each (own = the side
to move), in a seeded shuffle, with an all-zero row (a step's row without a leaf) after every
seventh: 1,097 rows, enough for 1,000 from an offset of 3.  The host solver's results for them
are computed once per session and shared, never modified.
"""
import functools

import numpy as np

from conftest import load_golden

PER_DEPTH = 64
MAX_DEPTH = 14
_BITS = np.arange(64, dtype=np.uint64)


def popc(x):
    return np.array([bin(int(v)).count("1") for v in np.asarray(x).reshape(-1)], np.int64)


def planes(own, opp):
    """Canonical planes float32 [n, 64]: own stones +1, the opponent's -1."""
    own, opp = np.asarray(own, np.uint64), np.asarray(opp, np.uint64)
    o = ((own[:, None] >> _BITS) & np.uint64(1)).astype(np.float32)
    p = ((opp[:, None] >> _BITS) & np.uint64(1)).astype(np.float32)
    return np.ascontiguousarray(o - p)


def sentinels(n):
    """A distinct finite float per row, none of them -1, 0 or +1."""
    return (np.float32(0.25) + np.arange(n, dtype=np.float32) / np.float32(4096)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def rows():
    """{"own", "opp" uint64 [n] (0 / 0 for the all-zero rows), "emp" int64 [n] (64 for them),
    "x" float32 [n, 64]}."""
    d = load_golden("board_corpus.npz")
    own = np.where(d["player"] == 1, d["pos"], d["neg"]).astype(np.uint64)
    opp = np.where(d["player"] == 1, d["neg"], d["pos"]).astype(np.uint64)
    # the corpus holds positions to move from, none of them full: the full boards are the
    # successors of its 1-empty positions (whose stones are whose does not matter there)
    full = np.flatnonzero(popc(d["npos"] | d["nneg"]) == 64)
    own = np.concatenate([own, d["npos"][full].astype(np.uint64)])
    opp = np.concatenate([opp, d["nneg"][full].astype(np.uint64)])
    emp = 64 - popc(own | opp)
    pick = np.concatenate([np.flatnonzero(emp == e)[:PER_DEPTH] for e in range(MAX_DEPTH + 1)])
    assert len(pick) == PER_DEPTH * (MAX_DEPTH + 1)
    pick = np.random.default_rng(7).permutation(pick)
    o, p = [], []
    for i, j in enumerate(pick):
        o.append(own[j])
        p.append(opp[j])
        if i % 7 == 6:
            o.append(np.uint64(0))
            p.append(np.uint64(0))
    o, p = np.array(o, np.uint64), np.array(p, np.uint64)
    out = {"own": o, "opp": p, "emp": 64 - popc(o | p), "x": planes(o, p)}
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def solved(node_limit=1 << 31):
    """oth_solve_deep_cpu in (-1, 1) on every row with 1..12 empties: (score int64 [n], nodes
    int64 [n]), score AZ_SOLVE_SKIPPED and nodes 0 on the other rows."""
    import az_native as nat

    r = rows()
    m = (r["emp"] >= 1) & (r["emp"] <= 12)
    score = np.full(len(m), nat.AZ_SOLVE_SKIPPED, np.int64)
    nodes = np.zeros(len(m), np.int64)
    s, _, nd = nat.solve_deep_cpu(r["own"][m], r["opp"][m], 12, -1, 1, node_limit)
    score[m], nodes[m] = s, nd.astype(np.int64)
    score.setflags(write=False)
    nodes.setflags(write=False)
    return score, nodes


def expected(E, node_limit=1 << 31, n=None, start=0):
    """What a leaf solve of rows [start, start + n) with max_empties E must leave: (values
    float32 from those rows of sentinels(len(rows)), stats dict)."""
    import az_native as nat

    r = rows()
    n = len(r["emp"]) - start if n is None else n
    sl = slice(start, start + n)
    score, nodes = solved(node_limit)
    emp = r["emp"][sl]
    task = (emp >= 1) & (emp <= E)
    ok = task & (score[sl] != nat.AZ_SOLVE_ABORTED)
    v = sentinels(len(r["emp"]))[sl].copy()  # a row's sentinel goes by its place in rows()
    v[ok] = np.sign(score[sl][ok]).astype(np.float32)
    return v, {"solved": int(ok.sum()), "limited": int((task & ~ok).sum()),
               "nodes": int(nodes[sl][task].sum())}


def exact_evaluate(evaluate, E, node_limit=None):
    """An oracle evaluator (own, opp, player) -> (priors, value) that swaps in the solved sign
    where the node has 1..E empties and its search stays within node_limit nodes (default:
    the engine's default limit)."""
    import az_native as nat
    import engine

    node_limit = engine.LEAF_SOLVE_NODES if node_limit is None else node_limit

    def wrapped(own, opp, player):
        p, v = evaluate(own, opp, player)
        e = 64 - bin(int(own) | int(opp)).count("1")
        if 1 <= e <= E:
            s, _, _ = nat.solve_deep_cpu(np.array([own], np.uint64), np.array([opp], np.uint64),
                                         E, -1, 1, node_limit)
            if s[0] != nat.AZ_SOLVE_ABORTED:
                v = float(np.sign(int(s[0])))
        return p, v

    return wrapped
