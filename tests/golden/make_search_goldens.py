"""Pins of the tree searches' behaviour per position: every array that oth_solve_cpu,
oth_solve_deep_cpu, oth_search_cpu and az_leaf_solve_cpu return (score or value, best, nodes;
values and the three statistics) on a fixed sample of tests/golden/board_corpus.npz, aborted
and skipped roots included.  Writes tests/golden/search_goldens.npz.

    python tests/golden/make_search_goldens.py

Runs the project's own host entry points and nothing else, through the library the process
loads (AZ_LIB_PATH, or the tree's): generate the file with the library whose behaviour is to
be kept, before the searches' sources change.  The git revision and the library's build id go
into the file.  tests/test_search_goldens_cpu.py recomputes everything with compute() and
compares exactly.

Samples (own = the side to move), all derived from the corpus:
  corpus positions at a fixed stride per entry point (below);
  roots that pass: corpus positions whose only action is the pass;
  terminal roots: the successors (npos / nneg) after which the game is over;
  full boards: the successors without an empty square;
  overlapping boards: corpus positions with the opponent's lowest stone added to own as well;
  roots above max_empties: corpus positions with up to three empties more than the cap.
"""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "search_goldens.npz")

BIG = 1 << 31
SOLVE_EMPTIES, SOLVE_LIMITS, SOLVE_STRIDE = 10, (BIG, 1000, 10), 2
DEEP_EMPTIES, DEEP_LIMITS, DEEP_STRIDE = 12, (BIG, 1000, 10), 3
DEEP_WINDOWS = ((-65, 65), (-1, 1), (-8, 3))
DEEP_LATE = (14, 15, 16)  # empties of the late roots, LATE_EACH of each, in (-1, 1) at cap 16
LATE_EACH = 3
SEARCH_DEPTHS, SEARCH_LIMITS, SEARCH_STRIDE = (1, 2, 3, 6), (BIG, 100), 40
SEARCH_DEEP_DEPTH, SEARCH_DEEP_STRIDE = 10, 6100
LEAF_EMPTIES, LEAF_LIMITS = 12, (BIG, 64)
EACH = 12  # special roots of each kind per sample, at the most
# roots of each special kind per sample ("pass" includes those the stride met itself); a
# regenerated file must hold the same sample
KINDS = {"solve": {"stride": 3150, "pass": 151, "terminal": 10, "full": 12, "overlapping": 12,
                   "above_cap": 12, "positions": 3208},
         "deep": {"stride": 2504, "pass": 90, "terminal": 10, "full": 12, "overlapping": 12,
                  "above_cap": 12, "positions": 2562},
         "search": {"stride": 915, "pass": 17, "terminal": 10, "full": 12, "overlapping": 12,
                    "positions": 961},
         "late": {"positions": 9}, "search_deep": {"positions": 6}}


def popc(x):
    x = np.ascontiguousarray(x, np.uint64)
    return np.unpackbits(x.view(np.uint8).reshape(-1, 8), axis=1).sum(axis=1).astype(np.int64)


def spread(idx, k):
    """k of idx, evenly spaced (all of them if there are no more)."""
    return idx if len(idx) <= k else idx[np.arange(k) * len(idx) // k]


def samples():
    """{"solve" | "deep" | "late" | "search" | "search_deep": (own, opp)} and the number of
    roots of each special kind in each sample (asserted against KINDS)."""
    with np.load(os.path.join(HERE, "board_corpus.npz")) as z:
        d = {k: z[k] for k in ("pos", "neg", "player", "pass_only", "npos", "nneg", "term_next")}
    own = np.where(d["player"] == 1, d["pos"], d["neg"]).astype(np.uint64)
    opp = np.where(d["player"] == 1, d["neg"], d["pos"]).astype(np.uint64)
    emp = 64 - popc(own | opp)
    # the successors, from the view of the side that did not just move
    n_own, n_opp = d["nneg"].astype(np.uint64), d["npos"].astype(np.uint64)
    n_emp = 64 - popc(n_own | n_opp)
    low = opp & (~opp + np.uint64(1))  # the opponent's lowest stone

    def build(lo, hi, stride, cap):
        o, p, kinds = [], [], {}

        def add(name, ao, ap):
            assert len(ao) > 0, (name, lo, hi)
            kinds[name] = len(ao)
            o.append(ao)
            p.append(ap)

        ok = (emp >= lo) & (emp <= hi)
        pick = np.flatnonzero(ok)[::stride]
        add("stride", own[pick], opp[pick])
        i = spread(np.flatnonzero(ok & (d["pass_only"] != 0)), EACH)
        add("pass", own[i], opp[i])
        kinds["pass"] += int((d["pass_only"][pick] != 0).sum())  # those the stride met itself
        i = spread(np.flatnonzero((d["term_next"] != 0) & (n_emp >= 1) & (n_emp <= hi)), EACH)
        add("terminal", n_own[i], n_opp[i])
        i = spread(np.flatnonzero(n_emp == 0), EACH)
        add("full", n_own[i], n_opp[i])
        i = spread(np.flatnonzero(ok & (low != 0)), EACH)
        add("overlapping", own[i] | low[i], opp[i])
        if cap is not None:
            i = spread(np.flatnonzero((emp > cap) & (emp <= cap + 3)), EACH)
            add("above_cap", own[i], opp[i])
        return (np.concatenate(o), np.concatenate(p)), kinds

    out, counts = {}, {}
    out["solve"], counts["solve"] = build(1, SOLVE_EMPTIES, SOLVE_STRIDE, SOLVE_EMPTIES)
    out["deep"], counts["deep"] = build(1, DEEP_EMPTIES, DEEP_STRIDE, DEEP_EMPTIES)
    out["search"], counts["search"] = build(1, 60, SEARCH_STRIDE, None)
    late = np.concatenate([spread(np.flatnonzero(emp == e), LATE_EACH) for e in DEEP_LATE])
    out["late"] = (own[late], opp[late])
    out["search_deep"] = (own[::SEARCH_DEEP_STRIDE], opp[::SEARCH_DEEP_STRIDE])
    for name, (o, p) in out.items():
        kinds = counts.setdefault(name, {})
        kinds["positions"] = len(o)
        if name in ("solve", "deep", "search"):
            # the kinds as the boards show them, whatever they were picked for
            assert int(((o & p) != 0).sum()) == kinds["overlapping"], name
            assert int((popc(o | p) == 64).sum()) == kinds["full"], name
    assert counts == KINDS, counts
    return out, counts


def planes(own, opp):
    """Canonical planes float32 [n, 64]: own stones +1, the opponent's -1 (overlapping
    squares 0)."""
    bits = np.arange(64, dtype=np.uint64)
    o = ((own[:, None] >> bits) & np.uint64(1)).astype(np.float32)
    p = ((opp[:, None] >> bits) & np.uint64(1)).astype(np.float32)
    return np.ascontiguousarray(o - p)


def compute(nat, sets):
    """Every result array, keyed "<entry point>/<configuration>/<array>"."""
    r = {}

    def keep(prefix, names, arrays):
        for name, a in zip(names, arrays):
            r[f"{prefix}/{name}"] = a

    svb = ("score", "best", "nodes")
    o, p = sets["solve"]
    for limit in SOLVE_LIMITS:
        keep(f"solve/limit{limit}", svb, nat.solve_cpu(o, p, SOLVE_EMPTIES, limit))
    o, p = sets["deep"]
    for a, b in DEEP_WINDOWS:
        for limit in DEEP_LIMITS:
            keep(f"deep/window{a}_{b}/limit{limit}", svb,
                 nat.solve_deep_cpu(o, p, DEEP_EMPTIES, a, b, limit))
    keep("deep/late", svb, nat.solve_deep_cpu(*sets["late"], DEEP_LATE[-1], -1, 1, BIG))
    o, p = sets["search"]
    for depth in SEARCH_DEPTHS:
        for limit in SEARCH_LIMITS:
            keep(f"search/depth{depth}/limit{limit}", ("value", "best", "nodes"),
                 nat.search_cpu(o, p, depth, limit))
    keep(f"search/depth{SEARCH_DEEP_DEPTH}", ("value", "best", "nodes"),
         nat.search_cpu(*sets["search_deep"], SEARCH_DEEP_DEPTH, BIG))
    o, p = sets["deep"]
    x = planes(o, p)
    for limit in LEAF_LIMITS:
        values = (np.float32(0.25) + np.arange(len(o), dtype=np.float32) / np.float32(4096))
        stats = nat.leaf_solve_cpu(x, values, LEAF_EMPTIES, limit)
        keep(f"leaf/limit{limit}", ("values", "stats"),
             (values, np.array([stats[k] for k in nat.LEAF_SOLVE_STATS], np.uint64)))
    return r


def main():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "alphazero-othello_amd")]
    import az_native as nat

    sets, counts = samples()
    out = compute(nat, sets)
    for name, (o, p) in sets.items():
        out[f"sample/{name}/own"], out[f"sample/{name}/opp"] = o, p
    rev = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], check=True,
                         capture_output=True, text=True).stdout.strip()
    out["revision"] = np.array(rev)
    out["build_id"] = np.array(nat.build_id())
    np.savez_compressed(OUT, **out)
    for name, kinds in counts.items():
        print(name, kinds)
    aborted = {k: int((v == (nat.AZ_SEARCH_ABORTED if k.startswith("search")
                             else nat.AZ_SOLVE_ABORTED)).sum())
               for k, v in out.items() if k.endswith(("/score", "/value"))}
    print("aborted roots:", aborted)
    print("wrote", OUT, os.path.getsize(OUT), "bytes; revision", rev)


if __name__ == "__main__":
    main()
