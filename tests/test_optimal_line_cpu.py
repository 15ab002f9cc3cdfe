"""endgame.optimal_line on the host (oth_line_step_cpu over the host's solve_moves tables)
against a brute-force negamax written here in plain Python integers: corpus positions with 0..8
empties, pass roots, terminal roots and a full board among them.  No GPU."""
import functools

import numpy as np
import pytest

from conftest import load_golden

nat = pytest.importorskip("az_native")

M64 = (1 << 64) - 1
# bit b = row * 8 + column: (shift, mask that removes the squares wrapped round an edge)
DIRS = [(1, 0xFEFEFEFEFEFEFEFE), (-1, 0x7F7F7F7F7F7F7F7F), (8, M64), (-8, M64),
        (9, 0xFEFEFEFEFEFEFEFE), (7, 0x7F7F7F7F7F7F7F7F), (-7, 0xFEFEFEFEFEFEFEFE),
        (-9, 0x7F7F7F7F7F7F7F7F)]
NONE = -128


def _shift(x, d, m):
    return ((x << d) if d > 0 else (x >> -d)) & m & M64


def flips(own, opp, sq):
    f = 0
    for d, m in DIRS:
        x, line = _shift(1 << sq, d, m), 0
        while x & opp:
            line |= x
            x = _shift(x, d, m)
        if x & own:
            f |= line
    return f


def moves(own, opp):
    """[(square, flipped stones)] of every placement of `own`."""
    out = []
    for sq in range(64):
        if not ((own | opp) >> sq) & 1:
            f = flips(own, opp, sq)
            if f:
                out.append((sq, f))
    return out


def children(own, opp):
    """[(action, child own, child opp)]: the placements, else the pass if the opponent can
    place, else nothing (the game is over)."""
    mv = moves(own, opp)
    if mv:
        return [(sq, opp ^ f, own | (1 << sq) | f) for sq, f in mv]
    return [(64, opp, own)] if moves(opp, own) else []


@functools.lru_cache(maxsize=None)
def negamax(own, opp):
    """The exact final disc difference own - opp with best play by both sides."""
    ch = children(own, opp)
    if not ch:
        return bin(own).count("1") - bin(opp).count("1")
    return max(-negamax(co, cp) for _, co, cp in ch)


def true_table(own, opp):
    t = np.full(65, NONE, np.int64)
    for a, co, cp in children(own, opp):
        t[a] = -negamax(co, cp)
    return t


def popc(x):
    x = np.ascontiguousarray(x, np.uint64)
    return np.unpackbits(x.view(np.uint8).reshape(-1, 8), axis=1).sum(axis=1).astype(np.int64)


@pytest.fixture(scope="module")
def roots():
    """Corpus roots by empties (fewer of the expensive ones), every kind the line must handle."""
    d = load_golden("board_corpus.npz")
    own = np.where(d["player"] == 1, d["pos"], d["neg"]).astype(np.uint64)
    opp = np.where(d["player"] == 1, d["neg"], d["pos"]).astype(np.uint64)
    emp = 64 - popc(own | opp)
    pick = []
    for e, k in zip(range(0, 9), (6, 12, 12, 12, 12, 12, 10, 5, 3)):
        idx = np.flatnonzero(emp == e)
        pick += idx[np.linspace(0, len(idx) - 1, min(k, len(idx))).astype(int)].tolist()
    lg = nat.legal_cpu(own, opp)
    passer = np.flatnonzero((lg == 0) & (nat.legal_cpu(opp, own) != 0) & (emp >= 1) & (emp <= 6))
    assert len(passer) >= 6
    pick += passer[:6].tolist()
    end = d["term_next"] == 1
    town = np.where(d["player"] == 1, d["nneg"], d["npos"])[end].astype(np.uint64)
    topp = np.where(d["player"] == 1, d["npos"], d["nneg"])[end].astype(np.uint64)
    temp = 64 - popc(town | topp)
    t_open = np.flatnonzero((temp >= 1) & (temp <= 8))[:4]  # over with empty squares left
    t_full = np.flatnonzero(temp == 0)[:1]                  # a full board
    assert len(t_open) >= 1 and len(t_full) == 1
    o = np.concatenate([own[pick], town[t_open], town[t_full]])
    p = np.concatenate([opp[pick], topp[t_open], topp[t_full]])
    kinds = {"pass": len(passer[:6]), "terminal": len(t_open) + 1}
    return o, p, kinds


@pytest.fixture(scope="module")
def line(roots):
    import endgame

    o, p, _ = roots
    return endgame.optimal_line(o, p, 8, device="cpu")


def test_python_rules_match_the_library(roots):
    o, p, _ = roots
    lg = nat.legal_cpu(o, p)
    for a, b, m in zip(o.tolist(), p.tolist(), lg.tolist()):
        assert sum(1 << sq for sq, _ in moves(a, b)) == m


def test_shapes_and_off(roots, line):
    o, _, _ = roots
    n = len(o)
    off = line["off"]
    assert off.dtype == np.int64 and off.shape == (n + 1,) and off[0] == 0
    assert (np.diff(off) >= 0).all()
    rows = int(off[-1])
    assert line["own"].dtype == np.uint64 and line["own"].shape == (rows,)
    assert line["opp"].dtype == np.uint64 and line["opp"].shape == (rows,)
    assert line["pi"].dtype == np.float32 and line["pi"].shape == (rows, 65)
    assert line["act"].dtype == np.uint8 and line["act"].shape == (rows,)
    assert line["z"].dtype == np.float32 and line["z"].shape == (rows,)
    assert line["score"].dtype == np.int8 and line["score"].shape == (n,)
    # a line of a root with E empties has E placements and at most one pass before each
    emp = 64 - popc(o | roots[1])
    assert (np.diff(off) <= 2 * emp).all()


def test_every_ply_against_negamax(roots, line):
    import endgame

    o, p, kinds = roots
    off = line["off"]
    seen_pass = seen_tie = seen_terminal = 0
    signs = set()
    for i, (ro, rp) in enumerate(zip(o.tolist(), p.tolist())):
        score = negamax(ro, rp)
        assert int(line["score"][i]) == score
        co, cp, sign = ro, rp, 1  # sign: the side to move seen from the root's side
        for r in range(int(off[i]), int(off[i + 1])):
            assert int(line["own"][r]) == co and int(line["opp"][r]) == cp
            t = true_table(co, cp)
            s = negamax(co, cp)
            assert s == sign * score  # the line keeps the root's score
            best = np.flatnonzero((t != NONE) & (t == s))
            act = int(line["act"][r])
            assert act == best[0]  # score-optimal, and the lowest such action
            want_pi = endgame.exact_policy(t[None, :].astype(np.int8))[0]
            assert line["pi"][r].tobytes() == want_pi.tobytes()
            assert line["z"][r] == float(np.sign(s))
            signs.add(int(np.sign(s)))
            seen_pass += act == 64
            seen_tie += len(best) > 1
            if act == 64:
                assert (line["pi"][r] == np.eye(65, dtype=np.float32)[64]).all()
            co, cp = next((a, b) for k, a, b in children(co, cp) if k == act)
            sign = -sign
        # the slice ends where the game does, at the root's score from the root's side
        assert children(co, cp) == []
        assert sign * (bin(co).count("1") - bin(cp).count("1")) == score
        seen_terminal += off[i] == off[i + 1]
    assert seen_pass >= kinds["pass"] and seen_tie >= 5 and signs == {-1, 0, 1}
    assert seen_terminal >= kinds["terminal"]


def test_terminal_roots_have_empty_slices(roots, line):
    o, p, kinds = roots
    k = kinds["terminal"]
    off = line["off"]
    assert (np.diff(off)[-k:] == 0).all()
    assert (line["score"][-k:] == (popc(o[-k:]) - popc(p[-k:]))).all()
    assert (o[-1] | p[-1]) == np.uint64(M64)  # the full board


def test_skipped_aborted_and_bad_arguments(roots):
    import endgame

    o, p, _ = roots
    emp = 64 - popc(o | p)
    # more empties than max_empties, and overlapping boards: the solvers' skipped code
    mixed_o = np.concatenate([o, [np.uint64(3)]])
    mixed_p = np.concatenate([p, [np.uint64(1)]])
    got = endgame.optimal_line(mixed_o, mixed_p, 4, device="cpu")
    skip = np.concatenate([emp > 4, [True]])
    assert (got["score"][skip] == nat.AZ_SOLVE_SKIPPED).all()
    assert (np.diff(got["off"])[skip] == 0).all()
    full = endgame.optimal_line(o, p, 8, device="cpu")
    keep = ~skip[:-1]
    assert (got["score"][:-1][keep] == full["score"][keep]).all()
    for i in np.flatnonzero(keep):
        a, b = slice(*got["off"][i:i + 2]), slice(*full["off"][i:i + 2])
        for k in ("own", "opp", "pi", "act", "z"):
            assert got[k][a].tobytes() == full[k][b].tobytes()
    # a search past node_limit: aborted like solve_moves, no partial line
    hard = emp >= 5
    assert hard.sum() >= 10
    ab = endgame.optimal_line(o[hard], p[hard], 8, device="cpu", node_limit=1)
    lg = nat.legal_cpu(o[hard], p[hard])
    over = (lg == 0) & (nat.legal_cpu(p[hard], o[hard]) == 0)
    assert (ab["score"][~over] == nat.AZ_SOLVE_ABORTED).all() and (~over).sum() >= 10
    assert ab["off"][-1] == 0 and len(ab["z"]) == 0
    # max_empties beyond the exact solver's 14, and below 0
    for e in (15, 20, -1):
        with pytest.raises(ValueError):
            endgame.optimal_line(o, p, e, device="cpu")
    # no roots at all
    none = endgame.optimal_line(np.zeros(0, np.uint64), np.zeros(0, np.uint64), 8, device="cpu")
    assert none["off"].tolist() == [0] and none["score"].shape == (0,)
    assert none["pi"].shape == (0, 65) and none["own"].shape == (0,)


def test_torch_tensors_in_torch_tensors_out(roots, line):
    import torch

    import endgame

    o, p, _ = roots
    got = endgame.optimal_line(torch.from_numpy(o.view(np.int64)), torch.from_numpy(p.view(np.int64)),
                               8, device="cpu")
    assert all(isinstance(v, torch.Tensor) for v in got.values())
    assert got["own"].dtype == torch.int64 and got["pi"].dtype == torch.float32
    for k in ("own", "opp", "pi", "act", "z", "off", "score"):
        assert got[k].numpy().tobytes() == np.ascontiguousarray(line[k]).tobytes()


def test_line_step_rejects_bad_arguments():
    z = np.zeros(1, np.int32)
    assert nat.lib.oth_line_step_cpu(*([None] * 4), 1, 16, 1, *([None] * 8), nat.ptr(z)) \
        == nat.AZ_ERR_ARG
    assert nat.lib.oth_line_step_cpu(*([None] * 4), 0, 0, 1, *([None] * 8), nat.ptr(z)) \
        == nat.AZ_ERR_ARG
    assert nat.lib.oth_line_step_cpu(*([None] * 4), 0, 16, 1, *([None] * 8), None) \
        == nat.AZ_ERR_ARG
    z[0] = 7
    assert nat.lib.oth_line_step_cpu(*([None] * 4), 0, 16, 1, *([None] * 8), nat.ptr(z)) \
        == nat.AZ_OK and z[0] == 0
