"""Generate tests/golden/records_cases.npz by running the REFERENCE's supervised data path
(supervised_benchmark.py: process_game, remove_conflicting_duplicates) on seeded random games.

Runs only in the build container, where the reference tree is mounted read-only at
/root/reference (like make_goldens.py); the tests read only the committed .npz.

    python tests/golden/make_records_goldens.py

Games are uniformly random legal playouts from the initial position through the project's
host board step (az_native), seed 20240607.  Boards are stored as bitboards (bit r*8+c) of
the canonical board the reference emits (board * player): own = its +1 squares.

  free_*   64 complete games WITHOUT a pass (selected by rejection: process_game alternates
           colours blindly and mislabels everything after a pass, so only these compare), and
           process_game's rows for winner = the true result from the first mover's view:
           free_acts [64, 64], free_len, free_winner, and the rows of all games in order
           (free_row_game, free_row_own / _opp, free_row_act, free_row_z, free_row_ply).
  trunc_*  the 16 truncations of game 0 to 0..15 moves, same winner, same row arrays.
  pass_*   24 complete games with at least one forced pass, as pass_acts_explicit (64s
           written) and pass_acts_omitted; expected rows from stepping oracle/board.py with
           the true mover (NOT from the reference): one row per entry of the explicit form,
           passes included (pass_row_game / _own / _opp / _act / _colour / _ply), pass_winner.
  vote_*   2,400 rows of 400 games cut to 6 plies from 5 two-move openings with random
           winners, so boards repeat with conflicting moves and outcomes and votes tie
           (vote_in_own / _opp / _act / _z), and remove_conflicting_duplicates' output in the
           reference's order (vote_out_own / _opp / _act / _z).
"""
import contextlib
import io
import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True

import numpy as np  # noqa: E402

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REF)
sys.path.append(ROOT)
sys.path.append(os.path.join(ROOT, "alphazero-othello_amd"))

import supervised_benchmark as sb  # noqa: E402  (the reference)

import az_native as nat  # noqa: E402
from oracle import board as ob  # noqa: E402

INIT_OWN, INIT_OPP = 0x0000000810000000, 0x0000001008000000
_W = np.uint64(1) << np.arange(64, dtype=np.uint64)


def playout(rng, prefix=(), max_plies=None):
    """Random legal game from the initial position: the action list with passes written."""
    o, p = INIT_OWN, INIT_OPP
    acts = []
    while max_plies is None or len(acts) < max_plies:
        lg = int(nat.legal_cpu([o], [p])[0])
        if not lg:
            if not int(nat.legal_cpu([p], [o])[0]):
                break
            acts.append(64)
            o, p = p, o
            continue
        moves = [a for a in range(64) if (lg >> a) & 1]
        a = prefix[len(acts)] if len(acts) < len(prefix) else int(rng.choice(moves))
        assert a in moves
        acts.append(a)
        no, np_ = nat.make_move_cpu([o], [p], [a])
        o, p = int(no[0]), int(np_[0])
    return acts


def true_winner(acts):
    """sign of the final disc difference from the first mover's view (oracle board)."""
    o, p, colour = INIT_OWN, INIT_OPP, 1
    for a in acts:
        o, p = (p, o) if a == 64 else ob.make_move(o, p, a)
        colour = -colour
    d = colour * (ob.popc(o) - ob.popc(p))
    return int(np.sign(d))


def transcript(acts):
    return "".join("abcdefgh"[a % 8] + "12345678"[a // 8] for a in acts)


def canon_bits(board):
    flat = np.asarray(board).reshape(-1)
    own = np.bitwise_or.reduce(np.where(flat == 1, _W, np.uint64(0)))
    opp = np.bitwise_or.reduce(np.where(flat == -1, _W, np.uint64(0)))
    return np.uint64(own), np.uint64(opp)


def pad(games, stride=64):
    out = np.full((len(games), stride), 255, np.uint8)
    for g, a in enumerate(games):
        out[g, :len(a)] = a
    return out


def reference_rows(games, winners, prefix):
    rows = {k: [] for k in ("game", "own", "opp", "act", "z", "ply")}
    for g, (acts, w) in enumerate(zip(games, winners)):
        for board, action, value, ply in sb.process_game(transcript(acts), float(w)):
            own, opp = canon_bits(board)
            rows["game"].append(g), rows["own"].append(own), rows["opp"].append(opp)
            rows["act"].append(action), rows["z"].append(int(value)), rows["ply"].append(ply)
    dt = {"game": np.int32, "own": np.uint64, "opp": np.uint64, "act": np.uint8, "z": np.int8,
          "ply": np.uint8}
    return {f"{prefix}_row_{k}": np.array(v, dt[k]) for k, v in rows.items()}


def main():
    rng = np.random.default_rng(20240607)
    free, passed = [], []
    while len(free) < 64 or len(passed) < 24:
        a = playout(rng)
        if 64 in a:
            if len(passed) < 24:
                passed.append(a)
        elif len(free) < 64:
            free.append(a)
    assert len(free) == 64 and len(passed) == 24
    out = {}
    # pass-free games against process_game
    fw = [true_winner(a) for a in free]
    out["free_acts"] = pad(free)
    out["free_len"] = np.array([len(a) for a in free], np.int32)
    out["free_winner"] = np.array(fw, np.int8)
    out.update(reference_rows(free, fw, "free"))
    trunc = [free[0][:k] for k in range(16)]
    out["trunc_acts"] = pad(trunc)
    out["trunc_len"] = np.arange(16, dtype=np.int32)
    out["trunc_winner"] = np.full(16, fw[0], np.int8)
    out.update(reference_rows(trunc, [fw[0]] * 16, "trunc"))
    # forced-pass games against the oracle board with the true mover
    rows = {k: [] for k in ("game", "own", "opp", "act", "colour", "ply")}
    for g, acts in enumerate(passed):
        o, p, colour = INIT_OWN, INIT_OPP, 1
        for ply, a in enumerate(acts):
            lg = ob.legal(o, p)
            assert (a == 64 and lg == 0 and ob.legal(p, o) != 0) or (a < 64 and (lg >> a) & 1)
            rows["game"].append(g), rows["own"].append(o), rows["opp"].append(p)
            rows["act"].append(a), rows["colour"].append(colour), rows["ply"].append(ply)
            o, p = (p, o) if a == 64 else ob.make_move(o, p, a)
            colour = -colour
        assert ob.legal(o, p) == 0 and ob.legal(p, o) == 0
    dt = {"game": np.int32, "own": np.uint64, "opp": np.uint64, "act": np.uint8,
          "colour": np.int8, "ply": np.uint8}
    out.update({f"pass_row_{k}": np.array(v, dt[k]) for k, v in rows.items()})
    out["pass_acts_explicit"] = pad(passed, 80)
    out["pass_acts_omitted"] = pad([[a for a in g if a != 64] for g in passed], 80)
    out["pass_winner"] = np.array([true_winner(a) for a in passed], np.int8)
    # majority vote: short games from few openings, random winners
    lg = int(nat.legal_cpu([INIT_OWN], [INIT_OPP])[0])
    firsts = [a for a in range(64) if (lg >> a) & 1]
    prefixes = []
    while len(prefixes) < 5:
        pre = tuple(playout(rng, (firsts[len(prefixes) % len(firsts)],), 2))
        if pre not in prefixes:
            prefixes.append(pre)
    examples = []
    for g in range(400):
        acts = playout(rng, prefixes[int(rng.integers(0, 5))], 6)
        w = float(rng.integers(-1, 2))
        examples += [(b, a, v) for b, a, v, _ in sb.process_game(transcript(acts), w)]
    with contextlib.redirect_stdout(io.StringIO()):  # it prints every conflict
        voted = sb.remove_conflicting_duplicates(examples)
    assert len(voted) < len(examples)
    for name, rows_ in (("in", examples), ("out", voted)):
        bits = [canon_bits(b) for b, _, _ in rows_]
        out[f"vote_{name}_own"] = np.array([b[0] for b in bits], np.uint64)
        out[f"vote_{name}_opp"] = np.array([b[1] for b in bits], np.uint64)
        out[f"vote_{name}_act"] = np.array([a for _, a, _ in rows_], np.uint8)
        out[f"vote_{name}_z"] = np.array([int(v) for _, _, v in rows_], np.int8)
    path = os.path.join(HERE, "records_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", len(examples), "vote rows ->", len(voted))


if __name__ == "__main__":
    main()
