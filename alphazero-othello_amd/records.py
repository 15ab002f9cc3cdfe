"""Game records to training rows: the data path of the reference's supervised_benchmark.py
(process_game, keep_by_ply, remove_conflicting_duplicates) on bitboards and in batches.

    acts = parse_transcripts(["f5d6c3...", ...])          # or from_arena(arena records)
    own, opp, act, z, ply, game, report = replay(acts, winner=w)
    rows = dedup(own, opp, act, z, how="vote")            # majority vote per board

`replay` runs the native transcript replay (csrc/records.h: one game per GPU lane, or
oth_records_cpu over a thread pool) with the true side to move: a pass the record omits is
inserted, where the reference alternates colours blindly and mislabels every row after it.
`vote` is the reference's majority-vote dedup (az_records_vote_gpu, with a NumPy mirror on the
host); `dedup(how="mean")` keeps the empirical move distribution and the mean outcome instead
(replay.aggregate_rows).

Boards are uint64 bitboards (bit r*8+c; own = the side to move): NumPy uint64 arrays on the
host, torch int64 tensors holding the same bits on the device.
"""
import ctypes
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

import az_native as nat
from endgame import MAX_THREADS

INIT_OWN, INIT_OPP = 0x0000000810000000, 0x0000001008000000
END = 255
STATUS_NAMES = {nat.AZ_REC_TERMINAL: "terminal", nat.AZ_REC_UNFINISHED: "unfinished",
                nat.AZ_REC_ILLEGAL: "illegal", nat.AZ_REC_OVERFLOW: "overflow"}

# Which side `replay(device=None)` takes for NumPy input when a GPU is present.  Measured by
# scripts/bench_records.py (profiles/records_bench.json; DESIGN.md "Game records"): NumPy in,
# NumPy out, 2^20 games take 0.30 s through the GPU against 1.12 s on 16 host threads.
PREFER_GPU = True


def _check_stride(stride):
    stride = int(stride)
    if stride <= 0 or stride % 16 or stride > nat.AZ_REC_MAX_STRIDE:
        raise ValueError(f"stride={stride}: must be a multiple of 16 in 16..{nat.AZ_REC_MAX_STRIDE}")
    return stride


def parse_transcripts(games, stride=64):
    """Transcript strings ("f5d6c3...": two characters per move, a column letter a-h in
    either case and a row digit 1-8, supervised_benchmark.py:130-139) -> uint8 [n, stride]
    actions row*8+col, padded with 255.  Odd length, a bad character or more than `stride`
    moves raise ValueError naming the game index."""
    stride = _check_stride(stride)
    games = list(games)
    n = len(games)
    acts = np.full((n, stride), END, np.uint8)
    if n == 0:
        return acts
    lens = np.fromiter((len(g) for g in games), np.int64, n)
    if (lens % 2).any():
        g = int(np.flatnonzero(lens % 2)[0])
        raise ValueError(f"game {g}: odd transcript length {int(lens[g])}")
    if (lens > 2 * stride).any():
        g = int(np.flatnonzero(lens > 2 * stride)[0])
        raise ValueError(f"game {g}: {int(lens[g]) // 2} moves, more than stride={stride}")
    try:
        flat = np.frombuffer("".join(games).encode("ascii"), np.uint8)
    except UnicodeEncodeError:
        g = next(i for i, s in enumerate(games) if not s.isascii())
        raise ValueError(f"game {g}: non-ASCII character in the transcript") from None
    col = (flat[0::2] | 0x20).astype(np.int16) - ord("a")  # ASCII letters fold to lower case
    row = flat[1::2].astype(np.int16) - ord("1")
    moves = lens // 2
    owner = np.repeat(np.arange(n), moves)
    bad = (col < 0) | (col > 7) | (row < 0) | (row > 7) | ((flat[0::2] & 0xC0) != 0x40)
    if bad.any():
        k = int(np.flatnonzero(bad)[0])
        g = int(owner[k])
        at = k - int(moves[:g].sum())
        raise ValueError(f"game {g}: bad move {games[g][2 * at:2 * at + 2]!r} at move {at}")
    within = np.arange(len(owner)) - np.repeat(np.cumsum(moves) - moves, moves)
    acts[owner, within] = (row * 8 + col).astype(np.uint8)
    return acts


def from_arena(records, stride=None):
    """The record dicts of BatchedArena.play(record=True) -> (acts uint8 [n, stride], own0,
    opp0 uint64 [n], winner int8 [n]).  The start position's side to move is the first mover;
    `result` (+1 = A won) becomes the winner from the first mover's view through `a_first`.
    stride None = the smallest multiple of 16 that holds the longest game."""
    records = list(records)
    n = len(records)
    longest = max((len(r["actions"]) for r in records), default=0)
    if stride is None:
        stride = max(16, -(-longest // 16) * 16)
    stride = _check_stride(stride)
    acts = np.full((n, stride), END, np.uint8)
    for g, r in enumerate(records):
        a = np.asarray(r["actions"], np.int64)
        if len(a) > stride:
            raise ValueError(f"game {g}: {len(a)} moves, more than stride={stride}")
        if len(a) and (a.min() < 0 or a.max() > 64):
            raise ValueError(f"game {g}: action outside 0..64")
        acts[g, :len(a)] = a
    own0 = np.array([r["own"] for r in records], np.uint64)
    opp0 = np.array([r["opp"] for r in records], np.uint64)
    winner = np.array([r["result"] if r["a_first"] else -r["result"] for r in records], np.int8)
    return acts, own0, opp0, winner


def random_playouts(n, seed=0, stride=64, write_passes=True):
    """n uniformly random legal games from the initial position as transcript lines uint8
    [n, stride] (the workload of scripts/bench_records.py and the tests), played in lockstep
    through the host board step.  write_passes: forced passes are written as 64, else left
    out.  A game whose line is full stops there."""
    stride = _check_stride(stride)
    rng = np.random.default_rng(seed)
    acts = np.full((n, stride), END, np.uint8)
    own, opp = np.full(n, INIT_OWN, np.uint64), np.full(n, INIT_OPP, np.uint64)
    used = np.zeros(n, np.int64)
    live = np.arange(n)
    while len(live):
        o, p = own[live], opp[live]
        lg = nat.legal_cpu(o, p)
        stuck = lg == 0
        other = np.zeros(len(live), bool)
        if stuck.any():
            other[stuck] = nat.legal_cpu(p[stuck], o[stuck]) != 0
        bits = np.unpackbits(lg.view(np.uint8).reshape(-1, 8), axis=1, bitorder="little")
        cnt = bits.sum(axis=1, dtype=np.int64)
        k = rng.integers(0, np.maximum(cnt, 1))
        a = (np.cumsum(bits, axis=1, dtype=np.uint8) > k[:, None].astype(np.uint8)).argmax(axis=1)
        a = np.where(stuck, 64, a).astype(np.uint8)
        go = ~stuck | other  # the game goes on: a placement or a pass
        write = go & (~stuck | write_passes)
        w = live[write]
        acts[w, used[w]] = a[write]
        used[w] += 1
        no, np_ = nat.make_move_cpu(o[go], p[go], a[go])
        own[live[go]], opp[live[go]] = no, np_
        live = live[go & (used[live] < stride)]
    return acts


# ---- native replay ---------------------------------------------------------------------

_ROW_FIELDS = (("own", np.uint64), ("opp", np.uint64), ("act", np.uint8), ("z", np.int8),
               ("ply", np.uint8))
_GAME_FIELDS = (("n_rows", np.int32), ("status", np.uint8), ("bad_ply", np.uint8),
                ("final_own", np.uint64), ("final_opp", np.uint64), ("final_colour", np.int8),
                ("final_diff", np.int8))
_ORDER = ("own", "opp", "act", "z", "ply", "n_rows", "status", "bad_ply", "final_own",
          "final_opp", "final_colour", "final_diff")
_TORCH = {np.uint64: torch.int64, np.uint8: torch.uint8, np.int8: torch.int8,
          np.int32: torch.int32}


def replay_cpu_raw(acts, own0, opp0, winner, max_rows, flags):
    """One oth_records_cpu call: dict of the ply-major row arrays [max_rows, n] (zero where no
    row was written) and the per-game arrays [n]."""
    n, stride = acts.shape
    out = {k: np.zeros((max_rows, n), dt) for k, dt in _ROW_FIELDS}
    out.update({k: np.zeros(n, dt) for k, dt in _GAME_FIELDS})
    nat.check(nat.lib.oth_records_cpu(nat.ptr(acts), stride, nat.ptr(own0), nat.ptr(opp0),
                                      nat.ptr(winner), n, int(max_rows), int(flags),
                                      *[nat.ptr(out[k]) for k in _ORDER]), "oth_records_cpu")
    return out


def replay_gpu_raw(acts, own0, opp0, winner, max_rows, flags, stream=None):
    """oth_records_gpu on device tensors (acts uint8 [n, stride], own0 / opp0 int64 bits,
    winner int8; the last three may be None), asynchronous on `stream`: dict of device tensors
    laid out as in replay_cpu_raw (uint64 fields as int64 bits)."""
    dev = acts.device
    n, stride = acts.shape
    with torch.cuda.device(dev):
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        with torch.cuda.stream(s):
            out = {k: torch.zeros((max_rows, n), dtype=_TORCH[dt], device=dev)
                   for k, dt in _ROW_FIELDS}
            out.update({k: torch.zeros(n, dtype=_TORCH[dt], device=dev) for k, dt in _GAME_FIELDS})
            nat.check(nat.lib.oth_records_gpu(nat.ptr(acts), stride, nat.ptr(own0), nat.ptr(opp0),
                                              nat.ptr(winner), n, int(max_rows), int(flags),
                                              *[nat.ptr(out[k]) for k in _ORDER],
                                              nat.stream_ptr(s)), "oth_records_gpu")
    return out


def _replay_cpu(acts, own0, opp0, winner, max_rows, flags):
    """oth_records_cpu over a thread pool (ctypes releases the GIL), one slice of games per
    call; the slices' ply-major outputs are joined along the game axis."""
    n = acts.shape[0]
    threads = max(1, min(MAX_THREADS, n // 256))
    if threads == 1:
        return replay_cpu_raw(acts, own0, opp0, winner, max_rows, flags)
    bounds = np.linspace(0, n, threads + 1).astype(np.int64)
    cut = lambda x, a, b: None if x is None else x[a:b]  # noqa: E731

    def run(k):
        a, b = int(bounds[k]), int(bounds[k + 1])
        return replay_cpu_raw(acts[a:b], cut(own0, a, b), cut(opp0, a, b), cut(winner, a, b),
                              max_rows, flags)

    with ThreadPoolExecutor(threads) as ex:
        parts = list(ex.map(run, range(threads)))
    return {k: np.concatenate([p[k] for p in parts], axis=-1) for k in _ORDER}


def _sign(x):
    return (x > 0).to(torch.int8) - (x < 0).to(torch.int8) if isinstance(x, torch.Tensor) \
        else np.sign(x).astype(np.int8)


def replay(acts, own0=None, opp0=None, winner=None, pass_rows=False, device=None,
           on_error="drop", max_rows=None):
    """Replay recorded games into training rows.

    acts: uint8 [n, stride] (parse_transcripts / from_arena; NumPy, or a torch tensor);
    own0 / opp0: start positions (None = the initial position); winner: int8 [n] in
    {+1, 0, -1} from the first mover's view (None = derived from the final position of a
    finished game, 0 for an unfinished one).  pass_rows: passes emit rows (action 64) too.

    Returns (own, opp, act, z, ply, game, report): the rows of all kept games, game after
    game and ply after ply -- canonical boards (own = the mover), the move, z = winner x the
    mover's colour, the ply of the game and the game's index -- and the per-game report, a dict
    of status, bad_ply, final_diff, n_rows (rows the replay emitted), winner_mismatch (a given
    winner that is not sign(final_diff) of a terminal game) and kept.  NumPy in, NumPy out;
    torch in, torch out (boards as int64 bits).

    on_error: what happens to a game that stopped with AZ_REC_ILLEGAL or AZ_REC_OVERFLOW --
    "drop" leaves out all its rows, "truncate" keeps the rows before the stop, "raise" raises
    ValueError naming the first such game.  Unfinished games are not errors.
    device None: the GPU for device tensors; for NumPy input the GPU when there is one and it
    is the faster side (PREFER_GPU), else the host entry on at most 16 threads."""
    if on_error not in ("drop", "truncate", "raise"):
        raise ValueError(f"on_error={on_error!r}: one of 'drop', 'truncate', 'raise'")
    want_torch = isinstance(acts, torch.Tensor)
    if device is not None:
        dev = torch.device(device)
    elif want_torch:
        dev = acts.device
    else:
        dev = torch.device("cuda", torch.cuda.current_device()) \
            if PREFER_GPU and torch.cuda.is_available() else torch.device("cpu")
    if acts.ndim != 2:
        raise ValueError("acts must be [n, stride]")
    n, stride = int(acts.shape[0]), _check_stride(acts.shape[1])
    if (own0 is None) != (opp0 is None):
        raise ValueError("own0 and opp0 must both be given or both be None")
    flags = nat.AZ_REC_PASS_ROWS if pass_rows else 0
    if max_rows is None:
        max_rows = min(nat.AZ_REC_MAX_ROWS, stride * 2 if pass_rows else stride)
    if dev.type == "cuda":
        def t(x, dt):
            if x is None:
                return None
            if not isinstance(x, torch.Tensor):
                x = np.ascontiguousarray(x)
                x = torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x)
            return x.to(device=dev, dtype=dt).contiguous()
        w = t(winner, torch.int8)
        raw = replay_gpu_raw(t(acts, torch.uint8), t(own0, torch.int64), t(opp0, torch.int64), w,
                             max_rows, flags)
        xp_arange = lambda k: torch.arange(k, device=dev)  # noqa: E731
    else:
        def a(x, dt):
            if x is None:
                return None
            if isinstance(x, torch.Tensor):
                x = x.detach().cpu().numpy()
                x = x.view(np.uint64) if dt == np.uint64 and x.dtype == np.int64 else x
            return np.ascontiguousarray(x, dtype=dt)
        w = a(winner, np.int8)
        raw = _replay_cpu(a(acts, np.uint8), a(own0, np.uint64), a(opp0, np.uint64), w, max_rows,
                          flags)
        xp_arange = np.arange
    status, n_rows = raw["status"], raw["n_rows"]
    error = (status == nat.AZ_REC_ILLEGAL) | (status == nat.AZ_REC_OVERFLOW)
    if on_error == "raise" and bool(error.any()):
        g = int(error.nonzero()[0][0]) if dev.type == "cuda" else int(np.flatnonzero(error)[0])
        raise ValueError(f"game {g}: {STATUS_NAMES[int(status[g])]} at entry "
                         f"{int(raw['bad_ply'][g])}")
    kept = ~error if on_error == "drop" else (error | ~error)
    take = n_rows * kept.to(torch.int32) if dev.type == "cuda" else n_rows * kept
    # [max_rows, n] ply-major -> game-major selection of the rows r < take[g]
    mask = (xp_arange(max_rows)[None, :] < take[:, None])
    rows = [raw[k].T[mask] for k in ("own", "opp", "act", "z", "ply")]
    game = (xp_arange(n)[:, None] + 0 * xp_arange(max_rows)[None, :])[mask]
    if w is None:
        mismatch = error & ~error
    else:
        mismatch = (status == nat.AZ_REC_TERMINAL) & (w != _sign(raw["final_diff"]))
    report = {"status": status, "bad_ply": raw["bad_ply"], "final_diff": raw["final_diff"],
              "n_rows": n_rows, "winner_mismatch": mismatch, "kept": kept}
    if dev.type == "cuda" and not want_torch:
        rows = [r.cpu().numpy() for r in rows]
        rows[0], rows[1] = rows[0].view(np.uint64), rows[1].view(np.uint64)
        game = game.cpu().numpy()
        report = {k: v.cpu().numpy() for k, v in report.items()}
    elif dev.type != "cuda" and want_torch:
        rows[0], rows[1] = rows[0].view(np.int64), rows[1].view(np.int64)
        rows = [torch.from_numpy(np.ascontiguousarray(r)).to(acts.device) for r in rows]
        game = torch.from_numpy(game).to(acts.device)
        report = {k: torch.from_numpy(v).to(acts.device) for k, v in report.items()}
    return (*rows, game, report)


def keep_mask(ply, u, schedule=((8, 0.30), (16, 0.70))):
    """The reference's keep_by_ply (supervised_benchmark.py:169-176) with the uniforms passed
    in: row i is kept iff u[i] < p(ply[i]), p = the probability of the first schedule entry
    (limit, p) with ply < limit, 1 past the last."""
    xp = torch if isinstance(ply, torch.Tensor) else np
    p = xp.ones_like(u)
    for limit, prob in reversed(sorted(schedule)):
        p = xp.where(ply < limit, prob * xp.ones_like(u), p)
    return u < p


# ---- dedup -----------------------------------------------------------------------------

def vote_numpy(own, opp, act, z, symmetry=False):
    """The host mirror of az_records_vote_gpu: (own, opp, act, z, count) with one row per
    distinct board in order of first occurrence, the most frequent action and outcome of its
    group, ties to the value that appeared first.  symmetry=True: per class of boards up to
    symmetry (`canonical_rows` on the host first)."""
    if symmetry:
        own, opp, act = canonical_rows(np.asarray(own), opp, act, device="cpu")
    own = np.ascontiguousarray(own, np.uint64).reshape(-1)
    opp = np.ascontiguousarray(opp, np.uint64).reshape(-1)
    act = np.ascontiguousarray(act, np.uint8).reshape(-1)
    z = np.ascontiguousarray(z, np.int8).reshape(-1)
    n = len(own)
    if n == 0:
        return own, opp, act, z, np.zeros(0, np.int32)
    order = np.lexsort((opp, own))  # stable: buffer order inside a group
    so, sp = own[order], opp[order]
    head = np.ones(n, bool)
    head[1:] = (so[1:] != so[:-1]) | (sp[1:] != sp[:-1])
    gid = np.cumsum(head) - 1
    starts = np.flatnonzero(head)
    first = order[starts]  # first occurrence of every group
    count = np.diff(np.append(starts, n)).astype(np.int32)

    def majority(val):
        key = gid * 256 + val[order].astype(np.int64)
        o2 = np.argsort(key, kind="stable")
        ks = key[o2]
        rh = np.ones(n, bool)
        rh[1:] = ks[1:] != ks[:-1]
        rs = np.flatnonzero(rh)
        rlen = np.diff(np.append(rs, n)).astype(np.int64)
        rfirst = order[o2][rs].astype(np.int64)
        score = (rlen << 32) | (0xFFFFFFFF - rfirst)
        best = np.zeros(len(starts), np.int64)
        np.maximum.at(best, ks[rs] >> 8, score)
        return val[0xFFFFFFFF - (best & 0xFFFFFFFF)]

    out_order = np.argsort(first, kind="stable")
    va, vz = majority(act), majority(z.view(np.uint8)).view(np.int8)
    f = first[out_order]
    return own[f], opp[f], va[out_order], vz[out_order], count[out_order]


def mean_numpy(own, opp, act, z, symmetry=False):
    """The host form of dedup(how="mean"): per distinct board, in order of first occurrence,
    pi = the share of every action (float32 count / size) and z = the mean outcome
    (float64 mean, cast to float32).  symmetry=True: per class of boards up to symmetry
    (`canonical_rows` on the host first)."""
    if symmetry:
        own, opp, act = canonical_rows(np.asarray(own), opp, act, device="cpu")
    own = np.ascontiguousarray(own, np.uint64).reshape(-1)
    opp = np.ascontiguousarray(opp, np.uint64).reshape(-1)
    n = len(own)
    order = np.lexsort((opp, own))
    so, sp = own[order], opp[order]
    head = np.ones(n, bool)
    head[1:] = (so[1:] != so[:-1]) | (sp[1:] != sp[:-1])
    gid = np.empty(n, np.int64)
    gid[order] = np.cumsum(head) - 1  # group of every row, numbered in board order
    first = order[np.flatnonzero(head)]
    rank = np.empty(len(first), np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(len(first))
    g = rank[gid]                     # ... renumbered in order of first occurrence
    m = len(first)
    cnt = np.bincount(g, minlength=m)
    pi = np.zeros((m, 65), np.float32)
    np.add.at(pi, (g, np.asarray(act).astype(np.int64)), np.float32(1))
    pi /= cnt[:, None].astype(np.float32)
    zsum = np.bincount(g, weights=np.asarray(z, np.float64), minlength=m)
    f = np.sort(first)
    return {"own": own[f], "opp": opp[f], "pi": pi, "z": (zsum / cnt).astype(np.float32),
            "count": cnt.astype(np.int32)}


def vote_gpu_tensors(own, opp, act, z, stream=None):
    """az_records_vote_gpu on device tensors (own / opp int64 bits, act uint8, z int8):
    (own, opp, act, z, count int32) of the voted rows."""
    dev = own.device
    n = int(own.numel())
    m = max(n, 1)
    with torch.cuda.device(dev):
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        with torch.cuda.stream(s):
            outs = [torch.empty(m, dtype=dt, device=dev)
                    for dt in (torch.int64, torch.int64, torch.uint8, torch.int8, torch.int32)]
            n_out = torch.zeros(1, dtype=torch.int32, device=dev)
            wsb = ctypes.c_size_t(0)
            args = [nat.ptr(own), nat.ptr(opp), nat.ptr(act), nat.ptr(z), n,
                    *[nat.ptr(o) for o in outs], nat.ptr(n_out)]
            nat.check(nat.lib.az_records_vote_gpu(*args, None, ctypes.byref(wsb),
                                                  nat.stream_ptr(s)), "az_records_vote_gpu")
            ws = torch.empty(max(int(wsb.value), 8), dtype=torch.uint8, device=dev)
            nat.check(nat.lib.az_records_vote_gpu(*args, nat.ptr(ws), ctypes.byref(wsb),
                                                  nat.stream_ptr(s)), "az_records_vote_gpu")
            k = int(n_out.item())
    return tuple(o[:k] for o in outs)


def _rows_to_device(own, opp, act, z, dev):
    def t(x, dt):
        if not isinstance(x, torch.Tensor):
            x = np.ascontiguousarray(x)
            x = torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x)
        return x.reshape(-1).to(device=dev, dtype=dt).contiguous()
    return t(own, torch.int64), t(opp, torch.int64), t(act, torch.uint8), t(z, torch.int8)


def _pick(device, x):
    if device is not None:
        return torch.device(device)
    if isinstance(x, torch.Tensor):
        return x.device
    return torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() \
        else torch.device("cpu")


def canonical_rows(own, opp, act, device=None):
    """(own, opp, act) of every row in the canonical frame of its board (symmetry.canon): the
    move goes through the board's symmetry and then to the smallest square of its orbit under
    the symmetries that fix the canonical board, so mirror-image moves of a symmetric position
    count as one.  Computed where dedup would run (`_pick`); types follow the input."""
    import symmetry as sym_mod

    dev = _pick(device, own)
    o, p, s, stab = sym_mod.canon(own, opp, device=dev)
    _, a = sym_mod.transform_rows(act=act, sym=s, stab=stab, device=dev)
    return o, p, a


def vote(own, opp, act, z, device=None, symmetry=False):
    """Majority-vote dedup (remove_conflicting_duplicates): (own, opp, act, z, count), one row
    per distinct board in order of first occurrence.  On the GPU (device None: when there is
    one, or where the tensors are) the kernel, on the host the NumPy mirror; NumPy in, NumPy
    out, torch in, torch out.  symmetry=True votes per class of boards up to the symmetries of
    the square (`canonical_rows` first; the boards come out canonical)."""
    if symmetry:
        own, opp, act = canonical_rows(own, opp, act, device)
    want_torch = isinstance(own, torch.Tensor)
    dev = _pick(device, own)
    if dev.type == "cuda":
        res = vote_gpu_tensors(*_rows_to_device(own, opp, act, z, dev))
        if want_torch:
            return res
        res = [r.cpu().numpy() for r in res]
        return (res[0].view(np.uint64), res[1].view(np.uint64), *res[2:])
    to_np = lambda x: x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)  # noqa: E731
    o, p = to_np(own), to_np(opp)
    o = o.view(np.uint64) if o.dtype == np.int64 else o
    p = p.view(np.uint64) if p.dtype == np.int64 else p
    res = vote_numpy(o, p, to_np(act), to_np(z))
    if want_torch:
        return (torch.from_numpy(res[0].view(np.int64)).to(own.device),
                torch.from_numpy(res[1].view(np.int64)).to(own.device),
                *[torch.from_numpy(r).to(own.device) for r in res[2:]])
    return res


def dedup(own, opp, act, z, how="vote", device=None, symmetry=False):
    """Collapse repeated boards.  Returns a dict: own, opp, count and
      how="vote": act uint8, z int8 -- the majority vote (`vote`);
      how="mean": pi float32 [m, 65] the empirical move distribution, z float32 the mean
                  outcome (on the GPU one-hot pi through replay.aggregate_rows with version
                  0, on the host `mean_numpy`);
      how=None:   the rows as they are (act, z), count 1.
    symmetry=True: boards that are images of each other under the symmetries of the square
    are one board -- every row is first brought to its canonical frame (`canonical_rows`)."""
    if how not in ("vote", "mean", None):
        raise ValueError(f"how={how!r}: one of 'vote', 'mean', None")
    if symmetry:
        own, opp, act = canonical_rows(own, opp, act, device)
    if how == "vote":
        o, p, a, zz, c = vote(own, opp, act, z, device=device)
        return {"own": o, "opp": p, "act": a, "z": zz, "count": c}
    if how is None:
        ones = torch.ones_like(act, dtype=torch.int32) if isinstance(act, torch.Tensor) \
            else np.ones(len(act), np.int32)
        return {"own": own, "opp": opp, "act": act, "z": z, "count": ones}
    import replay as replay_mod

    want_torch = isinstance(own, torch.Tensor)
    dev = _pick(device, own)
    if dev.type != "cuda":
        to_np = lambda x: x.detach().cpu().numpy() if want_torch else np.asarray(x)  # noqa: E731
        o, p = to_np(own), to_np(opp)
        out = mean_numpy(o.view(np.uint64) if o.dtype == np.int64 else o,
                         p.view(np.uint64) if p.dtype == np.int64 else p, to_np(act), to_np(z))
        if want_torch:
            out["own"], out["opp"] = out["own"].view(np.int64), out["opp"].view(np.int64)
            out = {k: torch.from_numpy(v).to(own.device) for k, v in out.items()}
        return out
    o, p, a, zz = _rows_to_device(own, opp, act, z, dev)
    pi = torch.zeros(o.numel(), 65, dtype=torch.float32, device=dev)
    pi.scatter_(1, a.to(torch.int64)[:, None], 1.0)
    res = replay_mod.aggregate_rows(o, p, torch.zeros(o.numel(), dtype=torch.int32, device=dev),
                                    pi, zz.to(torch.float64))
    out = {"own": res["own"], "opp": res["opp"], "pi": res["pi"], "z": res["v"],
           "count": res["count"]}
    if not want_torch:
        out = {k: v.cpu().numpy() for k, v in out.items()}
        out["own"], out["opp"] = out["own"].view(np.uint64), out["opp"].view(np.uint64)
    return out
