"""Classical yardstick opponent: a depth-limited alpha-beta search over a fixed integer
evaluation (csrc/search.h), an absolute strength reference that does not drift as the nets
change.  It stands in for the external engine of the reference's play_mcts_vs_egaroucid.py.

* `evaluate` / `search` run the native code over a batch of positions, on the GPU
  (oth_search_gpu: one lane per search, refilled from a queue, roots split into subtrees)
  or on the host (oth_search_cpu over a thread pool; ctypes releases the GIL).
* `AlphaBetaPlayer` picks moves: the search's best move, or the exact solver's
  (endgame.solve) once few enough squares are empty.  `arena.BatchedArena` takes one as
  either side, and `arena.ladder` scores a net against a range of levels.
* `openings` draws distinct start positions, so that two near-deterministic players do not
  repeat one game.

value = V(position, depth) of include/az_othello.h from the side to move's view, best = the
lowest optimal action (64 = pass).
"""
import ctypes
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

import az_native as nat
import endgame
from endgame import MAX_THREADS, _as_i64_tensor, _as_u64_numpy, _pick_device

# fastest at the arena's shape, 1,024 openings (scripts/bench_search.py,
# profiles/search_bench.json): two plies 0.7 / 12.8 / 734 ms at depth 4 / 6 / 8 against 1.8 /
# 66.6 / 3,538 ms at one ply, 7.5 / 319 / 16,093 ms unsplit and 11.2 / 61.1 / 1,127 ms on 16
# host threads, so the GPU at two plies is the default (None = the GPU when there is one)
DEFAULT_SPLIT_PLIES = 2
DEFAULT_DEVICE = None
MAX_EXACT_EMPTIES = 12
INIT_OWN, INIT_OPP = 0x0000000810000000, 0x0000001008000000


def _search_cpu(own, opp, depth, node_limit):
    n = own.size
    value, best = np.empty(n, np.int16), np.empty(n, np.uint8)
    nodes = np.empty(n, np.uint64)
    if n == 0 or not 1 <= depth <= nat.AZ_SEARCH_MAX_DEPTH:
        # the library validates the arguments (and accepts n = 0)
        nat.check(nat.lib.oth_search_cpu(nat.ptr(own), nat.ptr(opp), n, int(depth),
                                         int(node_limit), nat.ptr(value), nat.ptr(best),
                                         nat.ptr(nodes)), "oth_search_cpu")
        return value, best, nodes
    threads = min(MAX_THREADS, n)
    # interleaved chunks much smaller than a thread's share (endgame._solve_cpu): the cost
    # per position is heavy-tailed
    size = max(1, min(256, n // (threads * 8) or 1))
    bounds = [(a, min(n, a + size)) for a in range(0, n, size)]

    def run(ab):
        a, b = ab
        return nat.lib.oth_search_cpu(nat.ptr(own[a:b]), nat.ptr(opp[a:b]), b - a, int(depth),
                                      int(node_limit), nat.ptr(value[a:b]), nat.ptr(best[a:b]),
                                      nat.ptr(nodes[a:b]))

    if threads == 1:
        rcs = [run(ab) for ab in bounds]
    else:
        with ThreadPoolExecutor(threads) as ex:
            rcs = list(ex.map(run, bounds))
    for rc in rcs:
        nat.check(rc, "oth_search_cpu")
    return value, best, nodes


def search_gpu_tensors(own, opp, depth, node_limit, split_plies, stream=None):
    """oth_search_gpu on int64 device tensors (the uint64 bitboards' bits), asynchronous on
    `stream` (default: the current stream).  Returns device tensors (value int16, best uint8,
    nodes int64 = the uint64 counts' bits)."""
    dev = own.device
    n = own.numel()
    value = torch.empty(n, dtype=torch.int16, device=dev)
    best = torch.empty(n, dtype=torch.uint8, device=dev)
    nodes = torch.empty(n, dtype=torch.int64, device=dev)
    need = ctypes.c_size_t(0)
    args = (int(depth), int(node_limit), int(split_plies))
    nat.check(nat.lib.oth_search_gpu(None, None, n, *args, None, None, None, None,
                                     ctypes.byref(need), None), "oth_search_gpu")
    with torch.cuda.device(dev):
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        with torch.cuda.stream(s):
            ws = torch.empty(max(need.value, 8), dtype=torch.uint8, device=dev)
            nat.check(nat.lib.oth_search_gpu(nat.ptr(own), nat.ptr(opp), n, *args,
                                             nat.ptr(value), nat.ptr(best), nat.ptr(nodes),
                                             nat.ptr(ws), ctypes.byref(need), nat.stream_ptr(s)),
                      "oth_search_gpu")
    return value, best, nodes


def evaluate(own, opp, device=None):
    """The leaf evaluation of every position (own = side to move): int16, T(d) for terminal
    positions, else the heuristic h.  Inputs, outputs and `device` as in `search`."""
    want_torch = isinstance(own, torch.Tensor)
    dev = _pick_device(device, own, opp)
    if dev.type == "cuda":
        o, p = _as_i64_tensor(own, dev), _as_i64_tensor(opp, dev)
        v = torch.empty(o.numel(), dtype=torch.int16, device=dev)
        with torch.cuda.device(dev):
            nat.check(nat.lib.oth_eval_gpu(nat.ptr(o), nat.ptr(p), o.numel(), nat.ptr(v),
                                           nat.stream_ptr(torch.cuda.current_stream(dev))),
                      "oth_eval_gpu")
        return v if want_torch else v.cpu().numpy()
    v = nat.eval_cpu(_as_u64_numpy(own), _as_u64_numpy(opp))
    return torch.from_numpy(v).to(own.device) if want_torch else v


def search(own, opp, depth, device=None, node_limit=1 << 31, split_plies=None):
    """Alpha-beta search of every position (own = side to move) to `depth` plies (1..10):
    returns (value int16, best uint8, nodes uint64).  Overlapping boards get value
    AZ_SEARCH_SKIPPED (-32768) and best 255; a search beyond `node_limit` nodes gets
    AZ_SEARCH_ABORTED (-32767).

    own / opp: numpy uint64 arrays (numpy results) or torch int64 tensors holding the same
    bits (torch results on the tensors' device, nodes as int64 bits).  device None = the GPU
    when one is available, else the host; "cpu" forces the host path (thread pool of at most
    16 threads).  split_plies (GPU only) None = DEFAULT_SPLIT_PLIES."""
    want_torch = isinstance(own, torch.Tensor)
    dev = _pick_device(device, own, opp)
    if dev.type == "cuda":
        sp = DEFAULT_SPLIT_PLIES if split_plies is None else int(split_plies)
        v, b, nd = search_gpu_tensors(_as_i64_tensor(own, dev), _as_i64_tensor(opp, dev), depth,
                                      node_limit, sp)
        if want_torch:
            return v, b, nd
        return v.cpu().numpy(), b.cpu().numpy(), nd.cpu().numpy().view(np.uint64)
    v, b, nd = _search_cpu(_as_u64_numpy(own), _as_u64_numpy(opp), depth, node_limit)
    if want_torch:
        return (torch.from_numpy(v).to(own.device), torch.from_numpy(b).to(own.device),
                torch.from_numpy(nd.view(np.int64)).to(own.device))
    return v, b, nd


class AlphaBetaPlayer:
    """Moves by `search` to `depth` plies; positions with 1..exact_empties empties (at most
    12) take the exact solver's best move instead."""

    def __init__(self, depth, exact_empties=0, device=DEFAULT_DEVICE):
        if not 1 <= int(depth) <= nat.AZ_SEARCH_MAX_DEPTH:
            raise ValueError(f"depth={depth} outside 1..{nat.AZ_SEARCH_MAX_DEPTH}")
        if not 0 <= int(exact_empties) <= MAX_EXACT_EMPTIES:
            raise ValueError(f"exact_empties={exact_empties} outside 0..{MAX_EXACT_EMPTIES}")
        self.depth, self.exact_empties, self.device = int(depth), int(exact_empties), device

    @classmethod
    def level(cls, level, device=DEFAULT_DEVICE):
        """Level L in 1..8: depth L, exact from min(2 L, 12) empties."""
        if not 1 <= int(level) <= 8:
            raise ValueError(f"level={level} outside 1..8")
        return cls(int(level), min(2 * int(level), MAX_EXACT_EMPTIES), device)

    def moves(self, own, opp):
        """One action (uint8, 64 = pass) per position; numpy uint64 bitboards."""
        own, opp = _as_u64_numpy(own), _as_u64_numpy(opp)
        e = endgame.empties(own, opp)
        exact = (e >= 1) & (e <= self.exact_empties) & ((own & opp) == 0)
        act = np.empty(len(own), np.uint8)
        if exact.any():
            score, best, _ = endgame.solve(own[exact], opp[exact], self.exact_empties,
                                           device=self.device)
            if (score == nat.AZ_SOLVE_ABORTED).any():
                raise RuntimeError("AlphaBetaPlayer: an exact solve exceeded the node limit")
            act[exact] = best
        if not exact.all():
            value, best, _ = search(own[~exact], opp[~exact], self.depth, device=self.device)
            if (value == nat.AZ_SEARCH_ABORTED).any():
                raise RuntimeError("AlphaBetaPlayer: a search exceeded the node limit")
            if (value == nat.AZ_SEARCH_SKIPPED).any():
                raise ValueError("AlphaBetaPlayer: overlapping boards")
            act[~exact] = best
        return act


def _random_step(own, opp, rng):
    """One uniformly random legal placement per position; ok = the position had one."""
    lg = nat.legal_cpu(own, opp)
    bits = ((lg[:, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(np.int64)
    cnt = bits.sum(axis=1)
    ok = cnt > 0
    k = rng.integers(0, np.maximum(cnt, 1))
    act = (np.cumsum(bits, axis=1) > k[:, None]).argmax(axis=1).astype(np.uint8)
    act[~ok] = 64
    o, p = nat.make_move_cpu(own, opp, act)
    return o, p, ok


def _canon(own, opp):
    import symmetry as sym_mod

    o, p, _, _ = sym_mod.canon_cpu(own, opp)
    return o, p


def reachable(plies, symmetry=False):
    """The distinct positions (own, opp) after exactly `plies` placements from the initial
    position that still have a placement.  symmetry=True: distinct up to the eight symmetries
    of the square, each in canonical form (symmetry.canon): 1, 3, 14, 60, 322, 1,773 after
    1..6 plies where there are 4, 12, 54, 236, 1,288, 7,092 positions."""
    own, opp = np.array([INIT_OWN], np.uint64), np.array([INIT_OPP], np.uint64)
    if symmetry:
        own, opp = _canon(own, opp)
    sh = np.arange(64, dtype=np.uint64)
    for _ in range(plies):
        lg = nat.legal_cpu(own, opp)
        par, act = np.nonzero(((lg[:, None] >> sh) & np.uint64(1)).astype(bool))
        own, opp = nat.make_move_cpu(own[par], opp[par], act.astype(np.uint8))
        if symmetry:  # the children of one member of a class cover the children's classes
            own, opp = _canon(own, opp)
        pair = np.unique(np.stack([own, opp], axis=1), axis=0)
        own, opp = np.ascontiguousarray(pair[:, 0]), np.ascontiguousarray(pair[:, 1])
    keep = nat.legal_cpu(own, opp) != 0
    return own[keep], opp[keep]


def openings(n, plies, seed, symmetry=False):
    """n distinct start positions (own, opp, player): each reached by `plies` uniformly random
    legal placements from the initial position (plies even and at most 8: no game can have
    ended, and the first player is to move again), drawn with numpy.random.default_rng(seed);
    duplicates on (own, opp, player) are dropped and redrawn until n are distinct.  Raises
    ValueError if fewer than n positions can be reached in `plies` plies.

    symmetry=True: the same draws, but a position that is an image of an earlier one under
    the symmetries of the square is a duplicate too, and the positions are returned in
    canonical form (symmetry.canon) -- n different games, where the default may return mirror
    images of one game."""
    n, plies = int(n), int(plies)
    if plies < 0 or plies > 8 or plies % 2:
        raise ValueError(f"plies={plies}: must be even and in 0..8")
    # 12, 236, 7,092 and 269,328 distinct positions at 2, 4, 6 and 8 plies: the small levels
    # are counted on every call, the last only for a request anywhere near its size
    # (up to symmetry at least an eighth of that: 3, 60, 1,773 and 33,666 or more)
    if plies <= 6 or n > (25000 if symmetry else 200000):
        have = len(reachable(plies, symmetry)[0])
        if n > have:
            raise ValueError(f"openings: {plies} plies reach {have} distinct positions"
                             f"{' up to symmetry' if symmetry else ''}, fewer than n={n}")
    rng = np.random.default_rng(seed)
    seen, out = set(), []
    while len(out) < n:
        m = max(16, 2 * (n - len(out)))
        own, opp = np.full(m, INIT_OWN, np.uint64), np.full(m, INIT_OPP, np.uint64)
        ok = np.ones(m, bool)
        for _ in range(plies):
            own, opp, had = _random_step(own, opp, rng)
            ok &= had
        ok &= nat.legal_cpu(own, opp) != 0
        if symmetry:
            own, opp = _canon(own, opp)
        for o, p in zip(own[ok].tolist(), opp[ok].tolist()):
            if (o, p) not in seen and len(out) < n:
                seen.add((o, p))
                out.append((o, p))
    arr = np.array(out, np.uint64).reshape(-1, 2)
    return (np.ascontiguousarray(arr[:, 0]), np.ascontiguousarray(arr[:, 1]),
            np.ones(n, np.int32))
