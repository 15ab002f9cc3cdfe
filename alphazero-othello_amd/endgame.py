"""Exact endgame solver: game-theoretic scores, best moves and exact value targets.

`solve` runs the native alpha-beta (csrc/solve.h) over a batch of positions, on the GPU
(oth_solve_gpu: one lane per search, refilled from a queue) when there is one, else on the
host (oth_solve_cpu over a thread pool; ctypes releases the GIL).  On top of it:

* `relabel_rows` replaces the self-play value target z of late positions by the exact
  win / draw / loss, and
* `move_report` measures the search's preferred move (argmax pi) against the exact result:
  how often it is optimal, how often it keeps the win / draw / loss, how many discs it gives
  away.

`solve_deep` is a second solver beside it (csrc/solve_deep.h): a root window ("wld" = (-1, 1)
gives the exact win / draw / loss for a fraction of the nodes) and ordered moves, up to 20
empties; `relabel_rows(wld=True)` and `move_report` beyond 14 empties go through it.

`solve_moves` gives the exact value of every move of a position in one call
(csrc/solve_moves.hip on the host, composed from the board and solve_deep kernels on the
device): the whole 65-column table ("scores"), its win / draw / loss signs
("wld"), or the set of score-optimal moves for fewer nodes ("optimal").  `exact_policy` turns
a table into a policy target, `relabel_rows(policy=True)` writes it next to the exact z, and
`policy_report` measures how much of a searched pi lies on optimal moves.

score = final own - opp disc difference from the side to move's view (the reference's plain
count, envs/othello.py:214-220), best = the lowest optimal action (64 = pass).
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

import az_native as nat

# fastest on the 1..12-empties corpus workload (scripts/bench_solve.py,
# profiles/solve_bench.json: 11.5 s against 15.2 s unsplit and 14.9 s at two plies; two plies
# win when every root is hard: 3.2 s against 6.4 s on the 12-empties subset alone)
DEFAULT_SPLIT_PLIES = 1
MAX_THREADS = 16


def _popcount(x):
    x = np.ascontiguousarray(x, np.uint64)
    return np.unpackbits(x.view(np.uint8).reshape(-1, 8), axis=1).sum(axis=1).astype(np.int64)


def empties(own, opp):
    """Empty squares per position (numpy uint64 bitboards)."""
    return 64 - _popcount(np.asarray(own).view(np.uint64) | np.asarray(opp).view(np.uint64))


def _solve_cpu(own, opp, max_empties, node_limit):
    n = own.size
    score, best = np.empty(n, np.int8), np.empty(n, np.uint8)
    nodes = np.empty(n, np.uint64)
    if n == 0 or max_empties > nat.AZ_SOLVE_MAX_EMPTIES or max_empties < 0:
        # the library validates the arguments (and accepts n = 0)
        nat.check(nat.lib.oth_solve_cpu(nat.ptr(own), nat.ptr(opp), n, int(max_empties),
                                        int(node_limit), nat.ptr(score), nat.ptr(best),
                                        nat.ptr(nodes)), "oth_solve_cpu")
        return score, best, nodes
    threads = min(MAX_THREADS, n)
    # interleaved chunks much smaller than a thread's share: the cost per position is
    # heavy-tailed, so the hard ones must not all land in one thread's slice
    size = max(1, min(256, n // (threads * 8) or 1))
    bounds = [(a, min(n, a + size)) for a in range(0, n, size)]

    def run(ab):
        a, b = ab
        return nat.lib.oth_solve_cpu(nat.ptr(own[a:b]), nat.ptr(opp[a:b]), b - a,
                                     int(max_empties), int(node_limit), nat.ptr(score[a:b]),
                                     nat.ptr(best[a:b]), nat.ptr(nodes[a:b]))

    if threads == 1:
        rcs = [run(ab) for ab in bounds]
    else:
        with ThreadPoolExecutor(threads) as ex:
            rcs = list(ex.map(run, bounds))
    for rc in rcs:
        nat.check(rc, "oth_solve_cpu")
    return score, best, nodes


def _solve_deep_cpu(own, opp, max_empties, alpha, beta, node_limit):
    """oth_solve_deep_cpu over the same thread pool as _solve_cpu."""
    n = own.size
    score, best = np.empty(n, np.int8), np.empty(n, np.uint8)
    nodes = np.empty(n, np.uint64)
    window = (int(alpha), int(beta), int(node_limit))

    def run(ab):
        a, b = ab
        return nat.lib.oth_solve_deep_cpu(nat.ptr(own[a:b]), nat.ptr(opp[a:b]), b - a,
                                          int(max_empties), *window, nat.ptr(score[a:b]),
                                          nat.ptr(best[a:b]), nat.ptr(nodes[a:b]))

    threads = min(MAX_THREADS, n)
    if threads <= 1 or not 0 <= max_empties <= nat.AZ_SOLVE_DEEP_MAX_EMPTIES \
            or not -65 <= alpha < beta <= 65:
        # one call: the library validates the arguments (and accepts n = 0)
        nat.check(run((0, n)), "oth_solve_deep_cpu")
        return score, best, nodes
    size = max(1, min(256, n // (threads * 8) or 1))  # interleaved, as in _solve_cpu
    with ThreadPoolExecutor(threads) as ex:
        rcs = list(ex.map(run, [(a, min(n, a + size)) for a in range(0, n, size)]))
    for rc in rcs:
        nat.check(rc, "oth_solve_deep_cpu")
    return score, best, nodes


def solve_gpu_tensors(own, opp, max_empties, node_limit, split_plies, stream=None):
    """oth_solve_gpu on int64 device tensors (the uint64 bitboards' bits), asynchronous on
    `stream` (default: the current stream).  Returns device tensors (score int8, best uint8,
    nodes int64 = the uint64 counts' bits)."""
    dev = own.device
    n = own.numel()
    score = torch.empty(n, dtype=torch.int8, device=dev)
    best = torch.empty(n, dtype=torch.uint8, device=dev)
    nodes = torch.empty(n, dtype=torch.int64, device=dev)
    import ctypes

    need = ctypes.c_size_t(0)
    args = (int(max_empties), int(node_limit), int(split_plies))
    nat.check(nat.lib.oth_solve_gpu(None, None, n, *args, None, None, None, None,
                                    ctypes.byref(need), None), "oth_solve_gpu")
    with torch.cuda.device(dev):
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        with torch.cuda.stream(s):
            ws = torch.empty(max(need.value, 8), dtype=torch.uint8, device=dev)
            nat.check(nat.lib.oth_solve_gpu(nat.ptr(own), nat.ptr(opp), n, *args, nat.ptr(score),
                                            nat.ptr(best), nat.ptr(nodes), nat.ptr(ws),
                                            ctypes.byref(need), nat.stream_ptr(s)),
                      "oth_solve_gpu")
    return score, best, nodes


def _pick_device(device, *arrays):
    if device is not None:
        return torch.device(device)
    for a in arrays:
        if isinstance(a, torch.Tensor) and a.is_cuda:
            return a.device
    return torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() \
        else torch.device("cpu")


def _as_i64_tensor(a, dev):
    if isinstance(a, torch.Tensor):
        assert a.dtype == torch.int64, "bitboard tensors are int64 (the uint64's bits)"
        return a.reshape(-1).contiguous().to(dev)
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).reshape(-1).view(np.int64)).to(dev)


def _as_u64_numpy(a):
    if isinstance(a, torch.Tensor):
        return a.detach().cpu().contiguous().numpy().reshape(-1).view(np.uint64)
    return np.ascontiguousarray(a, np.uint64).reshape(-1)


def solve(own, opp, max_empties=12, device=None, node_limit=1 << 31, split_plies=None):
    """Exact solve of every position (own = side to move) with at most `max_empties`
    empties: returns (score int8, best uint8, nodes uint64).  Positions with more empties
    (or overlapping boards) get score AZ_SOLVE_SKIPPED (-128) and best 255; a search beyond
    `node_limit` nodes gets AZ_SOLVE_ABORTED (-127).

    own / opp: numpy uint64 arrays (numpy results) or torch int64 tensors holding the same
    bits (torch results on the tensors' device, nodes as int64 bits).  device None = the GPU
    when one is available, else the host; "cpu" forces the host path (thread pool of at most
    16 threads).  split_plies (GPU only) None = DEFAULT_SPLIT_PLIES."""
    want_torch = isinstance(own, torch.Tensor)
    dev = _pick_device(device, own, opp)
    if dev.type == "cuda":
        sp = DEFAULT_SPLIT_PLIES if split_plies is None else int(split_plies)
        s, b, nd = solve_gpu_tensors(_as_i64_tensor(own, dev), _as_i64_tensor(opp, dev),
                                     max_empties, node_limit, sp)
        if want_torch:
            return s, b, nd
        return s.cpu().numpy(), b.cpu().numpy(), nd.cpu().numpy().view(np.uint64)
    s, b, nd = _solve_cpu(_as_u64_numpy(own), _as_u64_numpy(opp), max_empties, node_limit)
    if want_torch:
        return (torch.from_numpy(s).to(own.device), torch.from_numpy(b).to(own.device),
                torch.from_numpy(nd.view(np.int64)).to(own.device))
    return s, b, nd


# fastest on the 1..12-empties corpus workload with the full window (scripts/bench_solve_deep.py,
# profiles/solve_deep_bench.json: 0.88 s against 0.90 s unsplit and 2.23 s at two plies) and
# level with split 0 in (-1, 1) (0.264 / 0.250 / 0.790 s, inside the repeats' spread).  Two
# plies win when every root is hard (256 roots at 14 / 16 empties in (-1, 1): 0.40 / 3.5 s
# against 0.71 / 4.5 s).
DEFAULT_DEEP_SPLIT_PLIES = 1


def _window(window):
    if window is None:
        return -65, 65
    if isinstance(window, str):
        if window != "wld":
            raise ValueError(f"window={window!r}: None, 'wld' or (alpha, beta)")
        return -1, 1
    alpha, beta = window
    return int(alpha), int(beta)


def solve_deep(own, opp, max_empties=16, window=None, device=None, node_limit=1 << 31,
               split_plies=None):
    """Windowed, move-ordered solve (csrc/solve_deep.h) of every position with at most
    `max_empties` <= 20 empties: returns (score, best, nodes) with `solve`'s array / tensor
    conventions, device choice, host thread pool and skipped / aborted codes.

    window None = the full window: score is exact and best an optimal action (not
    necessarily the lowest).  "wld" = (-1, 1): sign(score) is the exact win / draw / loss,
    score itself only a bound.  (alpha, beta): score is exact inside the window, else a
    bound on the true score on the same side of it (see include/az_othello.h).
    split_plies (GPU only) None = DEFAULT_DEEP_SPLIT_PLIES."""
    alpha, beta = _window(window)
    want_torch = isinstance(own, torch.Tensor)
    dev = _pick_device(device, own, opp)
    if dev.type == "cuda":
        sp = DEFAULT_DEEP_SPLIT_PLIES if split_plies is None else int(split_plies)
        s, b, nd = nat.solve_deep_gpu(_as_i64_tensor(own, dev), _as_i64_tensor(opp, dev),
                                      max_empties, alpha, beta, node_limit, sp)
        if want_torch:
            return s, b, nd
        return s.cpu().numpy(), b.cpu().numpy(), nd.cpu().numpy().view(np.uint64)
    s, b, nd = _solve_deep_cpu(_as_u64_numpy(own), _as_u64_numpy(opp), max_empties, alpha, beta,
                               node_limit)
    if want_torch:
        return (torch.from_numpy(s).to(own.device), torch.from_numpy(b).to(own.device),
                torch.from_numpy(nd.view(np.int64)).to(own.device))
    return s, b, nd


MOVES_MODES = {"scores": nat.AZ_MOVES_SCORES, "wld": nat.AZ_MOVES_WLD,
               "optimal": nat.AZ_MOVES_OPTIMAL}


def _solve_moves_cpu(own, opp, max_empties, mode, node_limit):
    """oth_solve_moves_cpu over the same thread pool as _solve_cpu."""
    n = own.size
    values = np.empty((n, 65), np.int8)
    score, nodes = np.empty(n, np.int8), np.empty(n, np.uint64)

    def run(ab):
        a, b = ab
        return nat.lib.oth_solve_moves_cpu(nat.ptr(own[a:b]), nat.ptr(opp[a:b]), b - a,
                                           int(max_empties), int(mode), int(node_limit),
                                           nat.ptr(values[a:b]), nat.ptr(score[a:b]),
                                           nat.ptr(nodes[a:b]))

    threads = min(MAX_THREADS, n)
    if threads <= 1 or not 0 <= max_empties <= nat.AZ_SOLVE_DEEP_MAX_EMPTIES:
        # one call: the library validates the arguments (and accepts n = 0)
        nat.check(run((0, n)), "oth_solve_moves_cpu")
        return values, score, nodes
    size = max(1, min(256, n // (threads * 8) or 1))  # interleaved, as in _solve_cpu
    with ThreadPoolExecutor(threads) as ex:
        rcs = list(ex.map(run, [(a, min(n, a + size)) for a in range(0, n, size)]))
    for rc in rcs:
        nat.check(rc, "oth_solve_moves_cpu")
    return values, score, nodes


_SQ = {}


def _squares(dev):
    if dev not in _SQ:
        _SQ[dev] = torch.arange(64, dtype=torch.int64, device=dev)
    return _SQ[dev]


def _legal_gpu(o_t, p_t):
    lg = torch.empty_like(o_t)
    nat.check(nat.lib.oth_legal_gpu(nat.ptr(o_t), nat.ptr(p_t), nat.ptr(lg), o_t.numel(),
                                    nat.stream_ptr()), "oth_legal_gpu")
    return lg


def solve_moves_gpu_tensors(own, opp, max_empties, mode, node_limit):
    """oth_solve_moves_cpu's table on int64 device tensors, composed on the current stream from
    the device entry points there are: oth_legal_gpu -> the available actions expanded in
    torch -> oth_step_gpu -> oth_solve_deep_gpu, unsplit, on the children (and on the roots
    first in "optimal" mode, then one children call per distinct root score: the solver takes
    one window per call) -> scatter.  The searches are the host's, so values (int8 [n, 65]),
    score (int8) and nodes (int64 bits) are the host's bit for bit.  The expansion reads sizes
    back to the host, so a call does not capture into a HIP graph."""
    # the library validates max_empties and mode
    nat.check(nat.lib.oth_solve_moves_cpu(None, None, 0, int(max_empties), int(mode),
                                          int(node_limit), None, None, None),
              "oth_solve_moves_cpu")
    dev, n = own.device, own.numel()
    with torch.cuda.device(dev):
        sq = _squares(dev)
        count = lambda x: ((x[:, None] >> sq) & 1).sum(dim=1)
        skip = ((own & opp) != 0) | (64 - count(own | opp) > int(max_empties))
        lg = torch.where(skip, torch.zeros_like(own), _legal_gpu(own, opp))
        passer = ~skip & (lg == 0) & (_legal_gpu(opp, own) != 0)
        par, act = torch.nonzero((lg[:, None] >> sq) & 1, as_tuple=True)
        pp = torch.nonzero(passer, as_tuple=True)[0]
        par, act = torch.cat([par, pp]), torch.cat([act, torch.full_like(pp, 64)])
        k = par.numel()
        co, cp, cl = (torch.empty(k, dtype=torch.int64, device=dev) for _ in range(3))
        st = torch.empty(k, dtype=torch.int16, device=dev)
        ro, rp, act8 = own[par].contiguous(), opp[par].contiguous(), act.to(torch.uint8)
        nat.check(nat.lib.oth_step_gpu(nat.ptr(ro), nat.ptr(rp), nat.ptr(act8),
                                       nat.ptr(co), nat.ptr(cp), nat.ptr(cl), nat.ptr(st), k,
                                       nat.stream_ptr()), "oth_step_gpu")
        has = torch.zeros(n, dtype=torch.bool, device=dev)
        has[par] = True
        # settled roots: skipped (no node), or the game is over (one node, the final difference)
        score = torch.where(skip, torch.full_like(own, nat.AZ_SOLVE_SKIPPED),
                            count(own) - count(opp)).to(torch.int8)
        nodes = (~skip).to(torch.int64)
        aborted = torch.zeros(n, dtype=torch.bool, device=dev)
        deep = lambda o, p, a, b: nat.solve_deep_gpu(o, p, nat.AZ_SOLVE_DEEP_MAX_EMPTIES, a, b,
                                                     node_limit, 0)
        cs = torch.full((k,), nat.AZ_SOLVE_ABORTED, dtype=torch.int8, device=dev)
        cn = torch.zeros(k, dtype=torch.int64, device=dev)
        if mode == nat.AZ_MOVES_OPTIMAL:
            roots = torch.nonzero(has, as_tuple=True)[0]
            rs, _, rn = deep(own[roots].contiguous(), opp[roots].contiguous(), -65, 65)
            score[roots] = rs
            nodes[roots] += rn
            aborted[roots] = rs == nat.AZ_SOLVE_ABORTED
            cw = score[par].to(torch.int64)
            live = ~aborted[par]  # the children of an aborted root are not searched
            for s in torch.unique(cw[live]).tolist():
                g = torch.nonzero(live & (cw == s), as_tuple=True)[0]
                cs[g], _, cn[g] = deep(co[g].contiguous(), cp[g].contiguous(), -s - 1, -s + 1)
            searched = live
        else:
            w = 1 if mode == nat.AZ_MOVES_WLD else 65
            cs, _, cn = deep(co, cp, -w, w)
            searched = torch.ones(k, dtype=torch.bool, device=dev)
        nodes.index_add_(0, par, cn)
        aborted[par[searched & (cs == nat.AZ_SOLVE_ABORTED)]] = True
        values = torch.full((n, 65), nat.AZ_MOVES_NONE, dtype=torch.int8, device=dev)
        values[par, act] = -(torch.sign(cs) if mode == nat.AZ_MOVES_WLD else cs)
        if mode != nat.AZ_MOVES_OPTIMAL:
            score = torch.where(has, values.max(dim=1).values, score)
        values[aborted] = nat.AZ_MOVES_NONE
        score[aborted] = nat.AZ_SOLVE_ABORTED
    return values, score, nodes


def solve_moves(own, opp, max_empties=12, mode="scores", device=None, node_limit=1 << 31):
    """The exact value of every move of every position with at most `max_empties` <= 20
    empties, in one call: returns (values int8 [n, 65], score, nodes) with `solve_deep`'s
    array / tensor conventions, device choice, host thread pool and skipped / aborted codes.
    values[i, a] is AZ_MOVES_NONE (-128) where action a is not available at root i (64 = the
    pass, available only when the side to move has no placement and the opponent has one).

    mode "scores": values = the exact disc difference each move leads to, score = their
    maximum.  "wld": values in {-1, 0, 1}, the win / draw / loss each move leads to.
    "optimal": score = the root's exact score, values == score exactly on the score-optimal
    moves and a bound below it elsewhere (see include/az_othello.h).  A terminal, skipped or
    aborted root has an all-NONE row."""
    if mode not in MOVES_MODES:
        raise ValueError(f"mode={mode!r}: 'scores', 'wld' or 'optimal'")
    m = MOVES_MODES[mode]
    want_torch = isinstance(own, torch.Tensor)
    dev = _pick_device(device, own, opp)
    if dev.type == "cuda":
        v, s, nd = solve_moves_gpu_tensors(_as_i64_tensor(own, dev), _as_i64_tensor(opp, dev),
                                           max_empties, m, node_limit)
        if want_torch:
            return v, s, nd
        return v.cpu().numpy(), s.cpu().numpy(), nd.cpu().numpy().view(np.uint64)
    v, s, nd = _solve_moves_cpu(_as_u64_numpy(own), _as_u64_numpy(opp), max_empties, m,
                                node_limit)
    if want_torch:
        return (torch.from_numpy(v).to(own.device), torch.from_numpy(s).to(own.device),
                torch.from_numpy(nd.view(np.int64)).to(own.device))
    return v, s, nd


def exact_policy(values):
    """Policy target of a `solve_moves` table (numpy or torch, [n, 65]): float32 [n, 65], each
    row uniform over the available actions whose value equals the row's maximum; a row
    without an available action is all zeros."""
    if isinstance(values, torch.Tensor):
        return torch.from_numpy(exact_policy(values.detach().cpu().numpy())).to(values.device)
    v = np.asarray(values).reshape(-1, 65).astype(np.int64)
    top = v.max(axis=1, keepdims=True)
    hit = (v == top) & (v != nat.AZ_MOVES_NONE)
    count = hit.sum(axis=1, keepdims=True)
    return (hit / np.maximum(count, 1)).astype(np.float32)


LINE_FIELDS = ("own", "opp", "pi", "act", "z")


def _line_cpu(own, opp, max_empties, node_limit):
    """optimal_line on the host: per ply one "optimal" table of every root
    (_solve_moves_cpu; a finished root is skipped without a node) and one oth_line_step_cpu."""
    n, stride = own.size, max(1, 2 * int(max_empties))
    wo, wp = own.copy(), opp.copy()
    count, done = np.zeros(n, np.int32), np.zeros(n, np.uint8)
    score = np.full(n, nat.AZ_SOLVE_SKIPPED, np.int8)
    rows = {"own": np.zeros(n * stride, np.uint64), "opp": np.zeros(n * stride, np.uint64),
            "pi": np.zeros((n * stride, 65), np.float32), "act": np.zeros(n * stride, np.uint8),
            "z": np.zeros(n * stride, np.float32)}
    live = np.zeros(1, np.int32)
    for ply in range(stride + 1):
        values, sc, _ = _solve_moves_cpu(wo, wp, max_empties, nat.AZ_MOVES_OPTIMAL, node_limit)
        nat.check(nat.lib.oth_line_step_cpu(
            nat.ptr(wo), nat.ptr(wp), nat.ptr(values), nat.ptr(sc), n, stride, int(ply == 0),
            nat.ptr(count), nat.ptr(done), nat.ptr(score),
            *[nat.ptr(rows[k]) for k in LINE_FIELDS], nat.ptr(live)), "oth_line_step_cpu")
        if live[0] == 0:
            break
    else:
        raise RuntimeError("optimal_line: roots alive after 2 * max_empties plies")
    keep = (np.arange(stride, dtype=np.int32)[None, :] < count[:, None]).reshape(-1)
    out = {k: rows[k][keep] for k in LINE_FIELDS}
    out["off"] = np.concatenate([[0], np.cumsum(count, dtype=np.int64)]).astype(np.int64)
    out["score"] = score
    return out


def _line_gpu(own, opp, max_empties, node_limit):
    """optimal_line on the device: per ply solve_moves_gpu_tensors over every root and one
    oth_line_step_gpu (one lane per root).  The step adds one host read per ply, the number of
    roots still alive, to those solve_moves_gpu_tensors makes itself (the sizes of its
    expansion, one solver call per distinct root score); the final compaction of the rows
    synchronises once more, after the loop."""
    dev, n, stride = own.device, own.numel(), max(1, 2 * int(max_empties))
    with torch.cuda.device(dev):
        wo, wp = own.clone(), opp.clone()
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        count, done = z(n, torch.int32), z(n, torch.uint8)
        score = torch.full((n,), nat.AZ_SOLVE_SKIPPED, dtype=torch.int8, device=dev)
        rows = {"own": z(n * stride, torch.int64), "opp": z(n * stride, torch.int64),
                "pi": z((n * stride, 65), torch.float32), "act": z(n * stride, torch.uint8),
                "z": z(n * stride, torch.float32)}
        live = z(1, torch.int32)
        for ply in range(stride + 1):
            values, sc, _ = solve_moves_gpu_tensors(wo, wp, max_empties, nat.AZ_MOVES_OPTIMAL,
                                                    node_limit)
            nat.check(nat.lib.oth_line_step_gpu(
                nat.ptr(wo), nat.ptr(wp), nat.ptr(values.contiguous()), nat.ptr(sc.contiguous()),
                n, stride, int(ply == 0), nat.ptr(count), nat.ptr(done), nat.ptr(score),
                *[nat.ptr(rows[k]) for k in LINE_FIELDS], nat.ptr(live), nat.stream_ptr()),
                "oth_line_step_gpu")
            if int(live.item()) == 0:
                break
        else:
            raise RuntimeError("optimal_line: roots alive after 2 * max_empties plies")
        keep = (torch.arange(stride, dtype=torch.int32, device=dev)[None, :]
                < count[:, None]).reshape(-1)
        out = {k: rows[k][keep] for k in LINE_FIELDS}
        out["off"] = torch.cat([z(1, torch.int64), torch.cumsum(count.to(torch.int64), 0)])
        out["score"] = score
    return out


def optimal_line(own, opp, max_empties=12, device=None, node_limit=1 << 31):
    """Every root (own = side to move, 0..max_empties <= 14 empties) played to the end of the
    game along score-optimal moves: one row per ply, all roots' rows flattened in root order.
    Returns a dict of
      own, opp   the ply's position from its side to move,
      pi         float32 [rows, 65] = exact_policy of the ply's solve_moves(mode="optimal")
                 table: uniform over the score-optimal actions, one-hot on 64 where the side to
                 move must pass and the opponent can place,
      act        uint8, the move played = the lowest optimal action (the solvers' `best`),
      z          float32 = sign(the exact score from the ply's side to move),
      off        int64 [n + 1]: root i's rows are off[i] .. off[i + 1] - 1,
      score      int8 [n], the root's exact disc difference.
    A terminal root has no rows (score = its final difference).  A root with more empties or
    overlapping boards has none and score AZ_SOLVE_SKIPPED; one whose search (at any ply) passes
    `node_limit` has none and score AZ_SOLVE_ABORTED, as in `solve_moves`.  max_empties outside
    0..14 is a ValueError.

    Arrays, tensors and the device choice follow `solve`.  On the device every ply is the
    existing solve_moves kernels over the roots and one oth_line_step_gpu; the host path runs
    the same step (oth_line_step_cpu) over the host's tables, so both give the same arrays bit
    for bit."""
    if not 0 <= int(max_empties) <= nat.AZ_SOLVE_MAX_EMPTIES:
        raise ValueError(f"max_empties={max_empties}: 0..{nat.AZ_SOLVE_MAX_EMPTIES}")
    want_torch = isinstance(own, torch.Tensor)
    dev = _pick_device(device, own, opp)
    if dev.type == "cuda":
        out = _line_gpu(_as_i64_tensor(own, dev), _as_i64_tensor(opp, dev), int(max_empties),
                        node_limit)
        if want_torch:
            return out
        out = {k: v.cpu().numpy() for k, v in out.items()}
        out["own"], out["opp"] = out["own"].view(np.uint64), out["opp"].view(np.uint64)
        return out
    out = _line_cpu(_as_u64_numpy(own), _as_u64_numpy(opp), int(max_empties), node_limit)
    if want_torch:
        out["own"], out["opp"] = out["own"].view(np.int64), out["opp"].view(np.int64)
        return {k: torch.from_numpy(np.ascontiguousarray(v)).to(own.device)
                for k, v in out.items()}
    return out


def _check_solved(score, what):
    if (score == nat.AZ_SOLVE_ABORTED).any():
        raise RuntimeError(f"{what}: {int((score == nat.AZ_SOLVE_ABORTED).sum())} searches "
                           "exceeded the node limit")


def relabel_rows(rows, max_empties, device=None, wld=False, policy=False):
    """Exact value targets: in engine sample rows (dict of own / opp / pi / z / player, z
    already from the side to move's view: canonical rows) replace z by float(sign(score)) for
    every row whose position has 1..max_empties empties; other rows and fields are untouched.
    Returns (rows, mask) with mask the boolean array of relabelled rows; `rows` is a new
    dict sharing every array but z.  wld=True takes the sign from solve_deep's (-1, 1)
    window instead of the exact disc count: the same labels for fewer nodes, and max_empties
    up to 20.

    policy=True: one `solve_moves` call gives both targets of the masked rows; max_empties up
    to 20 in both settings.  z is what policy=False gives; pi becomes a new array of the
    input's shape and dtype whose masked rows hold `exact_policy`: uniform over the
    score-optimal moves (mode "optimal"), or with wld=True over every move that keeps the best
    reachable win / draw / loss (mode "wld").  A masked row without an available action (the
    game is over) keeps its pi."""
    own, opp = _as_u64_numpy(rows["own"]), _as_u64_numpy(rows["opp"])
    e = empties(own, opp)
    mask = (e >= 1) & (e <= int(max_empties)) & ((own & opp) == 0)
    out = dict(rows)
    z = np.array(np.asarray(rows["z"]), dtype=np.float64, copy=True)
    if policy:
        src = np.asarray(rows["pi"])
        pi = np.array(src, copy=True)
        if mask.any():
            values, score, _ = solve_moves(own[mask], opp[mask], max_empties,
                                           mode="wld" if wld else "optimal", device=device)
            _check_solved(score, "relabel_rows")
            z[mask] = np.sign(score.astype(np.int64)).astype(np.float64)
            has = (values != nat.AZ_MOVES_NONE).any(axis=1)
            flat = pi.reshape(-1, 65)
            flat[np.flatnonzero(mask)[has]] = exact_policy(values[has]).astype(src.dtype)
        out["z"], out["pi"] = z, pi
        return out, mask
    if mask.any():
        if wld:
            score, _, _ = solve_deep(own[mask], opp[mask], max_empties, window="wld",
                                     device=device)
        else:
            score, _, _ = solve(own[mask], opp[mask], max_empties, device=device)
        _check_solved(score, "relabel_rows")
        z[mask] = np.sign(score.astype(np.int64)).astype(np.float64)
    out["z"] = z
    return out, mask


def _stats(score, value):
    n = len(score)
    if n == 0:
        return {"n": 0, "optimal_frac": None, "wld_kept_frac": None, "mean_disc_loss": None}
    return {"n": int(n), "optimal_frac": float((value == score).mean()),
            "wld_kept_frac": float((np.sign(value) == np.sign(score)).mean()),
            "mean_disc_loss": float((score - value).mean())}


def move_report(rows, max_empties, device=None):
    """How good is the search's preferred move a = argmax(pi) in every row with
    1..max_empties empties?  The value of a is minus the exact score of the position after it
    (made with the batched board step; after a placement or a pass the other side is to
    move), compared with the position's own exact score; roots and children are solved in
    one batch.  Returns {"by_empties": {e: stats}, "total": stats} with stats = n,
    optimal_frac (value of a == score), wld_kept_frac (same sign) and mean_disc_loss
    (score - value of a, in discs).  max_empties up to 14 is solved by `solve`, 15..20 by
    `solve_deep` with the full window."""
    own, opp = _as_u64_numpy(rows["own"]), _as_u64_numpy(rows["opp"])
    e = empties(own, opp)
    mask = (e >= 1) & (e <= int(max_empties)) & ((own & opp) == 0)
    own, opp, e = own[mask], opp[mask], e[mask]
    pi = np.asarray(rows["pi"], np.float32).reshape(-1, 65)[mask]
    act = pi.argmax(axis=1).astype(np.uint8)
    cown, copp, _, _ = nat.step_cpu(own, opp, act)
    n = len(own)
    deep = int(max_empties) > nat.AZ_SOLVE_MAX_EMPTIES  # 15..20: solve_deep, full window
    score, _, _ = (solve_deep if deep else solve)(
        np.concatenate([own, cown]), np.concatenate([opp, copp]), max_empties, device=device)
    _check_solved(score, "move_report")
    score = score.astype(np.int64)
    root, value = score[:n], -score[n:]
    by = {int(k): _stats(root[e == k], value[e == k]) for k in range(1, int(max_empties) + 1)}
    return {"by_empties": by, "total": _stats(root, value)}


def _mass(opt, wld):
    if len(opt) == 0:
        return {"n": 0, "optimal_mass": None, "wld_kept_mass": None}
    return {"n": int(len(opt)), "optimal_mass": float(opt.mean()),
            "wld_kept_mass": float(wld.mean())}


def policy_report(rows, max_empties, device=None):
    """How much of each row's pi lies on good moves, for every row with 1..max_empties empties
    and at least one available action (pi as given, not renormalised)?  Every move's exact
    value comes from one `solve_moves` call in "scores" mode.  Returns {"by_empties": {e:
    stats}, "total": stats} with stats = n, optimal_mass (mean mass of pi on the
    score-optimal moves) and wld_kept_mass (mean mass on the moves whose win / draw / loss is
    the position's own)."""
    own, opp = _as_u64_numpy(rows["own"]), _as_u64_numpy(rows["opp"])
    e = empties(own, opp)
    mask = (e >= 1) & (e <= int(max_empties)) & ((own & opp) == 0)
    own, opp, e = own[mask], opp[mask], e[mask]
    pi = np.asarray(rows["pi"], np.float64).reshape(-1, 65)[mask]
    values, score, _ = solve_moves(own, opp, max_empties, mode="scores", device=device)
    _check_solved(score, "policy_report")
    v, s = values.astype(np.int64), score.astype(np.int64)[:, None]
    avail = v != nat.AZ_MOVES_NONE
    has = avail.any(axis=1)
    opt = (pi * (avail & (v == s))).sum(axis=1)[has]
    wld = (pi * (avail & (np.sign(v) == np.sign(s)))).sum(axis=1)[has]
    e = e[has]
    by = {int(k): _mass(opt[e == k], wld[e == k]) for k in range(1, int(max_empties) + 1)}
    return {"by_empties": by, "total": _mass(opt, wld)}
