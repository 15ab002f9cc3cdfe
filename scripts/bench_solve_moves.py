"""Per-move endgame values: endgame.solve_moves on the device against 16 host threads, in one
run on one machine.

    python scripts/bench_solve_moves.py [--repeats 5] [--cpu-repeats 2]
                                        [--out profiles/solve_moves_bench.json]

Roots: positions of tests/golden/board_corpus.npz (a fixed stride) at 4, 8 and 10 empties (up
to 1,024 each) and at 12 and 14 empties (64 each), in the three modes.  Per set and mode:

  device    endgame.solve_moves_gpu_tensors on resident device tensors: oth_legal_gpu ->
            expansion in torch (nonzero, a host round trip) -> oth_step_gpu ->
            oth_solve_deep_gpu(split_plies=0) on the children -> scatter; "optimal" solves the
            roots first and then makes one children call per distinct root score, since the
            solver takes one window per call;
  host      endgame.solve_moves(device="cpu"): oth_solve_moves_cpu on 16 host threads.

Device configurations are timed with device events around the whole call (host gaps between
its launches included), warmed up once, then `repeats` times; the JSON keeps every repeat and
reports the median.  Every table is checked against the host's.  The figures go into
DESIGN.md."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "alphazero-othello_amd")]

import torch  # noqa: E402

import az_native as nat  # noqa: E402
import endgame  # noqa: E402

LIMIT = 1 << 40
MODES = ("scores", "wld", "optimal")


def event_timed(fn, repeats):
    """(warm-up ms, [ms per timed call], the last result): device events on the current
    stream around the call."""
    out, r = [], None
    for i in range(repeats + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out[0], out[1:], r


def wall_timed(fn, repeats):
    out, r = [], None
    for _ in range(repeats + 1):
        t = time.perf_counter()
        r = fn()
        out.append((time.perf_counter() - t) * 1e3)
    return out[0], out[1:], r


def summary(t, n, nodes):
    warm, times = t[:2]
    med = statistics.median(times)
    return {"warmup_ms": warm, "ms": times, "median_ms": med, "min_ms": min(times),
            "roots_per_s": n / med * 1e3, "nodes_total": int(nodes)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cpu-repeats", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "solve_moves_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_solve_moves.py needs the GPU"
    assert a.repeats >= 5, "the median of at least 5 calls"
    t_start = time.perf_counter()
    res = {"device": torch.cuda.get_device_name(0), "build_id": nat.build_id(),
           "host_threads": endgame.MAX_THREADS, "repeats": a.repeats,
           "cpu_repeats": a.cpu_repeats, "timing": "device events, ms", "sets": {}}

    def save():
        res["wall_s"] = time.perf_counter() - t_start
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    d = np.load(os.path.join(ROOT, "tests", "golden", "board_corpus.npz"))
    cown = np.where(d["player"] == 1, d["pos"], d["neg"]).astype(np.uint64)
    copp = np.where(d["player"] == 1, d["neg"], d["pos"]).astype(np.uint64)
    cemp = endgame.empties(cown, copp)
    for e, cap in ((4, 1024), (8, 1024), (10, 1024), (12, 64), (14, 64)):
        idx = np.flatnonzero(cemp == e)
        idx = idx[::max(1, len(idx) // cap)][:cap]
        o, p = cown[idx], copp[idx]
        n = len(o)
        o_t = torch.from_numpy(o.view(np.int64)).cuda()
        p_t = torch.from_numpy(p.view(np.int64)).cuda()
        entry = res["sets"][f"empties_{e}"] = {"roots": n, "max_empties": e}
        for mode in MODES:
            t_host = wall_timed(lambda: endgame.solve_moves(o, p, e, mode=mode, device="cpu",
                                                            node_limit=LIMIT), a.cpu_repeats)
            hv, hs, hn = t_host[2]
            m = endgame.MOVES_MODES[mode]
            t_dev = event_timed(lambda: endgame.solve_moves_gpu_tensors(o_t, p_t, e, m, LIMIT),
                                a.repeats)
            v, s, nd = (x.cpu().numpy() for x in t_dev[2])
            assert (v == hv).all() and (s == hs).all(), f"{e} {mode}: table differs"
            assert (nd.view(np.uint64) == hn).all(), f"{e} {mode}: nodes differ"
            r = {"host_16_threads": summary(t_host, n, hn.sum()),
                 "device": summary(t_dev, n, hn.sum()),
                 "nodes_hardest_root": int(hn.max())}
            r["host_over_device"] = r["host_16_threads"]["median_ms"] / r["device"]["median_ms"]
            entry[mode] = r
            print(f"{e} empties {mode}: device {r['device']['median_ms']:.2f} ms, host "
                  f"{r['host_16_threads']['median_ms']:.2f} ms (x{r['host_over_device']:.2f}), "
                  f"{int(hn.sum())} nodes", flush=True)
            save()


if __name__ == "__main__":
    main()
