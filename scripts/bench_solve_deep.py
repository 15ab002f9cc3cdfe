"""Windowed, move-ordered endgame solver (oth_solve_deep_*) against the exact solver it stands
beside (oth_solve_*), in one run on one machine.

    python scripts/bench_solve_deep.py [--repeats 5] [--cpu-repeats 2]
                                       [--out profiles/solve_deep_bench.json]

Part 1, scripts/bench_solve.py's own workload (every position of
tests/golden/board_corpus.npz with 1..12 empties under the four rotations, and its 12-empties
subset): oth_solve_gpu, oth_solve_deep_gpu with the full window and with (-1, 1), each at
split_plies 0 / 1 / 2, and 16 host threads of each.  Part 2, beyond the old solver's reach:
256 corpus positions (a fixed stride) at 14 / 16 / 18 / 20 empties in win / draw / loss mode
and at 14 / 16 with the full window, on 16 host threads and on the device at two split plies
(and at one where a run takes seconds): seconds, positions/s, total and hardest-root nodes.

Each configuration is warmed up once, then timed up to `repeats` times (wall clock around a
synchronised call, device buffers resident; a slow configuration stops once its repeats have
used 30 s, and one whose warm-up alone took more than 30 s is timed once more only); the JSON
keeps every repeat and reports the median.  The whole run takes about a quarter of an hour.
Scores are checked against the host's in every configuration.  The result picks
endgame.DEFAULT_DEEP_SPLIT_PLIES and goes into DESIGN.md."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "alphazero-othello_amd"), os.path.join(ROOT, "scripts")]

import torch  # noqa: E402

import az_native as nat  # noqa: E402
import endgame  # noqa: E402
from bench_solve import workload  # noqa: E402

LIMIT = 1 << 40
FULL, WLD = (-65, 65), (-1, 1)


def timed(fn, repeats, budget_s=30.0):
    """(warm-up seconds, timed seconds, the last call's result)."""
    t = time.perf_counter()
    r = fn()
    warm = time.perf_counter() - t
    out = []
    for _ in range(1 if warm > 30.0 else repeats):
        if warm > 30.0:
            print(f"  warm-up {warm:.0f} s, one timed run follows", flush=True)
        t = time.perf_counter()
        r = fn()
        out.append(time.perf_counter() - t)
        if len(out) >= 2 and sum(out) > budget_s:
            break
    return warm, out, r


def summary(warm_times, n, nodes, hardest=None):
    warm, times = warm_times[:2]
    med = statistics.median(times)
    d = {"warmup_s": warm, "seconds": times, "median_s": med, "min_s": min(times),
         "positions_per_s": n / med, "nodes_total": int(nodes), "nodes_per_s": nodes / med}
    if hardest is not None:
        d["nodes_hardest_root"] = int(hardest)
    return d


def gpu_config(kind, o_t, p_t, max_empties, window, split, check, repeats):
    """One device configuration: kind 'solve' (the exact solver) or 'deep'."""
    def run():
        if kind == "solve":
            r = endgame.solve_gpu_tensors(o_t, p_t, max_empties, LIMIT, split)
        else:
            r = nat.solve_deep_gpu(o_t, p_t, max_empties, *window, LIMIT, split)
        torch.cuda.synchronize()
        return r

    t = timed(run, repeats)
    s, b, nd = t[2]
    nd = nd.cpu().numpy().view(np.uint64)
    check(s.cpu().numpy().astype(np.int64))
    return summary(t, o_t.numel(), int(nd.sum()), int(nd.max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cpu-repeats", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "solve_deep_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_solve_deep.py needs the GPU"
    t_start = time.perf_counter()
    res = {"device": torch.cuda.get_device_name(0), "build_id": nat.build_id(),
           "split_min": 9, "host_threads": endgame.MAX_THREADS, "repeats": a.repeats,
           "cpu_repeats": a.cpu_repeats, "sets": {}, "deep_sets": {}}

    def save():
        res["wall_s"] = time.perf_counter() - t_start
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    def dev(x):
        return torch.from_numpy(x.view(np.int64)).cuda()

    # ---- part 1: bench_solve.py's workload ----------------------------------------------
    own, opp, emp = workload()
    for name, m in {"all_1_to_12": np.ones(len(own), bool), "empties_12": emp == 12}.items():
        o, p = own[m], opp[m]
        n = len(o)
        o_t, p_t = dev(o), dev(p)
        cs, _, cn = endgame.solve(o, p, 12, device="cpu", node_limit=LIMIT)
        cs = cs.astype(np.int64)

        def same(s):
            assert (s == cs).all(), "scores disagree with the host's exact solver"

        def same_sign(s):
            assert (np.sign(s) == np.sign(cs)).all(), "win / draw / loss disagrees"

        entry = {"positions": n}
        host = {"solve": lambda: endgame.solve(o, p, 12, device="cpu", node_limit=LIMIT),
                "deep_full": lambda: endgame.solve_deep(o, p, 12, device="cpu", node_limit=LIMIT),
                "deep_wld": lambda: endgame.solve_deep(o, p, 12, window="wld", device="cpu",
                                                       node_limit=LIMIT)}
        for key, fn in host.items():
            nd = fn()[2]
            entry[f"{key}_cpu_16_threads"] = summary(timed(fn, a.cpu_repeats), n, int(nd.sum()),
                                                     int(nd.max()))
        for key, kind, window, check in (("solve", "solve", None, same),
                                         ("deep_full", "deep", FULL, same),
                                         ("deep_wld", "deep", WLD, same_sign)):
            for split in (0, 1, 2):
                e = gpu_config(kind, o_t, p_t, 12, window, split, check, a.repeats)
                entry[f"{key}_gpu_split_{split}"] = e
                print(name, key, "split", split, round(e["median_s"], 4), flush=True)
            entry[f"{key}_gpu_best_split"] = min(
                (0, 1, 2), key=lambda k: entry[f"{key}_gpu_split_{k}"]["median_s"])
        old = entry[f"solve_gpu_split_{entry['solve_gpu_best_split']}"]["median_s"]
        for key in ("deep_full", "deep_wld"):
            new = entry[f"{key}_gpu_split_{entry[key + '_gpu_best_split']}"]["median_s"]
            entry[f"solve_over_{key}_best_median"] = old / new
        res["sets"][name] = entry
        save()

    # ---- part 2: beyond the old reach, cheap to dear -------------------------------------
    d = np.load(os.path.join(ROOT, "tests", "golden", "board_corpus.npz"))
    cown = np.where(d["player"] == 1, d["pos"], d["neg"]).astype(np.uint64)
    copp = np.where(d["player"] == 1, d["neg"], d["pos"]).astype(np.uint64)
    cemp = endgame.empties(cown, copp)
    # both split depths where a run takes seconds, two plies alone where it takes minutes
    plan = [(14, "wld", (2, 1)), (16, "wld", (2, 1)), (14, "full", (2, 1)), (18, "wld", (2,)),
            (16, "full", (2,)), (20, "wld", (2,))]
    for e, mode, splits in plan:
        name = f"empties_{e}_{mode}"
        idx = np.flatnonzero(cemp == e)
        idx = idx[::len(idx) // 256][:256]
        o, p = cown[idx], copp[idx]
        window = WLD if mode == "wld" else FULL

        def host():
            return endgame.solve_deep(o, p, e, window=window, device="cpu", node_limit=LIMIT)

        t_host = timed(host, a.cpu_repeats)
        hs, _, hn = t_host[2]
        hs = hs.astype(np.int64)

        def agree(s):
            ok = (np.sign(s) == np.sign(hs)) if mode == "wld" else (s == hs)
            assert ok.all(), f"{name}: disagrees with the host"

        entry = {"positions": len(o), "max_empties": e, "window": list(window),
                 "cpu_16_threads": summary(t_host, len(o), int(hn.sum()),
                                           int(hn.max()))}
        host_s = entry["cpu_16_threads"]["median_s"]
        o_t, p_t = dev(o), dev(p)
        for split in splits:
            g = gpu_config("deep", o_t, p_t, e, window, split, agree, a.repeats)
            entry[f"gpu_split_{split}"] = g
            print(name, "split", split, round(g["median_s"], 3), "host", round(host_s, 3),
                  flush=True)
        res["deep_sets"][name] = entry
        save()
    res["fastest_deep_split_plies"] = {
        k: res["sets"]["all_1_to_12"][f"{k}_gpu_best_split"] for k in ("deep_full", "deep_wld")}
    save()
    print(json.dumps({"sets": {k: {c: round(v[c]["median_s"], 4) for c in v
                                    if isinstance(v[c], dict)} for k, v in res["sets"].items()},
                      "deep_sets": {k: {c: round(v[c]["median_s"], 3) for c in v
                                         if isinstance(v[c], dict)}
                                    for k, v in res["deep_sets"].items()}}))


if __name__ == "__main__":
    main()
