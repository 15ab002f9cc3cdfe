"""Endgame solver throughput: oth_solve_gpu at split_plies 0 / 1 / 2 against oth_solve_cpu on
16 host threads, on the same positions.

    python scripts/bench_solve.py [--repeats 5] [--cpu-repeats 2] [--out profiles/solve_bench.json]

Workload: every position of tests/golden/board_corpus.npz with 1..12 empties under the four
rotations (oth_d4_cpu), about 30,000 positions, solved with max_empties = 12; and its
12-empties subset alone.  Each configuration is warmed up once, then timed `repeats` times
(wall clock around a synchronised call, device buffers resident); the JSON keeps every
repeat and reports the median.  No pass / fail number: the result picks
endgame.DEFAULT_SPLIT_PLIES and goes into DESIGN.md."""
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

LIMIT = 1 << 31


def workload():
    d = np.load(os.path.join(ROOT, "tests", "golden", "board_corpus.npz"))
    own = np.where(d["player"] == 1, d["pos"], d["neg"]).astype(np.uint64)
    opp = np.where(d["player"] == 1, d["neg"], d["pos"]).astype(np.uint64)
    emp = endgame.empties(own, opp)
    m = (emp >= 1) & (emp <= 12)
    own, opp = own[m], opp[m]
    own = np.concatenate([nat.d4_cpu(own, k) for k in range(4)])
    opp = np.concatenate([nat.d4_cpu(opp, k) for k in range(4)])
    return own, opp, endgame.empties(own, opp)


def timed(fn, repeats, budget_s=30.0):
    """Warm up once, then time up to `repeats` calls (at least two; a slow configuration stops
    once its repeats have used budget_s)."""
    fn()
    out = []
    for _ in range(repeats):
        t = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t)
        if len(out) >= 2 and sum(out) > budget_s:
            break
    return out


def summary(times, n, nodes):
    med = statistics.median(times)
    return {"seconds": times, "median_s": med, "min_s": min(times),
            "positions_per_s": n / med, "nodes_per_s": nodes / med}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cpu-repeats", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "solve_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_solve.py needs the GPU"
    own, opp, emp = workload()
    sets = {"all_1_to_12": np.ones(len(own), bool), "empties_12": emp == 12}
    res = {"device": torch.cuda.get_device_name(0), "build_id": nat.build_id(),
           "max_empties": 12, "split_min": 9, "host_threads": endgame.MAX_THREADS,
           "repeats": a.repeats, "cpu_repeats": a.cpu_repeats, "sets": {}}
    for name, m in sets.items():
        o, p = own[m], opp[m]
        n = len(o)
        cs, cb, cn = endgame.solve(o, p, 12, device="cpu", node_limit=LIMIT)
        entry = {"positions": n, "nodes_total": int(cn.sum()), "nodes_mean": float(cn.mean()),
                 "nodes_max": int(cn.max()), "max_over_mean": float(cn.max() / cn.mean())}
        entry["cpu_16_threads"] = summary(
            timed(lambda: endgame.solve(o, p, 12, device="cpu", node_limit=LIMIT), a.cpu_repeats),
            n, int(cn.sum()))
        o_t = torch.from_numpy(o.view(np.int64)).cuda()
        p_t = torch.from_numpy(p.view(np.int64)).cuda()
        for split in (0, 1, 2):
            def run():
                r = endgame.solve_gpu_tensors(o_t, p_t, 12, LIMIT, split)
                torch.cuda.synchronize()
                return r

            s, b, nd = run()
            s, b = s.cpu().numpy(), b.cpu().numpy()
            nodes = int(nd.cpu().numpy().view(np.uint64).sum())
            assert (s == cs).all() and (b == cb).all(), f"split {split} disagrees with the host"
            entry[f"gpu_split_{split}"] = dict(summary(timed(run, a.repeats), n, nodes),
                                               nodes_total=nodes)
            print(name, "split", split, entry[f"gpu_split_{split}"]["median_s"], flush=True)
        print(name, "cpu", entry["cpu_16_threads"]["median_s"], flush=True)
        res["sets"][name] = entry
    best = min((0, 1, 2), key=lambda k: res["sets"]["all_1_to_12"][f"gpu_split_{k}"]["median_s"])
    res["fastest_split_plies"] = best
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: {c: v[c]["median_s"] for c in v if isinstance(v[c], dict)}
                      for k, v in res["sets"].items()}))


if __name__ == "__main__":
    main()
