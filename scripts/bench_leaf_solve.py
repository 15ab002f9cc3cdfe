"""Cost and effect of exact leaf values (args["leaf_solve_empties"], csrc/leaf_solve.hip) on an
MI355X; writes profiles/leaf_solve_bench.json ("Exact leaf values").

    python scripts/bench_leaf_solve.py [--out profiles/leaf_solve_bench.json] [--quick]

  step_rate  PipelinedSelfPlay at bench.py's configs[2] shape (2 pipelines x 1,024 games, 400
             sims, AlphaZeroNet(5x128), staggered starts, warmed as bench.py warms), E = 0, 4,
             6, 8 one after another in this process: ms per step and games/s of three windows.
  kernel     the leaf-solve call alone on nn_in dumps taken from the E = 0 run after its
             warm-up (1,024 rows each, 32 dumps 97 steps apart): tasks and nodes per call,
             median and maximum time, E = 4, 6, 8; and the share of tasks left at node limits
             32 .. 1,024 for E = 6, from which the default limit is derived.
  play       2,048 self-play games at 100 simulations, a seeded random-init FastOthelloNet, E = 0
             and E = 6 with the same seed: endgame.move_report(rows, 10) of both.

Times are host clocks around work that ends in a device synchronise (windows) or device events
(single calls).  --quick shrinks every part (a rehearsal of the script, not a measurement).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (puts the package on sys.path; configs[2]'s net and args)

import az_native as nat  # noqa: E402
import endgame  # noqa: E402
from engine import LEAF_SOLVE_NODES, BatchedSelfPlay, PipelinedSelfPlay  # noqa: E402

E_LIST = (0, 4, 6, 8)


def empties_histogram(x):
    """Rows per number of empties (64 = no leaf) of planes [n, 64]."""
    e = 64 - (x.abs() > 0.5).sum(dim=1)
    h = torch.bincount(e.flatten(), minlength=65).cpu().numpy()
    return {int(k): int(v) for k, v in enumerate(h) if v}


def step_rate(quick, dumps):
    games, sims, pipelines = (128, 16, 2) if quick else (2048, 400, 2)
    steps, windows = (64, 2) if quick else (2000, 3)
    out = {"shape": {"games": games, "pipelines": pipelines, "sims": sims,
                     "net": "fast" if quick else "az5x128", "steps_per_window": steps}, "runs": []}
    net = bench.make_net("fast" if quick else "az5x128")
    stagger = (sims + 1) * int(bench.REF_PLIES_PER_GAME)
    for E in E_LIST:
        args = dict(bench.SELFPLAY_ARGS, num_simulations=sims, leaf_solve_empties=E)
        sp = PipelinedSelfPlay(net, args, games, pipelines=pipelines, seed=1234, use_graph=True,
                               require_graph=True,
                               sample_capacity=games // pipelines * 130 * 4)
        sp.reset(start_budget=-1, stagger_steps=stagger)
        sp.step(stagger)  # bench.py's warm-up: every slot playing, uniform game phases
        torch.cuda.synchronize()
        run = {"E": E, "node_limit": LEAF_SOLVE_NODES, "warmup_steps": stagger, "windows": []}
        for _ in range(windows):
            c0 = sp.counters()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sp.step(steps)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            c1 = sp.counters()
            plies = c1["samples"] / max(1, c1["games_finished"])
            rate = (c1["simulations"] - c0["simulations"]) / (sims * plies) / dt
            run["windows"].append({"ms_per_step": round(dt * 1000.0 / steps, 4),
                                   "games_per_s": round(rate, 3)})
        run["ms_per_step_median"] = float(np.median([w["ms_per_step"] for w in run["windows"]]))
        run["games_per_s_median"] = float(np.median([w["games_per_s"] for w in run["windows"]]))
        if E:
            st = [p.engine.leaf_solve_stats() for p in sp.parts]
            calls = sum(p.engine.counters()["steps"] for p in sp.parts)
            run["leaf_stats"] = {k: sum(s[k] for s in st) for k in st[0]}
            run["tasks_per_call"] = round((run["leaf_stats"]["solved"]
                                           + run["leaf_stats"]["limited"]) / max(1, calls), 3)
        else:  # the kernel's inputs: one pipeline's planes as the steps leave them
            e = sp.parts[0]
            for _ in range(4 if quick else 32):
                e.step(97)
                torch.cuda.synchronize()
                dumps.append(e.engine.nn_in.clone())
        out["runs"].append(run)
        print(json.dumps(run), flush=True)
        del sp
    base = out["runs"][0]["ms_per_step_median"]
    for run in out["runs"]:
        run["ms_per_step_over_E0"] = round(run["ms_per_step_median"] - base, 4)
    return out


def time_calls(dumps, values, E, limit, ws, reps):
    """Device-event time of every call (ms), and the counters the calls added."""
    s0 = nat.leaf_solve_stats_gpu(ws)
    ms = []
    for _ in range(reps):
        for x in dumps:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            nat.leaf_solve_gpu(x, values, E, limit, ws)
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
    s1 = nat.leaf_solve_stats_gpu(ws)
    return np.array(ms), {k: s1[k] - s0[k] for k in s1}


def kernel_alone(dumps, quick):
    R = dumps[0].shape[0]
    values = torch.zeros(R, dtype=torch.float32, device=dumps[0].device)
    ws = nat.leaf_solve_workspace(R, values.device)
    hist = empties_histogram(torch.cat(dumps))
    out = {"rows": R, "dumps": len(dumps),
           "source": "nn_in of one 1,024-game pipeline of the E = 0 configs[2] run, after its "
                     "warm-up, 97 steps apart",
           "rows_by_empties": hist, "node_limit": LEAF_SOLVE_NODES, "by_E": [], "limits_E6": []}
    reps = 2 if quick else 8
    for E in (4, 6, 8):
        time_calls(dumps, values, E, LEAF_SOLVE_NODES, ws, 1)  # warm
        ms, st = time_calls(dumps, values, E, LEAF_SOLVE_NODES, ws, reps)
        calls = len(ms)
        out["by_E"].append({"E": E, "calls": calls,
                            "tasks_per_call": round((st["solved"] + st["limited"]) / calls, 2),
                            "nodes_per_call": round(st["nodes"] / calls, 1),
                            "limited_frac": round(st["limited"] / max(1, st["solved"] + st["limited"]), 5),
                            "ms_median": round(float(np.median(ms)), 4),
                            "ms_p99": round(float(np.percentile(ms, 99)), 4),
                            "ms_max": round(float(ms.max()), 4)})
    # an empty call (no row qualifies): the floor of the three launches
    zero = [torch.zeros_like(dumps[0])]
    ms, _ = time_calls(zero * 32, values, 6, LEAF_SOLVE_NODES, ws, reps)
    out["ms_median_no_tasks"] = round(float(np.median(ms)), 4)
    for limit in (32, 64, 128, 256, 512, 1024):
        _, st = time_calls(dumps, values, 6, limit, ws, 1)
        tasks = st["solved"] + st["limited"]
        out["limits_E6"].append({"node_limit": limit, "tasks": tasks, "limited": st["limited"],
                                 "limited_frac": round(st["limited"] / max(1, tasks), 5)})
    under = [r["node_limit"] for r in out["limits_E6"] if r["limited_frac"] < 0.01]
    out["smallest_limit_under_1pct_E6"] = min(under) if under else None
    return out


def effect_on_play(quick):
    games, sims = (64, 16) if quick else (2048, 100)
    out = {"games": games, "sims": sims, "net": "FastOthelloNet, torch.manual_seed(0)",
           "report_max_empties": 10, "runs": []}
    for E in (0, 6):
        net = bench.make_net("fast")
        args = dict(bench.SELFPLAY_ARGS, num_simulations=sims, leaf_solve_empties=E)
        sp = BatchedSelfPlay(net, args, games, seed=99, sample_capacity=games * 130)
        t0 = time.perf_counter()
        sp.play_games(games)
        dt = time.perf_counter() - t0
        rows = sp.engine.samples()
        rep = endgame.move_report(rows, 10)
        run = {"E": E, "seconds": round(dt, 2), "rows": int(len(rows["z"])),
               "leaf_stats": sp.engine.leaf_solve_stats(), "total": rep["total"],
               "by_empties": {str(k): v for k, v in rep["by_empties"].items()}}
        out["runs"].append(run)
        print(json.dumps({"E": E, "total": rep["total"]}), flush=True)
        del sp
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "leaf_solve_bench.json"))
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    dumps = []
    result = {"device": torch.cuda.get_device_name(0), "build_id": nat.build_id(),
              "quick": a.quick}
    with torch.no_grad():
        result["step_rate"] = step_rate(a.quick, dumps)
        result["kernel"] = kernel_alone(dumps, a.quick)
        result["play"] = effect_on_play(a.quick)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
