"""endgame.optimal_line on an MI355X against 16 host threads; writes
profiles/optimal_line_bench.json ("Optimal lines of solved roots").

    python scripts/bench_optimal_line.py [--out profiles/optimal_line_bench.json] [--quick]

Roots: positions of tests/golden/board_corpus.npz with exactly E empties (E = 4, 8, 10, 12), at a
fixed stride, in lists of 10 (what a self-play run of a few thousand games would hand over at
one poll) and of 256.  Per E and list size: 16 lists (of 256 roots: the 2 a level holds), each
solved alone with endgame.optimal_line on each device after one warm-up call; the mean and
maximum wall time
of a call (host clocks; the device call ends in a synchronise), the rows per root, and whether
host and device returned the same bytes.  --quick shrinks every part (a rehearsal of the script,
not a measurement).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alphazero-othello_amd"))

import az_native as nat  # noqa: E402
import endgame  # noqa: E402

E_LIST = (4, 8, 10, 12)
FIELDS = ("own", "opp", "pi", "act", "z", "off", "score")


def corpus():
    with np.load(os.path.join(ROOT, "tests", "golden", "board_corpus.npz")) as z:
        d = {k: z[k] for k in z.files}
    own = np.where(d["player"] == 1, d["pos"], d["neg"]).astype(np.uint64)
    opp = np.where(d["player"] == 1, d["neg"], d["pos"]).astype(np.uint64)
    return own, opp, endgame.empties(own, opp)


def timed(own, opp, E, dev):
    t0 = time.perf_counter()
    out = endgame.optimal_line(own, opp, E, device=dev)
    if dev == "cuda":
        torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optimal_line_bench.json"))
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    own, opp, emp = corpus()
    result = {"device": torch.cuda.get_device_name(0), "build_id": nat.build_id(),
              "quick": a.quick, "host_threads": endgame.MAX_THREADS, "runs": []}
    for E in E_LIST:
        idx = np.flatnonzero(emp == E)
        for size, lists in ((10, 16), (256, 2)):
            if a.quick:
                lists = 2
            if size * lists > len(idx):
                lists = len(idx) // size
            pick = idx[np.linspace(0, len(idx) - 1, size * lists).astype(int)].reshape(lists, size)
            row = {"empties": E, "roots_per_call": size, "calls": lists}
            same, rows = True, 0
            for dev in ("cpu", "cuda"):
                timed(own[pick[0]], opp[pick[0]], E, dev)  # warm-up
                ts, outs = [], []
                for p in pick:
                    t, out = timed(own[p], opp[p], E, dev)
                    ts.append(t)
                    outs.append(out)
                row[dev + "_ms_mean"] = round(float(np.mean(ts)) * 1000.0, 3)
                row[dev + "_ms_max"] = round(float(np.max(ts)) * 1000.0, 3)
                if dev == "cpu":
                    ref = outs
                    rows = sum(int(o["off"][-1]) for o in outs)
                else:
                    same = all(np.ascontiguousarray(x[k]).tobytes()
                               == np.ascontiguousarray(y[k]).tobytes()
                               for x, y in zip(ref, outs) for k in FIELDS)
            row["rows_per_root"] = round(rows / (size * lists), 3)
            row["device_equals_host"] = bool(same)
            row["device_over_host"] = round(row["cuda_ms_mean"] / row["cpu_ms_mean"], 2)
            result["runs"].append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
