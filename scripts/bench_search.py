"""Alpha-beta search throughput: oth_search_gpu at split_plies 0 / 1 / 2 against oth_search_cpu
on 16 host threads, on the same roots.

    python scripts/bench_search.py [--depths 4,6,8] [--repeats 3] [--out profiles/search_bench.json]

Roots: alphabeta.openings(1024, 8, 0) (the arena's shape: 1,024 distinct openings) and 1,024
corpus positions with 20..40 empties (the first 1,024 of default_rng(0).permutation of that
class), timed separately at depth 4, 6 and 8.  Every step, one (depth, backend) pair, runs
in a child process under its own timeout; the parent never opens the GPU, and after a step
that fails or runs out of time it starts nothing more.  A step warms each set up once, then
times up to `repeats` calls (wall clock around a synchronised call, device buffers
resident; a slow configuration stops once its repeats have used the budget) and reports the
median, positions/s, nodes/s and the largest per-root node count; the parent checks that
every backend returned the same values and best moves.  No pass / fail number: the result
picks alphabeta.DEFAULT_SPLIT_PLIES and AlphaBetaPlayer's default device and goes into
DESIGN.md."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "alphazero-othello_amd")]

LIMIT = 1 << 31
BACKENDS = ("cpu_16_threads", "gpu_split_0", "gpu_split_1", "gpu_split_2")
STEP_TIMEOUT_S = {4: 120, 6: 180, 8: 420}


def workload():
    import alphabeta
    import endgame

    d = np.load(os.path.join(ROOT, "tests", "golden", "board_corpus.npz"))
    own = np.where(d["player"] == 1, d["pos"], d["neg"]).astype(np.uint64)
    opp = np.where(d["player"] == 1, d["neg"], d["pos"]).astype(np.uint64)
    emp = endgame.empties(own, opp)
    cls = np.flatnonzero((emp >= 20) & (emp <= 40))
    idx = cls[np.random.default_rng(0).permutation(len(cls))[:1024]]
    o, p, _ = alphabeta.openings(1024, 8, 0)
    return {"openings_1024": (o, p), "corpus_20_40_1024": (own[idx], opp[idx])}


def timed(fn, repeats, budget_s):
    fn()  # warm-up
    out = []
    for _ in range(repeats):
        t = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t)
        if sum(out) > budget_s:
            break
    return out


def step(depth, backend, repeats, budget_s):
    """One (depth, backend) pair on both root sets; prints one JSON line."""
    import torch

    import alphabeta
    import az_native as nat

    res = {"build_id": nat.build_id()}
    if backend != "cpu_16_threads":
        assert torch.cuda.is_available(), "bench_search.py needs the GPU"
        res["device"] = torch.cuda.get_device_name(0)
    for name, (o, p) in workload().items():
        if backend == "cpu_16_threads":
            def run():
                return alphabeta.search(o, p, depth, device="cpu", node_limit=LIMIT)
        else:
            o_t = torch.from_numpy(o.view(np.int64)).cuda()
            p_t = torch.from_numpy(p.view(np.int64)).cuda()

            def run(o_t=o_t, p_t=p_t):
                r = alphabeta.search_gpu_tensors(o_t, p_t, depth, LIMIT, int(backend[-1]))
                torch.cuda.synchronize()
                return r
        v, b, nd = (np.asarray(x.cpu()) if isinstance(x, torch.Tensor) else x for x in run())
        nd = nd.view(np.uint64)
        assert (v > nat.AZ_SEARCH_ABORTED).all()
        times = timed(run, repeats, budget_s)
        med = statistics.median(times)
        res[name] = {"seconds": times, "median_s": med, "positions_per_s": len(o) / med,
                     "nodes_total": int(nd.sum()), "nodes_per_s": int(nd.sum()) / med,
                     "nodes_max_per_root": int(nd.max()),
                     "result_sha256": hashlib.sha256(v.tobytes() + b.tobytes()).hexdigest()}
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--depths", default="4,6,8")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--budget-s", type=float, default=15.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_bench.json"))
    ap.add_argument("--step", default=None, help="internal: depth,backend of a child process")
    a = ap.parse_args()
    if a.step:
        depth, backend = a.step.split(",")
        return step(int(depth), backend, a.repeats, a.budget_s)
    res = {"host_threads": 16, "repeats": a.repeats, "budget_s": a.budget_s, "depths": {}}
    failed = None
    for depth in (int(x) for x in a.depths.split(",")):
        entry = {}
        for backend in BACKENDS:
            cmd = [sys.executable, os.path.abspath(__file__), "--step", f"{depth},{backend}",
                   "--repeats", str(a.repeats), "--budget-s", str(a.budget_s)]
            try:
                out = subprocess.run(cmd, capture_output=True, text=True,
                                     timeout=STEP_TIMEOUT_S.get(depth, 420))
            except subprocess.TimeoutExpired:
                failed = f"depth {depth} {backend}: timed out"
                break
            if out.returncode != 0:
                failed = f"depth {depth} {backend}: exit {out.returncode}: {out.stderr[-2000:]}"
                break
            r = json.loads(out.stdout.strip().splitlines()[-1])
            res.setdefault("build_id", r.pop("build_id"))
            if "device" in r:
                res.setdefault("device", r.pop("device"))
            r.pop("build_id", None)
            entry[backend] = r
            print(depth, backend, {k: round(v["median_s"], 4) for k, v in r.items()}, flush=True)
        res["depths"][str(depth)] = entry
        if failed:
            break
        for name in entry[BACKENDS[0]]:
            sums = {bk: entry[bk][name]["result_sha256"] for bk in BACKENDS}
            assert len(set(sums.values())) == 1, f"depth {depth} {name}: backends disagree {sums}"
        entry["fastest"] = {name: min(BACKENDS, key=lambda bk: entry[bk][name]["median_s"])
                            for name in entry[BACKENDS[0]]}
    if failed:
        res["failed"] = failed
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({d: e.get("fastest") for d, e in res["depths"].items()}))
    if failed:
        sys.exit(failed)


if __name__ == "__main__":
    main()
