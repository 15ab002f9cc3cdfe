"""Game-record replay and majority-vote throughput: oth_records_gpu against oth_records_cpu on
16 host threads, and az_records_vote_gpu on the replayed rows.

    python scripts/bench_records.py [--games 65536 1048576] [--out profiles/records_bench.json]

Workload: uniformly random legal playouts from the initial position (records.random_playouts,
seeded, in chunks of 2^16 games), passes left out as most record formats do, stride 64.
Timed per size, each after one warm-up call, repeated until at least half a second has been
timed, median reported, every repeat kept:

  gpu_kernel      oth_records_gpu alone on resident buffers (host clock around a synchronised
                  call);
  cpu_native      oth_records_cpu over 16 threads on preallocated buffers (the yardstick);
  gpu_end_to_end  records.replay(NumPy in, NumPy out, device="cuda"): copies, the kernel, the
                  compaction of the rows;
  cpu_end_to_end  records.replay(device="cpu"): the threads, then the same compaction in NumPy;
  vote_gpu        az_records_vote_gpu on the replayed rows, resident on the device.

The device's rows are compared with the host's before anything is timed.  No pass / fail
number: the result sets records.PREFER_GPU and goes into DESIGN.md."""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "alphazero-othello_amd")]

import torch  # noqa: E402

import az_native as nat  # noqa: E402
import records as R  # noqa: E402

THREADS = 16
STRIDE = MAX_ROWS = 64


def timed(fn, min_s=0.5, max_repeats=2000):
    fn()
    out = []
    while len(out) < 3 or (sum(out) < min_s and len(out) < max_repeats):
        t = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t)
    return out


def summary(times, games, rows):
    med = statistics.median(times)
    return {"seconds": times, "median_s": med, "min_s": min(times), "games_per_s": games / med,
            "rows_per_s": rows / med}


def host_buffers(n):
    out = {k: np.zeros((MAX_ROWS, n), dt) for k, dt in R._ROW_FIELDS}
    out.update({k: np.zeros(n, dt) for k, dt in R._GAME_FIELDS})
    return out


def cpu_native(acts, pool):
    """oth_records_cpu on THREADS slices, each into its own preallocated buffers"""
    n = len(acts)
    bounds = np.linspace(0, n, THREADS + 1).astype(np.int64)
    parts = [(acts[a:b], host_buffers(b - a)) for a, b in zip(bounds[:-1], bounds[1:])]

    def run(part):
        a, o = part
        return nat.lib.oth_records_cpu(nat.ptr(a), STRIDE, None, None, None, len(a), MAX_ROWS, 0,
                                       *[nat.ptr(o[k]) for k in R._ORDER])

    def call():
        for rc in pool.map(run, parts):
            nat.check(rc, "oth_records_cpu")

    return call, parts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, nargs="+", default=[1 << 16, 1 << 20])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "records_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_records.py needs the GPU"
    res = {"device": torch.cuda.get_device_name(0), "build_id": nat.build_id(),
           "host_threads": THREADS, "stride": STRIDE, "max_rows": MAX_ROWS,
           "workload": "random playouts, passes omitted", "sizes": {}}
    pool = ThreadPoolExecutor(THREADS)
    for n in a.games:
        acts = np.concatenate([R.random_playouts(min(1 << 16, n - b), seed=b, stride=STRIDE,
                                                 write_passes=False)
                               for b in range(0, n, 1 << 16)])
        d_acts = torch.from_numpy(acts).cuda()
        # the device computes what the host computes
        call_cpu, parts = cpu_native(acts, pool)
        call_cpu()
        raw = R.replay_gpu_raw(d_acts, None, None, None, MAX_ROWS, 0)
        torch.cuda.synchronize()
        for k in R._ORDER:
            host = np.concatenate([p[1][k] for p in parts], axis=-1)
            dev = raw[k].cpu().numpy()
            assert (host == (dev.view(np.uint64) if host.dtype == np.uint64 else dev)).all(), k
        rows = int(raw["n_rows"].sum())
        entry = {"games": n, "rows": rows,
                 "terminal_games": int((raw["status"] == nat.AZ_REC_TERMINAL).sum())}
        bufs = [nat.ptr(raw[k]) for k in R._ORDER]

        def gpu_kernel():
            nat.check(nat.lib.oth_records_gpu(nat.ptr(d_acts), STRIDE, None, None, None, n,
                                              MAX_ROWS, 0, *bufs, nat.stream_ptr()),
                      "oth_records_gpu")
            torch.cuda.synchronize()

        entry["gpu_kernel"] = summary(timed(gpu_kernel), n, rows)
        # bytes the replay has to move: the lines in, 19 B per row and 24 B per game out
        moved = n * STRIDE + rows * 19 + n * 24
        entry["gpu_kernel"]["bytes_moved"] = moved
        entry["gpu_kernel"]["bytes_per_s"] = moved / entry["gpu_kernel"]["median_s"]
        entry["cpu_native"] = summary(timed(call_cpu), n, rows)
        entry["gpu_end_to_end"] = summary(timed(lambda: R.replay(acts, device="cuda")), n, rows)
        entry["cpu_end_to_end"] = summary(timed(lambda: R.replay(acts, device="cpu")), n, rows)
        del raw, bufs, parts
        own, opp, act, z, _, _, _ = R.replay(d_acts)
        own, opp, act, z = (x.contiguous() for x in (own, opp, act, z))

        def vote():
            out = R.vote_gpu_tensors(own, opp, act, z)
            torch.cuda.synchronize()
            return out

        groups = len(vote()[0])
        entry["vote_gpu"] = dict(summary(timed(vote), n, rows), groups=groups)
        res["sizes"][str(n)] = entry
        print(n, {k: round(v["median_s"], 5) for k, v in entry.items() if isinstance(v, dict)},
              flush=True)
        del own, opp, act, z
        torch.cuda.empty_cache()
    big = res["sizes"][str(max(a.games))]
    res["gpu_faster_end_to_end"] = big["gpu_end_to_end"]["median_s"] < big["cpu_end_to_end"]["median_s"]
    res["gpu_faster_native"] = big["gpu_kernel"]["median_s"] < big["cpu_native"]["median_s"]
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"gpu_faster_end_to_end": res["gpu_faster_end_to_end"],
                      "gpu_faster_native": res["gpu_faster_native"]}))


if __name__ == "__main__":
    main()
