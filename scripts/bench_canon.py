"""Canonical positions: kernel rates against a float4 copy, and what symmetry merges in the
replay aggregation of one real generation.

    python scripts/bench_canon.py [--positions 16777216] [--rows 1048576] [--games 512]
                                  [--sims 32] [--out profiles/canon_bench.json]

Kernels ("Measuring it": 400 untimed launches, then 100 launches each
timed by its own event pair, all in one run so the rates share the chip's state):

  canon_two_per_lane  oth_canon_gpu on 16-byte aligned arrays (k_canon2), bench.py's playout
                      corpus tiled to --positions; 34 B of algorithmic traffic per position;
  canon_one_per_lane  the same on slices that start at an odd element (k_canon1);
  copy16              az_copy16_probe_gpu over as many bytes as canon reads (and writes them);
  oth_step            bench.py's StepKernelBench on the same corpus (43 B per position);
  rows_d4             az_rows_d4_gpu, pi only, --rows rows of random symmetries (521 B per row);
  rows_symmetrise     az_rows_symmetrise_gpu with the corpus' own stabilisers (almost all
                      trivial) and with every row under all eight symmetries.

The same entry points on 16 host threads (symmetry.canon_cpu and friends, median of at least
three calls).  Every device result is compared with the host's before it is timed.

End to end: one generation of self-play (collect_self_play_games, --games games of a
randomly initialised FastOthelloNet at --sims simulations), its rows through
replay.aggregate_rows with symmetry off and on: times, rows out, and by ply the distinct
boards against the classes up to symmetry.  No pass / fail number: the figures go into
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
import replay  # noqa: E402
import symmetry  # noqa: E402
from bench import StepKernelBench, launch_ms, playout_positions  # noqa: E402

WARM, REPS = 400, 100


def steady_ms(launch):
    for _ in range(WARM):
        launch()
    torch.cuda.synchronize()
    return launch_ms(launch, REPS)


def rate(ms, nbytes, items):
    return {"ms": ms, "gb_per_s": nbytes / ms / 1e6, "items_per_s": items / ms * 1e3}


def host_timed(fn, min_s=0.5):
    fn()
    out = []
    while len(out) < 3 or sum(out) < min_s:
        t = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t)
    return statistics.median(out)


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()


def kernels(n, n_rows):
    res = {}
    own, opp, _ = playout_positions()
    reps = -(-(n + 1) // len(own))
    own, opp = np.tile(own, reps)[:n + 1], np.tile(opp, reps)[:n + 1]
    d_own, d_opp = dev(own), dev(opp)
    outs = [torch.empty(n + 1, dtype=torch.int64, device="cuda") for _ in range(2)] + \
           [torch.empty(n + 2, dtype=torch.uint8, device="cuda") for _ in range(2)]
    s = nat.stream_ptr()
    want = symmetry.canon_cpu(own, opp)

    def canon(first):
        sl = slice(first, first + n)
        args = [nat.ptr(d_own[sl]), nat.ptr(d_opp[sl]), n] + [nat.ptr(o[sl]) for o in outs] + [s]
        nat.check(nat.lib.oth_canon_gpu(*args), "oth_canon_gpu")
        torch.cuda.synchronize()
        for o, w in zip(outs, want):
            got = o[sl].cpu().numpy()
            assert np.array_equal(got.view(np.uint64) if w.dtype == np.uint64 else got, w[sl])
        return steady_ms(lambda: nat.lib.oth_canon_gpu(*args))

    res["canon_two_per_lane"] = rate(canon(0), 34 * n, n)
    res["canon_one_per_lane"] = rate(canon(1), 34 * n, n)
    # the copy: as many bytes in as canon reads
    src = torch.empty(n * 2, dtype=torch.int64, device="cuda").random_()
    dst = torch.empty_like(src)
    cargs = [nat.ptr(src), nat.ptr(dst), n, s]
    nat.check(nat.lib.az_copy16_probe_gpu(*cargs), "az_copy16_probe_gpu")
    assert torch.equal(src, dst)
    res["copy16"] = rate(steady_ms(lambda: nat.lib.az_copy16_probe_gpu(*cargs)), 32 * n, n)
    del src, dst
    step = StepKernelBench(n, "cuda")
    res["oth_step"] = rate(step.time_ms(WARM, REPS), 43 * n, n)
    del step
    t = host_timed(lambda: symmetry.canon_cpu(own[:n], opp[:n]))
    res["canon_host_16_threads"] = rate(t * 1e3, 34 * n, n)
    stab_corpus = want[3][:n_rows].copy()
    del d_own, d_opp, outs, want
    torch.cuda.empty_cache()

    rng = np.random.default_rng(1)
    pi = rng.random((n_rows, 65), dtype=np.float32)
    sym = rng.integers(0, 8, n_rows).astype(np.uint8)
    d_pi, d_sym, d_out = dev(pi), dev(sym), torch.empty(n_rows, 65, device="cuda")
    rargs = [nat.ptr(d_pi), None, nat.ptr(d_sym), None, n_rows, nat.ptr(d_out), None, s]
    nat.check(nat.lib.az_rows_d4_gpu(*rargs), "az_rows_d4_gpu")
    assert np.array_equal(d_out.cpu().numpy(), symmetry.rows_d4_cpu(pi, None, sym, None)[0])
    res["rows_d4"] = rate(steady_ms(lambda: nat.lib.az_rows_d4_gpu(*rargs)), 521 * n_rows, n_rows)
    t = host_timed(lambda: symmetry.rows_d4_cpu(pi, None, sym, None))
    res["rows_d4_host_16_threads"] = rate(t * 1e3, 521 * n_rows, n_rows)
    for name, stab in (("rows_symmetrise", stab_corpus),
                       ("rows_symmetrise_all_eight", np.full(n_rows, 0xFF, np.uint8))):
        stab[stab == 0] = 1
        d_stab = dev(stab)
        sargs = [nat.ptr(d_pi), nat.ptr(d_stab), n_rows, nat.ptr(d_out), s]
        nat.check(nat.lib.az_rows_symmetrise_gpu(*sargs), "az_rows_symmetrise_gpu")
        assert np.array_equal(d_out.cpu().numpy(), symmetry.symmetrise_cpu(pi, stab))
        res[name] = rate(steady_ms(lambda: nat.lib.az_rows_symmetrise_gpu(*sargs)),
                         521 * n_rows, n_rows)
        t = host_timed(lambda: symmetry.symmetrise_cpu(pi, stab))
        res[name + "_host_16_threads"] = rate(t * 1e3, 521 * n_rows, n_rows)
    res["nontrivial_stabilisers_in_corpus_rows"] = int((stab_corpus != 1).sum())
    return res


def generation(games, sims, seed):
    from Models import FastOthelloNet
    from self_play_worker import collect_self_play_games

    torch.manual_seed(seed)
    net = FastOthelloNet(8, 65).cuda().eval()
    t = time.perf_counter()
    rows = collect_self_play_games(net, {"c_puct": 2.0, "num_simulations": sims}, games, seed=seed)
    took = time.perf_counter() - t
    states = np.stack([np.asarray(r[0], np.int8).reshape(64) for r in rows])
    own, opp = nat.pack_np(states, np.ones(len(rows), np.int8))
    pi = np.stack([np.asarray(r[1], np.float32) for r in rows])
    z = np.array([float(r[2]) for r in rows], np.float64)
    return own, opp, pi, z, took


def end_to_end(games, sims, seed):
    own, opp, pi, z, took = generation(games, sims, seed)
    n = len(own)
    args = (dev(own), dev(opp), torch.zeros(n, dtype=torch.int32, device="cuda"), dev(pi), dev(z))
    out = {"games": games, "simulations": sims, "rows": n, "self_play_s": took}
    for flag in (False, True):
        res = replay.aggregate_rows(*args, symmetry=flag)
        t = host_timed(lambda: replay.aggregate_rows(*args, symmetry=flag), min_s=0.2)
        out["symmetry_on" if flag else "symmetry_off"] = {"rows_out": int(res["own"].shape[0]),
                                                         "seconds": t}
    co, cp, _, stab = symmetry.canon_cpu(own, opp)
    ply = np.array([bin(int(a | b)).count("1") for a, b in zip(own, opp)]) - 4
    by_ply = []
    for p in range(int(ply.max()) + 1):
        m = ply == p
        if not m.any():
            continue
        boards = len(set(zip(own[m].tolist(), opp[m].tolist())))
        classes = len(set(zip(co[m].tolist(), cp[m].tolist())))
        by_ply.append({"ply": p, "rows": int(m.sum()), "boards": boards, "classes": classes,
                       "merge_ratio": boards / classes})
    out["by_ply"] = by_ply
    out["rows_with_nontrivial_stabiliser"] = int((stab != 1).sum())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--positions", type=int, default=1 << 24)
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--games", type=int, default=512)
    ap.add_argument("--sims", type=int, default=32)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "canon_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_canon.py needs the GPU"
    res = {"device": torch.cuda.get_device_name(0), "build_id": nat.build_id(),
           "warm_launches": WARM, "timed_launches": REPS, "positions": a.positions,
           "rows": a.rows, "host_threads": symmetry.MAX_THREADS}
    res["kernels"] = kernels(a.positions, a.rows)
    print(json.dumps({k: round(v["gb_per_s"], 1) for k, v in res["kernels"].items()
                      if isinstance(v, dict)}), flush=True)
    res["end_to_end"] = end_to_end(a.games, a.sims, a.seed)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    e = res["end_to_end"]
    print(json.dumps({"rows": e["rows"], "off": e["symmetry_off"], "on": e["symmetry_on"]}))


if __name__ == "__main__":
    main()
