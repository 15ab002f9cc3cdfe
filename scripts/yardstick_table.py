"""The yardstick's own scale, and one net on it.

    python scripts/yardstick_table.py [--levels 1,2,3,4,5] [--out profiles/yardstick_table.json]

1. Cross table: AlphaBetaPlayer.level(i) against level(j) for every pair i < j, each over the
   same 64 openings (alphabeta.openings(64, 8, 0)) x 2 colours = 128 matches; the entry is the
   row level's score (wins + draws / 2) / 128.  Both sides are deterministic, so the table is
   reproducible bit for bit.
2. Ladder: arena.ladder of a random-init FastOthelloNet (torch.manual_seed(0)) with
   --sims simulations per move, --matches matches per level.

A finding, not a test: a deeper level that fails to outscore a shallower one is reported as it
is."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "alphazero-othello_amd")]

import torch  # noqa: E402

import alphabeta  # noqa: E402
from arena import BatchedArena, ladder  # noqa: E402
from Models import FastOthelloNet  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--levels", default="1,2,3,4,5")
    ap.add_argument("--sims", type=int, default=100)
    ap.add_argument("--matches", type=int, default=128)
    ap.add_argument("--device", default=None, help="the alpha-beta players' device")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yardstick_table.json"))
    a = ap.parse_args()
    levels = [int(x) for x in a.levels.split(",")]
    ops = alphabeta.openings(64, 8, 0)
    args = {"c_puct": 2.0, "num_simulations": a.sims}
    res = {"openings": "openings(64, 8, 0)", "matches_per_pair": 128, "cross": {}, "seconds": {}}
    for i in levels:
        for j in levels:
            if i >= j:
                continue
            t = time.perf_counter()
            arena = BatchedArena(alphabeta.AlphaBetaPlayer.level(i, a.device),
                                 alphabeta.AlphaBetaPlayer.level(j, a.device), args, 128)
            wi, wj, dr, _ = arena.play(128, openings=ops)
            res["cross"][f"{i}v{j}"] = {"score": (wi + 0.5 * dr) / 128, "wins": wi, "draws": dr,
                                        "losses": wj}
            res["seconds"][f"{i}v{j}"] = time.perf_counter() - t
            print(f"level {i} v {j}:", res["cross"][f"{i}v{j}"], flush=True)
    if torch.cuda.is_available():
        torch.manual_seed(0)
        net = FastOthelloNet(8, 65).eval()
        t = time.perf_counter()
        res["ladder_random_init_fast_net"] = {
            "num_simulations": a.sims, "matches_per_level": a.matches,
            "levels": ladder(net, args, levels, a.matches, plies=8, seed=0)}
        res["seconds"]["ladder"] = time.perf_counter() - t
        print("ladder:", res["ladder_random_init_fast_net"], flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
