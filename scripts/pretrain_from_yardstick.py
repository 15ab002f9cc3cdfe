"""Warm-start a net from the yardstick's own games: a demonstration of the records path.

    python scripts/pretrain_from_yardstick.py [--level 3] [--games 2048] [--epochs 8]
                                              [--out profiles/pretrain_yardstick.json]

Level-L against level-L alpha-beta games from `alphabeta.openings` (each opening played twice)
-> records.from_arena -> records.replay -> endgame.relabel_rows (exact values for the late
rows) -> records.dedup (majority vote) -> a few train_gpu.supervised_epoch passes over a
fresh AlphaZeroNet, with `arena.ladder` scores of the net before and after.  One run's output
goes to the JSON; it is a demonstration, not a test, and promises no strength number."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "alphazero-othello_amd")]

import torch  # noqa: E402

import az_native as nat  # noqa: E402
import endgame  # noqa: E402
import records as R  # noqa: E402
import train_gpu  # noqa: E402
from alphabeta import AlphaBetaPlayer, openings  # noqa: E402
from arena import BatchedArena, ladder  # noqa: E402
from Models import AlphaZeroNet  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--level", type=int, default=3)
    ap.add_argument("--games", type=int, default=2048)
    ap.add_argument("--opening-plies", type=int, default=8)
    ap.add_argument("--epochs", type=int, default=8)
    ap.add_argument("--batch-size", type=int, default=1024)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--channels", type=int, default=128)
    ap.add_argument("--exact-empties", type=int, default=12)
    ap.add_argument("--ladder-levels", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--ladder-matches", type=int, default=64)
    ap.add_argument("--sims", type=int, default=64)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pretrain_yardstick.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "pretrain_from_yardstick.py needs the GPU"
    torch.manual_seed(a.seed)
    args = {"c_puct": 2.0, "num_simulations": a.sims, "num_threads": 4}
    res = {"device": torch.cuda.get_device_name(0), "build_id": nat.build_id(), "config": vars(a)}

    t = time.perf_counter()
    ops = openings(-(-a.games // 2), a.opening_plies, a.seed)
    player = AlphaBetaPlayer.level(a.level)
    out = BatchedArena(player, player, args, min(a.games, 1024)).play(a.games, openings=ops,
                                                                     record=True)
    res["games"] = {"n": a.games, "first_mover_results": None, "seconds": time.perf_counter() - t}
    acts, own0, opp0, winner = R.from_arena(out[4])
    res["games"]["first_mover_results"] = {str(k): int((winner == k).sum()) for k in (1, 0, -1)}

    t = time.perf_counter()
    own, opp, act, z, ply, game, report = R.replay(acts, own0, opp0, winner, on_error="raise")
    assert not report["winner_mismatch"].any(), "the arena's results disagree with its games"
    rows, exact = endgame.relabel_rows({"own": own, "opp": opp, "z": z}, a.exact_empties)
    changed = int((rows["z"][exact] != z[exact]).sum())
    z = rows["z"].astype(np.int8)
    voted = R.dedup(own, opp, act, z, how="vote")
    res["rows"] = {"replayed": len(own), "relabelled_exact": int(exact.sum()),
                   "relabel_changed": changed,
                   "after_vote": len(voted["own"]), "seconds": time.perf_counter() - t}

    net = AlphaZeroNet(8, 65, a.blocks, a.channels).cuda()
    t = time.perf_counter()
    res["ladder_before"] = ladder(net.eval(), args, a.ladder_levels, a.ladder_matches, seed=a.seed + 1)
    res["ladder_seconds"] = time.perf_counter() - t
    n = len(voted["own"])
    perm = np.random.default_rng(a.seed).permutation(n)
    cut = max(1, n // 20)
    pick = lambda idx: [voted[k][idx] for k in ("own", "opp", "act", "z")]  # noqa: E731
    train = train_gpu.DeviceReplayLoader.from_bitboards(*pick(perm[cut:]), batch_size=a.batch_size,
                                                        device="cuda", seed=a.seed)
    held = train_gpu.DeviceReplayLoader.from_bitboards(*pick(perm[:cut]), batch_size=a.batch_size,
                                                       shuffle=False, augment=False, device="cuda")
    opt = torch.optim.Adam(net.parameters(), lr=3e-3, weight_decay=1e-4)
    names = ("loss", "policy_loss", "value_loss", "top1")
    res["held_out_before"] = dict(zip(names, train_gpu.supervised_eval(net, held)))
    res["epochs"] = []
    t = time.perf_counter()
    for e in range(a.epochs):
        loss = train_gpu.supervised_epoch(net, opt, train)
        ev = dict(zip(names, train_gpu.supervised_eval(net, held)))
        res["epochs"].append({"epoch": e + 1, "train_loss": loss, "held_out": ev})
        print(e + 1, round(loss, 4), {k: round(v, 4) for k, v in ev.items()}, flush=True)
    res["fit_seconds"] = time.perf_counter() - t
    res["ladder_after"] = ladder(net.eval(), args, a.ladder_levels, a.ladder_matches, seed=a.seed + 1)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"before": res["ladder_before"], "after": res["ladder_after"]}))


if __name__ == "__main__":
    main()
