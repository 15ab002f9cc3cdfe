"""Golden vectors for the sharp mock policy (tests/mock_policy.py, sharp_eval), made by running
the REFERENCE itself.  Build container only (imports /root/reference read-only).

The mock policy's priors are never zero, never tiny and almost never equal, and its values are
never exactly +-1 or 0; a trained net's are.  The sharp policy gives exact zeros, priors of
2^-44 (a legal row of them sums to a non-zero value below the reference's 1e-12
renormalisation threshold), equal powers of two and saturated values, and this script records
what the reference computes from them:

  mcts_sharp_cases.npz     schema of mcts_cases.npz (make_goldens.py gen_mcts): num_threads = 1,
                           two searches with tree reuse per case.
  mcts_sharp_vl_cases.npz  schema of mcts_vl_cases.npz (make_vl_goldens.py): num_threads = 4
                           under the forced thread schedule.
  selfplay_sharp.npz       schema of selfplay_deep.npz (meta[:, 3] = K): complete one_self_play
                           games, K = 1 and K = 4 (forced schedule).

The files are written with fixed zip timestamps, so a second run reproduces them byte for
byte.  tests/test_sharp_cpu.py counts on the oracle what the cases reach.

    python tests/golden/make_sharp_goldens.py
"""
import io
import os
import sys
import time
import zipfile

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True

import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_goldens import RngRecorder, bb_from_state, encode_log, random_position  # noqa: E402
from make_vl_goldens import GatedPolicy, controlled_simulations  # noqa: E402
from make_deep_goldens import ControlledPool  # noqa: E402
from mock_policy import SharpPolicy, SharpPolicyNet  # noqa: E402

ROOT_PLIES = (0, 10, 30, 50, 55, 40, 20)  # random_position, rng 11, drawn in this order
# (sims, c_puct, eps, temp)
MCTS_SETTINGS = ((100, 2.0, 0.0, 0.0), (100, 1.0, 0.3, 1.0), (200, 2.0, 0.0, 1.0),
                 (25, 2.0, 0.3, 1.0))
VL_K = 4
VL_SETTINGS = ((100, 2.0, 0.3), (100, 1.0, 0.0))  # (sims, c_puct, eps)
GAMES = ((25, 1, 31), (25, 1, 32), (100, 1, 33), (25, 4, 34))  # (sims, K, seed)
# ARGS of tests/test_bench_path_gpu.py
SELFPLAY_ARGS = {"c_puct": 2.0, "dirichlet_alpha": 1.0, "dirichlet_epsilon": 0.3,
                 "mcts_temperature": 1.0, "num_exploratory_moves": 35, "lambda": 0.98}


def save_npz(name, arrays):
    """np.savez_compressed with every member's timestamp fixed: the same arrays give the same
    bytes."""
    with zipfile.ZipFile(os.path.join(HERE, name), "w", zipfile.ZIP_DEFLATED) as z:
        for k, v in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o600 << 16
            z.writestr(info, buf.getvalue())


class GatedSharpPolicy(GatedPolicy):
    def __init__(self):
        super().__init__()
        self.inner = SharpPolicy()


class GatedSharpPolicyNet(GatedSharpPolicy):
    """Constructible the way one_self_play builds its net (self_play_worker.py:43-46)."""

    def __init__(self, **cfg):
        super().__init__()

    def load_state_dict(self, sd):
        return None

    def eval(self):
        return self


def roots(g):
    rng = np.random.default_rng(11)
    return [random_position(g, rng, plies) for plies in ROOT_PLIES]


def _row(rows, m, st, pl, probs, case_id, mv, **extra):
    counts = np.zeros(65, np.int64)
    for a, ch in m.root.children.items():
        counts[a] = ch.visit_count
        assert ch.virtual_visits == 0
    p, n = bb_from_state(st)
    for k, v in dict(pos=p, neg=n, player=pl, moves=mv, counts=counts,
                     root_value=float(m.root.value), probs=np.asarray(probs, np.float32),
                     root_n=m.root.visit_count, log_case=case_id, **extra).items():
        rows.setdefault(k, []).append(v)
    return counts


def _pack(rows, ints, floats):
    out = {k: np.array(rows[k], np.uint64) for k in ("pos", "neg")}
    for k in ints:
        out[k] = np.array(rows[k], np.int64)
    for k in floats:
        out[k] = np.array(rows[k], np.float64)
    out["counts"] = np.array(rows["counts"], np.int64)
    out["probs"] = np.array(rows["probs"], np.float32)
    return out


def gen_mcts():
    from envs.othello import OthelloGameNew
    from MCTS_model import MCTS

    g = OthelloGameNew(8)
    rows, logs = {}, []
    case_id = 0
    for state, player in roots(g):
        for sims, cp, eps, temp in MCTS_SETTINGS:
            seed = 300 + case_id
            np.random.seed(seed)
            args = {"c_puct": cp, "num_simulations": sims, "num_threads": 1}
            m = MCTS(g, args, SharpPolicy(), dirichlet_alpha=1.0, dirichlet_epsilon=eps)
            st, pl = state.copy(), player
            with RngRecorder() as rec:
                for mv in range(2):
                    probs = m.policy_improve_step(st, pl, temp=temp)
                    counts = _row(rows, m, st, pl, probs, case_id, mv, sims=sims, c_puct=cp,
                                  eps=eps, alpha=1.0, temp=temp, seed=seed)
                    a = int(np.argmax(counts))
                    nxt = g.get_next_state(st, a, pl)
                    if g.get_value_and_terminated(nxt, a, pl)[1]:
                        break
                    m.make_move(a)
                    st, pl = nxt, -pl
            m.pool.shutdown()
            logs.append(encode_log(rec.log))
            case_id += 1
    out = _pack(rows, ("player", "sims", "seed", "moves", "root_n", "log_case"),
                ("c_puct", "eps", "alpha", "temp", "root_value"))
    out["n_cases"] = np.int64(case_id)
    out["log_offsets"] = np.cumsum([0] + [len(l[0]) for l in logs]).astype(np.int64)
    out["log_kind"] = np.concatenate([l[0] for l in logs])
    out["log_a"] = np.concatenate([l[1] for l in logs])
    out["log_b"] = np.concatenate([l[2] for l in logs])
    out["noise_offsets"] = np.cumsum([0] + [len(l[3]) for l in logs]).astype(np.int64)
    out["noise"] = np.concatenate([l[3] for l in logs])
    save_npz("mcts_sharp_cases.npz", out)
    print("mcts_sharp_cases:", case_id, "cases,", len(out["pos"]), "searches")


def gen_vl():
    from envs.othello import OthelloGameNew
    from MCTS_model import MCTS, Node

    g = OthelloGameNew(8)
    rows, logs = {}, []
    case_id = 0
    K = VL_K
    for state, player in roots(g):
        for sims, cp, eps in VL_SETTINGS:
            np.random.seed(600 + case_id)
            args = {"c_puct": cp, "num_simulations": sims, "num_threads": K}
            policy = GatedSharpPolicy()
            m = MCTS(g, args, policy, dirichlet_alpha=1.0, dirichlet_epsilon=eps)
            st, pl = state.copy(), player
            with RngRecorder() as rec:
                for mv in range(2):
                    # policy_improve_step (MCTS_model.py:217-235) up to its simulations ...
                    if m.root is None:
                        m.root = Node(env=g, args=args, state=st.copy(), player=pl, action=None)
                    if m.root.is_leaf():
                        m._expand_and_evaluate(m.root)
                    controlled_simulations(m, policy, sims, K)
                    # ... and its pi from the counts (no further simulations)
                    m.args = dict(args, num_simulations=0)
                    probs = m.policy_improve_step(st, pl, temp=1.0)
                    m.args = args
                    counts = _row(rows, m, st, pl, probs, case_id, mv, sims=sims, k=K,
                                  c_puct=cp, eps=eps)
                    a = int(np.argmax(counts))
                    nxt = g.get_next_state(st, a, pl)
                    if g.get_value_and_terminated(nxt, a, pl)[1]:
                        break
                    m.make_move(a)
                    st, pl = nxt, -pl
            m.pool.shutdown()
            kinds, _, _, noise = encode_log(rec.log)
            assert (kinds == 0).all(), "only Dirichlet draws at temperature 1"
            logs.append(noise)
            case_id += 1
    out = _pack(rows, ("player", "sims", "k", "moves", "root_n", "log_case"),
                ("c_puct", "eps", "root_value"))
    out["n_cases"] = np.int64(case_id)
    out["noise_offsets"] = np.cumsum([0] + [len(nz) for nz in logs]).astype(np.int64)
    out["noise"] = np.concatenate(logs)
    save_npz("mcts_sharp_vl_cases.npz", out)
    print("mcts_sharp_vl_cases:", case_id, "cases,", len(out["pos"]), "searches")


def play(sims, K, seed):
    import self_play_worker
    from MCTS_model import MCTS

    args = dict(SELFPLAY_ARGS, num_simulations=sims, num_threads=K)
    policy_cls = SharpPolicyNet
    orig = self_play_worker.MCTS
    if K > 1:
        class ControlledMCTS(MCTS):
            def __init__(self, *a, **kw):
                super().__init__(*a, **kw)
                self.pool.shutdown()
                self.pool = ControlledPool(self, K)

        self_play_worker.MCTS = ControlledMCTS
        policy_cls = GatedSharpPolicyNet
    try:
        np.random.seed(seed)
        with RngRecorder() as rec:
            out = self_play_worker.one_self_play((8, args, (policy_cls, {}, {}), None))
    finally:
        self_play_worker.MCTS = orig
    return out, rec.log


def gen_selfplay():
    rows = dict(game=[], ply=[], pos=[], neg=[], pi=[], z=[])
    meta, logs = [], []
    for gi, (sims, K, seed) in enumerate(GAMES):
        t0 = time.time()
        out, log = play(sims, K, seed)
        print(f"  game {gi}: sims={sims} K={K} plies={len(out)} {time.time() - t0:.1f}s",
              flush=True)
        for t, (s, pi, z) in enumerate(out):
            p, n = bb_from_state(s)  # canonical (state*player): +1 = side to move
            rows["game"].append(gi)
            rows["ply"].append(t)
            rows["pos"].append(p)
            rows["neg"].append(n)
            rows["pi"].append(np.asarray(pi, np.float32))
            rows["z"].append(float(z))
        logs.append(encode_log(log))
        meta.append((sims, seed, len(out), K))
    out = {"pos": np.array(rows["pos"], np.uint64), "neg": np.array(rows["neg"], np.uint64),
           "game": np.array(rows["game"], np.int32), "ply": np.array(rows["ply"], np.int32),
           "pi": np.array(rows["pi"], np.float32), "z": np.array(rows["z"], np.float64),
           "meta": np.array(meta, np.int64)}
    out["log_offsets"] = np.cumsum([0] + [len(l[0]) for l in logs]).astype(np.int64)
    out["log_kind"] = np.concatenate([l[0] for l in logs])
    out["log_a"] = np.concatenate([l[1] for l in logs])
    out["log_b"] = np.concatenate([l[2] for l in logs])
    out["noise_offsets"] = np.cumsum([0] + [len(l[3]) for l in logs]).astype(np.int64)
    out["noise"] = np.concatenate([l[3] for l in logs])
    save_npz("selfplay_sharp.npz", out)
    print("selfplay_sharp:", len(GAMES), "games,", len(out["pos"]), "samples")


GENS = {"mcts": gen_mcts, "vl": gen_vl, "selfplay": gen_selfplay}

if __name__ == "__main__":
    for w in sys.argv[1:] or list(GENS):
        t0 = time.time()
        GENS[w]()
        print(f"[{w}] {time.time() - t0:.1f}s")
