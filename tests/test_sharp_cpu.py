"""The sharp mock policy (tests/mock_policy.py sharp_eval) on the CPU: the oracle replays every
reference fixture recorded with it (tests/golden/make_sharp_goldens.py) exactly, and a census
over the oracle's searches shows that the fixtures reach what the GPU tests
(test_sharp_engine_gpu.py) lean on them for: expansions whose legal priors are all exactly 0
or sum to a non-zero value at or below the 1e-12 renormalisation threshold (MCTS_model.py:
345-349: the priors stay unnormalised), selections whose maximal PUCT score is shared, and
leaf values of exactly +1, -1 and 0."""
import functools
from collections import Counter

import numpy as np
import pytest

from conftest import load_golden
from mock_policy import SharpPolicy, sharp_eval
from oracle import board as ob
from oracle.mcts import LogRng, SeqMCTS, ucb_scores
from oracle.selfplay import play_game
from test_oracle_golden import replay_case, replay_vl_case

N_CASES, N_VL_CASES = 28, 14
SELFPLAY_ARGS = {"c_puct": 2.0, "dirichlet_alpha": 1.0, "dirichlet_epsilon": 0.3,
                 "mcts_temperature": 1.0, "num_exploratory_moves": 35, "lambda": 0.98}


def test_sharp_policy_is_float32_exact():
    x = np.random.default_rng(0).integers(-1, 2, size=(400, 64))
    p, v = sharp_eval(x)
    assert p.dtype == np.float32 and p.shape == (400, 65) and v.shape == (400,)
    # every prior is 0, 2^-44 or one of 2^0 .. 2^-23, each of them present
    mant, exp = np.frexp(p)
    assert ((mant == 0.5) | (p == 0)).all()
    assert set(np.unique(1 - exp[p > 0])) == set(range(24)) | {44}
    assert (p == 0).mean() > 0.4
    assert (np.float32(v).astype(np.float64) == v).all() and (np.abs(v) <= 1).all()
    for x0 in (1.0, -1.0, 0.0):
        assert (v == x0).mean() > 0.2
    assert ((v * 1024 == np.rint(v * 1024))).all()
    # 17 legal priors of 2^-44 sum to a non-zero value below the renormalisation threshold
    assert 0 < 17 * float(np.float32(2.0 ** -44)) <= 1e-12


def test_sharp_policy_leaves_the_mock_alone():
    """The additions changed nothing the other fixtures depend on (spot values of mock_eval)."""
    from mock_policy import mock_eval

    p, v = mock_eval(np.zeros(64, np.int64))
    assert p[0] * 1024 == 1 + (sum((j * 71) % 97 for j in range(64)) % 1021)
    assert v == ((sum((j * 37 + 11) % 89 for j in range(64)) % 2001) - 1000) / 1024.0


# ---- the oracle replays the fixtures ---------------------------------------------------

class Census(SeqMCTS):
    """SeqMCTS that counts what its searches meet; the search itself is untouched."""

    def __init__(self, *a, **kw):
        self.seen = Counter()
        super().__init__(*a, **kw)

    def _expand_only(self, i):
        before = len(self.kids[i])
        v = super()._expand_only(i)
        kids = self.kids[i]
        if kids and not before:
            net, _ = self.evaluate(self.own[i], self.opp[i], self.player[i])
            legal = np.asarray(net, np.float32)[[self.action[k] for k in kids]]
            tot = legal.sum()
            noised = i == self.root and self.eps > 0
            kind = "zero" if not legal.any() else ("tiny" if tot <= 1e-12 else "normal")
            self.seen["expand_" + kind] += 1
            if noised:
                self.seen["noised_root_net_" + kind] += 1
            else:
                got = np.array([self.prior[k] for k in kids], np.float32)
                if kind == "normal":
                    assert abs(float(got.sum()) - 1.0) < 1e-5
                else:  # below the threshold the children keep the net's priors as they are
                    assert (got == legal).all()
            if len(kids) == 1 and self.action[kids[0]] == 64:
                self.seen["pass_node"] += 1
        self.seen[f"leaf_value_{v:+.0f}" if v in (1.0, -1.0, 0.0) else "leaf_value_other"] += 1
        return v

    def _tie(self, i, vv=None):
        kids = self.kids[i]
        vv = vv or {}
        sc = ucb_scores([self.prior[k] for k in kids], [self.N[k] for k in kids],
                        [self.W[k] for k in kids], self.N[i], self.c_puct,
                        1 + vv.get(i, 0), [vv.get(k, 0) for k in kids])
        if sum(s == max(sc) for s in sc) >= 2:
            self.seen["tie" if self.K == 1 else "tie_vl"] += 1
            if all(s == sc[0] for s in sc):
                self.seen["tie_all"] += 1

    def _select(self, i):
        self._tie(i)
        return super()._select(i)

    def _select_vl(self, i, vv):
        self._tie(i, vv)
        return super()._select_vl(i, vv)

    def _backup(self, i, v):
        if self.term[i]:
            self.seen["terminal_backup"] += 1
        super()._backup(i, v)


@functools.lru_cache(maxsize=None)
def census():
    """Replays every mcts_sharp* case (asserting each against the reference's record) and
    returns what the oracle met, per fixture."""
    out = {}
    for name, n, replay in (("mcts_sharp_cases.npz", N_CASES, replay_case),
                            ("mcts_sharp_vl_cases.npz", N_VL_CASES, replay_vl_case)):
        d = load_golden(name)
        assert int(d["n_cases"]) == n
        tot = Counter()
        for c in range(n):
            tot += replay(d, c, SharpPolicy(), Census).seen
        out[name] = tot
    return out


def test_oracle_replays_every_sharp_search_exactly():
    """Counts, root value, probs and root N of all 84 searches (replay_case / replay_vl_case
    assert them), with every recorded draw consumed."""
    census()
    d, v = load_golden("mcts_sharp_cases.npz"), load_golden("mcts_sharp_vl_cases.npz")
    assert len(d["pos"]) == 2 * N_CASES and len(v["pos"]) == 2 * N_VL_CASES
    assert (v["k"] == 4).all()
    assert sorted(set(zip(d["sims"], d["c_puct"], d["eps"], d["temp"]))) == \
        [(25, 2.0, 0.3, 1.0), (100, 1.0, 0.3, 1.0), (100, 2.0, 0.0, 0.0), (200, 2.0, 0.0, 1.0)]
    assert sorted(set(zip(v["sims"], v["c_puct"], v["eps"]))) == [(100, 1.0, 0.0), (100, 2.0, 0.3)]


@pytest.mark.parametrize("game", [0, 1, 2, 3])
def test_sharp_selfplay_games_match_reference(game):
    d = load_golden("selfplay_sharp.npz")
    assert [tuple(m[[0, 3]]) for m in d["meta"]] == [(25, 1), (25, 1), (100, 1), (25, 4)]
    sims, seed, plies, K = d["meta"][game]
    lo, hi = d["log_offsets"][game], d["log_offsets"][game + 1]
    nlo, nhi = d["noise_offsets"][game], d["noise_offsets"][game + 1]
    rng = LogRng(d["log_kind"][lo:hi], d["log_a"][lo:hi], d["log_b"][lo:hi],
                 d["noise"][nlo:nhi])
    mp = SharpPolicy()

    def evaluate(own, opp, player):
        return mp.inference(ob.to_state(own, opp, player), player)

    samples, _ = play_game(dict(SELFPLAY_ARGS, num_simulations=int(sims)), evaluate, rng=rng,
                           leaves_per_step=int(K))
    assert rng.i == len(rng.kinds)
    sel = d["game"] == game
    assert len(samples) == plies == sel.sum()
    for t, (s, pi, z) in enumerate(samples):
        pos, neg = ob.to_bitboards(s, 1)
        assert pos == d["pos"][sel][t] and neg == d["neg"][sel][t]
        assert (pi.astype(np.float32) == d["pi"][sel][t]).all()
        assert z == d["z"][sel][t]


# ---- the census --------------------------------------------------------------------------
# What the oracle met in the searches of each fixture, counted once from the generator's
# output and fixed here; a regenerated fixture that reaches less fails the conditions below
# before it fails these.
CENSUS = {
    "mcts_sharp_cases.npz": {
        "expand_normal": 4121, "expand_tiny": 520, "expand_zero": 207,
        "leaf_value_+0": 1297, "leaf_value_+1": 1206, "leaf_value_-1": 1218,
        "leaf_value_other": 1127, "noised_root_net_normal": 12, "noised_root_net_tiny": 2,
        "pass_node": 24, "terminal_backup": 1130, "tie": 1135, "tie_all": 112},
    "mcts_sharp_vl_cases.npz": {
        "expand_normal": 1981, "expand_tiny": 238, "expand_zero": 89,
        "leaf_value_+0": 673, "leaf_value_+1": 544, "leaf_value_-1": 580,
        "leaf_value_other": 511, "noised_root_net_normal": 6, "noised_root_net_tiny": 1,
        "pass_node": 4, "terminal_backup": 418, "tie_all": 43, "tie_vl": 595},
}


@pytest.mark.parametrize("name", sorted(CENSUS))
def test_census_of_the_sharp_fixtures(name):
    """Each fixture on its own reaches, by the net's legal priors of every expansion
    (before the root's noise) and by ucb_scores recomputed at every selection:

      * >= 50 expansions with every legal prior exactly 0, and >= 50 with a non-zero sum at
        or below 1e-12 -- both sides of the reference's `if tot > 1e-12` are taken, in float32;
      * a Dirichlet-noised root whose net priors are of the second kind: the float64 noise
        path runs over net priors that stay far below the noise;
      * >= 50 selections whose maximal PUCT score two or more children share (K = 1: `tie`,
        the K = 4 virtual-loss schedule: `tie_vl`), some with every child tied;
      * leaf values of exactly +1, -1 and 0 backed up >= 50 times each;
      * terminal nodes backed up and pass nodes expanded."""
    seen = census()[name]
    assert seen["expand_zero"] >= 50 and seen["expand_tiny"] >= 50
    assert seen["noised_root_net_tiny"] >= 1
    assert seen["tie"] + seen["tie_vl"] >= 50 and seen["tie_all"] >= 1
    assert min(seen["leaf_value_+1"], seen["leaf_value_-1"], seen["leaf_value_+0"]) >= 50
    assert seen["terminal_backup"] >= 1 and seen["pass_node"] >= 1
    assert dict(seen) == CENSUS[name]


def test_sharp_selfplay_has_saturated_targets():
    """The self-play fixture holds TD(lambda) targets of exactly +-1 (a decided game's last
    row), and its pi rows are as sharp as the priors make them."""
    d = load_golden("selfplay_sharp.npz")
    assert (np.abs(d["z"]) == 1.0).sum() >= 1
    assert (np.abs(d["z"]) <= 1.0).all()
    # pi rows are as sharp as the priors make them: most rows put all visits on few moves
    assert ((d["pi"] > 0).sum(1) <= 3).mean() > 0.25


# ---- the whole-tree cases under the sharp policy (tests/test_engine_tree_gpu.py) -----------

def _groups_of(t):
    """(zero, tiny) sibling groups of a tree: every child prior exactly 0 / a non-zero sum at
    or below the threshold."""
    zero = tiny = 0
    for kids in t.kids:
        if kids:
            pr = np.array([float(t.prior[k]) for k in kids])
            zero += not pr.any()
            tiny += bool(pr.any()) and pr.sum() <= 1e-12
    return zero, tiny


def test_sharp_tree_cases_reach_what_they_are_for():
    import tree_cases as tc

    for p in tc.ROOMY_PARAMS:
        script = tc.roomy_script_sharp(*p)
        assert script is not tc.roomy_script(*p)
        zero = tiny = 0
        for steps in script:
            assert [s.kind for s in steps] == ["search", "move"] * 3 + ["search"]
            assert all(s.overflows == 0 for s in steps)
            z, t = _groups_of(steps[-1].tree)
            zero, tiny = zero + z, tiny + t
        assert zero >= 5 and tiny >= 5, p
    for K, sims in tc.OVERFLOW_PARAMS_SHARP:
        near, full, _ = tc.overflow_script_sharp(K, sims)
        first, _, second = full
        assert first.overflows >= 1 and second.overflows > first.overflows
        assert all(tc.CAPACITY - 33 < len(s.tree.own) <= tc.CAPACITY for s in (first, second))
        assert first.tree.N[0] == sims + 1
        # the neighbours' unbounded trees fit the arena: no expansion of theirs is refused
        assert all(s.overflows == 0 and len(s.tree.own) <= tc.CAPACITY for s in near)
