"""Whole-tree parity: the cases, their oracle trees, and the comparison.

tests/test_oracle_capacity_cpu.py shows on the oracle alone that the cases reach what they
are meant to reach (overflowing and roomy arenas, terminal and pass nodes, an overflowed
leaf chosen again); tests/test_engine_tree_gpu.py replays the same scripts on the engine
and compares every node.  The oracle runs once per case (lru_cache) and its snapshots are
shared, never modified.

A script is, per slot, a list of Steps: a search of `arg` simulations or a re-root on
action `arg`, each with a snapshot of the oracle's whole tree after it and the oracle's
overflow count so far.
"""
import functools
from collections import namedtuple

import numpy as np

from conftest import load_golden
from mock_policy import mock_eval, sharp_eval
from oracle.mcts import SeqMCTS

INIT_OWN, INIT_OPP = 0x0000000810000000, 0x0000001008000000
CAPACITY = 128  # the smallest node arena the engine accepts
NOISE_SLOTS = 4  # root expansions a slot can see: the first search and one per re-root

# (leaves per step, c_puct, dirichlet_epsilon)
ROOMY_PARAMS = [(K, c, eps) for K in (1, 4) for c in (2.0, 1.0) for eps in (0.0, 0.25)]
ROOMY_SCHEDULE = (120, 60, 60, 60)  # three re-roots: both arena halves and back
# board_corpus.npz (game, ply): a midgame position, and a late one (10 empties) whose tree
# holds terminal nodes and pass nodes within these searches (test_oracle_capacity_cpu.py)
MID_ROOT = (1, 11)
LATE_ROOT = (0, 54)
# (leaves per step, simulations of the overflowing slot); its neighbours search 10
OVERFLOW_PARAMS = [(K, S) for K in (1, 4) for S in (40, 120, 300)]
NEIGHBOUR_SIMS = 10
# the same under the sharp policy (mock_policy.sharp_eval: zero, tiny and equal priors, +-1 values)
OVERFLOW_PARAMS_SHARP = [(1, 120), (4, 120)]

Step = namedtuple("Step", "kind arg tree overflows")
_FIELDS = ("own", "opp", "legal", "N", "W", "prior", "action", "term", "tval")
_BITS = np.arange(64, dtype=np.uint64)


class Tree:
    """A frozen copy of a SeqMCTS tree (what assert_same_tree reads)."""

    def __init__(self, o):
        for f in _FIELDS:
            setattr(self, f, list(getattr(o, f)))
        self.kids = [list(k) for k in o.kids]
        self.root = o.root

    def counts(self):
        c = np.zeros(65, np.int64)
        for k in self.kids[self.root]:
            c[self.action[k]] = self.N[k]
        return c

    def vroot(self):
        r = self.root
        return 0.0 if self.N[r] == 0 else self.W[r] / self.N[r]


def _canon(own, opp):
    return (((np.uint64(own) >> _BITS) & np.uint64(1)).astype(np.int64)
            - ((np.uint64(opp) >> _BITS) & np.uint64(1)).astype(np.int64))


def evaluate(own, opp, player):
    """The mock policy on the canonical board (own stones +1), as the engine's rows see it."""
    p, v = mock_eval(_canon(own, opp))
    return p.astype(np.float32), float(v)


def evaluate_sharp(own, opp, player):
    """The sharp policy, the same way."""
    p, v = sharp_eval(_canon(own, opp))
    return p.astype(np.float32), float(v)


class NoiseRng:
    """Hands the oracle the Dirichlet vectors the engine gets through az_inject, in order."""

    def __init__(self, vectors):
        self.vectors, self.used = vectors, 0

    def dirichlet(self, alpha, n):
        v = np.array(self.vectors[self.used], np.float64)
        assert len(v) == n
        self.used += 1
        return v

    def choice_tie(self, best):
        return best[0]


def noise_vectors(slot):
    return np.random.default_rng(1000 + slot).dirichlet([1.0] * 65, size=NOISE_SLOTS)


@functools.lru_cache(maxsize=None)
def corpus_root(game, ply):
    d = load_golden("board_corpus.npz")
    i = np.nonzero((d["game"] == game) & (d["ply"] == ply))[0][0]
    player = int(d["player"][i])
    pos, neg = int(d["pos"][i]), int(d["neg"][i])
    return (pos, neg, player) if player == 1 else (neg, pos, player)


def roomy_roots():
    return [(INIT_OWN, INIT_OPP, 1), corpus_root(*MID_ROOT), corpus_root(*LATE_ROOT)]


def pick_move(o):
    """argmax of the root's child visit counts (lowest action on ties), never a terminal
    child: the game would be over and the reference never re-roots onto it.  None if every
    child is terminal."""
    best = None
    for k in o.kids[o.root]:
        if not o.term[k] and (best is None or o.N[k] > o.N[best]):
            best = k
    return None if best is None else o.action[best]


def run_schedule(o, root, schedule):
    own, opp, player = root
    steps = []
    for j, sims in enumerate(schedule):
        if j:
            a = pick_move(o)
            if a is None:
                break
            o.make_move(a)
            steps.append(Step("move", a, Tree(o), o.overflows))
            own, opp, player = o.own[o.root], o.opp[o.root], o.player[o.root]
        o.sims = sims
        o.search(own, opp, player)
        steps.append(Step("search", sims, Tree(o), o.overflows))
    return steps


@functools.lru_cache(maxsize=None)
def roomy_script(K, c_puct, eps, evaluate=evaluate):
    """Per root of roomy_roots(): its Steps under ROOMY_SCHEDULE."""
    out = []
    for slot, root in enumerate(roomy_roots()):
        o = SeqMCTS(c_puct, 0, evaluate, dirichlet_alpha=1.0, dirichlet_epsilon=eps,
                    rng=NoiseRng(noise_vectors(slot)), leaves_per_step=K)
        out.append(run_schedule(o, root, ROOMY_SCHEDULE))
    return out


def roomy_script_sharp(K, c_puct, eps):
    """roomy_script with the sharp policy: the same roots, noise and schedule."""
    return roomy_script(K, c_puct, eps, evaluate_sharp)


@functools.lru_cache(maxsize=None)
def overflow_script(K, sims, evaluate=evaluate):
    """Three slots from the initial position: slot 1 searches `sims` twice (one re-root
    between) in a CAPACITY-node arena, slots 0 and 2 search NEIGHBOUR_SIMS in the reference's
    unbounded tree (which CAPACITY nodes hold with room to spare)."""
    root = (INIT_OWN, INIT_OPP, 1)
    near = run_schedule(SeqMCTS(2.0, 0, evaluate, leaves_per_step=K), root,
                        (NEIGHBOUR_SIMS, NEIGHBOUR_SIMS))
    full = run_schedule(SeqMCTS(2.0, 0, evaluate, leaves_per_step=K, node_capacity=CAPACITY),
                        root, (sims, sims))
    return [near, full, near]


def overflow_script_sharp(K, sims):
    """overflow_script with the sharp policy."""
    return overflow_script(K, sims, evaluate_sharp)


def export_of(tree):
    """An oracle tree in az_export_tree's layout (Engine.export_tree's dict).  The oracle keeps
    node 0 as the root and every sibling group contiguous and ascending, as the engine does,
    so the node order carries over."""
    n = len(tree.own)
    assert tree.root == 0
    t = {"own": np.array(tree.own, np.uint64), "opp": np.array(tree.opp, np.uint64),
         "legal": np.array(tree.legal, np.uint64), "N": np.array(tree.N, np.int32),
         "W": np.array(tree.W, np.float64),
         "prior": np.array([float(x) for x in tree.prior], np.float64),
         "parent": np.full(n, -1, np.int32), "first": np.full(n, -1, np.int32),
         "nchild": np.zeros(n, np.uint8), "action": np.zeros(n, np.uint8),
         "flags": np.zeros(n, np.uint8), "tval": np.array(tree.tval, np.int8), "n_nodes": n}
    for i, kids in enumerate(tree.kids):
        if tree.term[i]:
            t["flags"][i] |= 2
        if i:
            t["action"][i] = tree.action[i]
        if kids:
            assert kids == list(range(kids[0], kids[0] + len(kids)))
            t["first"][i], t["nchild"][i] = kids[0], len(kids)
            t["flags"][i] |= 1 | (4 if isinstance(tree.prior[kids[0]], np.float64) else 0)
            t["parent"][kids] = i
    return t


def _path(o, i, parent):
    acts = []
    while i != o.root:
        acts.append(int(o.action[i]))
        i = parent[i]
    return acts[::-1]


def assert_same_tree(t, o, where=""):
    """The engine's exported tree `t` (Engine.export_tree) against the oracle tree `o` (a
    SeqMCTS or a Tree), node for node from the root, children matched by action.  Exact:
    boards, legal masks, N, W (the backups add the same doubles in the same order), priors,
    actions, child counts, the expanded / terminal / float64-children flags and terminal
    values.  The root's own prior, action and parent are left out (the reference never reads
    them).  Of the export itself: children contiguous from `first` and ascending in action,
    parent links pointing back, and exactly n_nodes nodes reachable -- the arena holds no
    garbage and lost nothing.  Returns n_nodes."""
    n = int(t["n_nodes"])
    assert n == len(o.own), f"{where}: {n} nodes, the oracle has {len(o.own)}"
    for k in ("own", "opp", "legal", "N", "W", "prior", "parent", "first", "nchild", "action",
              "flags", "tval"):
        assert len(t[k]) == n, f"{where}: {k} exported {len(t[k])} of {n} nodes"
    emap = np.full(n, -1, np.int64)  # oracle node -> engine node
    oparent = np.full(n, -1, np.int64)
    emap[o.root] = 0
    stack = [o.root]
    reached = 1
    while stack:
        oi = stack.pop()
        ei = int(emap[oi])
        kids = o.kids[oi]
        at = f"{where}: node {ei} (actions {_path(o, oi, oparent)})"
        assert int(t["nchild"][ei]) == len(kids), f"{at}: nchild {t['nchild'][ei]}, want {len(kids)}"
        assert bool(t["flags"][ei] & 1) == bool(kids), f"{at}: expanded flag"
        if not kids:
            continue
        fc, nc = int(t["first"][ei]), len(kids)
        assert 1 <= fc and fc + nc <= n, f"{at}: children {fc}..{fc + nc} outside the tree"
        acts = t["action"][fc:fc + nc].astype(np.int64)
        assert (np.diff(acts) > 0).all(), f"{at}: children not ascending in action: {acts}"
        assert acts.tolist() == [int(o.action[k]) for k in kids], f"{at}: child actions {acts}"
        assert (t["parent"][fc:fc + nc] == ei).all(), f"{at}: children's parent links"
        for j, k in enumerate(kids):
            assert emap[k] < 0
            emap[k] = fc + j
            oparent[k] = oi
        stack.extend(kids)
        reached += nc
    assert reached == n and len(set(emap.tolist())) == n, \
        f"{where}: {reached} nodes reached from the root, n_nodes {n}"

    def same(name, got, want, skip_root=False):
        bad = np.asarray(got)[emap] != np.asarray(want)
        if skip_root:
            bad[o.root] = False
        if bad.any():
            i = int(np.flatnonzero(bad)[0])
            raise AssertionError(
                f"{where}: {name} differs at {int(bad.sum())} nodes, first at node {emap[i]} "
                f"(actions {_path(o, i, oparent)}): {np.asarray(got)[emap[i]]!r}, "
                f"want {np.asarray(want)[i]!r}")

    flags = np.asarray(t["flags"])
    same("own", t["own"], np.array(o.own, np.uint64))
    same("opp", t["opp"], np.array(o.opp, np.uint64))
    same("legal", t["legal"], np.array(o.legal, np.uint64))
    same("N", t["N"], np.array(o.N, np.int64))
    same("W", np.asarray(t["W"], np.float64), np.array([float(w) for w in o.W], np.float64))
    same("prior", np.asarray(t["prior"], np.float64),
         np.array([float(x) for x in o.prior], np.float64), skip_root=True)
    same("action", t["action"], np.array([0 if a is None else int(a) for a in o.action]),
         skip_root=True)
    same("terminal flag", (flags & 2) != 0, np.array(o.term, bool))
    same("tval", t["tval"], np.array(o.tval, np.int64))
    f64 = np.array([bool(k) and isinstance(o.prior[k[0]], np.float64) for k in o.kids], bool)
    same("float64-children flag", (flags & 4) != 0, f64)
    assert not f64.any() or (f64[o.root] and f64.sum() == 1), f"{where}: noise below the root"
    assert not (flags & ~np.uint8(7)).any(), f"{where}: unknown flag bits"
    return n
