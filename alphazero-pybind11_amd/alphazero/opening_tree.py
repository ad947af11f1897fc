"""Opening trees by reach probability (the reference's opening_analysis.py build_tree), level by level on one MCTSBatch."""
import math

import numpy as np

from . import _args
from ._rng import MASK64, mix64
from .games import GameState, hash_game_state
from .search_batch import MCTSBatch, _evaluator


def temperature_at_depth(depth, start_temp=1.0, final_temp=0.2, half_life=10):
    """The sampling temperature `depth` plies from the root (opening_analysis.py:167-172): exponential decay from start_temp to
    final_temp, ln 2 taken as 0.693 as the reference does."""
    ld = 0.693 / max(1, half_life)
    return final_temp + (start_temp - final_temp) * math.exp(-ld * depth)


def node_seed(seed, b):
    """The tree seed of node b (BFS index, root 0) of build_opening_tree(..., seed=seed): MCTS(..., seed=node_seed(seed, b)) searched
    from tree.state(b) is that node's stand-alone twin."""
    return mix64((int(seed) + int(b)) & MASK64)


class OpeningNode:
    """One position of an opening tree, with the field names of the reference's TreeNode (opening_analysis.py:146-159)."""
    __slots__ = ("state_hash", "depth", "incoming_action", "reach_prob", "sampling_pi", "raw_pi", "value", "entropy", "is_terminal",
                 "children", "state")


class OpeningTree:
    """The result of build_opening_tree: flat arrays indexed by BFS order (root 0), children of a node neighbours in ascending
    action order.  parent int32 (-1: root), depth, incoming_action int32 (-1: root), reach_prob, state_hash uint64, is_terminal,
    searched (False: a terminal node or one at max_depth, whose policies are empty in nodes() and zero rows here), entropy,
    value [., 3], raw_pi / sampling_pi [., M], children [., 2] (index of the first child, count).  stats: levels, chunks,
    host_reads."""

    def __init__(self, start, moves, arrays, stats):
        self._start, self._moves = start, moves
        self.__dict__.update(arrays)
        self.stats = stats

    def __len__(self):
        return len(self.parent)

    def state(self, b):
        """The GameState of node b: the start state's copy with the node's actions appended (play_move is never called)."""
        g = self._start.copy()
        g._moves.extend(self._moves[b])
        g._snap = None
        return g

    def nodes(self):
        """The root as nested objects (children: action -> node) that the reference's extract_openings can walk."""
        out = [None] * len(self)
        for b in range(len(self) - 1, -1, -1):
            nd = OpeningNode()
            live = bool(self.searched[b])
            nd.state_hash, nd.depth = int(self.state_hash[b]), int(self.depth[b])
            nd.incoming_action = None if b == 0 else int(self.incoming_action[b])
            nd.reach_prob = float(self.reach_prob[b])
            nd.sampling_pi = self.sampling_pi[b].copy() if live else np.zeros(0)
            nd.raw_pi = self.raw_pi[b].copy() if live else np.zeros(0)
            nd.value, nd.entropy, nd.is_terminal = self.value[b].copy(), float(self.entropy[b]), bool(self.is_terminal[b])
            first, count = (int(x) for x in self.children[b])
            nd.children = {int(self.incoming_action[c]): out[c] for c in range(first, first + count)}
            nd.state = self.state(b)
            out[b] = nd
        return out[0]


def _tree_args(game, start_state, sims, evaluator, net, cache, start_temp, final_temp, half_life, min_reach, batch, seed, max_depth, mcts_args):
    """every argument error of build_opening_tree, by name, before any device call -> (game class, EvalType)"""
    what = "build_opening_tree"
    game = game if isinstance(game, type) else type(game)
    if not (isinstance(game, type) and issubclass(game, GameState)) or game.GAME_ID < 0:
        raise RuntimeError(f"{what}: game must be a game class or a state of one, got {game!r}")
    if getattr(start_state, "GAME_ID", None) != game.GAME_ID:
        raise RuntimeError(f"{what}: start_state must be a state of the tree's game")
    _args.integer(sims, f"{what}: sims must be an integer >= 1, got {sims!r}", 1)
    _args.integer(batch, f"{what}: batch must be an integer >= 1, got {batch!r}", 1)
    _args.integer(max_depth, f"{what}: max_depth must be an integer >= 0, got {max_depth!r}", 0)
    _args.integer(seed, f"{what}: seed must be an integer, got {seed!r}")
    _args.number(min_reach, f"{what}: min_reach must be a finite positive number, got {min_reach!r}", positive=True)
    for name, v in (("start_temp", start_temp), ("final_temp", final_temp), ("half_life", half_life)):
        _args.number(v, f"{what}: {name} must be a finite non-negative number, got {v!r}")
    for name in ("max_simulations", "seeds", "capture", "n", "game"):
        if name in mcts_args:
            raise RuntimeError(f"{what}: {name} is set by the builder (one MCTSBatch of `batch` trees with max_simulations = sims, "
                               "node b searched with seed node_seed(seed, b))")
    return game, _evaluator(what, evaluator, net, cache)


def build_opening_tree(game, start_state, sims, net=None, cache=None, evaluator=None, start_temp=1.0, final_temp=0.2, half_life=10,
                       min_reach=0.01, batch=256, seed=0, max_depth=1000, **mcts_args):
    """The reference's opening tree (opening_analysis.py build_tree, :261-355) breadth first on one MCTSBatch: every position is
    searched with `sims` simulations, the counts become the distribution self-play samples from (temperature_at_depth(depth); on
    a Gumbel batch the improved policy at temperature 1), and every move whose reach probability reach * p is at least
    `min_reach` is followed - no top-K and, up to `max_depth`, no depth limit.  Transpositions stay separate nodes.
    A level's frontier is cut into chunks of `batch` positions; a chunk is one reset(), one search(sims) and one
    expand_frontier(), whose read-out is the only host read of the tree's data (the last chunk of a level is padded with the start
    state at reach 0).  Children are appended in (parent's BFS index, action) order.  A terminal child is a node with value =
    scores(), is_terminal True, and is never searched; so is a node at max_depth, with a zero value and is_terminal False.
    Node b is searched by the tree seed node_seed(seed, b), so the result does not depend on `batch`.
    net / cache / evaluator: MCTSBatch.search()'s.  **mcts_args: MCTSBatch's search arguments (cpuct, default 1.25, epsilon,
    fpu_reduction, gumbel_enabled, ..., device, leaves_per_step, descents_per_step).  -> OpeningTree"""
    game, ev = _tree_args(game, start_state, sims, evaluator, net, cache, start_temp, final_temp, half_life, min_reach, batch, seed,
                          max_depth, mcts_args)
    P, M, _ = game._info()
    mcts_args = dict(mcts_args)
    cpuct = mcts_args.pop("cpuct", 1.25)
    gumbel = bool(mcts_args.get("gumbel_enabled", False))
    start = start_state.copy()
    zero_pi = np.zeros(M, np.float64)
    # node columns, appended in BFS order
    parent, depth, action, reach, hashes, terminal, searched = [-1], [0], [-1], [1.0], [0], [False], [False]
    entropy, value, raw_pi, samp_pi, children, moves = [0.0], [np.zeros(3)], [zero_pi], [zero_pi], [(0, 0)], [[]]
    stats = dict(levels=0, chunks=0, host_reads=0)
    frontier = [0] if max_depth > 0 else []
    if not frontier:
        hashes[0] = int(hash_game_state(start))
    mb = MCTSBatch(game, int(batch), cpuct, max_simulations=int(sims), **mcts_args) if frontier else None
    n = int(batch)
    while frontier:
        stats["levels"] += 1
        nxt = []
        for lo in range(0, len(frontier), n):
            chunk = frontier[lo: lo + n]
            pad = n - len(chunk)
            states = []
            for b in chunk:
                g = start.copy()
                g._moves.extend(moves[b])
                g._snap = None
                states.append(g)
            mb.reset(states + [start] * pad, seeds=[node_seed(seed, b) for b in chunk] + [0] * pad)
            mb.search(int(sims), net=net, cache=cache, evaluator=ev)
            temps = [1.0 if gumbel else temperature_at_depth(depth[b], start_temp, final_temp, half_life) for b in chunk]
            fr = mb.expand_frontier([reach[b] for b in chunk] + [0.0] * pad, temps + [1.0] * pad, min_reach)
            stats["chunks"] += 1
            stats["host_reads"] += 1
            for j, b in enumerate(chunk):
                kind = int(fr["kind"][j])
                if kind == 2:
                    raise RuntimeError(f"build_opening_tree: node {b} was not searched (its tree is finished or stopped)")
                hashes[b], value[b] = int(fr["key"][j]), fr["value"][j].copy()
                if kind == 1:      # (only the start state: a terminal child is never reset into a tree)
                    terminal[b] = True
                    continue
                searched[b], entropy[b] = True, float(fr["entropy"][j])
                raw_pi[b], samp_pi[b] = fr["raw_pi"][j].copy(), fr["sampling_pi"][j].copy()
                r0, r1 = int(fr["first_child"][j]), int(fr["first_child"][j + 1])
                children[b] = (len(parent), r1 - r0)
                for r in range(r0, r1):
                    c, a, term = len(parent), int(fr["action"][r]), bool(fr["child_terminal"][r])
                    parent.append(b); depth.append(depth[b] + 1); action.append(a); reach.append(float(fr["child_reach"][r]))
                    hashes.append(int(fr["child_key"][r])); terminal.append(term); searched.append(False)
                    entropy.append(0.0); value.append(fr["child_scores"][r].astype(np.float64) if term else np.zeros(P + 1))
                    raw_pi.append(zero_pi); samp_pi.append(zero_pi); children.append((0, 0)); moves.append(moves[b] + [a])
                    if not term and depth[c] < max_depth:
                        nxt.append(c)
        frontier = nxt
    arrays = dict(parent=np.array(parent, np.int32), depth=np.array(depth, np.int32), incoming_action=np.array(action, np.int32),
                  reach_prob=np.array(reach, np.float64), state_hash=np.array(hashes, np.uint64), is_terminal=np.array(terminal, bool),
                  searched=np.array(searched, bool), entropy=np.array(entropy, np.float64), value=np.stack(value).astype(np.float64),
                  raw_pi=np.stack(raw_pi), sampling_pi=np.stack(samp_pi), children=np.array(children, np.int64).reshape(-1, 2))
    return OpeningTree(start, moves, arrays, stats)
