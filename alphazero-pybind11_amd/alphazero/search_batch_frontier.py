"""MCTSBatch's opening-tree frontier (azmi_search_expand / azmi_search_frontier; the host's search_batch_frontier.hip): the
methods of `_Frontier`, which MCTSBatch (search_batch.py) is built on.

Opening trees: from n searched roots to the next level's frontier (opening_analysis.py:261-355).  See expand_frontier();
opening_tree.py builds whole trees with it, level by level."""
import numpy as np

from . import _args
from ._capi import lib, check
from .mcts import _ENGINE_STREAM


class _Frontier:
    """expand_frontier of MCTSBatch, the one class built on this one: the fields are those of MCTSBatch.__init__."""

    def _frontier_args(self, reach, temp, min_reach, max_children):
        """-> (reach float64 [n], temp float64 [n], min_reach, max_children); every argument error before any device call"""
        n = self._n
        try:
            r = np.ascontiguousarray(reach, dtype=np.float64)
        except (TypeError, ValueError):
            raise RuntimeError(f"expand_frontier: reach must be {n} numbers, got {reach!r}") from None
        if r.shape != (n,):
            raise RuntimeError(f"expand_frontier: reach: one per tree ({n}), got shape {r.shape}")
        if not np.all(np.isfinite(r)) or np.any(r < 0):
            raise RuntimeError("expand_frontier: reach must be finite and not negative")
        try:
            t = np.asarray(temp, dtype=np.float64)
        except (TypeError, ValueError):
            raise RuntimeError(f"expand_frontier: temp must be a number or {n} numbers, got {temp!r}") from None
        t = np.full(n, float(t), np.float64) if t.ndim == 0 else np.ascontiguousarray(t)
        if t.shape != (n,):
            raise RuntimeError(f"expand_frontier: temp: a number or one per tree ({n}), got shape {t.shape}")
        if not np.all(np.isfinite(t)) or np.any(t < 0):
            raise RuntimeError("expand_frontier: temp must be finite and not negative")
        min_reach = _args.number(min_reach, f"expand_frontier: min_reach must be a positive finite number, got {min_reach!r}", positive=True)
        if max_children is None:
            max_children = n * self._M
        max_children = _args.integer(max_children, f"expand_frontier: max_children must be an integer in [1, 2^32), got {max_children!r}",
                                     1, 0xFFFFFFFF)
        return r, t, min_reach, max_children

    def expand_frontier(self, reach, temp, min_reach, max_children=None):
        """The step between two levels of the reference's opening tree (opening_analysis.py build_tree, :261-355), for every tree
        at once on the device, in float64: the distribution self-play samples from at the searched root, the moves worth
        following, and the rules applied to every one of them.  `reach`: n reach probabilities; `temp`: a number or n of them.
        Per tree i: kind 0 a searched live root, 1 a terminal root (value = its scores, no children), 2 the tree takes no part
        (finished, stopped or reach[i] == 0: zero rows).  For kind 0, expression for expression: raw_pi = counts / total
        (uniform over the legal moves for a root without visits below it; on a Gumbel batch the improved policy over its
        float64 sum), sampling_pi = play.py's apply_temperature(raw_pi, temp[i]) (temp 0: one-hot at the first arg-max, 1:
        raw_pi itself, else (raw_pi + 1e-10) ** (1 / temp) over its sum), entropy = -sum p ln p over p > 0, value =
        root_values()[i], key = hash_game_state of the root.  Move a is kept when sampling_pi[a] > 0 and
        reach[i] * sampling_pi[a] >= min_reach and a is legal.  Three launches whatever n is, one synchronising read-out; no
        tree is changed, GameState.play_move is never called.
        -> dict.  Per tree: kind uint8 [n], key uint64 [n], raw_pi / sampling_pi float64 [n, M], entropy float64 [n], value
        float64 [n, 3], first_child uint32 [n + 1] (tree i's records are first_child[i] : first_child[i + 1]).  Per kept
        move, in (tree, action) order: parent, action uint32, child_reach float64, child_key uint64 (hash_game_state of the
        successor), child_player uint8, child_variant int8 (-1 for a game without variants), child_terminal bool,
        child_scores float32 [., P + 1] (scores() of a terminal successor, zeros otherwise).
        `max_children` (default n * M: always enough) is the room for records; when the trees keep more, RuntimeError names
        the total and the capacity, the batch stays usable and a call with room gives the full answer."""
        r, t, mr, cap = self._frontier_args(reach, temp, min_reach, max_children)
        n, M, V = self._n, self._M, self._P + 1
        check(lib.azmi_search_expand(self._h, r.ctypes.data, t.ctypes.data, mr, cap, _ENGINE_STREAM))
        out = dict(kind=np.zeros(n, np.uint8), key=np.zeros(n, np.uint64), raw_pi=np.zeros((n, M), np.float64),
                   sampling_pi=np.zeros((n, M), np.float64), entropy=np.zeros(n, np.float64), value=np.zeros((n, 3), np.float64),
                   first_child=np.zeros(n + 1, np.uint32))
        rec = dict(parent=np.empty(cap, np.uint32), action=np.empty(cap, np.uint32), child_reach=np.empty(cap, np.float64),
                   child_key=np.empty(cap, np.uint64), child_player=np.empty(cap, np.uint8), child_variant=np.empty(cap, np.int8),
                   child_terminal=np.empty(cap, np.uint8), child_scores=np.empty((cap, V), np.float32))
        check(lib.azmi_search_frontier(self._h, *(a.ctypes.data for a in out.values()), *(a.ctypes.data for a in rec.values())))
        total = int(out["first_child"][n])
        out.update({k: a[:total].copy() for k, a in rec.items()})
        out["child_terminal"] = out["child_terminal"].astype(bool)
        return out
