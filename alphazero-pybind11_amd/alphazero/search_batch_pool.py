"""MCTSBatch's frozen evaluation set (azmi_search_set_capture / _capture_roots / _captured / _net_metrics, azmi_pool_unique; the
host's search_batch_pool.hip): the methods of `_Pool`, which MCTSBatch (search_batch.py) is built on, and pool_unique.

A frozen evaluation set (frozen_eval.py:330-413, 541-672): with `capture=True` (set_capture(), play(..., capture=)) every
move of play() records the root of every live tree before its search, one launch more per move and none with capture off;
position_pool() keeps the first record of every engine key in (tree, ply) order (pool_unique on the device),
pool_states() / sample_pool() turn the pool back into GameStates and the reference's records, and net_vs_search(net)
compares every root's search with one raw forward of the net on the device.  The search and play kernels are unchanged."""
import ctypes as C

import numpy as np

from ._capi import lib, check
from .mcts import _ENGINE_STREAM


def pool_unique(keys, valid=None, device=0):
    """First occurrences on the device (azmi_pool_unique): of the records with valid[i] (default: all), the ascending indices i
    such that no valid j < i has keys[j] == keys[i] - the sorted `return_index` of np.unique over the valid subset, and what the
    `seen_keys` set of frozen_eval.py:367-378 keeps.  Every uint64 is a key, 0 included; the result does not depend on
    scheduling.  -> (first_index uint32 [n_unique], n_duplicates)"""
    k = np.ascontiguousarray(keys, dtype=np.uint64)
    if k.ndim != 1:
        raise RuntimeError(f"pool_unique: keys must be one-dimensional, got shape {k.shape}")
    v = None
    if valid is not None:
        v = np.ascontiguousarray(valid).astype(np.uint8)
        if v.shape != k.shape:
            raise RuntimeError(f"pool_unique: one valid flag per key ({k.shape[0]}), got {v.shape}")
    out = np.zeros(max(k.size, 1), np.uint32)
    nu, nd = C.c_uint32(), C.c_uint32()
    check(lib.azmi_pool_unique(k.ctypes.data if k.size else None, None if v is None or not k.size else v.ctypes.data, int(k.size),
                               out.ctypes.data, C.byref(nu), C.byref(nd), int(device), None))
    return out[: nu.value].copy(), int(nd.value)


class _Pool:
    """The capture, pool and net-versus-search methods of MCTSBatch, the one class built on this one: the fields are those of
    MCTSBatch.__init__, and move_logs() is found on it."""

    def set_capture(self, on):
        """With capture on, play() records the root of every live tree before each move's search - engine key
        (hash_game_state), player to move, variant - at [tree][ply]; capture_roots() does it for a caller that walks the
        moves itself.  The arrays are allocated the first time capture is turned on; reset() forgets what was captured."""
        check(lib.azmi_search_set_capture(self._h, int(bool(on))))
        self._capture = bool(on)

    def capture_roots(self):
        """Record the current root of every live tree (one launch): what play() does before each move's search."""
        check(lib.azmi_search_capture_roots(self._h, _ENGINE_STREAM))

    def position_pool(self):
        """The captured roots without repeats: the first record of every engine key, in (tree, ply) order - the order in
        which the reference's capture loop would have met them, had it played tree 0's game, then tree 1's, and so on
        (frozen_eval.py:362-378).  Equal keys are what the position cache serves one answer for.
        -> dict: tree, ply (uint32), key (uint64), player (uint8), variant (int8; -1 for a game without variants), one entry
        per kept position; captured (records seen) and duplicates (records left out), ints.  Synchronises."""
        cap = self._game.MAX_TURNS + 8
        key = np.zeros((self._n, cap), np.uint64); player = np.zeros((self._n, cap), np.uint8)
        variant = np.zeros((self._n, cap), np.int8); length = np.zeros(self._n, np.uint32)
        check(lib.azmi_search_captured(self._h, key.ctypes.data, player.ctypes.data, variant.ctypes.data, length.ctypes.data))
        valid = np.arange(cap, dtype=np.uint32)[None, :] < length[:, None]
        first, dups = pool_unique(key.reshape(-1), valid.reshape(-1), self._device)
        return dict(tree=(first // cap).astype(np.uint32), ply=(first % cap).astype(np.uint32), key=key.reshape(-1)[first],
                    player=player.reshape(-1)[first], variant=variant.reshape(-1)[first], captured=int(valid.sum()), duplicates=dups)

    def pool_states(self, pool, indices=None):
        """The GameStates of a position_pool() (entries `indices`, default all): the tree's reset() state + the first `ply`
        moves of its log, as states() builds the roots.  Valid until the next reset()."""
        if self._start is None:
            raise RuntimeError("pool_states: the trees have no positions; call reset first")
        logs = self.move_logs()
        out = []
        for j in (range(len(pool["tree"])) if indices is None else indices):
            t, p = int(pool["tree"][j]), int(pool["ply"][j])
            if p > len(logs[t]):
                raise RuntimeError(f"pool_states: entry {j} is ply {p} of tree {t}, which has played {len(logs[t])} moves since reset")
            g = self._start[t].copy()
            g._moves.extend(int(m) for m in logs[t][:p])
            g._snap = None
            out.append(g)
        return out

    def sample_pool(self, pool, k, rng=None):
        """At most k positions of a position_pool(), drawn as frozen_eval.py:410-413 draws them - rng.choice(len, size=k,
        replace=False) (rng: a numpy Generator or RandomState, default np.random), everything when len <= k -> the
        reference's records {"gs", "variant", "move_number", "player"}."""
        n = len(pool["tree"])
        idx = range(n) if n <= int(k) else [int(i) for i in (np.random if rng is None else rng).choice(n, size=int(k), replace=False)]
        idx = list(idx)
        return [{"gs": g, "variant": int(pool["variant"][j]), "move_number": int(pool["ply"][j]), "player": int(pool["player"][j])}
                for j, g in zip(idx, self.pool_states(pool, idx))]

    def net_vs_search(self, net):
        """The metric extraction of frozen_eval.py:573-575, 649-672 on the device: one raw forward of `net` over the roots'
        canonical planes, then per tree, in float64, kl_mcts_net = KL(counts / total || raw_pi + 1e-10) (uniform 1 / M for a
        root without visits), value_mae = mean |raw_v - root_value|, top1_agreement = 1.0 when the arg-maxes of counts and
        raw_pi agree.  Three launches, one synchronisation.
        -> dict: kl_mcts_net, value_mae, top1_agreement float64 [n]; raw_v [n, P+1], raw_pi [n, M] float32; valid bool [n];
        mean: the three means over the valid trees.  A finished or stopped tree and a tree whose root is terminal take no
        part: valid False, NaN everywhere."""
        if net.desc.num_moves != self._M or (net.desc.in_channels, net.desc.height, net.desc.width) != self._chw:
            raise RuntimeError("net_vs_search: the net's shape does not match the game")
        out = np.zeros((self._n, 3), np.float64)
        raw_v = np.zeros((self._n, self._P + 1), np.float32); raw_pi = np.zeros((self._n, self._M), np.float32)
        valid = np.zeros(self._n, np.uint8)
        check(lib.azmi_search_net_metrics(self._h, net._h, out.ctypes.data, raw_v.ctypes.data, raw_pi.ctypes.data, valid.ctypes.data,
                                          _ENGINE_STREAM))
        ok = valid.astype(bool)
        names = ("kl_mcts_net", "value_mae", "top1_agreement")
        res = {k: out[:, i].copy() for i, k in enumerate(names)}
        res.update(raw_v=raw_v, raw_pi=raw_pi, valid=ok,
                   mean={k: (float(res[k][ok].mean()) if ok.any() else float("nan")) for k in names})
        return res
