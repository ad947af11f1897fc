"""MCTSBatch: N independent search trees advanced together on the device (azmi_search_*)."""
import ctypes as C
import os

import numpy as np

from . import _capi
from ._capi import lib, check
from .games import StarGambitUnifiedGS
from .mcts import Query, _ENGINE_STREAM
from .params import EvalType


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


POLICY_COLUMNS = ("jsd", "tv", "hellinger", "top1", "top3", "top9")
SWEEP_COLUMNS = POLICY_COLUMNS + ("reward", "regret", "pressure", "benefit", "entropy", "value_gap", "abs_err", "closer_than_anchor",
                                  "closer_than_raw")      # the column order of azmi_search_sweep_metrics


def policy_divergences(p, q, device=0):
    """The six policy figures of policy_metrics.py for every row of two [rows, M] policy arrays, on the device
    (azmi_policy_divergences), in float64 from the float32 inputs: jsd, tv, hellinger and top1 / top3 / top9 =
    |top_k(p) & top_k(q)| / k.  top_k(x) is np.argsort(x, kind="stable")[-k:] - among equal values the higher index ranks
    higher; with M < k every index is in both sets and the divisor stays k.  A pair of one-dimensional arrays is one row.
    -> dict of six float64 [rows] arrays.  rows == 0 touches no device."""
    try:
        a = np.asarray(p, dtype=np.float32)
        b = np.asarray(q, dtype=np.float32)
    except (TypeError, ValueError):
        raise RuntimeError("policy_divergences: p and q must be arrays of numbers") from None
    if a.ndim == 1 and b.ndim == 1:
        a, b = a[None, :], b[None, :]
    if a.ndim != 2 or b.ndim != 2:
        raise RuntimeError(f"policy_divergences: p and q must be [rows, M] arrays, got shapes {a.shape} and {b.shape}")
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape:
        raise RuntimeError(f"policy_divergences: p and q must have one shape, got {a.shape} and {b.shape}")
    rows, M = a.shape
    if M < 1 or M > 1 << 20:
        raise RuntimeError(f"policy_divergences: M must be in [1, 2^20], got {M}")
    if rows > 1 << 30:
        raise RuntimeError(f"policy_divergences: at most 2^30 rows, got {rows}")
    if isinstance(device, bool) or not isinstance(device, (int, np.integer)) or device < 0:
        raise RuntimeError(f"policy_divergences: device must be a device index, got {device!r}")
    out = np.zeros((rows, len(POLICY_COLUMNS)), np.float64)
    check(lib.azmi_policy_divergences(a.ctypes.data if rows else None, b.ctypes.data if rows else None, rows, M,
                                      out.ctypes.data if rows else None, int(device), None))
    return {k: out[:, c].copy() for c, k in enumerate(POLICY_COLUMNS)}


class MCTSBatch:
    """N independent search trees on N positions of one game, advanced together on the device (azmi_search_*): the job of the
    reference's evaluation tools, which hold a list of MCTS objects, step them in lock step and batch the leaves into one net
    call (frozen_eval.py:545-660, mcts_analysis.py:923-1049, play.py:292-343).  Tree i is bit for bit the stand-alone
    `MCTS(..., seed=seeds[i])` driven call by call from states[i] with the same evaluator values.  The constructor takes the
    MCTS constructor's search arguments; `max_simulations` (required) sizes every tree's arena.  Read-outs return one row per tree.

    Moves are played on the device with tree reuse, the way the tools walk a game (play.py:274-346, mcts_analysis.py:995-1051):
    pick_moves(temp) is m.pick_move(m.probs(temp)) of every tree from its own stream (gumbel_final_action() for a Gumbel
    search), update_roots() is m.update_root(gs, move) + gs.play_move(move) on every tree, add_root_noise() /
    apply_root_policy_temp() are the object's, and play(visits, ..., max_moves=m) enqueues m x (search, pick, update_roots,
    root prior) without a host round trip - whole games in one call.  Tree i stays bit for bit the stand-alone MCTS driven by
    the same calls.  A tree whose game is over is finished(): it is skipped by every later step (its read-outs stay legal),
    takes no further move, and its result is final_scores()[i]; move_logs() / states() give the moves played since reset()
    and the current root states.  The budget: a Connect4 arena never reclaims, so `max_simulations` counts every descent
    since reset(), moves included (a game needs visits x moves); the wide games compact their arenas behind update_roots(),
    so it counts the descents since the last update_roots() that moved every tree.

    `leaves_per_step=K` (1 <= K <= 64, default 1) holds K leaves of every tree in flight per step (WU-UCT), for a few
    positions searched deeply: the net then sees up to n * K rows per call instead of n.  With K > 1 one step of tree i is

        for k in 0..K-1:                      # exactly K descents: a step is K simulations of every live tree
            leaf = find_leaf_batched(root)    # sees the in-flight marks of descents 0..k-1
            terminal leaf, RANDOM evaluator or cache hit: process_result_batched(k, ...) at once
            otherwise: the leaf's planes become one row of the step's batch
        evaluate all rows in one call
        for the pending k, ascending: process_result_batched(k, v, pi, root_noise)
        reset_batch()

    and tree i is bit for bit the stand-alone `MCTS(seed=seeds[i])` driven by those calls.  This is play.py's _run_one_batch
    with the attempt count fixed at K: the reference loops "until K misses or 2K attempts", which gives the trees of one
    batch different simulation counts per step, and a lock-step batch cannot budget that against `max_simulations`.  Rows of
    a step are ordered by tree, then by descent (find_leaves() returns `tree_index` with repeats); two in-flight leaves on
    the same position both miss the cache and are both evaluated; search(visits) runs visits // K steps and one of
    visits % K descents; `max_simulations` and stats()["simulations"] count descents, stats()["steps"] counts steps.  After
    every completed step no in-flight mark is left.  Gumbel search needs K == 1 (the reference's batched descent is plain
    PUCT, mcts.cc:752-784).

    The evaluator of search() / play(): `evaluator=None | "net" | "random" | "playout"` (or an EvalType member); None is the
    net when one is given and RANDOM (dumb_eval) otherwise.  With "playout" every non-terminal leaf of tree i is evaluated on
    the device as `alphazero.playout_eval(leaf, seed=s)` - the uniform policy over its legal moves, the scores of one
    uniformly random rollout - and backed up by the unchanged process_result: the "playout" agent of play.py:306 and the
    playout_eval_batch loops of mcts_analysis.py:649, with no net at all, for all five games.  Every rollout draws from a
    fresh pcg32 stream, so a tree's result depends neither on n, on leaves_per_step's launch shape nor on the other trees:
    the j-th rollout of tree i since reset() (j from 0, in descent order, running on across the moves of a game) has the
    seed s = MCTSBatch.rollout_seed(rollout_seeds[i], j), and rollout_seeds[i] defaults to mix64(seeds[i] ^ kRollSalt)
    (reset(..., rollout_seeds=...) sets them, rollout_seeds() reads them).  With leaves_per_step > 1 a playout leaf is an
    immediate: its process_result_batched runs at once, in descent order, so the tree's next descent sees the back-up.  A
    cache with "playout" is an error (the reference's playout branch bypasses the cache), as is "playout" or "random" with a
    net and "net" without one.  stats()["evaluator_leaves"] counts the rollouts.

    `descents_per_step=L` (1 <= L <= 256, default 1: everything above unchanged) keeps a tree descending inside a step while
    its leaves need nothing from the net - the per-tree loop of mcts_analysis.py:921-951.  With L > 1 one step of a live tree i
    of search() / play() is

        d = 0
        while d < L and todo[i] > 0:
            leaf = find_leaf(root); d += 1; todo[i] -= 1
            terminal leaf, RANDOM evaluator or cache hit: process_result at once, continue
            otherwise: the leaf's planes become the tree's ONE row of the step ("playout": its one rollout); break
        evaluate all rows in one call; insert them into the cache
        process_result for every tree with a pending row

    so a search needs fewer steps than visits where the leaves are mostly immediate for every tree at once: a warm shared
    cache (measured 2.0 x / 2.7 x faster at L = 4 / 16), evaluator="random", where search(visits) is ceil(visits / L) launches,
    the last plies of games.  A step lasts as long as the longest chain of immediate descents among the trees and the step
    count falls only as fast as the least lucky tree allows, so with a cold cache, and over whole games from the opening,
    L > 1 measured slower than L = 1: the default stays 1.  Tree i makes the same find_leaf /
    process_result calls in the same order as with L = 1 and stays bit for bit the stand-alone MCTS(seed=seeds[i]); only the
    cache's hit / miss counts and eviction state may differ.  The j-th rollout of a tree keeps its seed; a Gumbel batch is the
    same loop.  search(visits) and every move of play() give every live tree exactly `visits` descents through a per-tree
    counter on the device.  The read policy: "random" enqueues exactly ceil(visits / L) steps and reads nothing; with a net or
    "playout" the call enqueues ceil(visits / L) steps, then repeats { read r, the largest count any tree has left (one
    4-byte word); stop at 0; enqueue m more steps }, where m = ceil(r / L) behind the first read (the fewest steps that can
    finish), max(ceil(r / L), twice the previous m) behind every later one, and never more than r.  Every step gives every
    unfinished tree at least one descent, so r steps always finish and the rounds at least double: at most
    1 + ceil(log2(visits)) reads per search, counted in stats()["host_reads"]; stats()["steps"] counts enqueued steps, those in which no tree had work left included.  play()
    picks a move only behind the read of 0.  L > 1 together with leaves_per_step > 1, search_to() and the step API
    (find_leaves / process_results: the caller owns the evaluator and the step) raise RuntimeError before any launch.

    A visit sweep (mcts_analysis.py:884-972): search_to(targets, ..., checkpoints=(c0, c1, ...)) searches tree i until
    root_n(i) >= targets[i] and records counts / probs / root_values / root_q_values on the device the first time root_n(i)
    reaches each checkpoint; checkpoints() returns the snapshots.  See search_to().  sweep_metrics(anchor, raw, reference,
    outcomes) scores every snapshot against the anchor one on the device (:1150-1400): divergences, top-k agreement, expected
    reward and regret, the signal figures against the one-visit policy, the value gaps, and their per-checkpoint means.

    A frozen evaluation set (frozen_eval.py:330-413, 541-672): with `capture=True` (set_capture(), play(..., capture=)) every
    move of play() records the root of every live tree before its search, one launch more per move and none with capture off;
    position_pool() keeps the first record of every engine key in (tree, ply) order (pool_unique on the device),
    pool_states() / sample_pool() turn the pool back into GameStates and the reference's records, and net_vs_search(net)
    compares every root's search with one raw forward of the net on the device.  The search and play kernels are unchanged."""

    _MASK64 = 0xFFFFFFFFFFFFFFFF
    _ROLL_SALT = 0x9E3779B97F4A7C15      # kRollSalt, csrc/dev_rng.h

    @staticmethod
    def _mix64(x):                       # mix64, csrc/dev_rng.h
        m = MCTSBatch._MASK64
        x = (x + 0x9E3779B97F4A7C15) & m
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & m
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & m
        return x ^ (x >> 31)

    @staticmethod
    def rollout_seed(rollout_seed_i, j):
        """The seed of the j-th rollout (j from 0) of a tree whose rollout seed is `rollout_seed_i`: playout_eval(leaf,
        seed=MCTSBatch.rollout_seed(rs, j)) is that rollout.  Pure Python, no device."""
        j = int(j)
        if j < 0:
            raise RuntimeError(f"rollout_seed: j counts from 0, got {j}")
        m = MCTSBatch._MASK64
        return MCTSBatch._mix64(((int(rollout_seed_i) & m) + MCTSBatch._ROLL_SALT * (j + 1)) & m)

    @staticmethod
    def _evaluator(what, evaluator, net, cache):
        """-> the EvalType of a search()/play() call; every argument error before any device call"""
        if evaluator is None:
            return EvalType.NN if net is not None else EvalType.RANDOM
        names = {"net": EvalType.NN, "random": EvalType.RANDOM, "playout": EvalType.PLAYOUT}
        if isinstance(evaluator, str):
            if evaluator not in names:
                raise RuntimeError(f"{what}: evaluator must be None, 'net', 'random', 'playout' or an EvalType, got {evaluator!r}")
            ev = names[evaluator]
        elif isinstance(evaluator, EvalType):
            ev = evaluator
        else:
            raise RuntimeError(f"{what}: evaluator must be None, 'net', 'random', 'playout' or an EvalType, got {evaluator!r}")
        if ev == EvalType.NN and net is None:
            raise RuntimeError(f"{what}: evaluator 'net' needs a net")
        if ev != EvalType.NN and net is not None:
            raise RuntimeError(f"{what}: evaluator '{ev.name.lower()}' takes no net")
        if ev == EvalType.PLAYOUT and cache is not None:
            raise RuntimeError(f"{what}: evaluator 'playout' takes no cache: the reference's playout branch bypasses it "
                               "(a rollout's answer is not a function of the position)")
        return ev

    def __init__(self, game, n, cpuct, epsilon=0.0, root_policy_temp=1.0, fpu_reduction=0.0, root_fpu_zero=False,
                 shaped_dirichlet=False, gumbel_enabled=False, gumbel_m=16, gumbel_c_visit=50.0, gumbel_c_scale=1.0,
                 gumbel_full=False, *, max_simulations, seeds=None, device=0, leaves_per_step=1,
                 descents_per_step=1, capture=False):
        if isinstance(leaves_per_step, bool) or not isinstance(leaves_per_step, (int, np.integer)) or not 1 <= leaves_per_step <= 64:
            raise RuntimeError(f"leaves_per_step must be an integer in [1, 64], got {leaves_per_step!r}")
        if (isinstance(descents_per_step, bool) or not isinstance(descents_per_step, (int, np.integer))
                or not 1 <= descents_per_step <= 256):
            raise RuntimeError(f"descents_per_step must be an integer in [1, 256], got {descents_per_step!r}")
        if descents_per_step > 1 and leaves_per_step > 1:
            raise RuntimeError(f"descents_per_step = {descents_per_step} with leaves_per_step = {leaves_per_step}: a step holds "
                               "either several leaves of a tree in flight or goes on descending past the leaves that need no "
                               "evaluator, not both")
        if leaves_per_step > 1 and gumbel_enabled:
            raise RuntimeError(f"leaves_per_step = {leaves_per_step} with gumbel_enabled: the batched descent (find_leaf_batched) "
                               "is plain PUCT; use leaves_per_step = 1 for a Gumbel search")
        game = game if isinstance(game, type) else type(game)
        P, M, chw = game._info()
        cfg = _capi.MctsConfigC(cpuct, P, M, epsilon, root_policy_temp, fpu_reduction, int(game.GAME_ID == StarGambitUnifiedGS.GAME_ID),
                                int(root_fpu_zero), int(shaped_dirichlet), int(gumbel_enabled), gumbel_m, gumbel_c_visit,
                                gumbel_c_scale, int(gumbel_full), int(max_simulations))
        h = C.c_void_p()
        check(lib.azmi_search_create(game.GAME_ID, C.byref(cfg), int(n), int(device), C.byref(h)))
        self._h, self._game, self._n, self._P, self._M, self._chw = h, game, int(n), P, M, tuple(chw)
        self._gumbel, self._device = bool(gumbel_enabled), int(device)
        self._vec = max(M, 64)
        self._seeds = None if seeds is None else self._seed_array(seeds)
        self._rows = None          # rows of the pending find_leaves() batch
        self._start = None         # the states of the last reset()
        self._k = int(leaves_per_step)
        self._dl = 1
        if self._k > 1:
            check(lib.azmi_search_set_leaves_per_step(self._h, self._k))
        if descents_per_step > 1:
            check(lib.azmi_search_set_descents_per_step(self._h, int(descents_per_step)))
            self._dl = int(descents_per_step)
        self._capture = False
        if capture:
            self.set_capture(True)

    @property
    def leaves_per_step(self):
        return self._k

    @property
    def descents_per_step(self):
        return getattr(self, "_dl", 1)

    def _one_descent_per_step(self, what, why):
        if self.descents_per_step > 1:
            raise RuntimeError(f"{what} with descents_per_step = {self.descents_per_step}: {why}; use search / play, or "
                               "descents_per_step = 1")

    def __del__(self):
        if getattr(self, "_h", None) and lib is not None:
            lib.azmi_search_destroy(self._h)
            self._h = None

    def __len__(self):
        return self._n

    def _seed_array(self, seeds, what="seeds"):
        a = np.ascontiguousarray([int(x) & 0xFFFFFFFFFFFFFFFF for x in seeds], dtype=np.uint64)
        if a.shape != (self._n,):
            raise RuntimeError(f"{what}: one per tree ({self._n}), got {a.shape}")
        return a

    def reset(self, states, seeds=None, rollout_seeds=None):
        """Positions + streams; the trees are emptied.  `states`: n GameState objects of the batch's game, any mix of positions.
        `seeds` (default: the constructor's, else fresh random ones): tree i's stream is that of MCTS(seed=seeds[i]).
        `rollout_seeds` (default: mix64(seeds[i] ^ kRollSalt)): the seeds of the "playout" evaluator's rollouts, whose
        per-tree count starts again at 0."""
        states = list(states)
        rs = None if rollout_seeds is None else self._seed_array(rollout_seeds, "rollout_seeds")
        if len(states) != self._n:
            raise RuntimeError(f"reset: {self._n} positions expected, got {len(states)}")
        for g in states:
            if getattr(g, "GAME_ID", None) != self._game.GAME_ID:
                raise RuntimeError("reset: every position must be a state of the batch's game")
        if seeds is not None:
            self._seeds = self._seed_array(seeds)
        sd = self._seeds if self._seeds is not None else np.frombuffer(os.urandom(8 * self._n), np.uint64).copy()
        offs = np.zeros(self._n + 1, np.uint32)
        offs[1:] = np.cumsum([len(g._moves) for g in states])
        moves = np.ascontiguousarray([m for g in states for m in g._moves], dtype=np.int32)
        init, stride = None, 0
        if any(g._init is not None for g in states):
            # one image per tree, zero-padded to a common stride; a state without one starts from its class's fresh image
            images = [bytes(g._init) if g._init is not None else type(g)().to_bytes() for g in states]
            stride = max(len(b) for b in images)
            init = np.zeros((self._n, stride), np.uint8)
            for i, b in enumerate(images):
                init[i, : len(b)] = np.frombuffer(b, np.uint8)
        self._rows = None
        self._start = None
        check(lib.azmi_search_reset(self._h, None if init is None else init.ctypes.data, stride, moves.ctypes.data if moves.size else None,
                                    offs.ctypes.data, sd.ctypes.data))
        if rs is not None:
            check(lib.azmi_search_set_rollout_seeds(self._h, rs.ctypes.data))
        self._roll = rs if rs is not None else np.array([self._mix64(int(x) ^ self._ROLL_SALT) for x in sd], dtype=np.uint64)
        self._start = [g.copy() for g in states]

    def rollout_seeds(self):
        """uint64 [n]: the rollout seed of every tree since the last reset()."""
        if self._start is None:
            raise RuntimeError("rollout_seeds: the trees have no positions; call reset first")
        return self._roll.copy()

    def search(self, visits, net=None, cache=None, root_noise=False, evaluator=None):
        """`visits` simulations of every tree, enqueued without host synchronisation (the read-outs and synchronize() wait);
        with leaves_per_step = K: visits // K steps of K descents and one of visits % K.  With descents_per_step = L > 1 the
        call gives every live tree exactly `visits` descents in ceil(visits / L) steps ("random": exactly, nothing read) or
        more (net, "playout": one 4-byte read after them, then more steps per read of r > 0, at most
        1 + ceil(log2(visits)) reads; the call returns behind the read of 0) - see the class for the policy.
        net: a HipLeafNet (None = EvalType.RANDOM, dumb_eval); cache: a ShardedS3FIFOCache shared by all trees;
        evaluator: None (the net if given, else RANDOM), "net", "random", "playout" or an EvalType - see the class."""
        ev = self._evaluator("search", evaluator, net, cache)
        if net is not None and (net.desc.num_moves != self._M or (net.desc.in_channels, net.desc.height, net.desc.width) != self._chw):
            raise RuntimeError("search: the net's shape does not match the game")
        if cache is not None:
            cache._ensure_engine_layout()
        check(lib.azmi_search_run_eval(self._h, int(ev), None if net is None else net._h, None if cache is None else cache._h, int(visits),
                                       int(bool(root_noise)), _ENGINE_STREAM))

    def search_to(self, targets, net=None, cache=None, root_noise=False, evaluator=None, checkpoints=None, temp=1.0, pruned=False):
        """Search every tree to its own visit target: tree i descends while root_n(i) < targets[i] (`targets`: an int or n
        integers) - the `while mcts.root_n() < target` loop of mcts_analysis.py:884-972.  A tree at or above its target (a root
        reused by update_roots() already holds visits) and a finished tree take no descent.  net / cache / root_noise /
        evaluator are search()'s.  With leaves_per_step = K every step is K descents of every tree still below its target, so
        a tree may overshoot by fewer than K (mcts_analysis.py:982-1058).
        `checkpoints`: None, or at most 32 strictly ascending positive visit counts.  Snapshot j of tree i is taken once, on the
        device, at the first step boundary at which root_n(i) >= checkpoints[j] - before the first descent for a tree that
        starts there; a checkpoint above the tree's target is never taken.  checkpoints() returns the snapshots; every
        search_to starts a fresh set.  `temp`, `pruned`: the snapshots hold probs(temp), or probs_pruned(temp).
        The call reads root_n once, then enqueues every step without reading anything back; the budget is checked for the
        longest tree's steps x K before anything is enqueued.  A Gumbel batch raises: use search(visits)."""
        self._one_descent_per_step("search_to", "the checkpoint launches are planned from one root_n read and one descent of "
                                   "every tree per step")
        ev = self._evaluator("search_to", evaluator, net, cache)
        if net is not None and (net.desc.num_moves != self._M or (net.desc.in_channels, net.desc.height, net.desc.width) != self._chw):
            raise RuntimeError("search_to: the net's shape does not match the game")
        if self._gumbel:
            raise RuntimeError("search_to on a Gumbel batch: sequential halving plans a fixed budget at its first descent, and a "
                               "root_n target on a reused tree is not one; use search(visits)")
        tg = [int(targets)] * self._n if np.ndim(targets) == 0 else [int(x) for x in targets]
        if len(tg) != self._n:
            raise RuntimeError(f"search_to: one target per tree ({self._n}), got {len(tg)}")
        if any(x < 0 or x > 0xFFFFFFFF for x in tg):
            raise RuntimeError("search_to: targets must be visit counts in [0, 2^32)")
        cp = [] if checkpoints is None else [int(x) for x in checkpoints]
        if len(cp) > 32:
            raise RuntimeError(f"search_to: at most 32 checkpoints, got {len(cp)}")
        if any(x <= 0 or x > 0xFFFFFFFF for x in cp) or any(b <= a for a, b in zip(cp, cp[1:])):
            raise RuntimeError(f"search_to: checkpoints must be positive and strictly ascending, got {cp}")
        if cache is not None:
            cache._ensure_engine_layout()
        tga, cpa = np.ascontiguousarray(tg, dtype=np.uint32), np.ascontiguousarray(cp, dtype=np.uint32)
        check(lib.azmi_search_run_to(self._h, int(ev), None if net is None else net._h, None if cache is None else cache._h,
                                     tga.ctypes.data, cpa.ctypes.data if cp else None, len(cp), float(temp), int(bool(pruned)),
                                     int(bool(root_noise)), _ENGINE_STREAM))
        self._sweep_j = len(cp)

    def checkpoints(self):
        """The snapshots of the last search_to(), one row per tree and checkpoint, as recorded on the device at snapshot time:
        taken bool [n, J], root_n uint32 [n, J], counts uint32 [n, J, M], probs float32 [n, J, M] (probs(temp), or
        probs_pruned(temp) with pruned=True), root_values float32 [n, J, 3], root_q_values float32 [n, J, M].  Rows that were
        not taken are zero.  Synchronises."""
        J = getattr(self, "_sweep_j", None)
        if J is None:
            raise RuntimeError("checkpoints: no search_to call has been made on this batch")
        n, M = self._n, self._M
        mask = np.zeros(n, np.uint32)
        out = dict(root_n=np.zeros((n, J), np.uint32), counts=np.zeros((n, J, M), np.uint32), probs=np.zeros((n, J, M), np.float32),
                   root_values=np.zeros((n, J, 3), np.float32), root_q_values=np.zeros((n, J, M), np.float32))
        check(lib.azmi_search_checkpoints(self._h, mask.ctypes.data, out["root_n"].ctypes.data, out["counts"].ctypes.data,
                                          out["probs"].ctypes.data, out["root_values"].ctypes.data, out["root_q_values"].ctypes.data))
        out["taken"] = ((mask[:, None] >> np.arange(J, dtype=np.uint32)[None, :]) & 1).astype(bool)
        return out

    @staticmethod
    def _sweep_index(what, x, J):
        """-> x as a checkpoint index of a set of J, negative values counting from its end"""
        if isinstance(x, bool) or not isinstance(x, (int, np.integer)):
            raise RuntimeError(f"sweep_metrics: {what} must be a checkpoint index (an integer), got {x!r}")
        if not -J <= x < J:
            raise RuntimeError(f"sweep_metrics: {what} = {x} out of range: the reference set has {J} checkpoints")
        return int(x) % J

    def _sweep_args(self, anchor, raw, reference, outcomes):
        """-> (reference batch, anchor, raw or -1, outcomes float64 [n] or None); every argument error before any device call"""
        J = getattr(self, "_sweep_j", None)
        if J is None:
            raise RuntimeError("sweep_metrics: no search_to call has been made on this batch")
        if getattr(self, "_rows", None) is not None:
            raise RuntimeError("sweep_metrics: a find_leaves step is pending; call process_results first")
        ref = self if reference is None else reference
        if not isinstance(ref, MCTSBatch):
            raise RuntimeError(f"sweep_metrics: reference must be an MCTSBatch or None, got {type(reference).__name__}")
        if ref is not self:
            if getattr(ref._game, "GAME_ID", None) != getattr(self._game, "GAME_ID", None):
                raise RuntimeError(f"sweep_metrics: the reference batch holds another game ({ref._game.__name__}, "
                                   f"this batch {self._game.__name__})")
            if ref._n != self._n:
                raise RuntimeError(f"sweep_metrics: the reference batch holds {ref._n} trees, this batch {self._n}")
            if ref._device != self._device:
                raise RuntimeError(f"sweep_metrics: the reference batch is on device {ref._device}, this batch on {self._device}")
            if getattr(ref, "_sweep_j", None) is None:
                raise RuntimeError("sweep_metrics: no search_to call has been made on the reference batch")
            if getattr(ref, "_rows", None) is not None:
                raise RuntimeError("sweep_metrics: a find_leaves step is pending on the reference batch; call process_results first")
        Jr = ref._sweep_j
        if Jr == 0:
            raise RuntimeError("sweep_metrics: the reference set has no checkpoints: nothing to anchor on")
        a = self._sweep_index("anchor", anchor, Jr)
        r = -1 if raw is None else self._sweep_index("raw", raw, Jr)
        o = None
        if outcomes is not None:
            try:
                o = np.ascontiguousarray(outcomes, dtype=np.float64)
            except (TypeError, ValueError):
                raise RuntimeError(f"sweep_metrics: outcomes must be {self._n} numbers, got {outcomes!r}") from None
            if o.shape != (self._n,):
                raise RuntimeError(f"sweep_metrics: outcomes: one per tree ({self._n}), got shape {o.shape}")
        return ref, a, r, o

    def sweep_metrics(self, anchor=-1, raw=None, reference=None, outcomes=None):
        """Score every snapshot of the last search_to() against the anchor snapshot of the same tree, on the device
        (azmi_search_sweep_metrics): what mcts_analysis.run_analysis does with its sweep once the search is over
        (mcts_analysis.py:1150-1400), without copying the [n, J, M] snapshots out.  `reference`: the batch whose snapshot set
        supplies the anchor row, the raw row and root_q_values (default: this batch; the reference's `base_ref` tree when the
        swept trees search with root noise) - same game, n and device.  `anchor`, `raw`: checkpoint indices into the
        reference's set, negative ones counting from its end; raw (None: none) is the one-visit checkpoint the "signal"
        figures compare against.  `outcomes`: None or n game outcomes.
        With p the anchor policy, q the policy of row (i, j), r the raw policy, Q the anchor's root_q_values and v =
        root_values[..., 0], all float32 snapshots computed with in float64:
          jsd, tv, hellinger, top1, top3, top9    policy_divergences(p, q)
          reward = sum q Q, regret = reward(anchor row) - reward
          pressure = KL(q || r + 1e-10), benefit = reward - sum r Q, entropy = -sum q ln q         (pressure, benefit: need raw)
          value_gap = |v_j - v_anchor|
          abs_err = |v_j - outcome|, closer_than_anchor, closer_than_raw (1.0 / 0.0)               (need outcomes; the last, raw)
          ceiling[i] = KL(p || r + 1e-10)                                                          (needs raw)
        A row is valid when snapshot j of tree i and the reference's anchor snapshot of tree i were both taken; an invalid row
        is NaN everywhere, and what needs a raw row or outcomes that are not there is NaN.
        -> dict: one float64 [n, J] array per name above, ceiling [n], valid bool [n, J], and mean / count: dicts of [J] arrays,
        per column the mean over the trees that are not NaN there and their number.  Two launches and one synchronisation
        whatever n and J are; the sums run in a fixed order, so two calls give the same bits.  Correlations and calibration
        bins (mcts_analysis.py:1289-1353) are a few numpy lines over the returned arrays."""
        ref, a, r, o = self._sweep_args(anchor, raw, reference, outcomes)
        n, J, C_ = self._n, self._sweep_j, len(SWEEP_COLUMNS)
        rows = np.zeros((n, J, C_), np.float64); ceiling = np.zeros(n, np.float64)
        mean = np.zeros((J, C_), np.float64); count = np.zeros((J, C_), np.uint32); valid = np.zeros((n, J), np.uint8)
        check(lib.azmi_search_sweep_metrics(self._h, None if ref is self else ref._h, a, r, None if o is None else o.ctypes.data,
                                            rows.ctypes.data, ceiling.ctypes.data, mean.ctypes.data, count.ctypes.data,
                                            valid.ctypes.data, _ENGINE_STREAM))
        out = {k: rows[:, :, c].copy() for c, k in enumerate(SWEEP_COLUMNS)}
        out.update(ceiling=ceiling, valid=valid.astype(bool),
                   mean={k: mean[:, c].copy() for c, k in enumerate(SWEEP_COLUMNS)},
                   count={k: count[:, c].astype(np.int64) for c, k in enumerate(SWEEP_COLUMNS)})
        return out

    def synchronize(self):
        check(lib.azmi_search_sync(self._h))

    # ---- moves: tree reuse on the device ----------------------------------------------------------------
    def pick_moves(self, temp):
        """pick_move(probs(temp)) of every tree from its own stream (a Gumbel search: gumbel_final_action(), no draw)
        -> int32 [n], -1 for a finished tree.  The moves also stay on the device for update_roots()."""
        out = np.full(self._n, -1, np.int32)
        check(lib.azmi_search_pick_moves(self._h, float(temp), out.ctypes.data, _ENGINE_STREAM))
        return out

    def update_roots(self, moves=None):
        """update_root + play_move on every tree: moves[i] (< 0: tree i stays), default the moves of the last pick_moves()
        (a pick is played once: without a new pick_moves() nothing moves).
        A move that is not one of a tree's root raises RuntimeError naming the tree; that tree is left where it was, the other
        trees' moves of the call are applied."""
        mv = None
        if moves is not None:
            mv = np.ascontiguousarray(moves, dtype=np.int32)
            if mv.shape != (self._n,):
                raise RuntimeError(f"update_roots: one move per tree ({self._n}), got {mv.shape}")
        check(lib.azmi_search_update_roots(self._h, None if mv is None else mv.ctypes.data, _ENGINE_STREAM))

    def add_root_noise(self): check(lib.azmi_search_root_prior(self._h, 0, 1, _ENGINE_STREAM))
    def apply_root_policy_temp(self): check(lib.azmi_search_root_prior(self._h, 1, 0, _ENGINE_STREAM))

    def play(self, visits, net=None, cache=None, temp=1.0, max_moves=1, root_noise=False, evaluator=None, capture=None):
        """max_moves x (search(visits, net, cache, root_noise, evaluator); pick_moves(temp); update_roots(); on the reused root
        apply_root_policy_temp() when the root temperature is not 1 and add_root_noise() when root_noise), enqueued without
        host synchronisation.  Finished trees are skipped, so `max_moves` of a game's length plays whole games.  The rollout
        count of the "playout" evaluator runs on across the moves.  `capture`: None leaves set_capture() as it is, a bool is
        set_capture(capture) first; with capture on, the root of every live tree is recorded before each move's search."""
        ev = self._evaluator("play", evaluator, net, cache)
        if capture is not None:
            self.set_capture(capture)
        if net is not None and (net.desc.num_moves != self._M or (net.desc.in_channels, net.desc.height, net.desc.width) != self._chw):
            raise RuntimeError("play: the net's shape does not match the game")
        if cache is not None:
            cache._ensure_engine_layout()
        check(lib.azmi_search_play_eval(self._h, int(ev), None if net is None else net._h, None if cache is None else cache._h, int(visits),
                                        float(temp), int(max_moves), int(bool(root_noise)), _ENGINE_STREAM))

    def _game_state(self, log=False, final=False):
        cap = self._game.MAX_TURNS + 8
        status = np.zeros(self._n, np.int32); length = np.zeros(self._n, np.uint32)
        lg = np.zeros((self._n, cap), np.int32) if log else None
        fs = np.zeros((self._n, self._P + 1), np.float32) if final else None
        check(lib.azmi_search_game_state(self._h, status.ctypes.data, length.ctypes.data, None if lg is None else lg.ctypes.data,
                                         None if fs is None else fs.ctypes.data))
        return status, length, lg, fs

    def finished(self):
        """bool [n]: the tree's game is over (a move played on the batch reached a terminal state)."""
        return self._game_state()[0] > 0

    def move_logs(self):
        """The moves played on every tree since reset(): a list of int32 arrays."""
        _, length, lg, _ = self._game_state(log=True)
        return [lg[i, : int(length[i])].copy() for i in range(self._n)]

    def final_scores(self):
        """[n, P+1]: GameState.scores() of every finished tree (rows of live trees are zero)."""
        status, _, _, fs = self._game_state(final=True)
        fs[status <= 0] = 0
        return fs

    def states(self):
        """The current root GameState of every tree: its reset() state + its move log."""
        if self._start is None:
            raise RuntimeError("states: the trees have no positions; call reset first")
        out = []
        for g, lg in zip(self._start, self.move_logs()):
            g = g.copy()
            g._moves.extend(int(m) for m in lg)      # (children of a root: legal by construction)
            g._snap = None
            out.append(g)
        return out

    # ---- a frozen evaluation set: capture, pool, net versus search (frozen_eval.py:330-413, 541-672) -----------------
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

    # ---- opening trees: from n searched roots to the next level's frontier (opening_analysis.py:261-355) -------------
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
        if isinstance(min_reach, bool) or not isinstance(min_reach, (int, float, np.integer, np.floating)) \
                or not np.isfinite(min_reach) or not min_reach > 0:
            raise RuntimeError(f"expand_frontier: min_reach must be a positive finite number, got {min_reach!r}")
        if max_children is None:
            max_children = n * self._M
        if isinstance(max_children, bool) or not isinstance(max_children, (int, np.integer)) or not 1 <= max_children <= 0xFFFFFFFF:
            raise RuntimeError(f"expand_frontier: max_children must be an integer in [1, 2^32), got {max_children!r}")
        return r, t, float(min_reach), int(max_children)

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

    # ---- step API: any evaluator --------------------------------------------------------------------
    def find_leaves(self, numpy=None):
        """One simulation's descent of every tree (leaves_per_step = K: K descents, or as many as max_simulations leaves)
        -> (canonical [n_rows, C, H, W], tree_index [n_rows]): the leaves that need an evaluation, rows in ascending tree
        order, then descent order (terminal leaves are backed up at once and take no row).  Device tensors
        (views of the object's buffers, valid until the next find_leaves) when torch is importable, numpy arrays otherwise or
        with numpy=True."""
        self._one_descent_per_step("find_leaves", "the step API's caller owns the evaluator and the step")
        pc, pt, n = C.c_void_p(), C.c_void_p(), C.c_uint32()
        check(lib.azmi_search_find_leaves(self._h, _ENGINE_STREAM, C.byref(pc), C.byref(pt), C.byref(n)))
        self._rows = n.value
        if numpy is None:
            try:
                import torch  # noqa: F401
                numpy = False
            except ImportError:
                numpy = True
        if numpy or n.value == 0:
            canon = np.zeros((n.value,) + self._chw, np.float32)
            idx = np.zeros(n.value, np.uint32)
            check(lib.azmi_search_leaves_to_host(self._h, canon.ctypes.data, idx.ctypes.data))
            if numpy:
                return canon, idx
            import torch
            dev = torch.device("cuda", self._device)
            return torch.from_numpy(canon).to(dev), torch.from_numpy(idx.astype(np.int32)).to(dev)
        import torch
        from ._torch_view import device_tensor
        dev = torch.device("cuda", self._device)
        return (device_tensor(pc.value, (n.value,) + self._chw, torch.float32, dev),
                device_tensor(pt.value, (n.value,), torch.int32, dev))

    def process_results(self, v, pi, root_noise=False):
        """The evaluator's answers for the rows of the last find_leaves(): v [n_rows, P+1], pi [n_rows, M] probabilities,
        device tensors or numpy arrays."""
        self._one_descent_per_step("process_results", "the step API's caller owns the evaluator and the step")
        if self._rows is None:
            raise RuntimeError("process_results: no leaf batch is pending; call find_leaves first")
        rows = self._rows
        if tuple(v.shape) != (rows, self._P + 1) or tuple(pi.shape) != (rows, self._M):
            raise RuntimeError(f"process_results: the step has {rows} rows: v must be [{rows}, {self._P + 1}] and pi "
                               f"[{rows}, {self._M}], got {tuple(v.shape)} and {tuple(pi.shape)}")
        if isinstance(v, np.ndarray) or isinstance(pi, np.ndarray):
            vv = np.ascontiguousarray(v, dtype=np.float32); pp = np.ascontiguousarray(pi, dtype=np.float32)
            check(lib.azmi_search_process_results_host(self._h, vv.ctypes.data, pp.ctypes.data, int(bool(root_noise))))
        else:
            import torch
            vv = v.contiguous().float(); pp = pi.contiguous().float()
            torch.cuda.current_stream(vv.device).synchronize()       # the evaluator ran on torch's stream, the trees on the engine's
            check(lib.azmi_search_process_results(self._h, vv.data_ptr(), pp.data_ptr(), int(bool(root_noise)), _ENGINE_STREAM))
            self.synchronize()                                       # vv / pp may be temporaries
        self._rows = None

    # ---- read-outs: one row per tree -------------------------------------------------------------------
    def _query(self, kind, temp=0.0, arg=0):
        f = np.zeros((self._n, self._vec), np.float32); u = np.zeros((self._n, self._vec + 64), np.uint32)
        check(lib.azmi_search_query(self._h, kind, float(temp), int(arg), f.ctypes.data, u.ctypes.data))
        return f, u

    def counts(self): return self._query(Query.COUNTS)[1][:, : self._M].copy()
    def probs(self, temp): return self._query(Query.PROBS, temp)[0][:, : self._M].copy()
    def probs_pruned(self, temp): return self._query(Query.PROBS_PRUNED, temp)[0][:, : self._M].copy()
    def root_values(self): return self._query(Query.ROOT_VALUE)[0][:, :3].copy()
    def root_q_values(self): return self._query(Query.ROOT_Q)[0][:, : self._M].copy()
    def depths(self): return self._query(Query.SCALARS)[1][:, 0].copy()
    def root_ns(self): return self._query(Query.SCALARS)[1][:, 1].copy()
    def avg_leaf_depths(self): return self._query(Query.SCALARS)[0][:, 0].copy()
    def normalized_root_entropies(self): return self._query(Query.SCALARS)[0][:, 1].copy()
    def gumbel_enabled(self): return self._gumbel
    def gumbel_improved_policies(self): return self._query(Query.GUMBEL_POLICY)[0][:, : self._M].copy()
    def gumbel_final_actions(self): return self._query(Query.GUMBEL_FINAL)[1][:, 0].copy()
    def set_gumbel_num_sims(self, n): check(lib.azmi_search_query(self._h, Query.SET_GUMBEL_SIMS, 0.0, int(n), None, None))

    def principal_variations(self, depth=5):
        u = self._query(Query.PRINCIPAL_VARIATION, arg=depth)[1]
        return [u[i, 1: 1 + int(u[i, 0])].copy() for i in range(self._n)]

    def stats(self):
        """launches: kernel launches the object has enqueued since creation (the net's own not included); net_calls; steps;
        simulations / evaluator_leaves / terminal_leaves since the last reset, summed over the trees; host_reads: the 4-byte
        reads search() / play() have made since creation (descents_per_step > 1 with a net or "playout"; 0 otherwise)."""
        out = np.zeros(6, np.uint64)
        check(lib.azmi_search_stats(self._h, out.ctypes.data))
        reads = C.c_uint64()
        check(lib.azmi_search_host_reads(self._h, C.byref(reads)))
        st = dict(zip(("launches", "net_calls", "steps", "simulations", "evaluator_leaves", "terminal_leaves"), (int(x) for x in out)))
        st["host_reads"] = int(reads.value)
        return st
