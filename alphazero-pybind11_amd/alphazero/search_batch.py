"""MCTSBatch: N independent search trees advanced together on the device (azmi_search_*).  This file holds the core, as the
host's search_batch.hip does; the visit sweep, the frozen evaluation set and the opening-tree frontier are the base classes of
search_batch_sweep.py, search_batch_pool.py and search_batch_frontier.py."""
import ctypes as C
import os

import numpy as np

from . import _args, _capi, _rng
from ._capi import lib, check
from .games import StarGambitUnifiedGS
from .mcts import Query, _ENGINE_STREAM
from .params import EvalType
from .search_batch_frontier import _Frontier
from .search_batch_pool import _Pool
from .search_batch_sweep import _Sweep


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


class MCTSBatch(_Sweep, _Pool, _Frontier):
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

    The visit sweep - search_to(), checkpoints(), sweep_metrics() - is described at the top of search_batch_sweep.py.
    The frozen evaluation set - capture, position_pool(), pool_states(), sample_pool(), net_vs_search() - at the top of
    search_batch_pool.py.  The opening-tree frontier - expand_frontier() - at the top of search_batch_frontier.py."""

    rollout_seed = staticmethod(_rng.rollout_seed)
    _mix64 = staticmethod(_rng.mix64)            # the tests of the draws name the mixer through the class
    _evaluator = staticmethod(_evaluator)        # search_to() (search_batch_sweep.py) and the tests reach it through the class

    def __init__(self, game, n, cpuct, epsilon=0.0, root_policy_temp=1.0, fpu_reduction=0.0, root_fpu_zero=False,
                 shaped_dirichlet=False, gumbel_enabled=False, gumbel_m=16, gumbel_c_visit=50.0, gumbel_c_scale=1.0,
                 gumbel_full=False, *, max_simulations, seeds=None, device=0, leaves_per_step=1,
                 descents_per_step=1, capture=False):
        _args.integer(leaves_per_step, f"leaves_per_step must be an integer in [1, 64], got {leaves_per_step!r}", 1, 64)
        _args.integer(descents_per_step, f"descents_per_step must be an integer in [1, 256], got {descents_per_step!r}", 1, 256)
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
        a = np.ascontiguousarray([int(x) & _rng.MASK64 for x in seeds], dtype=np.uint64)
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
        self._roll = rs if rs is not None else np.array([_rng.mix64(int(x) ^ _rng.ROLL_SALT) for x in sd], dtype=np.uint64)
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
        ev = _evaluator("search", evaluator, net, cache)
        if net is not None and (net.desc.num_moves != self._M or (net.desc.in_channels, net.desc.height, net.desc.width) != self._chw):
            raise RuntimeError("search: the net's shape does not match the game")
        if cache is not None:
            cache._ensure_engine_layout()
        check(lib.azmi_search_run_eval(self._h, int(ev), None if net is None else net._h, None if cache is None else cache._h, int(visits),
                                       int(bool(root_noise)), _ENGINE_STREAM))

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
        ev = _evaluator("play", evaluator, net, cache)
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

    def leaf_keys(self):
        """The engine key (hash_game_state) of every row of the last find_leaves(), in row order: an int64 CUDA tensor [n_rows]
        (the key's 64 bits; a view of the object's buffer, valid until the next find_leaves).  The find kernel hashed every leaf
        it handed out - the device hash search() and capture_roots() use - and one launch brings the keys into row order, so a
        step with a cache reads
            canonical, tree = mb.find_leaves()
            v, pi, hit = alphazero.cached_forward(net, cache, canonical, mb.leaf_keys())
            mb.process_results(v, pi)
        (with leaves_per_step > 1 a key of 0 reads 0x9E3779B97F4A7C15, the value every cache stores it as)."""
        if self._rows is None:
            raise RuntimeError("leaf_keys: no leaf batch is pending; call find_leaves first")
        import torch
        from ._torch_view import device_tensor
        pk, n = C.c_void_p(), C.c_uint32()
        check(lib.azmi_search_leaf_keys(self._h, _ENGINE_STREAM, C.byref(pk), C.byref(n)))
        dev = torch.device("cuda", self._device)
        if n.value == 0:
            return torch.zeros(0, dtype=torch.int64, device=dev)
        return device_tensor(pk.value, (n.value,), torch.int64, dev)

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
