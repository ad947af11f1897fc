"""PlayManager and the GameData view of one of its slots."""
import ctypes as C
import struct

import numpy as np

from . import _capi
from ._capi import lib, check
from .cache import ShardedS3FIFOCache
from .games import Connect4GS, StarGambitUnifiedGS, _TaflBoardGS
from .mcts import _ENGINE_STREAM


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


class GameData:
    """GameData (py_wrapper.cc:265-288) of one slot: gs(), valid_moves(), canonical() read the device state; v() and pi()
    are the host rows push_inference(i) hands to the engine."""

    def __init__(self, pm, i):
        self._pm, self._i = pm, i
        self._v = np.zeros(pm._P + 1, np.float32)
        self._pi = np.zeros(pm._M, np.float32)

    def v(self): return self._v
    def pi(self): return self._pi

    def canonical(self):
        out = np.zeros(tuple(self._pm._chw), np.float32)
        check(lib.azmi_pm_slot_canonical(self._pm._h, self._i, out.ctypes.data))
        return out

    @property
    def perm_index(self):
        """GameData::perm_index (play_manager.h:41): the seat permutation this slot's game runs under."""
        w = np.zeros(8, np.uint64); n = C.c_uint32()
        check(lib.azmi_pm_slot_state(self._pm._h, self._i, w.ctypes.data, 8, C.byref(n)))
        return int(w[n.value - 1])

    def gs(self):
        pm = self._pm
        game = pm._game
        if issubclass(game, StarGambitUnifiedGS):     # the to_bytes image from the packed units, the scalars and the position history
            w = np.zeros(16, np.uint64); n = C.c_uint32()
            check(lib.azmi_pm_slot_state(pm._h, self._i, w.ctypes.data, 16, C.byref(n)))
            hist = np.zeros(4100, np.uint64); hn = C.c_uint32()
            check(lib.azmi_pm_slot_history(pm._h, self._i, hist.ctypes.data, hist.size, C.byref(hn)))
            sc = int(w[10]); misc = (sc >> 24) & 0xFFFF; res = (sc >> 40) & 0x3FFFF
            units = b""
            for i in range(misc & 31):
                u = (int(w[i // 2]) >> (32 * (i % 2))) & 0xFFFFFFFF
                units += struct.pack("<5B2b2B", u & 3, (u >> 2) & 1, (u >> 3) & 7, (u >> 6) & 7, (u >> 9) & 7, ((u >> 12) & 15) - 6,
                                     ((u >> 16) & 15) - 6, (u >> 20) & 3, (u >> 22) & 15)
            reserves = bytes([(res >> (3 * (p * 3 + t))) & 7 if t < 3 else 0 for p in range(2) for t in range(4)])
            winner = (misc >> 7) & 3
            inner = (struct.pack("<I", misc & 31) + units + reserves + struct.pack("<BIBBbI", sc & 1, (sc >> 8) & 0xFFFF, (misc >> 5) & 1,
                                                                                    (misc >> 6) & 1, winner if winner < 3 else -1, hn.value)
                     + hist[: hn.value].tobytes())
            base = pm._sg_base
            return game.from_bytes(struct.pack("<4fiBI", *base[1], base[0], (misc >> 9) & 3, len(inner)) + inner)
        w = np.zeros(8, np.uint64); n = C.c_uint32()
        check(lib.azmi_pm_slot_state(pm._h, self._i, w.ctypes.data, 8, C.byref(n)))
        if game is Connect4GS:
            board = np.zeros((2, 6, 7), np.int8)
            for p in range(2):
                bits = int(w[p])
                for c in range(42):
                    board[p].flat[c] = (bits >> c) & 1
            return Connect4GS(board, int(w[2]) >> 32, int(w[2]) & 0xFFFFFFFF)
        if issubclass(game, _TaflBoardGS):
            sq = game.BOARD * game.BOARD
            d = int(w[0]) | (int(w[1]) << 64); a = int(w[2]) | (int(w[3]) << 64)
            king = int(w[4]) & 0xFF
            board = np.zeros((3, game.BOARD, game.BOARD), np.int8)
            for c in range(sq):
                board[1].flat[c] = (d >> c) & 1
                board[2].flat[c] = (a >> c) & 1
            if king < sq:
                board[0].flat[king] = 1
            return game.from_board(board, (int(w[4]) >> 24) & 0xFF, (int(w[4]) >> 8) & 0xFFFF)
        raise RuntimeError("game_data(i).gs() is not available for this game (its state carries a repetition history)")

    def valid_moves(self):
        return self.gs().valid_moves()


class PlayManager:
    """py_wrapper.cc:351-504 over libazmi.

    Reference methods: play, build_batch, update_inferences, build_history_batch, scores,
    resign_scores, games_completed, remaining_games, params, avg_* getters, hist_count.
    Device fast path (no reference counterpart): round(), io_tensors(), poll().
    """

    def __init__(self, gs, params, caches=None, seed=None, device=0, max_inline=0, log_moves=False, history_capacity=0):
        if gs is None:
            raise TypeError("PlayManager(): gs must not be None")  # py::arg().none(false)
        game_id = gs.GAME_ID
        is_sg = (gs if isinstance(gs, type) else type(gs)).GAME_ID == StarGambitUnifiedGS.GAME_ID
        if not isinstance(gs, type) and not is_sg and (gs._moves or gs._init is not None):
            raise RuntimeError("the MI355X PlayManager starts every game from the game's initial position")
        nplayers = type(gs).NUM_PLAYERS() if not isinstance(gs, type) else gs.NUM_PLAYERS()
        self._game = gs if isinstance(gs, type) else type(gs)
        self._params = params
        cparams = params._to_c(nplayers)
        opts = _capi.EngineOptsC()
        lib.azmi_engine_opts_default(C.byref(opts))
        if seed is not None:
            opts.seed = int(seed)
        opts.device = int(device)
        opts.max_inline = int(max_inline)
        opts.log_moves = int(bool(log_moves))
        opts.history_capacity = int(history_capacity)
        if is_sg:   # every game re-draws its variant (randomize_start): only the base game's constructor arguments matter
            base = gs() if isinstance(gs, type) else gs
            self._sg_base = (base._pinned, base._probs)
            opts.sg_pinned_variant = base._pinned
            for i in range(4):
                opts.sg_variant_probs[i] = base._probs[i]
            if not any(base._probs):
                raise RuntimeError("StarGambitUnifiedGS: the variant weights are all zero")
        h = C.c_void_p()
        self._caches = None
        if caches is None:
            check(lib.azmi_pm_create(game_id, C.byref(cparams), C.byref(opts), C.byref(h)))
        else:   # PlayManager(gs, params, caches): py_wrapper.cc:355-360, one (possibly None) cache per model group
            self._caches = list(caches)     # the engine borrows them: keep them alive as long as the engine
            arr = (C.c_void_p * max(1, len(self._caches)))()
            for i, c in enumerate(self._caches):
                if c is not None and not isinstance(c, ShardedS3FIFOCache):
                    raise TypeError("caches must hold ShardedS3FIFOCache objects or None")
                if c is not None:
                    c._ensure_engine_layout()
                arr[i] = None if c is None else c._h
            check(lib.azmi_pm_create_with_caches(game_id, C.byref(cparams), C.byref(opts), arr, len(self._caches), C.byref(h)))
        self._h = h
        self._eager = False
        self._slot_rows = {}
        self._P, self._M, self._chw = self._game._info()
        self._S = int(params.concurrent_games)
        self._last_stream = _ENGINE_STREAM

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and lib is not None:   # `lib` is already None while the interpreter shuts down
            lib.azmi_pm_destroy(h)
            self._h = None

    # ---- reference surface --------------------------------------------------------------
    def params(self):
        return self._params

    def play(self):
        """PlayManager::play (play_manager.cc:258-600).  Engines whose seats need no net (RANDOM / PLAYOUT) run to completion
        here; any number of threads may call it at once, like the reference's mcts_workers.  With NN seats the engine is
        driven by whoever calls build_batch / update_inferences (the reference's batcher threads), so a worker thread that
        calls play() just waits for the games to finish or for stop(), as the reference's workers do when they find
        their queue empty."""
        rc = lib.azmi_pm_play(self._h, _ENGINE_STREAM)
        if rc == -5:                                       # AZMI_ERR_STATE: NN seats
            import time
            while self.remaining_games() > 0 and not self.stopped():
                time.sleep(0.0005)
            return
        check(rc)

    def games_completed(self):
        done, live = C.c_uint32(), C.c_uint32()
        check(lib.azmi_pm_poll(self._h, self._stream_arg(None), C.byref(done), C.byref(live)))
        return done.value

    def stop(self):                                        # play_manager.h:177
        check(lib.azmi_pm_stop(self._h))

    def stopped(self):                                     # play_manager.h:178
        f = C.c_int()
        check(lib.azmi_pm_stopped(self._h, C.byref(f)))
        return bool(f.value)

    def set_eager(self, e):
        """play_manager.h:277: the reference's batcher hands over partial batches while this is set; the engine's
        build_batch never waits for a batch to fill, so the flag is only remembered."""
        self._eager = bool(e)

    def _queue_counts(self):
        a, b = C.c_uint32(), C.c_uint32()
        check(lib.azmi_pm_queue_counts(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def awaiting_inference_count(self): return self._queue_counts()[0]    # play_manager.h:317-323
    def awaiting_mcts_count(self): return self._queue_counts()[1]         # play_manager.h:316

    def remaining_games(self):
        if self.stopped():                                 # play_manager.h:179-182
            return 0
        done, live = C.c_uint32(), C.c_uint32()
        check(lib.azmi_pm_poll(self._h, self._stream_arg(None), C.byref(done), C.byref(live)))
        if live.value == 0:
            return 0
        return max(0, int(self._params.games_to_play) - done.value)

    def scores(self):
        out = np.zeros(self._P + 1, np.float32)
        check(lib.azmi_pm_scores(self._h, out.ctypes.data))
        return out

    def resign_scores(self):
        out = np.zeros(self._P + 1, np.float32)
        check(lib.azmi_pm_resign_scores(self._h, out.ctypes.data))
        return out

    # the rows of azmi_pm_stats, azmi_pm_stat_sums / azmi_pm_variant_sums and azmi_pm_cache_stats, in the engine's order
    _STAT_KEYS = ("avg_game_length", "avg_leaf_depth", "avg_search_entropy", "fast_avg_leaf_depth", "fast_avg_search_entropy",
                  "avg_moves_per_turn", "avg_valid_moves")
    _SUM_KEYS = ("game_length", "games", "moves", "full_moves", "fast_moves", "leaf_depth", "entropy", "fast_leaf_depth",
                 "fast_entropy", "valid_moves")
    _CACHE_KEYS = ("hits", "misses", "evictions", "reinserts", "size", "max_size")

    def _stats(self):
        out = np.zeros(len(self._STAT_KEYS), np.float32)
        check(lib.azmi_pm_stats(self._h, out.ctypes.data))
        return dict(zip(self._STAT_KEYS, (float(x) for x in out)))

    def stat_sums(self):
        """The accumulators behind the avg_* figures (play_manager.h:398-424), for exact aggregation over several engines."""
        out = np.zeros(len(self._SUM_KEYS), np.float64)
        check(lib.azmi_pm_stat_sums(self._h, out.ctypes.data))
        return dict(zip(self._SUM_KEYS, (float(x) for x in out)))

    def avg_game_length(self): return self._stats()["avg_game_length"]
    def avg_leaf_depth(self): return self._stats()["avg_leaf_depth"]
    def avg_search_entropy(self): return self._stats()["avg_search_entropy"]
    def fast_avg_leaf_depth(self): return self._stats()["fast_avg_leaf_depth"]
    def fast_avg_search_entropy(self): return self._stats()["fast_avg_search_entropy"]
    def avg_moves_per_turn(self): return self._stats()["avg_moves_per_turn"]
    def avg_valid_moves(self): return self._stats()["avg_valid_moves"]

    def counters(self):
        out = np.zeros(6, np.uint64)
        check(lib.azmi_pm_counters(self._h, out.ctypes.data))
        return dict(zip(("sims", "evals", "cache_hits", "cache_misses", "hist_rows", "rounds"), (int(x) for x in out)))

    def hist_count(self):
        return self.counters()["hist_rows"]

    def _cache_stats(self):
        out = np.zeros(len(self._CACHE_KEYS), np.uint64)
        check(lib.azmi_pm_cache_stats(self._h, out.ctypes.data))
        return [int(x) for x in out]

    def _cache_stat(self, key):
        return self._cache_stats()[self._CACHE_KEYS.index(key)]

    # play_manager.h:325-366: sums over the model groups' caches
    def cache_hits(self): return self._cache_stat("hits")
    def cache_misses(self): return self._cache_stat("misses")
    def cache_evictions(self): return self._cache_stat("evictions")
    def cache_reinserts(self): return self._cache_stat("reinserts")
    def cache_size(self): return self._cache_stat("size")
    def cache_max_size(self):
        if self._caches is not None:      # external caches report the size they were created with (see _ensure_engine_layout)
            return sum(c.max_size() for c in self._caches if c is not None)
        return self._cache_stat("max_size")

    # per-variant tables (play_manager.h:218-275): only for games with variants (StarGambitUnifiedGS)
    def num_tracked_variants(self): return int(lib.azmi_pm_num_variants(self._h))

    def _variant(self, v):
        v = int(v)
        if not 0 <= v < self.num_tracked_variants():
            raise IndexError("variant index out of range")
        npm = self.num_seat_perms()
        ps = np.zeros((npm, self._P + 1), np.float32); pg = np.zeros(npm, np.uint32); sums = np.zeros(len(self._SUM_KEYS), np.float64)
        check(lib.azmi_pm_variant_sums(self._h, v, ps.ctypes.data, pg.ctypes.data, sums.ctypes.data))
        return ps, pg, sums

    def variant_sums(self, v): return self._variant(v)[2]
    def variant_scores(self, v): return self._variant(v)[0].sum(0)
    def variant_games_completed(self, v): return int(self._variant(v)[1].sum())
    def variant_perm_scores(self, v, p): return self._variant(v)[0][int(p)].copy()
    def variant_perm_games_completed(self, v, p): return int(self._variant(v)[1][int(p)])

    def _variant_ratio(self, v, num, den, single=False):
        """variant_sums(v)[num] / variant_sums(v)[den], the fields by their _SUM_KEYS names; 0 for an empty denominator"""
        s = self.variant_sums(v)
        a, b = s[self._SUM_KEYS.index(num)], s[self._SUM_KEYS.index(den)]
        if b == 0:
            return 0.0
        return float(np.float32(a) / np.float32(b)) if single else float(np.float32(a / b))

    # the variant_avg_* getters with the reference's own divisions (play_manager.h:233-275)
    def variant_avg_game_length(self, v): return self._variant_ratio(v, "game_length", "games", True)
    def variant_avg_leaf_depth(self, v): return self._variant_ratio(v, "leaf_depth", "full_moves")
    def variant_avg_search_entropy(self, v): return self._variant_ratio(v, "entropy", "full_moves")
    def variant_fast_avg_leaf_depth(self, v): return self._variant_ratio(v, "fast_leaf_depth", "fast_moves")
    def variant_fast_avg_search_entropy(self, v): return self._variant_ratio(v, "fast_entropy", "fast_moves")
    def variant_avg_moves_per_turn(self, v): return self._variant_ratio(v, "moves", "game_length", True)
    def variant_avg_valid_moves(self, v): return self._variant_ratio(v, "valid_moves", "moves")

    # ---- the raw queue interface (play_manager.h:186-192, 285-286): pop leaf indices, read the slot through
    # game_data(i), write its v() / pi() rows, push_inference(i)
    def pop_games_upto(self, group, n):
        idx = np.zeros(max(int(n), 1), np.uint32)
        cnt = C.c_uint32()
        check(lib.azmi_pm_build_batch_group(self._h, int(group), None, int(n), idx.ctypes.data, C.byref(cnt)))
        return [int(i) for i in idx[: cnt.value]]

    def pop_game(self, group):
        got = self.pop_games_upto(group, 1)
        return got[0] if got else None

    def game_data(self, i):
        i = int(i)
        if not 0 <= i < self._S:
            raise IndexError("game index out of range")
        gd = self._slot_rows.get(i)
        if gd is None:
            gd = self._slot_rows[i] = GameData(self, i)
        return gd

    def push_inference(self, i):
        gd = self.game_data(i)
        self.update_inferences(0, [int(i)], gd._v[None, :], gd._pi[None, :])
    def _groups(self):
        g, p = C.c_uint32(), C.c_uint32()
        check(lib.azmi_pm_groups(self._h, C.byref(g), C.byref(p)))
        return g.value, p.value

    def num_model_groups(self): return self._groups()[0]   # play_manager.h:210
    def num_seat_perms(self): return self._groups()[1]     # play_manager.h:211

    def perm_scores(self, idx):                            # play_manager.h:212-214
        out = np.zeros(self._P + 1, np.float32)
        check(lib.azmi_pm_perm_scores(self._h, int(idx), out.ctypes.data, None))
        return out

    def perm_games_completed(self, idx):                   # play_manager.h:215-217
        n = C.c_uint32()
        check(lib.azmi_pm_perm_scores(self._h, int(idx), None, C.byref(n)))
        return n.value

    def build_batch(self, group, batch, shard=0):
        """py_wrapper.cc:449-504: fills the caller's [max_batch, C, H, W] float32 array, returns slot ids."""
        arr = np.asarray(batch) if not hasattr(batch, "numpy") else batch.numpy()
        if arr.ndim != 4 or tuple(arr.shape[1:]) != tuple(self._chw) or arr.dtype != np.float32 or not arr.flags.c_contiguous:
            raise RuntimeError("Improper batch size")
        idx = np.zeros(arr.shape[0], np.uint32)
        n = C.c_uint32()
        cap = min(arr.shape[0], int(self._params.max_batch_size)) if self._params.max_batch_size else arr.shape[0]
        check(lib.azmi_pm_build_batch_group(self._h, int(group), arr.ctypes.data, cap, idx.ctypes.data, C.byref(n)))
        return [int(i) for i in idx[: n.value]]

    def update_inferences(self, group, indices, v, pi):
        idx = np.ascontiguousarray(indices, dtype=np.uint32)
        v = _f32(v); pi = _f32(pi)
        if v.shape != (len(idx), self._P + 1) or pi.shape != (len(idx), self._M):
            raise RuntimeError("Eigen is angry!!!")  # shapes.h:4-6 bounds assertion
        check(lib.azmi_pm_update_inferences(self._h, idx.ctypes.data, len(idx), v.ctypes.data, pi.ctypes.data))

    def build_history_batch(self, canonical, v, pi):
        """py_wrapper.cc:393-424: fills the caller arrays with finished samples, returns rows written."""
        c = np.asarray(canonical); vv = np.asarray(v); p = np.asarray(pi)
        for a in (c, vv, p):
            if a.dtype != np.float32 or not a.flags.c_contiguous:
                raise RuntimeError("history buffers must be C-contiguous float32")
        n = C.c_uint32()
        check(lib.azmi_pm_pop_history(self._h, c.ctypes.data, vv.ctypes.data, p.ctypes.data, c.shape[0], C.byref(n)))
        return n.value

    # ---- device fast path ------------------------------------------------------------------
    def _stream_arg(self, stream):
        """None -> the stream of the previous call (initially the engine's own); an int (0 included, the HIP
        null stream) -> that hipStream_t."""
        if stream is None:
            return self._last_stream
        self._last_stream = C.c_void_p(int(stream))
        return self._last_stream

    def round(self, stream=None):
        """One engine round on `stream` (a hipStream_t as int, e.g. torch.cuda.current_stream().cuda_stream)."""
        check(lib.azmi_pm_round(self._h, self._stream_arg(stream)))

    def net_forward(self, net, stream=None):
        """The HIP leaf net on this engine's leaf batch, restricted to the rows the last round listed as needing
        an evaluation (azmi_pm_net_forward); `net` is a HipLeafNet."""
        if isinstance(net, (list, tuple)):     # one HipLeafNet per model group
            for g, one in enumerate(net):
                check(lib.azmi_pm_net_forward_group(self._h, g, one._h, self._stream_arg(stream)))
        else:
            check(lib.azmi_pm_net_forward(self._h, net._h, self._stream_arg(stream)))

    def round_net(self, net, stream=None, part=0):
        """One round with its leaf evaluation exactly as the native loop (run_rounds) issues it (azmi_pm_round_net):
        part 0 = all of it, 1 = the tree half, 2 = the net half (with the move step of a split round fused in)."""
        check(lib.azmi_pm_round_net(self._h, net._h, self._stream_arg(stream), int(part)))

    def poll(self, stream=None):
        done, live = C.c_uint32(), C.c_uint32()
        check(lib.azmi_pm_poll(self._h, self._stream_arg(stream), C.byref(done), C.byref(live)))
        return done.value, live.value

    def io_pointers(self):
        c, v, p = C.c_void_p(), C.c_void_p(), C.c_void_p()
        check(lib.azmi_pm_io_buffers(self._h, C.byref(c), C.byref(v), C.byref(p)))
        return c.value, v.value, p.value

    def io_tensors(self):
        """torch views (no copy) of the slot-indexed canonical / v / pi buffers in HBM."""
        import torch
        from ._torch_view import device_tensor
        c, v, p = self.io_pointers()
        S = self._S
        dev = torch.device("cuda", torch.cuda.current_device())
        return (device_tensor(c, (S,) + tuple(self._chw), torch.float32, dev),
                device_tensor(v, (S, self._P + 1), torch.float32, dev),
                device_tensor(p, (S, self._M), torch.float32, dev))

    def history_device_tensors(self, dev=None):
        """Finished samples left in HBM as torch views: canonical [n,C,H,W], v [n,P+1], pi [n,M], meta [n,4] u32."""
        import torch
        from ._torch_view import device_tensor
        c, v, p, m = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        rows = C.c_uint32()
        check(lib.azmi_pm_history_device(self._h, C.byref(c), C.byref(v), C.byref(p), C.byref(m), C.byref(rows)))
        n = rows.value
        # these are views of the ring's first rows: only the whole story while nothing has been consumed and nothing has wrapped
        first, live, cap = C.c_uint32(), C.c_uint32(), C.c_uint32()
        check(lib.azmi_pm_history_window(self._h, C.byref(first), C.byref(live), C.byref(cap)))
        if first.value != 0 or live.value != n:
            raise RuntimeError("history_device_tensors: rows of this engine's sample ring have been consumed or overwritten; "
                               "read it with take_history_device()")
        dev = dev or torch.device("cuda", torch.cuda.current_device())
        if n == 0:
            z = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)
            return z(0, *self._chw), z(0, self._P + 1), z(0, self._M), torch.zeros((0, 4), dtype=torch.int32, device=dev)
        return (device_tensor(c.value, (n,) + tuple(self._chw), torch.float32, dev),
                device_tensor(v.value, (n, self._P + 1), torch.float32, dev),
                device_tensor(p.value, (n, self._M), torch.float32, dev),
                device_tensor(m.value, (n, 4), torch.int32, dev))

    def take_history_device(self, dev=None, consume=True):
        """The UNREAD finished samples as device tensors (canonical, v, pi, meta) — copies out of the engine's ring
        (azmi_pm_history_window: the window may wrap) — and, with `consume`, their release (azmi_pm_history_consume): the
        device-side counterpart of build_history_batch for the RCCL sample gather and for long self-play streams."""
        import torch
        from ._torch_view import device_tensor
        first, rows, cap = C.c_uint32(), C.c_uint32(), C.c_uint32()
        check(lib.azmi_pm_history_window(self._h, C.byref(first), C.byref(rows), C.byref(cap)))
        n, f, cp = rows.value, first.value, cap.value
        dev = dev or torch.device("cuda", torch.cuda.current_device())
        if n == 0:
            z = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)
            return z(0, *self._chw), z(0, self._P + 1), z(0, self._M), torch.zeros((0, 4), dtype=torch.int32, device=dev)
        c, v, p, m = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        check(lib.azmi_pm_history_device(self._h, C.byref(c), C.byref(v), C.byref(p), C.byref(m), None))
        full = (device_tensor(c.value, (cp,) + tuple(self._chw), torch.float32, dev),
                device_tensor(v.value, (cp, self._P + 1), torch.float32, dev),
                device_tensor(p.value, (cp, self._M), torch.float32, dev),
                device_tensor(m.value, (cp, 4), torch.int32, dev))
        n1 = min(n, cp - f)
        out = tuple(torch.cat([t[f:f + n1], t[:n - n1]], 0) if n1 < n else t[f:f + n].clone() for t in full)
        if consume:
            # the copies above run on torch's current stream, asynchronously: the rows may only be released to the engine
            # (whose later rounds overwrite them) once they have been read
            torch.cuda.current_stream(dev).synchronize()
            check(lib.azmi_pm_history_consume(self._h, n))
        return out

    def move_log(self):
        cap = (int(self._params.games_to_play) + self._S) * 512
        rows = np.zeros((cap, 8), np.uint32)
        counts = np.zeros((cap, self._M), np.uint32)
        n = C.c_uint32()
        check(lib.azmi_pm_move_log(self._h, rows.ctypes.data, counts.ctypes.data, cap, C.byref(n)))
        return rows[: n.value].copy(), counts[: n.value].copy()

    def slot_games(self):
        out = np.zeros(self._S, np.uint32)
        check(lib.azmi_pm_slot_games(self._h, out.ctypes.data))
        return out

    def history(self):
        """All finished samples not yet popped, as numpy arrays (canonical, v, pi)."""
        n = self.hist_count()
        c = np.zeros((n,) + tuple(self._chw), np.float32)
        v = np.zeros((n, self._P + 1), np.float32)
        p = np.zeros((n, self._M), np.float32)
        got = self.build_history_batch(c, v, p) if n else 0
        return c[:got], v[:got], p[:got]
