"""The stand-alone search tree on the device (azmi_mcts_*) and the names of its read-out kinds."""
import ctypes as C
import enum
import os

import numpy as np

from . import _capi
from ._capi import lib, check
from .games import Connect4GS


_ENGINE_STREAM = C.c_void_p(-1)  # AZMI_STREAM_ENGINE


class Query(enum.IntEnum):
    """The read-out kinds of azmi_mcts_query / azmi_search_query: enum MctsQuery (kQCounts ... kQRootChildren) of
    csrc/mcts_object_kernels.h, same names and values (tests/test_package_surface.py compares the two)."""
    COUNTS = 0
    PROBS = 1
    PROBS_PRUNED = 2
    ROOT_VALUE = 3
    ROOT_Q = 4
    SCALARS = 5                # u: depth, root_n; f: avg_leaf_depth, normalized_root_entropy
    GUMBEL_POLICY = 6
    GUMBEL_FINAL = 7
    ADD_ROOT_NOISE = 8
    APPLY_ROOT_TEMP = 9
    PICK_MOVE = 10
    PRINCIPAL_VARIATION = 11
    SET_GUMBEL_SIMS = 12
    ROOT_CHILDREN = 13


class MCTS:
    """The stand-alone search tree (py_wrapper.cc:192-220, mcts.h:50-200) on the device: find_leaf / process_result /
    update_root and the read-outs, call by call; pass game=<GS class> for anything but Connect4.  `seed` seeds the object's pcg32 stream (the
    reference shares one unseedable-from-Python thread_local stream; its C++ tests call MCTS::seed_thread_rng)."""

    def __init__(self, cpuct, num_players, num_moves, epsilon=0.0, root_policy_temp=1.0, fpu_reduction=0.0,
                 relative_values=False, root_fpu_zero=False, shaped_dirichlet=False, gumbel_enabled=False, gumbel_m=16,
                 gumbel_c_visit=50.0, gumbel_c_scale=1.0, gumbel_full=False, *, game=None, seed=None, device=0,
                 max_simulations=0):
        game = Connect4GS if game is None else (game if isinstance(game, type) else type(game))
        cfg = _capi.MctsConfigC(cpuct, num_players, num_moves, epsilon, root_policy_temp, fpu_reduction, int(relative_values),
                                int(root_fpu_zero), int(shaped_dirichlet), int(gumbel_enabled), gumbel_m, gumbel_c_visit,
                                gumbel_c_scale, int(gumbel_full), int(max_simulations))
        if seed is None:
            seed = int.from_bytes(os.urandom(8), "little")     # std::random_device, mcts.cc:19
        h = C.c_void_p()
        check(lib.azmi_mcts_create(game.GAME_ID, C.byref(cfg), C.c_uint64(seed), int(device), C.byref(h)))
        self._h, self._game, self._P, self._M = h, game, num_players, num_moves
        self._gumbel = bool(gumbel_enabled)
        self._vec = max(num_moves, 64)

    def __del__(self):
        if getattr(self, "_h", None) and lib is not None:
            lib.azmi_mcts_destroy(self._h)
            self._h = None

    @staticmethod
    def _gs_args(gs):
        init = None if gs._init is None else np.frombuffer(gs._init, np.uint8)
        mv = np.array(gs._moves, dtype=np.int32)
        return init, mv

    def _descend(self, entry, gs):
        """find_leaf / find_leaf_batched: one descent from `gs` through the C entry point `entry` -> the leaf's state"""
        init, mv = self._gs_args(gs)
        out = np.zeros(512, np.int32)
        n = C.c_uint32()
        check(entry(self._h, None if init is None else init.ctypes.data, 0 if init is None else init.size,
                    mv.ctypes.data if mv.size else None, mv.size, out.ctypes.data, out.size, C.byref(n)))
        leaf = gs.copy()
        for m in out[: n.value]:
            leaf._moves.append(int(m))
        leaf._snap = None
        return leaf

    def _back_up(self, what, entry, head, value, pi, root_noise_enabled):
        """process_result / process_result_batched (`what` names the caller in the error text): `entry` takes the handle,
        the integers of `head`, then value, pi, the noise flag and the row the backed-up value is written to"""
        v = np.ascontiguousarray(value, dtype=np.float32); p = np.ascontiguousarray(pi, dtype=np.float32)
        if v.shape != (self._P + 1,) or p.shape != (self._M,):
            raise RuntimeError(f"{what}: value must be [num_players + 1] and pi [num_moves]")
        out = np.zeros(self._P + 1, np.float32)
        check(entry(self._h, *(int(x) for x in head), v.ctypes.data, p.ctypes.data, int(bool(root_noise_enabled)), out.ctypes.data))
        if isinstance(value, np.ndarray) and value.dtype == np.float32:
            value[...] = out
        return out

    def find_leaf(self, gs):
        return self._descend(lib.azmi_mcts_find_leaf, gs)

    def process_result(self, gs, value, pi, root_noise_enabled=False):
        """value is updated in place like the reference's by-reference argument (terminal leaves: the cached scores)."""
        return self._back_up("process_result", lib.azmi_mcts_process_result, (), value, pi, root_noise_enabled)

    def update_root(self, gs, move):
        init, mv = self._gs_args(gs)
        check(lib.azmi_mcts_update_root(self._h, None if init is None else init.ctypes.data, 0 if init is None else init.size,
                                        mv.ctypes.data if mv.size else None, mv.size, int(move)))

    def _query(self, kind, temp=0.0, arg=0, in_f=None):
        f = np.zeros(self._vec, np.float32); u = np.zeros(self._vec + 64, np.uint32)
        inp = None if in_f is None else np.ascontiguousarray(in_f, dtype=np.float32)
        check(lib.azmi_mcts_query(self._h, kind, float(temp), int(arg), None if inp is None else inp.ctypes.data, f.ctypes.data, u.ctypes.data))
        return f, u

    def counts(self): return self._query(Query.COUNTS)[1][: self._M].copy()
    def probs(self, temp): return self._query(Query.PROBS, temp)[0][: self._M].copy()
    def probs_pruned(self, temp): return self._query(Query.PROBS_PRUNED, temp)[0][: self._M].copy()
    def root_value(self): return self._query(Query.ROOT_VALUE)[0][:3].copy()
    def root_q_values(self): return self._query(Query.ROOT_Q)[0][: self._M].copy()
    def depth(self): return int(self._query(Query.SCALARS)[1][0])
    def root_n(self): return int(self._query(Query.SCALARS)[1][1])
    def avg_leaf_depth(self): return float(self._query(Query.SCALARS)[0][0])
    def normalized_root_entropy(self): return float(self._query(Query.SCALARS)[0][1])
    def gumbel_enabled(self): return self._gumbel
    def gumbel_improved_policy(self): return self._query(Query.GUMBEL_POLICY)[0][: self._M].copy()
    def gumbel_final_action(self): return int(self._query(Query.GUMBEL_FINAL)[1][0])
    def add_root_noise(self): self._query(Query.ADD_ROOT_NOISE)
    def apply_root_policy_temp(self): self._query(Query.APPLY_ROOT_TEMP)
    def set_gumbel_num_sims(self, n): self._query(Query.SET_GUMBEL_SIMS, arg=n)

    def principal_variation(self, depth=5):
        u = self._query(Query.PRINCIPAL_VARIATION, arg=depth)[1]
        return u[1: 1 + int(u[0])].copy()

    def pick_move(self, pi):
        """MCTS::pick_move (static in the reference, drawing from the thread's stream): draws from this object's stream."""
        return int(self._query(Query.PICK_MOVE, in_f=pi)[1][0])

    # ---- WU-UCT batched API (py_wrapper.cc:212-215, mcts.cc:752-851) ----
    def find_leaf_batched(self, gs):
        return self._descend(lib.azmi_mcts_find_leaf_batched, gs)

    def process_result_batched(self, gs, leaf_index, value, pi, root_noise_enabled=False):
        return self._back_up("process_result_batched", lib.azmi_mcts_process_result_batched, (leaf_index,), value, pi, root_noise_enabled)

    def in_flight_count(self):
        n = C.c_uint32()
        check(lib.azmi_mcts_in_flight_count(self._h, C.byref(n)))
        return n.value

    def reset_batch(self):
        check(lib.azmi_mcts_reset_batch(self._h))
