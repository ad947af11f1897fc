"""EvalType, PlayParams (and its marshalling into the C struct) and PlayHistory."""
import ctypes as C
import enum

import numpy as np

from . import _capi
from ._capi import lib


class EvalType(enum.IntEnum):  # py_wrapper.cc:290-293
    NN = 0
    RANDOM = 1
    PLAYOUT = 2


class PlayParams:
    """py_wrapper.cc:295-349 / play_manager.h:60-154 — same field names and defaults."""

    def __init__(self):
        self.games_to_play = 0
        self.concurrent_games = 0
        self.max_batch_size = 1
        self.max_cache_size = 0
        self.cache_shards = 1
        self.queue_shards = 1
        self.eval_pipelines = 1
        self.mcts_visits = []
        self.cpuct = 2.0
        self.start_temp = 1.0
        self.final_temp = 1.0
        self.temp_decay_half_life = 0.0
        self.temp_decay_half_life_by_variant = []
        self.history_enabled = False
        self.self_play = False
        self.tree_reuse = True
        self.epsilon = 0.0
        self.mcts_root_temp = 1.0
        self.playout_cap_randomization = False
        self.playout_cap_depth = 25
        self.playout_cap_percent = 0.75
        self.fpu_reduction = 0.0
        self.root_fpu_zero = False
        self.shaped_dirichlet = False
        self.policy_target_pruning = False
        self.gumbel_enabled = False
        self.gumbel_m = 16
        self.gumbel_c_visit = 50.0
        self.gumbel_c_scale = 1.0
        self.gumbel_full = False
        self.fast_search_uses_gumbel = False
        self.resign_percent = 0.0
        self.resign_playthrough_percent = 0.0
        self.eval_type = []
        self.model_groups = []
        self.seat_perms = []
        self.seat_visits = []
        self.seat_cap_visits = []
        self.seat_epsilon = []
        self.seat_mcts_root_temp = []
        self.seat_root_fpu_zero = []
        self.seat_gumbel_enabled = []
        self.seat_gumbel_m = []
        self.seat_gumbel_c_visit = []
        self.seat_gumbel_c_scale = []
        self.seat_gumbel_full = []
        self.seat_gumbel_use_improved_policy = []
        self.seat_resign_threshold = []
        self.seat_resign_consecutive = []

    # fields the device engine does not implement yet: anything but the default is an error.
    # (temp_decay_half_life_by_variant is NOT one of them: play_manager.cc:289-296 applies entry get_variant_id() only when
    # that id is >= 0, and every device game answers -1 (game_state.h:79), so the reference itself ignores the list there.)
    _UNSUPPORTED = ()

    def _to_c(self, num_players):
        c = _capi.PlayParamsC()
        lib.azmi_play_params_default(C.byref(c))
        for name in self._UNSUPPORTED:
            if getattr(self, name):
                raise RuntimeError(f"PlayParams.{name} is not supported by the MI355X engine yet")
        # model groups / seat permutations / per-seat matrices: same validation messages as play_manager.cc:57-113
        groups = [int(g) for g in self.model_groups]
        if groups and len(groups) != num_players:
            raise RuntimeError("model_groups must be empty or have one entry per player")
        perms = [[int(g) for g in row] for row in self.seat_perms]
        if len(perms) > _capi.AZMI_MAX_PERMS:
            raise RuntimeError(f"at most {_capi.AZMI_MAX_PERMS} seat permutations")
        n_perms = len(perms) if perms else 1
        c.num_model_groups_given = len(groups)
        for i, g in enumerate(groups):
            c.model_groups[i] = g
        c.num_seat_perms = len(perms)
        for q, row in enumerate(perms):
            if len(row) != num_players:
                raise RuntimeError("seat_perms inner dimension must match number of players")
            for sidx, g in enumerate(row):
                c.seat_perms[q][sidx] = g
        for name, cast in (("seat_visits", int), ("seat_cap_visits", int), ("seat_epsilon", float),
                           ("seat_mcts_root_temp", float), ("seat_root_fpu_zero", int),
                           ("seat_gumbel_enabled", int), ("seat_gumbel_m", int), ("seat_gumbel_c_visit", float),
                           ("seat_gumbel_c_scale", float), ("seat_gumbel_full", int), ("seat_gumbel_use_improved_policy", int),
                           ("seat_resign_threshold", float), ("seat_resign_consecutive", int)):
            mat = [list(row) for row in getattr(self, name)]
            setattr(c, "has_" + name, int(bool(mat)))
            if not mat:
                continue
            if len(mat) != n_perms:
                raise RuntimeError(f"{name} outer dimension must match number of seat permutations")
            for q, row in enumerate(mat):
                if len(row) != num_players:
                    raise RuntimeError(f"{name} inner dimension must match number of players")
                for sidx, x in enumerate(row):
                    getattr(c, name)[q][sidx] = cast(x)
        c.games_to_play = int(self.games_to_play)
        c.concurrent_games = int(self.concurrent_games)
        c.max_batch_size = int(self.max_batch_size)
        c.max_cache_size = int(self.max_cache_size)
        c.cache_shards = int(self.cache_shards)
        visits = list(self.mcts_visits)
        if len(visits) > _capi.AZMI_MAX_PLAYERS:
            raise RuntimeError("You must specify MCTS visits for each player")
        c.num_mcts_visits = len(visits)
        for i, v in enumerate(visits):
            c.mcts_visits[i] = int(v)
        c.cpuct = self.cpuct
        c.start_temp = self.start_temp
        c.final_temp = self.final_temp
        c.temp_decay_half_life = self.temp_decay_half_life
        hl = [float(x) for x in self.temp_decay_half_life_by_variant]     # play_manager.h:87-90 (entry get_variant_id())
        if len(hl) > 4:
            raise RuntimeError("temp_decay_half_life_by_variant: at most 4 variants")
        c.num_temp_decay_half_life_by_variant = len(hl)
        for i, x in enumerate(hl):
            c.temp_decay_half_life_by_variant[i] = x
        c.history_enabled = int(bool(self.history_enabled))
        c.self_play = int(bool(self.self_play))
        c.tree_reuse = int(bool(self.tree_reuse))
        c.epsilon = self.epsilon
        c.mcts_root_temp = self.mcts_root_temp
        c.playout_cap_randomization = int(bool(self.playout_cap_randomization))
        c.playout_cap_depth = int(self.playout_cap_depth)
        c.playout_cap_percent = self.playout_cap_percent
        c.fpu_reduction = self.fpu_reduction
        c.root_fpu_zero = int(bool(self.root_fpu_zero))
        c.shaped_dirichlet = int(bool(self.shaped_dirichlet))
        c.policy_target_pruning = int(bool(self.policy_target_pruning))
        c.resign_percent = self.resign_percent
        c.resign_playthrough_percent = self.resign_playthrough_percent
        c.gumbel_enabled = int(bool(self.gumbel_enabled))
        c.gumbel_m = int(self.gumbel_m)
        c.gumbel_c_visit = float(self.gumbel_c_visit)
        c.gumbel_c_scale = float(self.gumbel_c_scale)
        c.gumbel_full = int(bool(self.gumbel_full))
        c.fast_search_uses_gumbel = int(bool(self.fast_search_uses_gumbel))
        ets = list(self.eval_type)
        c.num_eval_type = len(ets)
        for i, e in enumerate(ets[: _capi.AZMI_MAX_PLAYERS]):
            c.eval_type[i] = int(e)
        return c


class PlayHistory:
    """One training sample (game_state.h:31-35, py_wrapper.cc:111-155): canonical [C,H,W], v [P+1], pi [M]."""

    def __init__(self, canonical, v, pi):
        if canonical is None or v is None or pi is None:
            raise TypeError("PlayHistory(canonical, v, pi): arguments must not be None")
        self._c = np.array(canonical, dtype=np.float32, order="C")
        self._v = np.array(v, dtype=np.float32).reshape(-1)
        self._pi = np.array(pi, dtype=np.float32).reshape(-1)
        if self._c.ndim != 3:
            raise RuntimeError("PlayHistory: canonical must have 3 dimensions")

    def canonical(self):
        return memoryview(self._c)

    def v(self):
        return self._v

    def pi(self):
        return self._pi
