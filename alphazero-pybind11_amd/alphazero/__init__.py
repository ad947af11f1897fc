"""`alphazero` — host-side mirror of the reference's pybind11 module
(/root/reference/src/py_wrapper.cc:108-788) for the self-play hot path, backed by
the MI355X engine in libazmi.so (include/azmi.h).

Same names, argument meaning and error behaviour as the reference for
PlayParams / EvalType / PlayManager and the game classes' static facts, so
`game_runner.py`-style callers work unchanged; plus the device fast path the
reference lacks (`PlayManager.round`, `io_tensors`).

Put the directory that contains this package on sys.path:
    sys.path.insert(0, "<repo>/alphazero-pybind11_amd"); import alphazero

This file only re-exports; the code lives in the sibling modules (params, games, mcts, search_batch_sweep, search_batch_pool,
search_batch_frontier, search_batch, opening_tree, evaluators, cache, play_manager, drivers, samples), whose imports follow that order
and never form a cycle; _args (the shared argument checks) and _rng (the seed derivations of csrc/dev_rng.h) import none of them.
"""
from . import _capi
from ._capi import lib, check
from .params import EvalType, PlayParams, PlayHistory
from .games import (GameState, Connect4GS, _TaflBoardGS, TawlbwrddGS, BrandubhGS, OpenTaflGS, UnitInfo, StarGambitUnifiedGS, _pinned_sg,
                    StarGambitUnifiedSkirmishGS, StarGambitUnifiedShowdownGS, StarGambitUnifiedClashGS, StarGambitUnifiedBattleGS,
                    _StarGambitPlainGS, StarGambitSkirmishGS, StarGambitShowdownGS, StarGambitClashGS, StarGambitBattleGS, StarGambitGS,
                    _c4_from_bytes, _tafl_from_bytes, _sg_from_bytes, hash_game_state, game_replay, symmetries_batch, tafl_symmetries)
from .mcts import MCTS, Query, _ENGINE_STREAM
from .search_batch_sweep import policy_divergences, POLICY_COLUMNS, SWEEP_COLUMNS
from .search_batch_pool import pool_unique
from .search_batch import MCTSBatch
from .opening_tree import build_opening_tree, OpeningTree, OpeningNode, temperature_at_depth, node_seed
from .evaluators import dumb_eval, playout_eval_batch, playout_eval
from .cache import ShardedS3FIFOCache, S3FIFOCache, cached_forward
from .play_manager import GameData, PlayManager, _f32
from .drivers import (run_rounds, run_rounds_groups, pipeline_supported, pipeline_supported_groups, run_pipeline, run_pipeline_groups,
                      _pipe_stats, _PIPE_KEYS, pipeline_log_duplicates, cache_find_group, cache_insert_locked, rng_probe, tracy_is_enabled, tracy_frame_mark,
                      _tracy_zone_begin, _tracy_zone_end, _tracy_set_thread_name)
from . import samples
from .samples import (sample_loss, resample_plan, resample_rows, resample_by_surprise, iteration_losses, sample_metrics, plane_argmax,
                      eval_metrics, analyze_samples, reservoir_keys, select_top, window_batches, SampleWindow, feature_rank, effective_rank)


def __getattr__(name):  # torch-dependent pieces are imported on first use
    if name == "HipLeafNet":
        from .hip_net import HipLeafNet
        return HipLeafNet
    raise AttributeError(name)

__all__ = [
    "EvalType", "PlayParams", "PlayManager", "GameState", "Connect4GS", "TawlbwrddGS", "S3FIFOCache", "ShardedS3FIFOCache",
    "tracy_is_enabled", "tracy_frame_mark",
]
