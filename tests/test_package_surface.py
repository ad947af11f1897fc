"""CPU: the `alphazero` package is split into modules behind an unchanged surface.  Every name the one-file package exposed still
resolves, importing it does not import torch, the read-out kinds carry the device's names and values, and the unpicklers that
pickles written before the split name are the ones of alphazero.games."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "alphazero-pybind11_amd")

# dir(alphazero) of the last one-file package, without dunders and the stdlib / numpy modules it imported (C, enum, os, struct, np)
SURFACE = (
    "BrandubhGS", "Connect4GS", "EvalType", "GameData", "GameState", "MCTS", "MCTSBatch", "OpenTaflGS", "PlayHistory", "PlayManager",
    "PlayParams", "S3FIFOCache", "ShardedS3FIFOCache", "StarGambitBattleGS", "StarGambitClashGS", "StarGambitGS", "StarGambitShowdownGS",
    "StarGambitSkirmishGS", "StarGambitUnifiedBattleGS", "StarGambitUnifiedClashGS", "StarGambitUnifiedGS", "StarGambitUnifiedShowdownGS",
    "StarGambitUnifiedSkirmishGS", "TawlbwrddGS", "UnitInfo", "_ENGINE_STREAM", "_PIPE_KEYS", "_StarGambitPlainGS", "_TaflBoardGS",
    "_c4_from_bytes", "_capi", "_f32", "_pinned_sg", "_pipe_stats", "_sg_from_bytes", "_tafl_from_bytes", "_tracy_set_thread_name",
    "_tracy_zone_begin", "_tracy_zone_end", "check", "dumb_eval", "game_replay", "hash_game_state", "lib", "pipeline_log_duplicates",
    "pipeline_supported", "pipeline_supported_groups", "playout_eval", "playout_eval_batch", "rng_probe", "run_pipeline",
    "run_pipeline_groups", "run_rounds", "run_rounds_groups", "symmetries_batch", "tafl_symmetries", "tracy_frame_mark", "tracy_is_enabled",
)


@pytest.fixture(scope="module")
def az():
    import __graft_entry__ as g
    g.build()
    import alphazero
    return alphazero


def test_every_name_of_the_one_file_package_still_resolves(az):
    missing = [n for n in SURFACE if not hasattr(az, n)]
    assert not missing, f"no longer attributes of alphazero: {missing}"


def test_importing_the_package_does_not_import_torch(az):
    code = "import sys; sys.path.insert(0, %r); import alphazero; print('torch' in sys.modules)" % PKG
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == "False", "import alphazero pulled in torch"


def test_query_kinds_are_the_device_enum(az):
    header = open(os.path.join(PKG, "csrc", "search_batch_types.h")).read()
    body = re.search(r"enum\s+MctsQuery\b[^{]*\{(.*?)\}", header, re.S).group(1)
    device = {re.sub(r"(?<!^)(?=[A-Z])", "_", name).upper(): int(value) for name, value in re.findall(r"\bkQ(\w+)\s*=\s*(\d+)", body)}
    assert len(device) == 14 and device["COUNTS"] == 0 and device["ROOT_CHILDREN"] == 13, device
    assert {m.name: int(m) for m in az.Query} == device
    assert len(az.Query.__members__) == len(device), "an alias in Query"


def test_pickles_written_before_the_split_find_their_unpicklers(az):
    from alphazero import games
    for name in ("_c4_from_bytes", "_tafl_from_bytes", "_sg_from_bytes"):
        assert getattr(az, name) is getattr(games, name), name
