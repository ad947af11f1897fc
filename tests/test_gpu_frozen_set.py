"""-m gpu: a frozen evaluation set on the device - root capture during play(), first-occurrence dedup (pool_unique /
position_pool / pool_states / sample_pool) and net_vs_search, the parts of the reference's frozen_eval.py around its search
loop (frozen_eval.py:330-413, 509-514, 573-575, 649-672).  The expected pools are rebuilt in Python from move_logs() with the
device rules (hash_game_state); the expected metrics are a float64 numpy restatement of the reference lines fed with the
batch's own read-outs."""
import os
import random

import numpy as np
import pytest

from test_gpu_search_batch import _c4_at, az  # noqa: F401
from test_gpu_search_batch_play import _C4_LAST_CELL

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = 0x9E3779B97F4A7C15


# ---- 1. azmi_pool_unique against numpy -----------------------------------------------------------------------------------
def _expect_unique(keys, valid=None):
    keys = np.asarray(keys, np.uint64)
    idx = np.arange(keys.size) if valid is None else np.flatnonzero(valid)
    if idx.size == 0:
        return np.zeros(0, np.uint32), 0
    _, first = np.unique(keys[idx], return_index=True)
    return np.sort(idx[first]).astype(np.uint32), int(idx.size - first.size)


_RNG = np.random.default_rng(20261019)
_BIG = _RNG.integers(0, 2 ** 64, 20000, dtype=np.uint64)[_RNG.integers(0, 20000, 70000)]
_POOL_CASES = {
    "n = 0": (np.zeros(0, np.uint64), None),
    "n = 1": (np.array([77], np.uint64), None),
    "all equal": (np.full(300, 5, np.uint64), None),
    "all distinct": (np.arange(1000, dtype=np.uint64) * np.uint64(GOLDEN), None),
    "key 0 is a key": (np.array([0, 0, GOLDEN, 0], np.uint64), None),
    "high halves differ": ((np.arange(500, dtype=np.uint64) % np.uint64(50)) << np.uint64(32), None),
    "low halves differ": ((np.uint64(0xABCDEF01) << np.uint64(32)) | (np.arange(500, dtype=np.uint64) % np.uint64(50)), None),
    "70000 of 20000": (_BIG, None),
    "70000 of 20000, every third invalid": (_BIG, np.arange(70000) % 3 != 0),
}


@pytest.mark.parametrize("case", list(_POOL_CASES))
def test_pool_unique_is_numpy_first_occurrence(az, case):
    keys, valid = _POOL_CASES[case]
    want, want_dups = _expect_unique(keys, valid)
    got, dups = az.pool_unique(keys, valid)
    assert got.dtype == np.uint32 and np.array_equal(got, want) and dups == want_dups, case
    if case == "key 0 is a key":
        assert got.tolist() == [0, 2] and dups == 2
    again, dups2 = az.pool_unique(keys, valid)        # the same input twice: the same output
    assert np.array_equal(again, got) and dups2 == dups


# ---- 2. / 3. capture against a Python rebuild ------------------------------------------------------------------------------
def _keys_players(az, states):
    """hash_game_state and current_player of many states: one rules replay for states that start from their game's initial
    position (what GameState._state() runs per object), the objects themselves otherwise"""
    if not states:
        return [], []
    if all(g._init is None for g in states):
        moves = -np.ones((len(states), max(len(g._moves) for g in states) + 1), np.int32)
        for r, g in enumerate(states):
            moves[r, : len(g._moves)] = g._moves
        out = az.game_replay(type(states[0]), moves)
        assert (out["status"] == 0).all()
        return out["key"].tolist(), out["player"].tolist()
    return [az.hash_game_state(g) for g in states], [g.current_player() for g in states]


def _expected_pool(az, start, logs):
    """first-occurrence dedup, in (tree, ply) order, of hash_game_state(start[i] + logs[i][:ply]) for every ply tree i was live
    at: a root is recorded before its search, so the plies 0 .. len(log) - 1 -> rows (tree, ply, key, player, variant), records"""
    where, states = [], []
    for i, (g0, lg) in enumerate(zip(start, logs)):
        for ply in range(len(lg)):
            g = g0.copy()
            g._moves.extend(int(m) for m in lg[:ply])
            g._snap = None
            where.append((i, ply)); states.append(g)
    keys, players = _keys_players(az, states)
    seen, rows = set(), []
    for (i, ply), key, player, g in zip(where, keys, players, states):
        if key not in seen:
            seen.add(key)
            rows.append((i, ply, key, player, g.get_variant_id()))
    return rows, len(states)


def _assert_pool(az, mb, pool, start):
    logs = mb.move_logs()
    rows, captured = _expected_pool(az, start, logs)
    got = list(zip(pool["tree"].tolist(), pool["ply"].tolist(), pool["key"].tolist(), pool["player"].tolist(), pool["variant"].tolist()))
    assert got == rows
    assert pool["captured"] == captured and pool["duplicates"] == captured - len(rows)
    assert pool["key"].dtype == np.uint64 and pool["variant"].dtype == np.int8
    assert _keys_players(az, mb.pool_states(pool))[0] == pool["key"].tolist(), "pool_states does not round-trip"
    return logs


def _c4_batch(az, n=64, capture=False, budget=16 * 42):
    mb = az.MCTSBatch(az.Connect4GS, n, 1.25, max_simulations=budget, seeds=[7000 + 3 * i for i in range(n)], capture=capture)
    mb.reset([az.Connect4GS() for _ in range(n)])
    return mb


@pytest.fixture(scope="module")
def c4_games(az):
    """Connect4, 64 games from the initial position, RANDOM evaluator, 16 visits, play(max_moves=42, capture=True)"""
    mb = _c4_batch(az)
    l0 = mb.stats()["launches"]
    mb.play(16, temp=1.0, max_moves=42, capture=True)
    launches = mb.stats()["launches"] - l0
    return dict(mb=mb, pool=mb.position_pool(), launches=launches)


def test_connect4_capture_is_the_python_dedup(az, c4_games):
    mb, pool = c4_games["mb"], c4_games["pool"]
    assert mb.finished().all(), "42 moves end every Connect4 game"
    logs = _assert_pool(az, mb, pool, [az.Connect4GS() for _ in range(64)])
    assert pool["captured"] == sum(len(lg) for lg in logs)
    assert pool["duplicates"] >= 63, "every game shares ply 0"
    assert (pool["variant"] == -1).all() and pool["tree"][0] == 0 and pool["ply"][0] == 0
    rec = mb.sample_pool(pool, 10, np.random.default_rng(3))
    assert len(rec) == 10 and all(set(r) == {"gs", "variant", "move_number", "player"} for r in rec)
    assert all(r["gs"].current_player() == r["player"] and len(r["gs"]._moves) == r["move_number"] for r in rec)
    assert len(mb.sample_pool(pool, 10 ** 6)) == len(pool["tree"])


def _same_pool(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("tree", "ply", "key", "player", "variant")) and \
        (a["captured"], a["duplicates"]) == (b["captured"], b["duplicates"])


def test_two_half_plays_and_a_walk_give_the_same_pool(az, c4_games):
    two = _c4_batch(az, capture=True)
    two.play(16, max_moves=21)
    two.play(16, max_moves=21)
    assert _same_pool(two.position_pool(), c4_games["pool"])
    walk = _c4_batch(az)
    walk.set_capture(True)
    for _ in range(42):
        walk.capture_roots()
        walk.search(16)
        walk.pick_moves(1.0)
        walk.update_roots()
    assert _same_pool(walk.position_pool(), c4_games["pool"])
    walk.capture_roots()      # every tree is finished: nothing is recorded, and a ply written twice keeps its values
    assert _same_pool(walk.position_pool(), c4_games["pool"])
    walk.reset([az.Connect4GS() for _ in range(64)])
    empty = walk.position_pool()
    assert empty["captured"] == 0 and len(empty["tree"]) == 0, "reset() clears the captured lengths"


@pytest.mark.parametrize("name,n,visits,moves", [("BrandubhGS", 8, 8, 12), ("StarGambitUnifiedGS", 4, 4, 6)])
def test_wide_game_capture_and_the_variant_field(az, name, n, visits, moves):
    Game = getattr(az, name)
    random.seed(7)      # an unpinned StarGambit object draws its variant from Python's `random`
    start = [Game(-1, [0.25] * 4) if name == "StarGambitUnifiedGS" else Game() for _ in range(n)]
    mb = az.MCTSBatch(Game, n, 1.25, max_simulations=visits, seeds=[50 + i for i in range(n)], capture=True)
    mb.reset(start)
    mb.play(visits, max_moves=moves)
    pool = mb.position_pool()
    _assert_pool(az, mb, pool, start)
    want = [g.get_variant_id() for g in mb.pool_states(pool)]
    assert pool["variant"].tolist() == want
    if name == "BrandubhGS":
        assert set(want) == {-1}
    else:
        assert set(want) <= {0, 1, 2, 3} and pool["variant"][0] == start[0].get_variant_id()


# ---- 4. capture leaves play alone --------------------------------------------------------------------------------------------
def test_capture_leaves_play_alone(az, c4_games):
    on = c4_games["mb"]
    never = _c4_batch(az)
    l0 = never.stats()["launches"]
    never.play(16, max_moves=42)
    plain = never.stats()["launches"] - l0
    assert c4_games["launches"] == plain + 42, "capture is one launch per move"
    for a, b in zip(on.move_logs(), never.move_logs()):
        assert np.array_equal(a, b)
    assert np.array_equal(on.counts(), never.counts()) and np.array_equal(on.final_scores(), never.final_scores())
    off = _c4_batch(az, capture=True)      # had capture, turned off: what a batch that never had it launches
    off.set_capture(False)
    l1 = off.stats()["launches"]
    off.play(16, max_moves=42)
    assert off.stats()["launches"] - l1 == plain
    assert off.position_pool()["captured"] == 0
    with pytest.raises(RuntimeError, match="capture was never on"):
        never.position_pool()
    with pytest.raises(RuntimeError, match="capture is off"):
        never.capture_roots()
    never.search(0)      # still usable


# ---- 5. net versus search --------------------------------------------------------------------------------------------------
def _fixture_net(az, fname, spec_fn):
    import torch
    from alphazero import torch_net
    fx = np.load(os.path.join(HERE, "golden", fname))
    net = torch_net.LeafNet(getattr(torch_net, spec_fn)())
    net.load_state_dict({k[3:]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith("sd.")})
    return az.HipLeafNet(net.eval())


@pytest.fixture(scope="module")
def c4_fixture_net(az):
    return _fixture_net(az, "nn_connect4_6b64c.npz", "connect4_spec")


@pytest.fixture(scope="module")
def brandubh_fixture_net(az):
    return _fixture_net(az, "nn_brandubh_4b32c.npz", "brandubh_spec")


def _kl(p, q, eps=1e-10):      # frozen_eval.py:509-514, q widened to float64 first
    mask = p > 0
    if not mask.any():
        return 0.0
    return float(np.sum(p[mask] * np.log(p[mask] / (q[mask] + eps))))


def _assert_net_vs_search(az, mb, net, r, invalid):
    """r = mb.net_vs_search(net) against the raw forward of mb.states() and the numpy restatement of frozen_eval.py:653-671"""
    import torch
    n = len(mb)
    assert r["valid"].dtype == np.bool_ and r["valid"].tolist() == [i not in invalid for i in range(n)]
    states = mb.states()
    x = torch.from_numpy(np.stack([g.canonicalized() for g in states])).to(torch.device("cuda", 0))
    v, pi = net.process(x)      # the same rows in the same order and batch size
    torch.cuda.synchronize()
    v, pi = v.cpu().numpy(), pi.cpu().numpy()
    counts, rv = mb.counts(), mb.root_values()
    ok = r["valid"]
    assert np.array_equal(r["raw_v"][ok], v[ok]) and np.array_equal(r["raw_pi"][ok], pi[ok]), "raw forward is not bit-equal"
    for k in ("kl_mcts_net", "value_mae", "top1_agreement"):
        assert r[k].dtype == np.float64 and np.isnan(r[k][~ok]).all() and not np.isnan(r[k][ok]).any()
    assert np.isnan(r["raw_v"][~ok]).all() and np.isnan(r["raw_pi"][~ok]).all()
    worst = {"kl_mcts_net": 0.0, "value_mae": 0.0}
    for i in np.flatnonzero(ok):
        c = np.array(counts[i], dtype=np.float64)
        total = c.sum()
        pi_mcts = (c / total) if total > 0 else np.full_like(c, 1.0 / len(c))
        v_mcts = np.asarray(rv[i], dtype=np.float64)
        raw_v, raw_pi = r["raw_v"][i], r["raw_pi"][i]
        want = {"kl_mcts_net": _kl(pi_mcts, raw_pi.astype(np.float64)),
                "value_mae": float(np.mean(np.abs(raw_v[:len(v_mcts)] - v_mcts))),
                "top1_agreement": 1.0 if int(np.argmax(pi_mcts)) == int(np.argmax(raw_pi)) else 0.0}
        assert r["top1_agreement"][i] == want["top1_agreement"], f"tree {i}"
        for k in worst:
            d = abs(r[k][i] - want[k])
            worst[k] = max(worst[k], d / (1 + abs(want[k])))
            assert d <= 1e-9 * (1 + abs(want[k])), f"tree {i}: {k} {r[k][i]!r} vs {want[k]!r}"
    print("net_vs_search: worst |d| / (1 + |x|):", worst)
    for k in ("kl_mcts_net", "value_mae", "top1_agreement"):
        assert r["mean"][k] == float(r[k][ok].mean())


def test_connect4_net_vs_search(az, c4_games, c4_fixture_net):
    """64 trees: 63 distinct positions of a short capture, tree 0 never searched (total == 0), tree 63 played to the end"""
    n = 64
    short = _c4_batch(az, capture=True, budget=16 * 8)
    short.play(16, max_moves=8)
    pool = short.position_pool()
    assert len(pool["tree"]) >= n - 1
    states = short.pool_states(pool, range(n - 1)) + [_c4_at(az, _C4_LAST_CELL)]
    assert len({az.hash_game_state(g) for g in states}) == n
    mb = az.MCTSBatch(az.Connect4GS, n, 1.25, fpu_reduction=0.25, max_simulations=32, seeds=[900 + i for i in range(n)])
    mb.reset(states)
    last = int(np.flatnonzero(states[-1].valid_moves())[0])
    mb.update_roots([-1] * (n - 1) + [last])
    assert mb.finished().tolist() == [False] * (n - 1) + [True]
    mb.search_to([0] + [32] * (n - 1), net=c4_fixture_net)
    assert mb.root_ns()[0] == 0 and mb.counts()[0].sum() == 0 and (mb.root_ns()[1:-1] == 32).all()
    st0 = mb.stats()
    r = mb.net_vs_search(c4_fixture_net)
    st1 = mb.stats()
    assert st1["launches"] - st0["launches"] == 2 and st1["net_calls"] - st0["net_calls"] == 1, "root planes, the net, the comparison"
    _assert_net_vs_search(az, mb, c4_fixture_net, r, invalid={n - 1})
    # the read-outs the comparison went through are untouched, and the call repeats itself
    r2 = mb.net_vs_search(c4_fixture_net)
    for k in ("kl_mcts_net", "value_mae", "top1_agreement", "raw_v", "raw_pi"):
        assert np.array_equal(r[k], r2[k], equal_nan=True)


def _brandubh_one_move_from_the_end(az):
    """a Brandubh position with the king beside a corner and the move that ends the game"""
    board = np.zeros((3, 7, 7), np.int8)
    board[0, 0, 1] = 1; board[1, 5, 5] = 1; board[2, 3, 0] = 1; board[2, 6, 3] = 1; board[2, 3, 6] = 1
    for player in (0, 1):
        g = az.BrandubhGS.from_board(board, player, 4)
        if g.scores() is not None:
            continue
        for mv in np.flatnonzero(g.valid_moves()):
            h = g.copy()
            h.play_move(int(mv))
            if h.scores() is not None:
                return g, int(mv)
    raise AssertionError("no position one move from the end")


def test_brandubh_net_vs_search(az, brandubh_fixture_net):
    """the wavefront twin: 8 trees, tree 0 never searched, tree 7 played to the end"""
    n = 8
    rng = np.random.default_rng(11)
    states, gs = [], az.BrandubhGS()
    for _ in range(n - 1):
        states.append(gs.copy())
        for _ in range(2):
            gs.play_move(int(rng.choice(np.flatnonzero(gs.valid_moves()))))
    end, mv = _brandubh_one_move_from_the_end(az)
    states.append(end)
    mb = az.MCTSBatch(az.BrandubhGS, n, 1.25, max_simulations=32, seeds=[300 + i for i in range(n)])
    mb.reset(states)
    mb.update_roots([-1] * (n - 1) + [mv])
    assert mb.finished().tolist() == [False] * (n - 1) + [True]
    mb.search_to([0] + [32] * (n - 1), net=brandubh_fixture_net)
    r = mb.net_vs_search(brandubh_fixture_net)
    _assert_net_vs_search(az, mb, brandubh_fixture_net, r, invalid={n - 1})


# ---- 5. / 6. errors, and the object after them -------------------------------------------------------------------------------
def test_net_vs_search_errors_leave_the_object_usable(az, c4_fixture_net, brandubh_fixture_net):
    n = 4
    mb = az.MCTSBatch(az.Connect4GS, n, 1.25, max_simulations=64, seeds=[1, 2, 3, 4], capture=True)
    with pytest.raises(RuntimeError, match="call reset first"):
        mb.net_vs_search(c4_fixture_net)
    mb.reset([az.Connect4GS() for _ in range(n)])
    with pytest.raises(RuntimeError, match="the net's shape does not match the game"):
        mb.net_vs_search(brandubh_fixture_net)
    canon, idx = mb.find_leaves(numpy=True)
    with pytest.raises(RuntimeError, match="net_vs_search: a find_leaves step is pending"):
        mb.net_vs_search(c4_fixture_net)
    with pytest.raises(RuntimeError, match="capture_roots: a find_leaves step is pending"):
        mb.capture_roots()
    rows = len(idx)
    mb.process_results(np.full((rows, 3), 1 / 3, np.float32), np.full((rows, 7), 1 / 7, np.float32))
    with pytest.raises(RuntimeError, match="one valid flag per key"):
        az.pool_unique(np.arange(4, dtype=np.uint64), np.ones(3, bool))
    # after every error: the whole pipeline on the same object
    mb.play(8, net=c4_fixture_net, max_moves=3)
    pool = mb.position_pool()
    assert pool["captured"] == 3 * n and len(pool["tree"]) >= 3
    r = mb.net_vs_search(c4_fixture_net)
    assert r["valid"].all() and not np.isnan(r["kl_mcts_net"]).any() and 0.0 <= r["mean"]["top1_agreement"] <= 1.0


# ---- the README example --------------------------------------------------------------------------------------------------------
def test_readme_frozen_set_snippet():
    import alphazero
    from alphazero import torch_net
    net = alphazero.HipLeafNet(torch_net.random_init(torch_net.connect4_spec()), torch_net.connect4_spec())
    games = alphazero.MCTSBatch(alphazero.Connect4GS, 32, 1.25, max_simulations=16 * 42, capture=True)
    games.reset([alphazero.Connect4GS() for _ in range(32)])
    games.play(16, net=net, max_moves=42)                      # whole games, every searched root recorded
    pool = games.position_pool()                               # first occurrence of every position, in (tree, ply) order
    frozen = games.sample_pool(pool, 32, np.random.default_rng(0))
    trees = alphazero.MCTSBatch(alphazero.Connect4GS, 32, 1.25, max_simulations=24)
    trees.reset([rec["gs"] for rec in frozen])
    trees.search(24, net=net)
    metrics = trees.net_vs_search(net)
    assert len(frozen) == 32 and pool["duplicates"] >= 31 and metrics["valid"].all()
    assert set(metrics["mean"]) == {"kl_mcts_net", "value_mae", "top1_agreement"} and metrics["mean"]["kl_mcts_net"] >= 0
