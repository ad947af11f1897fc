"""-m gpu: `MCTSBatch.search_to(targets, checkpoints=...)` / `checkpoints()`: every tree searched to its own root_n target, the
read-outs snapshotted on the device at checkpoints on the way (the inner loop of mcts_analysis.py:run_analysis).  The yardstick
is the stand-alone `alphazero.MCTS(seed=seeds[i])` (pinned to the oracle by tests/test_gpu_mcts_object.py) driven call by call
with that loop and the same evaluator values:

    snapshot every checkpoint <= root_n
    while m.root_n() < target:
        find_leaf / evaluate / process_result        (K > 1: K x find_leaf_batched / process_result_batched, reset_batch)
        snapshot every checkpoint <= root_n, once

Every comparison is bit for bit (floats by their 32-bit patterns: the probs of a root without children are 0 / 0 on both sides):
no tolerance is involved."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# Connect4: columns 0-5 full without a four (cell (row, col) belongs to player (row + col // 2) % 2), column 6 empty
_C4_ONE_COLUMN = tuple([0] * 6 + [1] * 6 + [4] + [2] * 6 + [3] * 6 + [4] * 5 + [5] * 6)
_C4_LAST_CELL = _C4_ONE_COLUMN + (6,) * 5          # one empty cell: the next move ends the game
_C4_WIN_IN_ONE = (0, 1, 0, 1, 0, 1)
_C4_MIXED = [(), (3, 3, 2), _C4_WIN_IN_ONE, (1, 6, 3, 6, 4, 2, 2), _C4_ONE_COLUMN, (3, 3, 3, 3, 3, 3)]
_SNAP_KEYS = ("root_n", "counts", "probs", "root_values", "root_q_values")


@pytest.fixture(scope="module")
def az():
    import alphazero
    return alphazero


def _c4_at(az, moves):
    gs = az.Connect4GS()
    for mv in moves:
        gs.play_move(mv)
    return gs


def _c4_mixed(az, n):
    out = [_c4_at(az, _C4_MIXED[i % len(_C4_MIXED)]) for i in range(n)]
    assert all(g.scores() is None for g in out)
    return out


def _random_eval(az):
    def evaluate(i, leaf):
        if leaf.scores() is not None:       # a terminal leaf: the values are not read
            P, M = leaf.num_players(), leaf.num_moves()
            return np.full(P + 1, 1.0 / (P + 1), np.float32), np.full(M, 1.0 / M, np.float32)
        return az.dumb_eval(leaf)
    return evaluate


def _snap_one(m, temp, pruned):
    return dict(root_n=m.root_n(), counts=m.counts(), probs=m.probs_pruned(temp) if pruned else m.probs(temp),
                root_values=m.root_value(), root_q_values=m.root_q_values())


def _loop_alone(m, gs, i, target, cps, evaluate, K=1, temp=1.0, pruned=False):
    """The reference's loop on one object -> {j: snapshot}, the descents it took"""
    snaps, descents = {}, 0

    def take():
        for j, c in enumerate(cps):
            if j not in snaps and c <= m.root_n():
                snaps[j] = _snap_one(m, temp, pruned)
    take()
    while m.root_n() < target:
        if K == 1:
            leaf = m.find_leaf(gs)
            v, pi = evaluate(i, leaf)
            m.process_result(gs, v, pi, False)
        else:
            for k in range(K):
                leaf = m.find_leaf_batched(gs)
                v, pi = evaluate(i, leaf)
                m.process_result_batched(gs, k, v, pi, False)
            m.reset_batch()
        descents += K
        take()
    return snaps, descents


def _final(mb):
    return dict(counts=mb.counts(), probs=mb.probs(1.0), root_values=mb.root_values(), root_q_values=mb.root_q_values(),
                root_n=mb.root_ns(), depth=mb.depths())


def _final_one(m):
    return dict(counts=m.counts(), probs=m.probs(1.0), root_values=m.root_value(), root_q_values=m.root_q_values(),
                root_n=m.root_n(), depth=m.depth())


def _same(got, ref):
    got, ref = np.atleast_1d(np.asarray(got)), np.atleast_1d(np.asarray(ref))
    if got.dtype.kind == "f":
        return got.shape == ref.shape and np.array_equal(got.astype(np.float32).view(np.uint32), ref.astype(np.float32).view(np.uint32))
    return np.array_equal(got, ref)


def _assert_snaps(snap, i, want, J, what):
    """row i of the batch's snapshot set against the loop's {j: snapshot}; rows that were not taken are zero"""
    assert snap["taken"].dtype == np.bool_ and snap["taken"].shape[1] == J
    assert snap["taken"][i].tolist() == [j in want for j in range(J)], f"{what}: tree {i}: taken {snap['taken'][i]}, the loop took {sorted(want)}"
    for j in range(J):
        for k in _SNAP_KEYS:
            got = np.asarray(snap[k][i, j])
            ref = np.asarray(want[j][k]) if j in want else np.zeros_like(got)
            assert _same(got, ref), f"{what}: tree {i}, checkpoint {j}: {k} differs: {got} vs {ref}"


def _assert_final(out, i, m, what):
    for k, ref in _final_one(m).items():
        assert _same(out[k][i], ref), f"{what}: tree {i}: final {k} differs: {out[k][i]} vs {ref}"


def _assert_snaps_well_formed(snap, n, J, M):
    assert snap["root_n"].dtype == np.uint32 and snap["root_n"].shape == (n, J)
    assert snap["counts"].dtype == np.uint32 and snap["counts"].shape == (n, J, M)
    assert snap["probs"].dtype == np.float32 and snap["probs"].shape == (n, J, M)
    assert snap["root_values"].dtype == np.float32 and snap["root_values"].shape == (n, J, 3)
    assert snap["root_q_values"].dtype == np.float32 and snap["root_q_values"].shape == (n, J, M)


# ---- 1. Connect4, RANDOM evaluator, per-tree targets ------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 33])
@pytest.mark.parametrize("pruned", [False, True])
def test_connect4_targets_and_checkpoints_equal_the_stand_alone_loop(az, n, pruned):
    """n = 3: fewer than 8 lane groups; n = 33: more than one 32-tree workgroup, the last wavefront not full.  Targets
    [0, 5, 24] cycled, checkpoints (1, 8, 24, 40): the 40 is never taken, a tree with target 0 takes nothing."""
    cps = (1, 8, 24, 40)
    targets = [(0, 5, 24)[i % 3] for i in range(n)]
    states = _c4_mixed(az, n)
    seeds = [700 + 11 * i for i in range(n)]
    mb = az.MCTSBatch(az.Connect4GS, n, 1.25, fpu_reduction=0.25, max_simulations=24, seeds=seeds)
    mb.reset(states)
    mb.search_to(targets, checkpoints=cps, pruned=pruned)
    snap, out = mb.checkpoints(), _final(mb)
    _assert_snaps_well_formed(snap, n, len(cps), 7)
    assert out["root_n"].tolist() == targets
    assert not snap["taken"][:, 3].any()
    for i in range(n):
        m = az.MCTS(1.25, 2, 7, fpu_reduction=0.25, seed=seeds[i], max_simulations=24)
        want, _ = _loop_alone(m, states[i], i, targets[i], cps, _random_eval(az), pruned=pruned)
        _assert_snaps(snap, i, want, len(cps), f"n = {n}")
        _assert_final(out, i, m, f"n = {n}")
    assert mb.stats()["simulations"] == sum(targets)


# ---- 2. reused trees ------------------------------------------------------------------------------------------------------------
def test_reused_trees_need_fewer_descents_and_snapshot_before_the_first(az):
    """search(16), pick_moves(1.0), update_roots(), then search_to(20, checkpoints=(4, 20)): a reused root holds the visits of
    its subtree, so its first snapshot is taken before any descent and it needs 20 - root_n descents."""
    n, cps = 6, (4, 20)
    positions = [(), (3, 3, 2), _C4_WIN_IN_ONE, (1, 6, 3, 6, 4, 2, 2), _C4_LAST_CELL, _C4_ONE_COLUMN]      # (one legal move: every visit is reused)
    gss = [_c4_at(az, p) for p in positions]
    seeds = [4100 + 13 * i for i in range(n)]
    ev = _random_eval(az)
    mb = az.MCTSBatch(az.Connect4GS, n, 1.25, fpu_reduction=0.25, max_simulations=40, seeds=seeds)
    mb.reset(gss)
    ms = [az.MCTS(1.25, 2, 7, fpu_reduction=0.25, seed=seeds[i], max_simulations=40) for i in range(n)]
    mb.search(16)
    picked = mb.pick_moves(1.0)
    mb.update_roots()
    for i in range(n):
        _loop_alone(ms[i], gss[i], i, 16, (), ev)
        mv = ms[i].pick_move(ms[i].probs(1.0))
        assert int(picked[i]) == mv
        ms[i].update_root(gss[i], mv)
        gss[i].play_move(mv)
    live = [g.scores() is None for g in gss]
    assert not live[4] and any(live)
    reused = [m.root_n() for m in ms]
    assert mb.root_ns().tolist() == reused
    assert any(r >= 4 for r, l in zip(reused, live) if l) and len({r for r, l in zip(reused, live) if l}) > 1
    s0 = mb.stats()["simulations"]
    mb.search_to(20, checkpoints=cps)
    snap, out = mb.checkpoints(), _final(mb)
    assert mb.stats()["simulations"] - s0 == sum(max(0, 20 - r) for r, l in zip(reused, live) if l)
    assert mb.finished().tolist() == [not l for l in live]
    for i in range(n):
        if not live[i]:      # finished by the move: skipped, no snapshot
            assert not snap["taken"][i].any() and not snap["counts"][i].any() and not snap["root_n"][i].any()
            continue
        want, _ = _loop_alone(ms[i], gss[i], i, 20, cps, ev)
        _assert_snaps(snap, i, want, 2, "reused")
        _assert_final(out, i, ms[i], "reused")
        if reused[i] >= 4:
            assert snap["taken"][i, 0] and int(snap["root_n"][i, 0]) == reused[i], "taken before any descent"


# ---- 3. K > 1 -------------------------------------------------------------------------------------------------------------------
def test_leaves_per_step_overshoots_by_fewer_than_k_and_snapshots_at_step_boundaries(az):
    n, K, cps = 5, 4, (1, 4, 5)
    states = _c4_mixed(az, n)
    seeds = [90 + i for i in range(n)]
    mb = az.MCTSBatch(az.Connect4GS, n, 1.25, fpu_reduction=0.25, max_simulations=12, seeds=seeds, leaves_per_step=K)
    mb.reset(states)
    mb.search_to(10, checkpoints=cps)
    snap, out = mb.checkpoints(), _final(mb)
    assert out["root_n"].tolist() == [12] * n
    assert snap["taken"].all() and snap["root_n"].tolist() == [[4, 4, 8]] * n
    st = mb.stats()
    assert st["simulations"] == 12 * n and st["steps"] == 3
    for i in range(n):
        m = az.MCTS(1.25, 2, 7, fpu_reduction=0.25, seed=seeds[i], max_simulations=12)
        want, _ = _loop_alone(m, states[i], i, 10, cps, _random_eval(az), K=K)
        _assert_snaps(snap, i, want, 3, "K = 4")
        _assert_final(out, i, m, "K = 4")


# ---- 4. wide games ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n,targets,cps", [("BrandubhGS", 3, [3, 12, 7], (1, 7)), ("StarGambitUnifiedGS", 2, [6, 6], (3,))])
def test_wide_games_equal_the_stand_alone_loop(az, name, n, targets, cps):
    Game = getattr(az, name)
    M = Game.NUM_MOVES()
    rng = np.random.default_rng(11)
    states = []
    gs = Game(0) if name == "StarGambitUnifiedGS" else Game()
    for _ in range(n):
        states.append(gs.copy())
        for _ in range(2):                      # the next position is two plies further down a random playout
            gs.play_move(int(rng.choice(np.flatnonzero(gs.valid_moves()))))
            assert gs.scores() is None
    seeds = [31 + i for i in range(n)]
    mb = az.MCTSBatch(Game, n, 1.25, fpu_reduction=0.25, max_simulations=max(targets), seeds=seeds)
    mb.reset(states)
    mb.search_to(targets[0] if name == "StarGambitUnifiedGS" else targets, checkpoints=cps)
    snap, out = mb.checkpoints(), _final(mb)
    _assert_snaps_well_formed(snap, n, len(cps), M)
    assert out["root_n"].tolist() == targets
    for i in range(n):
        m = az.MCTS(1.25, 2, M, game=Game, seed=seeds[i], max_simulations=max(targets), relative_values=(name == "StarGambitUnifiedGS"),
                    fpu_reduction=0.25)
        want, _ = _loop_alone(m, states[i], i, targets[i], cps, _random_eval(az))
        _assert_snaps(snap, i, want, len(cps), name)
        _assert_final(out, i, m, name)


# ---- 5. net and cache ---------------------------------------------------------------------------------------------------------------
def test_net_and_cache_equal_the_stand_alone_loop_fed_the_same_net(az):
    """Connect4 with the fixture net and a device cache, n = 9, targets [6, 12, 9] cycled, checkpoints (3, 12): equal to the
    same call without a cache, and to objects fed net.process of their own leaves."""
    import os
    import torch
    from alphazero import torch_net
    fx = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nn_connect4_6b64c.npz"))
    spec = torch_net.connect4_spec()
    ref = torch_net.LeafNet(spec)
    ref.load_state_dict({k[3:]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith("sd.")})
    net = az.HipLeafNet(ref.eval(), spec, precision="bf16")
    n, cps = 9, (3, 12)
    targets = [(6, 12, 9)[i % 3] for i in range(n)]
    states = _c4_mixed(az, n)
    seeds = [9000 + i for i in range(n)]
    runs = []
    for cache in (az.ShardedS3FIFOCache.for_engine(1 << 12, 7, 3), None):
        mb = az.MCTSBatch(az.Connect4GS, n, 1.25, fpu_reduction=0.25, max_simulations=12, seeds=seeds)
        mb.reset(states)
        mb.search_to(targets, net=net, cache=cache, checkpoints=cps)
        runs.append((mb.checkpoints(), _final(mb)))
        assert mb.stats()["net_calls"] == 12
    (snap, out), (snap_plain, out_plain) = runs
    for k in snap:
        assert _same(snap[k], snap_plain[k]), f"with a cache vs without: snapshot {k}"
    for k in out:
        assert _same(out[k], out_plain[k]), f"with a cache vs without: final {k}"
    dev = torch.device("cuda", 0)

    def evaluate(i, leaf):
        if leaf.scores() is not None:
            return np.full(3, 1 / 3, np.float32), np.full(7, 1 / 7, np.float32)
        v, pi = net.process(torch.from_numpy(np.ascontiguousarray(leaf.canonicalized()[None])).to(dev))
        torch.cuda.synchronize()
        return v.cpu().numpy()[0], pi.cpu().numpy()[0]
    for i in range(n):
        m = az.MCTS(1.25, 2, 7, fpu_reduction=0.25, seed=seeds[i], max_simulations=12)
        want, _ = _loop_alone(m, states[i], i, targets[i], cps, evaluate)
        _assert_snaps(snap, i, want, 2, "net + cache")
        _assert_final(out, i, m, "net + cache")


# ---- 6. PLAYOUT -------------------------------------------------------------------------------------------------------------------
def test_playout_rollout_index_counts_only_the_trees_own_descents(az):
    n, targets, cps = 4, [9, 0, 14, 5], (2, 9)
    states = _c4_mixed(az, n)
    seeds = [55 + i for i in range(n)]
    mb = az.MCTSBatch(az.Connect4GS, n, 1.25, fpu_reduction=0.25, max_simulations=14, seeds=seeds)
    mb.reset(states)
    rs = [int(x) for x in mb.rollout_seeds()]
    mb.search_to(targets, evaluator="playout", checkpoints=cps)
    snap, out = mb.checkpoints(), _final(mb)
    j = [0] * n

    def evaluate(i, leaf):
        if leaf.scores() is not None:
            return np.full(3, 1 / 3, np.float32), np.full(7, 1 / 7, np.float32)
        ans = az.playout_eval(leaf, seed=az.MCTSBatch.rollout_seed(rs[i], j[i]))
        j[i] += 1
        return ans
    for i in range(n):
        m = az.MCTS(1.25, 2, 7, fpu_reduction=0.25, seed=seeds[i], max_simulations=14)
        want, _ = _loop_alone(m, states[i], i, targets[i], cps, evaluate)
        _assert_snaps(snap, i, want, 2, "playout")
        _assert_final(out, i, m, "playout")
    assert mb.stats()["evaluator_leaves"] == sum(j)


# ---- 7. launch count, independence from N ------------------------------------------------------------------------------------------
def test_launches_are_those_of_search_plus_the_event_steps_whatever_n_is(az):
    """Fresh trees, target 24, checkpoints (1, 8, 24): the checkpoint kernel runs behind steps 1, 8 and 24 only."""
    cps, rise, snaps = (1, 8, 24), {}, {}
    for n in (8, 256):
        seeds = [1 + i for i in range(n)]
        states = [az.Connect4GS() for _ in range(n)]
        mb = az.MCTSBatch(az.Connect4GS, n, 1.25, max_simulations=24, seeds=seeds)
        mb.reset(states)
        l0 = mb.stats()["launches"]
        mb.search_to(24, checkpoints=cps)
        rise[n] = mb.stats()["launches"] - l0
        snaps[n] = mb.checkpoints()
        assert snaps[n]["taken"].all() and snaps[n]["root_n"].tolist() == [[1, 8, 24]] * n
        plain = az.MCTSBatch(az.Connect4GS, n, 1.25, max_simulations=24, seeds=seeds)
        plain.reset(states)
        p0 = plain.stats()["launches"]
        plain.search(24)
        assert rise[n] == plain.stats()["launches"] - p0 + 3
        assert np.array_equal(plain.counts(), mb.counts())
    assert rise[8] == rise[256]
    for k in snaps[8]:
        assert _same(snaps[8][k][0], snaps[256][k][0]), f"tree 0: {k} depends on n"


# ---- 8. afterwards the object is as before -----------------------------------------------------------------------------------------
def test_the_object_is_as_before_after_search_to(az):
    n = 6
    states = _c4_mixed(az, n)
    seeds = [300 + i for i in range(n)]
    ev = _random_eval(az)
    mb = az.MCTSBatch(az.Connect4GS, n, 1.25, fpu_reduction=0.25, max_simulations=40, seeds=seeds)
    mb.reset(states)
    mb.search_to([24, 8, 0, 16, 24, 3])
    assert not mb.finished().any(), "a tree that reached its target is not a finished tree"
    assert not mb.checkpoints()["taken"].size
    mb.search(4)
    ms = [az.MCTS(1.25, 2, 7, fpu_reduction=0.25, seed=seeds[i], max_simulations=40) for i in range(n)]
    for i, t in enumerate([24, 8, 0, 16, 24, 3]):
        _loop_alone(ms[i], states[i], i, t + 4, (), ev)
    out = _final(mb)
    assert out["root_n"].tolist() == [28, 12, 4, 20, 28, 7]
    for i in range(n):
        _assert_final(out, i, ms[i], "search(4) behind search_to")
    l0 = mb.stats()
    with pytest.raises(RuntimeError, match="max_simulations"):
        mb.search_to(45)                       # 28 of 40 are used; the longest tree needs 45 - 4 = 41 more
    assert mb.stats() == l0, "a refused search_to launches nothing"
    # the moves still work, and a search_to on the reused roots inside what is left of the budget (12) equals the objects
    picked = mb.pick_moves(1.0)
    mb.update_roots()
    gss = [g.copy() for g in states]
    for i in range(n):
        mv = ms[i].pick_move(ms[i].probs(1.0))
        assert int(picked[i]) == mv
        ms[i].update_root(gss[i], mv)
        gss[i].play_move(mv)
    live = [g.scores() is None for g in gss]
    assert mb.finished().tolist() == [not l for l in live] and any(live)
    reused = [m.root_n() for m in ms]
    assert mb.root_ns().tolist() == reused
    targets = [r + (i % 3) * 5 for i, r in enumerate(reused)]
    mb.search_to(targets, checkpoints=(max(reused) + 2,))
    snap, out = mb.checkpoints(), _final(mb)
    for i in range(n):
        if live[i]:
            want, _ = _loop_alone(ms[i], gss[i], i, targets[i], (max(reused) + 2,), ev)
            _assert_snaps(snap, i, want, 1, "behind a move")
            _assert_final(out, i, ms[i], "behind a move")
    assert not mb.finished()[[i for i in range(n) if live[i]]].any()


# ---- 9. the snapshot block and the metric block regrow on a live batch ---------------------------------------------------------------
def _bits_of(x):
    if isinstance(x, dict):
        return {k: _bits_of(v) for k, v in x.items()}
    a = np.asarray(x)
    return a.dtype.str, a.shape, a.tobytes()


@pytest.mark.parametrize("name,n", [("Connect4GS", 3), ("BrandubhGS", 2)])
def test_more_checkpoints_then_fewer_on_one_batch_equal_fresh_batches(az, name, n):
    """One checkpoint, then four (the snapshot block and the sweep-metrics block are allocated again, larger, and cut again),
    then one (the grown blocks serve fewer): snapshots and sweep_metrics of every call on the one batch are the bits of the
    same call on a batch created for it.  8 visits, evaluator="random"."""
    Game = getattr(az, name)
    seeds = [900 + 7 * i for i in range(n)]

    def run(mb, cps):
        states = [Game() for _ in range(n)]
        for skip, g in enumerate(states[1:]):
            g.play_move(int(np.flatnonzero(g.valid_moves())[skip]))
        mb.reset(states)
        mb.search_to(8, evaluator="random", checkpoints=cps)
        snap = mb.checkpoints()
        assert snap["taken"].shape == (n, len(cps)) and snap["taken"].all()
        return _bits_of(snap), _bits_of(mb.sweep_metrics(anchor=-1, raw=0, outcomes=np.linspace(-1.0, 1.0, n)))

    live = az.MCTSBatch(Game, n, 1.25, max_simulations=8, seeds=seeds)
    for cps in ((8,), (1, 2, 4, 8), (8,)):
        got = run(live, cps)
        assert got == run(az.MCTSBatch(Game, n, 1.25, max_simulations=8, seeds=seeds), cps), f"checkpoints {cps}"
