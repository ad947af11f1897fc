"""-m gpu: `alphazero.MCTSBatch(..., leaves_per_step=K)`: K leaves of every tree in flight per step (WU-UCT).  The contract is
that of tests/test_gpu_search_batch.py, bit-exactness per tree: tree i equals the stand-alone `alphazero.MCTS(seed=seeds[i])`
driven by the step's calls (K x find_leaf_batched, a process_result_batched at once for every leaf that needs no evaluator,
one evaluator call, the pending process_result_batched in ascending order, reset_batch) with the same evaluator values.
Every comparison is np.array_equal."""
import numpy as np
import pytest

from test_gpu_search_batch import (_assert_same, _assert_tree_equals, _c4_at, _c4_states, _readout, _readout_one,  # noqa: F401
                                   az, c4_net)

pytestmark = pytest.mark.gpu

# Connect4: columns 0-5 full without a four (cell (row, col) belongs to player (row + col // 2) % 2), column 6 empty
_C4_ONE_COLUMN = [0] * 6 + [1] * 6 + [4] + [2] * 6 + [3] * 6 + [4] * 5 + [5] * 6
_C4_POSITIONS = [(), (3, 3, 2), (1, 6, 3, 6, 4, 2, 2), (0, 1, 0, 1, 0, 1), tuple(_C4_ONE_COLUMN)]


def _synth(az, pending):
    """The deterministic evaluator of the step: dumb_eval of the leaf, shaped by the row's tree AND descent index, so that an
    answer delivered to another descent of the same tree changes the search."""
    if not pending:
        return np.zeros((0, 3), np.float32), None
    V, PI = [], []
    for t, k, leaf in pending:
        v, pi = az.dumb_eval(leaf)
        w = np.float32(0.2 * np.sin(t + 3 * k))
        v = (v + np.float32([w, -w, 0])).astype(np.float32)
        pi = (pi * (1 + 0.3 * np.sin(np.arange(pi.size) + t + 2 * k))).astype(np.float32); pi /= pi.sum()
        V.append(v); PI.append(pi)
    return np.stack(V), np.stack(PI)


def _objects_find(az, ms, states, kk, noise=False, now=None):
    """The find half of one step on stand-alone objects: kk x find_leaf_batched per tree; a terminal leaf, and a leaf for which
    now(t, leaf) has an answer (RANDOM evaluator, cache hit), is backed up at once.  -> (pending [(tree, k, leaf)] in row
    order, number of terminal leaves)"""
    pending, n_term = [], 0
    for t, m in enumerate(ms):
        P, M = m._P, m._M
        for k in range(kk):
            leaf = m.find_leaf_batched(states[t])
            if leaf.scores() is not None:
                m.process_result_batched(states[t], k, np.full(P + 1, 1 / (P + 1), np.float32), np.full(M, 1 / M, np.float32), noise)
                n_term += 1
                continue
            ans = None if now is None else now(t, leaf)
            if ans is not None:
                m.process_result_batched(states[t], k, ans[0], ans[1], noise)
            else:
                pending.append((t, k, leaf))
    return pending, n_term


def _objects_back(ms, states, pending, V, PI, noise=False):
    for r, (t, k, _) in enumerate(pending):
        ms[t].process_result_batched(states[t], k, V[r], PI[r], noise)
    for m in ms:
        m.reset_batch()


def _lockstep(az, mb, ms, states, visits, noise=False, evaluate=None):
    """The batch through the step API beside the objects, both fed by `evaluate(pending)`; every step's rows are compared."""
    K = mb.leaves_per_step
    evaluate = evaluate or (lambda pending: _synth(az, pending))
    left, n_term, steps = visits, 0, 0
    while left:
        kk = min(K, left)
        canon, idx = mb.find_leaves(numpy=True)
        pending, nt = _objects_find(az, ms, states, kk, noise)
        n_term += nt
        assert idx.tolist() == [t for t, _, _ in pending], f"step {steps}: rows are not ordered by tree, then descent"
        for r, (t, k, leaf) in enumerate(pending):
            assert np.array_equal(canon[r], leaf.canonicalized()), f"step {steps}: row {r} is not descent {k} of tree {t}"
        V, PI = evaluate(pending)
        if not pending:
            V = np.zeros((0, ms[0]._P + 1), np.float32); PI = np.zeros((0, ms[0]._M), np.float32)
        mb.process_results(V, PI, noise)
        _objects_back(ms, states, pending, V, PI, noise)
        left -= kk; steps += 1
    return n_term, steps


def _objects(az, Game, n, seeds, visits, cpuct=1.25, **kw):
    relative = Game.__name__ == "StarGambitUnifiedGS"
    return [az.MCTS(cpuct, 2, Game.NUM_MOVES(), game=Game, seed=seeds[i], max_simulations=visits, relative_values=relative, **kw)
            for i in range(n)]


def _compare(mb, ms, what):
    out = _readout(mb)
    for i, m in enumerate(ms):
        _assert_tree_equals(out, i, _readout_one(m), what)
    return out


# ---- 1. bit for bit against the stand-alone object, through the step API ----------------------------------------------------
@pytest.mark.parametrize("noise", [False, True])
def test_step_api_equals_stand_alone_objects(az, noise):
    """Connect4, five different positions (empty, two mid-game, a win in one, one legal column), K = 8 > 7 root children so
    that descents pass through in-flight nodes, 44 visits = 5 full steps and a tail of 4."""
    n, K, visits = 5, 8, 44
    states = [_c4_at(az, p) for p in _C4_POSITIONS]
    assert all(g.scores() is None for g in states)
    assert int(states[4].valid_moves().sum()) == 1
    seeds = [700 + 11 * i for i in range(n)]
    kw = dict(cpuct=1.25, fpu_reduction=0.25, epsilon=0.25 if noise else 0.0)
    mb = az.MCTSBatch(az.Connect4GS, n, kw["cpuct"], epsilon=kw["epsilon"], fpu_reduction=0.25, max_simulations=visits, seeds=seeds,
                      leaves_per_step=K)
    assert mb.leaves_per_step == K
    mb.reset(states)
    ms = _objects(az, az.Connect4GS, n, seeds, visits, **kw)
    _, steps = _lockstep(az, mb, ms, states, visits, noise)
    assert steps == 6
    out = _compare(mb, ms, f"K = {K}, noise = {noise}")
    assert out["depth"].tolist() == [visits] * n
    st = mb.stats()
    assert st["steps"] == 6 and st["simulations"] == n * visits


# ---- 2. against the oracle ---------------------------------------------------------------------------------------------------------
def test_step_api_against_the_oracle(az, oracle):
    n, K, visits = 3, 4, 40
    prefixes = [(), (3, 3, 2), (1, 6, 3, 6, 4, 2, 2)]
    seeds = [500 + 7 * i for i in range(n)]
    mb = az.MCTSBatch(az.Connect4GS, n, 1.25, fpu_reduction=0.25, max_simulations=visits, leaves_per_step=K)
    mb.reset([_c4_at(az, p) for p in prefixes], seeds=seeds)
    os_, ogs = [], []
    for i in range(n):
        os_.append(oracle.Mcts(1.25, 2, 7, seed=seeds[i], fpu_reduction=0.25))
        og = oracle.Game(oracle.GAME_CONNECT4)
        for mv in prefixes[i]:
            og.play(mv)
        ogs.append(og)
    for _ in range(visits // K):
        canon, idx = mb.find_leaves(numpy=True)
        pending = []
        for t in range(n):
            for k in range(K):
                oleaf = os_[t].find_leaf_batched(ogs[t])
                if oleaf.scores() is not None:
                    os_[t].process_result_batched(k, np.full(3, 1 / 3, np.float32), np.full(7, 1 / 7, np.float32), False)
                    continue
                assert np.array_equal(canon[len(pending)], oleaf.canonical()), f"tree {t}, descent {k}: another leaf than the oracle's"
                v, pi = oracle.dumb_eval(oleaf)
                pi = (pi * (1 + 0.3 * np.sin(np.arange(7) + t + 2 * k))).astype(np.float32); pi /= pi.sum()
                pending.append((t, k, v, pi))
        assert idx.tolist() == [p[0] for p in pending]
        V = np.stack([p[2] for p in pending]) if pending else np.zeros((0, 3), np.float32)
        PI = np.stack([p[3] for p in pending]) if pending else np.zeros((0, 7), np.float32)
        mb.process_results(V, PI)
        for t, k, v, pi in pending:
            os_[t].process_result_batched(k, v, pi, False)
        for o in os_:
            o.reset_batch()
    out = _readout(mb)
    for t, o in enumerate(os_):
        assert np.array_equal(out["counts"][t], o.counts()), f"tree {t}"
        assert np.array_equal(out["q"][t], o.root_q()), f"tree {t}"
        assert np.array_equal(out["p1"][t], o.probs(1.0)) and np.array_equal(out["p0"][t], o.probs(0.0)), f"tree {t}"
        assert np.array_equal(out["pp"][t], o.probs(1.0, pruned=True)), f"tree {t}"
        assert np.array_equal(out["rv"][t], o.root_value()), f"tree {t}"
        assert int(out["depth"][t]) == o.depth() == visits and int(out["root_n"][t]) == o.root_n()
        assert np.array_equal(out["pv"][t], o.principal_variation(5)), f"tree {t}"


# ---- 3. wide games ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n,K,visits", [("BrandubhGS", 3, 4, 18), ("StarGambitUnifiedGS", 2, 3, 10)])
def test_wide_games_equal_stand_alone_objects(az, name, n, K, visits):
    Game = getattr(az, name)
    rng = np.random.default_rng(11)
    states = []
    gs = Game(0) if name == "StarGambitUnifiedGS" else Game()
    for _ in range(n):
        states.append(gs.copy())
        for _ in range(2):
            gs.play_move(int(rng.choice(np.flatnonzero(gs.valid_moves()))))
            assert gs.scores() is None
    seeds = [31 + i for i in range(n)]
    mb = az.MCTSBatch(Game, n, 1.25, fpu_reduction=0.25, max_simulations=visits, seeds=seeds, leaves_per_step=K)
    mb.reset(states)
    ms = _objects(az, Game, n, seeds, visits, cpuct=1.25, fpu_reduction=0.25)
    _lockstep(az, mb, ms, states, visits)
    out = _compare(mb, ms, name)
    assert out["depth"].tolist() == [visits] * n


# ---- 4. one tree --------------------------------------------------------------------------------------------------------------------
def test_one_tree_with_32_leaves_in_flight(az):
    K, visits = 32, 64
    states = [_c4_at(az, (3, 3, 2))]
    mb = az.MCTSBatch(az.Connect4GS, 1, 1.25, fpu_reduction=0.25, max_simulations=visits, seeds=[5], leaves_per_step=K)
    mb.reset(states)
    ms = _objects(az, az.Connect4GS, 1, [5], visits, cpuct=1.25, fpu_reduction=0.25)
    _lockstep(az, mb, ms, states, visits)
    _compare(mb, ms, "one tree, K = 32")
    assert mb.stats()["steps"] == 2
    # the RANDOM evaluator through search(): every leaf is backed up by the find kernel
    mb.reset(states)
    mb.search(visits)
    ms = _objects(az, az.Connect4GS, 1, [5], visits, cpuct=1.25, fpu_reduction=0.25)
    for _ in range(2):
        pending, _ = _objects_find(az, ms, states, K, now=lambda t, leaf: az.dumb_eval(leaf))
        assert not pending
        _objects_back(ms, states, [], None, None)
    _compare(mb, ms, "one tree, K = 32, dumb_eval")


# ---- 5. the net on the device ---------------------------------------------------------------------------------------------------------
def _net_rows(c4_net, canon):
    return c4_net.process(canon) if canon.shape[0] else (np.zeros((0, 3), np.float32), np.zeros((0, 7), np.float32))


def test_net_on_the_device_equals_the_step_api(az, c4_net):
    n, K, visits = 4, 8, 40
    states = _c4_states(az, n, seed=5)
    seeds = [9000 + i for i in range(n)]
    mb = az.MCTSBatch(az.Connect4GS, n, 1.25, fpu_reduction=0.25, max_simulations=visits, seeds=seeds, leaves_per_step=K)
    mb.reset(states)
    s0 = mb.stats()
    mb.search(visits, net=c4_net)
    a = _readout(mb)
    s1 = mb.stats()
    assert s1["net_calls"] - s0["net_calls"] == 5 and s1["steps"] - s0["steps"] == 5
    assert a["depth"].tolist() == [visits] * n and s1["simulations"] == n * visits
    mb.reset(states)
    for _ in range(5):
        canon, idx = mb.find_leaves()
        v, pi = _net_rows(c4_net, canon)
        mb.process_results(v, pi)
    _assert_same(a, _readout(mb), "search() vs the step API with net.process")


def test_launches_per_step_depend_on_neither_n_nor_k(az, c4_net):
    per_step = set()
    for n, K in ((4, 4), (64, 4), (4, 16)):
        mb = az.MCTSBatch(az.Connect4GS, n, 1.25, max_simulations=64, seeds=list(range(n)), leaves_per_step=K)
        mb.reset(_c4_states(az, n, seed=21))
        l0 = mb.stats(); mb.search(64, net=c4_net); l1 = mb.stats()
        steps = l1["steps"] - l0["steps"]
        assert steps == 64 // K
        per_step.add(((l1["launches"] - l0["launches"]) / steps, (l1["net_calls"] - l0["net_calls"]) / steps))
        assert mb.depths().tolist() == [64] * n
    assert per_step == {(3.0, 1.0)}           # find-leaves, compaction, process-results + one net call, as with K = 1


# ---- 6. the cache ----------------------------------------------------------------------------------------------------------------------
def test_cache_probe_at_descent_insert_after_the_net(az, c4_net):
    import torch
    n, K, visits = 4, 8, 40
    states = [_c4_at(az, p) for p in ((3, 3, 2), (3, 3, 2), (2, 3, 3), (1, 6, 3, 6))]     # trees that meet the same positions
    seeds = [40 + i for i in range(n)]
    cache = az.ShardedS3FIFOCache.for_engine(1 << 14, 7, 3)
    mb = az.MCTSBatch(az.Connect4GS, n, 1.25, fpu_reduction=0.25, max_simulations=visits, seeds=seeds, leaves_per_step=K)
    # the objects with a dictionary for the cache: every probe of a step comes before the step's inserts
    known, tally = {}, dict(hits=0, evaluated=0)
    dev = torch.device("cuda", 0)

    def probe(t, leaf):
        ans = known.get(leaf.canonicalized().tobytes())
        tally["hits"] += ans is not None
        return ans

    def objects_search():
        ms = _objects(az, az.Connect4GS, n, seeds, visits, cpuct=1.25, fpu_reduction=0.25)
        for _ in range(visits // K):
            pending, _ = _objects_find(az, ms, states, K, now=probe)
            V = PI = None
            if pending:
                canon = np.stack([leaf.canonicalized() for _, _, leaf in pending]).astype(np.float32)
                v, pi = c4_net.process(torch.from_numpy(np.ascontiguousarray(canon)).to(dev))
                torch.cuda.synchronize()
                V, PI = v.cpu().numpy(), pi.cpu().numpy()
                for r, (_, _, leaf) in enumerate(pending):
                    known[leaf.canonicalized().tobytes()] = (V[r].copy(), PI[r].copy())
                tally["evaluated"] += len(pending)
            _objects_back(ms, states, pending, V, PI)
        return ms

    mb.reset(states)
    mb.search(visits, net=c4_net, cache=cache)
    _compare(mb, objects_search(), "with a cache")
    assert mb.stats()["evaluator_leaves"] == tally["evaluated"] == cache.misses()
    assert cache.hits() == tally["hits"]
    # a second search of the same positions: the root and most leaves are hits, which are backed up at once, so this is another
    # search than the first - and again the objects'
    h0 = cache.hits()
    mb.reset(states)
    mb.search(visits, net=c4_net, cache=cache)
    assert cache.hits() > h0
    _compare(mb, objects_search(), "second search, answers from the cache")
    assert cache.hits() == tally["hits"] and cache.misses() == tally["evaluated"]


# ---- 7. immediates ---------------------------------------------------------------------------------------------------------------------
def test_terminal_leaves_take_no_row(az):
    """One move from the end of the game: the root's only child is terminal.  After the root's own row every step is backed up
    by the find kernel alone and completes through process_results with empty arrays."""
    K, visits = 8, 24
    states = [_c4_at(az, tuple(_C4_ONE_COLUMN) + (6,) * 5), _c4_at(az, (3, 3, 2))]
    assert all(g.scores() is None for g in states) and int(states[0].valid_moves().sum()) == 1
    one = [states[0]]
    mb = az.MCTSBatch(az.Connect4GS, 1, 1.25, max_simulations=visits, seeds=[3], leaves_per_step=K)
    mb.reset(one)
    ms = _objects(az, az.Connect4GS, 1, [3], visits, cpuct=1.25)
    rows = []
    left = visits
    n_term = 0
    while left:
        canon, idx = mb.find_leaves(numpy=True)
        pending, nt = _objects_find(az, ms, one, K)
        n_term += nt
        rows.append(len(idx))
        assert len(idx) == len(pending)
        V, PI = _synth(az, pending)
        if not pending:
            V = np.zeros((0, 3), np.float32); PI = np.zeros((0, 7), np.float32)
        mb.process_results(V, PI)
        _objects_back(ms, one, pending, V, PI)
        left -= K
    assert rows == [1, 0, 0]
    _compare(mb, ms, "one move from the end")
    assert mb.stats()["terminal_leaves"] == n_term == visits - 1
    # beside a tree that does need rows
    seeds = [3, 4]
    mb2 = az.MCTSBatch(az.Connect4GS, 2, 1.25, max_simulations=visits, seeds=seeds, leaves_per_step=K)
    mb2.reset(states)
    ms2 = _objects(az, az.Connect4GS, 2, seeds, visits, cpuct=1.25)
    n_term2, _ = _lockstep(az, mb2, ms2, states, visits)
    _compare(mb2, ms2, "a finished tree beside a live one")
    assert mb2.stats()["terminal_leaves"] == n_term2


# ---- 8. the budget counts descents -----------------------------------------------------------------------------------------------------
def test_budget_is_counted_in_descents(az):
    n, K = 3, 8
    states = _c4_states(az, n, seed=13)
    mb = az.MCTSBatch(az.Connect4GS, n, 2.0, max_simulations=20, seeds=list(range(n)), leaves_per_step=K)
    mb.reset(states)
    with pytest.raises(RuntimeError, match="max_simulations"):
        mb.search(24)
    mb.search(16)
    assert mb.depths().tolist() == [16] * n
    with pytest.raises(RuntimeError, match="max_simulations"):
        mb.search(5)
    canon, idx = mb.find_leaves(numpy=True)                 # 4 descents are left: the remainder only
    assert len(idx) <= 4 * n and max(np.bincount(idx.astype(np.int64), minlength=n)) <= 4
    with pytest.raises(RuntimeError, match=rf"the step has {len(idx)} rows"):
        mb.process_results(np.zeros((len(idx) + 1, 3), np.float32), np.zeros((len(idx) + 1, 7), np.float32))
    mb.process_results(np.full((len(idx), 3), 1 / 3, np.float32), np.full((len(idx), 7), 1 / 7, np.float32))
    assert mb.depths().tolist() == [20] * n
    st = mb.stats()
    assert st["simulations"] == 20 * n and st["steps"] == 3
    with pytest.raises(RuntimeError, match="max_simulations"):
        mb.find_leaves()
    mb.reset(states)                                          # and the object goes on
    mb.search(20)
    assert mb.depths().tolist() == [20] * n
    with pytest.raises(RuntimeError, match="gumbel"):
        az.MCTSBatch(az.Connect4GS, n, 2.0, gumbel_enabled=True, max_simulations=20, leaves_per_step=2)


# ---- 9. K = 1 is the code it was ---------------------------------------------------------------------------------------------------------
def test_one_leaf_per_step_is_untouched(az):
    n, visits = 3, 20
    states = _c4_states(az, n, seed=9)
    seeds = [77 + 3 * i for i in range(n)]
    outs, stats = [], []
    for kw in ({}, dict(leaves_per_step=1)):
        mb = az.MCTSBatch(az.Connect4GS, n, 1.25, fpu_reduction=0.25, epsilon=0.25, max_simulations=visits, seeds=seeds, **kw)
        assert mb.leaves_per_step == 1
        mb.reset(states)
        mb.search(visits, root_noise=True)
        stats.append(mb.stats()); outs.append(_readout(mb))
    _assert_same(outs[0], outs[1], "leaves_per_step = 1 vs the default")
    assert stats[0] == stats[1]
    assert stats[0]["steps"] == visits and stats[0]["launches"] == 1 + 3 * visits      # the seed kernel + three a step
