"""-m gpu: `alphazero.MCTSBatch` (azmi_search_*): N search trees on N positions advanced per launch.  The contract is
bit-exactness per tree: tree i of a batch seeded seeds[i] equals a stand-alone `alphazero.MCTS(seed=seeds[i])` driven call by
call from the same position with the same evaluator values (which tests/test_gpu_mcts_object.py pins to the oracle).  Every
comparison is np.array_equal."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def az():
    import alphazero
    return alphazero


# ---- Connect4 positions without the device: random legal, non-terminal prefixes -----------------------------------------
def _c4_wins(board, r, c):
    p = board[r, c]
    for dr, dc in ((0, 1), (1, 0), (1, 1), (1, -1)):
        run = 1
        for s in (1, -1):
            rr, cc = r + s * dr, c + s * dc
            while 0 <= rr < 6 and 0 <= cc < 7 and board[rr, cc] == p:
                run += 1; rr += s * dr; cc += s * dc
        if run >= 4:
            return True
    return False


def _c4_prefix(rng, length):
    """`length` random legal moves after which the game is not over (retried until so)."""
    while True:
        board = np.zeros((6, 7), np.int8); heights = [0] * 7; moves = []; over = False
        for t in range(length):
            legal = [c for c in range(7) if heights[c] < 6]
            c = int(rng.choice(legal))
            r = heights[c]; board[r, c] = 1 + (t & 1); heights[c] += 1; moves.append(c)
            if _c4_wins(board, r, c) or all(h == 6 for h in heights):
                over = True
                break
        if not over:
            return moves


def _c4_states(az, n, seed, max_len=12):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        gs = az.Connect4GS()
        for mv in _c4_prefix(rng, int(rng.integers(0, max_len + 1))):
            gs.play_move(mv)
        out.append(gs)
    return out


def _c4_at(az, moves):
    gs = az.Connect4GS()
    for mv in moves:
        gs.play_move(mv)
    return gs


def _readout(mb):
    return dict(counts=mb.counts(), q=mb.root_q_values(), p1=mb.probs(1.0), p0=mb.probs(0.0), pp=mb.probs_pruned(1.0),
                rv=mb.root_values(), depth=mb.depths(), root_n=mb.root_ns(), ald=mb.avg_leaf_depths(),
                ent=mb.normalized_root_entropies(), pv=mb.principal_variations(5))


def _readout_one(m):
    return dict(counts=m.counts(), q=m.root_q_values(), p1=m.probs(1.0), p0=m.probs(0.0), pp=m.probs_pruned(1.0),
                rv=m.root_value(), depth=m.depth(), root_n=m.root_n(), ald=np.float32(m.avg_leaf_depth()),
                ent=np.float32(m.normalized_root_entropy()), pv=m.principal_variation(5))


def _assert_tree_equals(batch_out, i, one_out, what):
    for k, want in one_out.items():
        got = batch_out[k][i]
        assert np.array_equal(np.asarray(got), np.asarray(want)), f"{what}: tree {i}: {k} differs: {got} vs {want}"


def _assert_same(a, b, what, perm=None):
    for k in a:
        for i in range(len(a["counts"])):
            j = i if perm is None else perm[i]
            assert np.array_equal(np.asarray(a[k][i]), np.asarray(b[k][j])), f"{what}: {k} of tree {i} differs"


def _drive_alone(az, m, gs, sims, noise=False):
    for _ in range(sims):
        leaf = m.find_leaf(gs)
        v, pi = az.dumb_eval(leaf)
        m.process_result(gs, v, pi, noise)


# ---- 1. the reference's known answer inside a batch ----------------------------------------------------------------------
def test_reference_known_answer_inside_a_batch(az):
    """Connect4 after 1,6,3,6; MCTS{2,2,7}; 800 x dumb_eval; the stream seeded 12345 (mcts_test.cc:41-72)."""
    n = 64
    seeds = [1000 + i for i in range(n)]
    seeds[5] = 12345
    mb = az.MCTSBatch(az.Connect4GS, n, 2.0, max_simulations=800, seeds=seeds)
    mb.reset([_c4_at(az, (1, 6, 3, 6)) for _ in range(n)])
    mb.search(800)
    counts = mb.counts()
    assert counts[5].tolist() == [62, 21, 631, 21, 22, 21, 21]
    assert int(mb.depths()[5]) == 800 and int(mb.root_ns()[5]) == 800
    assert int(np.argmax(mb.probs(0.0)[5])) == 2
    assert any(counts[i].tolist() != counts[5].tolist() for i in range(n) if i != 5)      # the other streams search differently
    mb.reset([_c4_at(az, (1, 6, 3, 6, 4)) for _ in range(n)])
    mb.search(800)
    assert int(np.argmax(mb.counts()[5])) == 2 and int(mb.depths()[5]) == 800


# ---- 2. against the oracle, through the step API ---------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [
    dict(cpuct=1.25, fpu_reduction=0.25),
    dict(cpuct=1.25, fpu_reduction=0.25, epsilon=0.25, root_policy_temp=1.25, root_fpu_zero=True, shaped_dirichlet=True),
    dict(cpuct=2.0, gumbel_enabled=True, gumbel_m=4),
])
def test_step_api_against_the_oracle(az, oracle, cfg):
    """32 different positions, 40 visits, the synthetic evaluator of test_call_by_call_parity_with_oracle shaped by the row's
    tree index; oracle.Mcts(seed=seeds[i]) from the same position must agree in every read-out."""
    n, visits = 32, 40
    noise = cfg.get("epsilon", 0) > 0
    kw = dict(cfg); cpuct = kw.pop("cpuct")
    rng = np.random.default_rng(20260101)
    prefixes = [_c4_prefix(rng, int(rng.integers(0, 13))) for _ in range(n)]
    seeds = [500 + 7 * i for i in range(n)]
    mb = az.MCTSBatch(az.Connect4GS, n, cpuct, max_simulations=visits, **kw)
    mb.reset([_c4_at(az, p) for p in prefixes], seeds=seeds)
    os_, ogs = [], []
    for i in range(n):
        os_.append(oracle.Mcts(cpuct, 2, 7, seed=seeds[i], **kw))
        og = oracle.Game(oracle.GAME_CONNECT4)
        for mv in prefixes[i]:
            og.play(mv)
        ogs.append(og)
    if cfg.get("gumbel_enabled"):
        mb.set_gumbel_num_sims(visits)
        for o in os_:
            o.set_gumbel_num_sims(visits)
    for _ in range(visits):
        canon, idx = mb.find_leaves(numpy=True)
        assert np.all(np.diff(idx.astype(np.int64)) > 0)                      # compacted rows: ascending tree order
        row_of = {int(t): r for r, t in enumerate(idx)}
        V = np.zeros((len(idx), 3), np.float32); PI = np.zeros((len(idx), 7), np.float32)
        for t in range(n):
            oleaf = os_[t].find_leaf(ogs[t])
            v, pi = (np.full(3, 1 / 3, np.float32), np.full(7, 1 / 7, np.float32)) if oleaf.scores() is not None else oracle.dumb_eval(oleaf)
            if t in row_of:
                assert oleaf.scores() is None
                assert np.array_equal(canon[row_of[t]], oleaf.canonical()), f"tree {t}: another leaf than the oracle's"
                pi = (pi * (1 + 0.3 * np.sin(np.arange(7) + t))).astype(np.float32); pi /= pi.sum()
                V[row_of[t]] = v; PI[row_of[t]] = pi
            else:
                assert oleaf.scores() is not None, f"tree {t}: a non-terminal leaf got no row"
            os_[t].process_result(v.copy(), pi, noise)
        mb.process_results(V, PI, noise)
    out = _readout(mb)
    gp = mb.gumbel_improved_policies() if cfg.get("gumbel_enabled") else None
    ga = mb.gumbel_final_actions() if cfg.get("gumbel_enabled") else None
    for t, o in enumerate(os_):
        assert np.array_equal(out["counts"][t], o.counts()), f"tree {t}"
        assert np.array_equal(out["q"][t], o.root_q()), f"tree {t}"
        assert np.array_equal(out["p1"][t], o.probs(1.0)) and np.array_equal(out["p0"][t], o.probs(0.0)), f"tree {t}"
        assert np.array_equal(out["pp"][t], o.probs(1.0, pruned=True)), f"tree {t}"
        assert np.array_equal(out["rv"][t], o.root_value()), f"tree {t}"
        assert int(out["depth"][t]) == o.depth() == visits and int(out["root_n"][t]) == o.root_n()
        assert np.array_equal(out["pv"][t], o.principal_variation(5)), f"tree {t}"
        if gp is not None:
            assert np.array_equal(gp[t], o.gumbel_improved_policy()), f"tree {t}"
            assert int(ga[t]) == o.gumbel_final_action(), f"tree {t}"


# ---- 3. every game ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["TawlbwrddGS", "BrandubhGS", "OpenTaflGS", "StarGambitUnifiedGS"])
def test_every_wide_game_equals_stand_alone_objects(az, name):
    """8 positions (prefixes of a seeded random playout, legality from the rules kernels' valid masks), 30 visits, RANDOM
    evaluator: the batch against 8 stand-alone MCTS objects read out the same way."""
    Game = getattr(az, name)
    n, visits = 8, 30
    M = Game.NUM_MOVES()
    rng = np.random.default_rng(11)
    states = []
    gs = Game(0) if name == "StarGambitUnifiedGS" else Game()
    for i in range(n):
        states.append(gs.copy())
        for _ in range(2):                      # the next position is two plies further down the playout
            valid = np.flatnonzero(gs.valid_moves())
            gs.play_move(int(rng.choice(valid)))
            assert gs.scores() is None
    seeds = [31 + i for i in range(n)]
    kw = dict(fpu_reduction=0.25)
    mb = az.MCTSBatch(Game, n, 1.25, max_simulations=visits, seeds=seeds, **kw)
    mb.reset(states)
    mb.search(visits)
    out = _readout(mb)
    assert out["depth"].tolist() == [visits] * n
    for i in range(n):
        m = az.MCTS(1.25, 2, M, game=Game, seed=seeds[i], max_simulations=visits, relative_values=(name == "StarGambitUnifiedGS"), **kw)
        _drive_alone(az, m, states[i], visits)
        _assert_tree_equals(out, i, _readout_one(m), name)


# ---- 4. / 5. the net and the cache on the device ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def c4_net(az):
    from alphazero import torch_net
    spec = torch_net.connect4_spec()
    return az.HipLeafNet(torch_net.random_init(spec, seed=3), spec, precision="bf16")


@pytest.fixture(scope="module")
def net_search(az, c4_net):
    """Connect4, 256 positions x 120 visits with the HIP leaf net through search(): shared by the net and cache tests."""
    n, visits = 256, 120
    states = _c4_states(az, n, seed=5)
    seeds = [9000 + i for i in range(n)]
    mb = az.MCTSBatch(az.Connect4GS, n, 1.25, fpu_reduction=0.25, max_simulations=visits, seeds=seeds)
    mb.reset(states)
    mb.search(visits, net=c4_net)
    return dict(n=n, visits=visits, states=states, seeds=seeds, out=_readout(mb), stats=mb.stats())


def test_net_on_the_device_equals_the_step_api_and_stand_alone_objects(az, c4_net, net_search):
    import torch
    n, visits, states, seeds = net_search["n"], net_search["visits"], net_search["states"], net_search["seeds"]
    assert net_search["out"]["depth"].tolist() == [visits] * n
    mb = az.MCTSBatch(az.Connect4GS, n, 1.25, fpu_reduction=0.25, max_simulations=visits, seeds=seeds)
    mb.reset(states)
    recorded = {t: [] for t in (0, 1, 100, 255)}          # the rows these trees were answered with, step by step
    for _ in range(visits):
        canon, idx = mb.find_leaves()
        v, pi = c4_net.process(canon) if canon.shape[0] else (np.zeros((0, 3), np.float32), np.zeros((0, 7), np.float32))
        if canon.shape[0]:
            vh, ph, ih = v.cpu().numpy(), pi.cpu().numpy(), idx.cpu().numpy()
            for r, t in enumerate(ih):
                if int(t) in recorded:
                    recorded[int(t)].append((vh[r].copy(), ph[r].copy()))
        mb.process_results(v, pi)
    _assert_same(net_search["out"], _readout(mb), "search() vs the step API with net.process")
    # stand-alone objects fed net.process of their own leaves, one at a time (the rows of a tile do not depend on the batch)
    dev = torch.device("cuda", 0)
    for t in recorded:
        m = az.MCTS(1.25, 2, 7, fpu_reduction=0.25, seed=seeds[t], max_simulations=visits)
        for _ in range(visits):
            leaf = m.find_leaf(states[t])
            if leaf.scores() is None:
                v, pi = c4_net.process(torch.from_numpy(np.ascontiguousarray(leaf.canonicalized()[None])).to(dev))
                torch.cuda.synchronize()
                m.process_result(states[t], v.cpu().numpy()[0], pi.cpu().numpy()[0])
            else:
                m.process_result(states[t], np.full(3, 1 / 3, np.float32), np.full(7, 1 / 7, np.float32))
        _assert_tree_equals(net_search["out"], t, _readout_one(m), "stand-alone object fed net.process of its own leaves")


def test_cache_serves_the_answers_the_net_gave(az, c4_net, net_search):
    n, visits, states, seeds = net_search["n"], net_search["visits"], net_search["states"], net_search["seeds"]
    cache = az.ShardedS3FIFOCache.for_engine(1 << 17, 7, 3)
    mb = az.MCTSBatch(az.Connect4GS, n, 1.25, fpu_reduction=0.25, max_simulations=visits, seeds=seeds)
    mb.reset(states)
    mb.search(visits, net=c4_net, cache=cache)
    out = _readout(mb)
    assert np.array_equal(out["counts"], net_search["out"]["counts"])
    _assert_same(net_search["out"], out, "with a cache vs without")
    st = mb.stats()
    assert st["simulations"] == n * visits
    assert cache.hits() + cache.misses() == st["simulations"] - st["terminal_leaves"]
    assert cache.misses() == st["evaluator_leaves"]
    # 64 trees on ONE position: what one tree asked the net, the others find in the cache.  (Root noise from 64 different
    # streams makes the trees differ; without it PUCT is deterministic, all 64 descend to the same leaf in the same step and
    # every probe comes before that step's insert.)
    cache2 = az.ShardedS3FIFOCache.for_engine(1 << 16, 7, 3)
    mb2 = az.MCTSBatch(az.Connect4GS, 64, 1.25, epsilon=0.25, max_simulations=60, seeds=list(range(64)))
    mb2.reset([_c4_at(az, (3, 3, 2)) for _ in range(64)])
    mb2.search(60, net=c4_net, cache=cache2, root_noise=True)
    assert int(mb2.depths().min()) == 60
    assert cache2.hits() > 0
    st2 = mb2.stats()
    assert cache2.hits() + cache2.misses() == st2["simulations"] - st2["terminal_leaves"]


@pytest.fixture(scope="module")
def brandubh_net(az):
    from alphazero import torch_net
    spec = torch_net.brandubh_spec()
    return az.HipLeafNet(torch_net.random_init(spec, seed=3), spec, precision="bf16")


def _assert_cache_accounts_for_every_leaf(mb, cache):
    st = mb.stats()
    assert cache.hits() + cache.misses() == st["simulations"] - st["terminal_leaves"]
    assert cache.misses() == st["evaluator_leaves"]


@pytest.mark.parametrize("K", [1, 3])
def test_wide_game_cache_serves_the_answers_the_net_gave(az, brandubh_net, K):
    """The cache on the wavefront-per-tree engine (Brandubh), which writes a leaf's planes before it probes (Connect4 probes
    first), with K leaves of every tree in flight per step.  (a) 3 trees on 3 positions, 24 visits: every read-out with a cache
    equals the one without, and every non-terminal leaf is either a hit or a miss that went to the net.  (b) 4 trees on the start
    position told apart by root noise: what one tree asked the net, another finds in the cache.
    (a)'s equality is asserted for K = 3 as for K = 1."""
    visits = 24
    kw = dict(max_simulations=visits, leaves_per_step=K)
    rng = np.random.default_rng(17)
    states, gs = [], az.BrandubhGS()
    for _ in range(3):
        for _ in range(2):                      # the next position is two plies further down a random playout
            gs.play_move(int(rng.choice(np.flatnonzero(gs.valid_moves()))))
            assert gs.scores() is None
        states.append(gs.copy())
    seeds = [41, 42, 43]
    plain = az.MCTSBatch(az.BrandubhGS, 3, 1.25, fpu_reduction=0.25, seeds=seeds, **kw)
    plain.reset(states)
    plain.search(visits, net=brandubh_net)
    cache = az.ShardedS3FIFOCache.for_engine(1 << 12, az.BrandubhGS.NUM_MOVES(), 3)
    mb = az.MCTSBatch(az.BrandubhGS, 3, 1.25, fpu_reduction=0.25, seeds=seeds, **kw)
    mb.reset(states)
    mb.search(visits, net=brandubh_net, cache=cache)
    assert mb.depths().tolist() == [visits] * 3
    _assert_same(_readout(plain), _readout(mb), f"K = {K}: with a cache vs without")
    assert mb.stats()["simulations"] == 3 * visits
    _assert_cache_accounts_for_every_leaf(mb, cache)

    cache2 = az.ShardedS3FIFOCache.for_engine(1 << 12, az.BrandubhGS.NUM_MOVES(), 3)
    mb2 = az.MCTSBatch(az.BrandubhGS, 4, 1.25, epsilon=0.25, seeds=[1, 2, 3, 4], **kw)
    mb2.reset([az.BrandubhGS() for _ in range(4)])
    mb2.search(visits, net=brandubh_net, cache=cache2, root_noise=True)
    assert int(mb2.depths().min()) == visits
    assert cache2.hits() > 0
    _assert_cache_accounts_for_every_leaf(mb2, cache2)


# ---- 6. order independence -------------------------------------------------------------------------------------------------------
def test_order_independence_and_a_batch_of_one(az):
    n, visits = 48, 50
    states = _c4_states(az, n, seed=9)
    seeds = [77 + 3 * i for i in range(n)]
    kw = dict(fpu_reduction=0.25, epsilon=0.25, root_policy_temp=1.25, shaped_dirichlet=True)
    mb = az.MCTSBatch(az.Connect4GS, n, 1.25, max_simulations=visits, **kw)
    mb.reset(states, seeds=seeds)
    mb.search(visits, root_noise=True)
    a = _readout(mb)
    perm = np.random.default_rng(2).permutation(n)
    mb.reset([states[j] for j in perm], seeds=[seeds[j] for j in perm])       # tree i of the second run = tree perm[i] of the first
    mb.search(visits, root_noise=True)
    b = _readout(mb)
    _assert_same(b, a, "permuted batch", perm=perm)
    for t in (0, 17):
        one = az.MCTSBatch(az.Connect4GS, 1, 1.25, max_simulations=visits, **kw)
        one.reset([states[t]], seeds=[seeds[t]])
        one.search(visits, root_noise=True)
        m = az.MCTS(1.25, 2, 7, seed=seeds[t], max_simulations=visits, **kw)
        _drive_alone(az, m, states[t], visits, noise=True)
        alone = _readout_one(m)
        _assert_tree_equals(_readout(one), 0, alone, "batch of one vs the stand-alone object")
        _assert_tree_equals(a, t, alone, "tree of the batch vs the stand-alone object")


# ---- 7. errors ------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_object_usable(az):
    n = 24
    good = _c4_states(az, n, seed=13)
    bad = [g.copy() for g in good]
    full = az.Connect4GS()
    for mv in (0, 0, 0, 0, 0, 0):
        full.play_move(mv)
    full._moves.append(0); full._snap = None          # a seventh stone in column 0
    bad[17] = full
    mb = az.MCTSBatch(az.Connect4GS, n, 2.0, max_simulations=30, seeds=list(range(n)))
    with pytest.raises(RuntimeError, match=r"tree 17\b"):
        mb.reset(bad)
    with pytest.raises(RuntimeError, match="reset"):
        mb.search(5)
    mb.reset(good)                                     # still usable
    mb.search(20)
    assert mb.depths().tolist() == [20] * n
    with pytest.raises(RuntimeError, match="max_simulations"):
        mb.search(11)
    mb.search(10)
    assert mb.depths().tolist() == [30] * n
    with pytest.raises(RuntimeError, match="max_simulations"):
        mb.find_leaves()
    mb.reset(good)
    canon, idx = mb.find_leaves(numpy=True)
    assert canon.shape == (n, 4, 6, 7) and idx.tolist() == list(range(n))
    with pytest.raises(RuntimeError, match="process_results"):
        mb.process_results(np.zeros((n, 2), np.float32), np.zeros((n, 7), np.float32))
    with pytest.raises(RuntimeError, match="process_results"):
        mb.process_results(np.zeros((n, 3), np.float32), np.zeros((n - 1, 7), np.float32))
    with pytest.raises(RuntimeError):
        mb.find_leaves()                               # the pending step has to be answered first
    mb.process_results(np.full((n, 3), 1 / 3, np.float32), np.full((n, 7), 1 / 7, np.float32))
    assert mb.depths().tolist() == [1] * n
    with pytest.raises(RuntimeError, match="max_simulations"):
        az.MCTSBatch(az.Connect4GS, 4, 2.0, max_simulations=0)
    with pytest.raises(RuntimeError, match="bytes"):
        az.MCTSBatch(az.Connect4GS, 1 << 22, 2.0, max_simulations=100000)
    with pytest.raises(RuntimeError, match=f"{n} positions"):
        mb.reset(good[:-1])


# ---- the structural condition of the speed claim ----------------------------------------------------------------------------------
def test_search_enqueues_a_constant_number_of_launches_and_needs_no_synchronisation(az, c4_net):
    """search(visits) is `visits` step pairs on one stream with no host synchronisation inside: the results are the same
    whether or not the caller synchronises between searches, and the launches per step do not depend on N."""
    visits = 60
    per_step = {}
    for n in (8, 1024):
        states = _c4_states(az, n, seed=21)
        seeds = [5 + i for i in range(n)]
        mb = az.MCTSBatch(az.Connect4GS, n, 1.25, max_simulations=visits, seeds=seeds)
        mb.reset(states)
        l0 = mb.stats()
        mb.search(visits, net=c4_net)              # one call, nothing in between
        l1 = mb.stats()
        a = _readout(mb)
        mb.reset(states)
        for _ in range(visits // 10):              # six calls, the host waiting after each
            mb.search(10, net=c4_net)
            mb.synchronize()
        _assert_same(a, _readout(mb), f"{n} trees: one search vs synchronised pieces")
        assert l1["steps"] - l0["steps"] == visits
        per_step[n] = ((l1["launches"] - l0["launches"]) / visits, (l1["net_calls"] - l0["net_calls"]) / visits)
    assert per_step[8] == per_step[1024] == (3.0, 1.0)      # find-leaves, compaction, process-results + one net call
    # RANDOM evaluator: three launches a step; with a cache: one insert launch more
    mb = az.MCTSBatch(az.Connect4GS, 16, 1.25, max_simulations=40, seeds=list(range(16)))
    mb.reset(_c4_states(az, 16, seed=22))
    l0 = mb.stats(); mb.search(20); l1 = mb.stats()
    assert (l1["launches"] - l0["launches"], l1["net_calls"] - l0["net_calls"]) == (60, 0)
    cache = az.ShardedS3FIFOCache.for_engine(1 << 12, 7, 3)
    mb.search(20, net=c4_net, cache=cache); l2 = mb.stats()
    assert (l2["launches"] - l1["launches"], l2["net_calls"] - l1["net_calls"]) == (80, 20)
