"""-m gpu: `alphazero.MCTSBatch.search / play(..., evaluator="playout")`: every non-terminal leaf evaluated by a random rollout
on the device.  The contract is that of tests/test_gpu_search_batch.py, bit-exactness per tree: tree i equals the stand-alone
`alphazero.MCTS(seed=seeds[i])` driven from Python, its j-th evaluator leaf since reset() answered by
`alphazero.playout_eval(leaf, seed=MCTSBatch.rollout_seed(rollout_seeds[i], j))`.  Every comparison is np.array_equal."""
import numpy as np
import pytest

from test_gpu_search_batch import _assert_tree_equals, _c4_at, _c4_prefix, az  # noqa: F401
from test_gpu_search_batch_wu import _objects, _objects_back, _objects_find

pytestmark = pytest.mark.gpu

_C4_WIN_IN_ONE = (0, 1, 0, 1, 0, 1)                      # rollouts of length 1 and terminal leaves mix
_C4_FULL_COLUMNS = (0,) * 6 + (3,) * 6                   # columns 0 and 3 are full, nobody has four
_C4_LATE = tuple(_c4_prefix(np.random.default_rng(77), 30))   # ~30 moves: short rollouts, many terminal leaves


def _c4_mixed(az, n):
    kinds = [(), _C4_WIN_IN_ONE, _C4_FULL_COLUMNS, _C4_LATE]
    out = [_c4_at(az, kinds[i % 4]) for i in range(n)]
    assert all(g.scores() is None for g in out)
    return out


def _out(mb):
    return dict(counts=mb.counts(), p1=mb.probs(1.0), rv=mb.root_values(), q=mb.root_q_values(), depth=mb.depths(), root_n=mb.root_ns())


def _out_one(m):
    return dict(counts=m.counts(), p1=m.probs(1.0), rv=m.root_value(), q=m.root_q_values(), depth=m.depth(), root_n=m.root_n())


def _compare(mb, ms, what):
    out = _out(mb)
    for i, m in enumerate(ms):
        _assert_tree_equals(out, i, _out_one(m), what)
    return out


def _search_objects(az, ms, gss, live, visits, rs, j, noise=False, one_by_one=False):
    """`visits` simulations of the live stand-alone objects in lock step; tree i's evaluator leaf number j[i] is answered by
    playout_eval with the seed rollout_seed(rs[i], j[i]) (one playout_eval_batch per step), a terminal leaf takes no rollout.
    -> (rollouts, terminal leaves)"""
    n_roll = n_term = 0
    for _ in range(visits):
        leaves = [ms[i].find_leaf(gss[i]) for i in live]
        need = [(i, leaf) for i, leaf in zip(live, leaves) if leaf.scores() is None]
        ans = {}
        if need:
            sd = [az.MCTSBatch.rollout_seed(rs[i], j[i]) for i, _ in need]
            if one_by_one:
                V, PI = zip(*[az.playout_eval(leaf, seed=s) for (_, leaf), s in zip(need, sd)])
            else:
                V, PI = az.playout_eval_batch([leaf for _, leaf in need], sd)
            for (i, _), v, pi in zip(need, V, PI):
                ans[i] = (v, pi)
                j[i] += 1
        n_roll += len(need); n_term += len(leaves) - len(need)
        for i, leaf in zip(live, leaves):
            v, pi = ans[i] if i in ans else az.dumb_eval(leaf)      # (a terminal leaf's evaluation is never used)
            ms[i].process_result(gss[i], v, pi, noise)
    return n_roll, n_term


def _c4_run(az, n, visits, states, seeds, rs, **kw):
    mb = az.MCTSBatch(az.Connect4GS, n, 1.25, fpu_reduction=0.25, max_simulations=visits, seeds=seeds, **kw)
    mb.reset(states, rollout_seeds=rs)
    mb.search(visits, evaluator="playout")
    return mb


# ---- 1. Connect4, K = 1, against the stand-alone objects ------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 33, 65])
def test_connect4_equals_stand_alone_objects(az, n):
    """48 visits on mixed positions (start, a win in one, full columns, ~30 moves in).  N = 33 crosses the 32 trees of a
    workgroup of the find kernel, N = 65 a wavefront of the one-lane-per-rollout kernel."""
    visits = 48
    states = _c4_mixed(az, n)
    seeds = [8100 + 13 * i for i in range(n)]
    rs = [(0x1234567 * (i + 1)) ^ 0xABCDEF for i in range(n)]
    mb = _c4_run(az, n, visits, states, seeds, rs)
    assert mb.rollout_seeds().tolist() == rs
    ms = [az.MCTS(1.25, 2, 7, fpu_reduction=0.25, seed=seeds[i], max_simulations=visits) for i in range(n)]
    n_roll, n_term = _search_objects(az, ms, states, list(range(n)), visits, rs, [0] * n)
    out = _compare(mb, ms, f"N = {n}")
    assert out["root_n"].tolist() == [visits] * n
    st = mb.stats()
    assert st["simulations"] == n * visits and st["net_calls"] == 0
    assert (st["evaluator_leaves"], st["terminal_leaves"]) == (n_roll, n_term) and n_term > 0 and n_roll > 0


def test_default_rollout_seeds_derive_from_the_tree_seeds(az):
    """reset() without rollout_seeds: mix64(seeds[i] ^ kRollSalt), restated here; the search with them equals the objects."""
    n, visits = 4, 24
    M64, SALT = (1 << 64) - 1, 0x9E3779B97F4A7C15

    def mix64(x):
        x = (x + 0x9E3779B97F4A7C15) & M64
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
        return x ^ (x >> 31)
    states = _c4_mixed(az, n)
    seeds = [5 + 3 * i for i in range(n)]
    mb = _c4_run(az, n, visits, states, seeds, None)
    rs = [mix64(s ^ SALT) for s in seeds]
    assert mb.rollout_seeds().tolist() == rs
    ms = [az.MCTS(1.25, 2, 7, fpu_reduction=0.25, seed=seeds[i], max_simulations=visits) for i in range(n)]
    _search_objects(az, ms, states, list(range(n)), visits, rs, [0] * n)
    _compare(mb, ms, "default rollout seeds")


# ---- 2. a tree's result does not depend on the batch around it --------------------------------------------------------------
def test_rows_do_not_depend_on_the_batch_size(az):
    visits = 48
    states = _c4_mixed(az, 8)
    seeds = [8100 + 13 * i for i in range(8)]
    rs = [(0x1234567 * (i + 1)) ^ 0xABCDEF for i in range(8)]
    a = _out(_c4_run(az, 8, visits, states, seeds, rs))
    b = _out(_c4_run(az, 3, visits, states[:3], seeds[:3], rs[:3]))
    for k in a:
        assert np.array_equal(a[k][:3], b[k]), f"{k}: rows 0..2 of the N = 8 run differ from the N = 3 run"


# ---- 3. K > 1: a playout leaf is an immediate, backed up in descent order ------------------------------------------------
@pytest.mark.parametrize("visits", [40, 42])
def test_wu_uct_equals_the_batched_object_calls(az, visits):
    """Connect4, N = 4, K = 4 against find_leaf_batched / process_result_batched with the rollout's answer processed at once,
    before the tree's next descent; 42 visits end in a step of 2 descents."""
    n, K = 4, 4
    states = _c4_mixed(az, n)
    seeds = [700 + 11 * i for i in range(n)]
    rs = [900 + 7 * i for i in range(n)]
    mb = _c4_run(az, n, visits, states, seeds, rs, leaves_per_step=K)
    ms = _objects(az, az.Connect4GS, n, seeds, visits, fpu_reduction=0.25)
    j = [0] * n

    def now(t, leaf):
        ans = az.playout_eval(leaf, seed=az.MCTSBatch.rollout_seed(rs[t], j[t]))
        j[t] += 1
        return ans
    left, n_term = visits, 0
    while left:
        kk = min(K, left)
        pending, nt = _objects_find(az, ms, states, kk, now=now)
        assert not pending
        _objects_back(ms, states, [], None, None)
        left -= kk; n_term += nt
    _compare(mb, ms, f"K = {K}, {visits} visits")
    st = mb.stats()
    assert st["steps"] == -(-visits // K) and st["simulations"] == n * visits
    assert (st["evaluator_leaves"], st["terminal_leaves"]) == (sum(j), n_term)


# ---- 4. the wide games: the rollout continues the descent's repetition list ----------------------------------------------
def _wide_states(az, name, n):
    """n different non-terminal positions a few random moves in; tree 0 of a Tafl game starts from an IMAGE whose repetition
    record holds the positions of those moves (from_bytes(to_bytes())), so the rollout's repetition counts start there."""
    rng = np.random.default_rng(23)
    Game = getattr(az, name)
    out = []
    while len(out) < n:
        i = len(out)
        gs = Game(i % 2) if name == "StarGambitUnifiedGS" else Game()      # StarGambit: two different variants
        for _ in range(4 + 2 * i):
            gs.play_move(int(rng.choice(np.flatnonzero(gs.valid_moves()))))
            if gs.scores() is not None:
                break                                                      # (random play ended the game: another prefix)
        else:
            out.append(gs)
    if name != "StarGambitUnifiedGS":
        bb = 3 * Game.BOARD * Game.BOARD
        image = bytes(out[0].to_bytes())
        assert int(np.frombuffer(image[bb + 6: bb + 10], np.uint32)[0]) > 0, "the repetition record of tree 0's image is empty"
        out[0] = Game.from_bytes(image)
    return out


@pytest.mark.parametrize("name,n,visits,K", [("BrandubhGS", 4, 24, 1), ("TawlbwrddGS", 2, 16, 1), ("OpenTaflGS", 2, 16, 1),
                                             ("StarGambitUnifiedGS", 2, 12, 1), ("BrandubhGS", 4, 24, 2)])
def test_wide_games_equal_stand_alone_objects(az, name, n, visits, K):
    Game = getattr(az, name)
    states = _wide_states(az, name, n)
    seeds = [31 + 5 * i for i in range(n)]
    rs = [77 + 3 * i for i in range(n)]
    mb = az.MCTSBatch(Game, n, 1.25, fpu_reduction=0.25, max_simulations=visits, seeds=seeds, leaves_per_step=K)
    mb.reset(states, rollout_seeds=rs)
    mb.search(visits, evaluator="playout")
    ms = _objects(az, Game, n, seeds, visits, fpu_reduction=0.25)
    j = [0] * n
    if K == 1:
        _search_objects(az, ms, states, list(range(n)), visits, rs, j, one_by_one=(name == "StarGambitUnifiedGS"))
    else:
        def now(t, leaf):
            ans = az.playout_eval(leaf, seed=az.MCTSBatch.rollout_seed(rs[t], j[t]))
            j[t] += 1
            return ans
        for _ in range(visits // K):
            pending, _ = _objects_find(az, ms, states, K, now=now)
            assert not pending
            _objects_back(ms, states, [], None, None)
    _compare(mb, ms, f"{name}, K = {K}")
    assert mb.stats()["evaluator_leaves"] == sum(j)


# ---- 5. Gumbel ------------------------------------------------------------------------------------------------------------------
def test_gumbel_search_with_rollouts(az):
    n, visits = 4, 32
    states = _c4_mixed(az, n)
    seeds = [900 + 5 * i for i in range(n)]
    rs = [40 + i for i in range(n)]
    kw = dict(gumbel_enabled=True, gumbel_m=4)
    mb = az.MCTSBatch(az.Connect4GS, n, 2.0, max_simulations=visits, seeds=seeds, **kw)
    mb.reset(states, rollout_seeds=rs)
    mb.search(visits, evaluator=az.EvalType.PLAYOUT)
    ms = [az.MCTS(2.0, 2, 7, seed=seeds[i], max_simulations=visits, **kw) for i in range(n)]
    for m in ms:
        m.set_gumbel_num_sims(visits)
    _search_objects(az, ms, states, list(range(n)), visits, rs, [0] * n)
    assert mb.gumbel_final_actions().tolist() == [m.gumbel_final_action() for m in ms]
    counts = mb.counts()
    for i, m in enumerate(ms):
        assert np.array_equal(counts[i], m.counts()), f"tree {i}"


# ---- 6. games: the rollout count runs on across moves ---------------------------------------------------------------------
@pytest.mark.parametrize("name,n,visits,moves", [("Connect4GS", 8, 16, 6), ("BrandubhGS", 2, 12, 3)])
def test_play_equals_the_object_loop(az, name, n, visits, moves):
    Game = getattr(az, name)
    c4 = name == "Connect4GS"
    gss = _c4_mixed(az, n) if c4 else _wide_states(az, name, n)
    seeds = [4100 + 13 * i for i in range(n)]
    rs = [61 + 9 * i for i in range(n)]
    mb = az.MCTSBatch(Game, n, 1.25, fpu_reduction=0.25, max_simulations=visits * moves if c4 else visits, seeds=seeds)
    mb.reset(gss, rollout_seeds=rs)
    mb.play(visits, evaluator="playout", max_moves=moves, temp=1.0)
    ms = _objects(az, Game, n, seeds, visits * moves, fpu_reduction=0.25)
    gss = [g.copy() for g in gss]
    logs = [[] for _ in range(n)]
    j = [0] * n
    live = list(range(n))
    for _ in range(moves):
        _search_objects(az, ms, gss, live, visits, rs, j)
        for i in live:
            mv = int(ms[i].pick_move(ms[i].probs(1.0)))
            ms[i].update_root(gss[i], mv)
            gss[i].play_move(mv)
            logs[i].append(mv)
        live = [i for i in live if gss[i].scores() is None]
    assert [l.tolist() for l in mb.move_logs()] == logs
    fin = mb.finished()
    assert fin.tolist() == [g.scores() is not None for g in gss]
    fs = mb.final_scores()
    for i in range(n):
        if fin[i]:
            assert np.array_equal(fs[i], gss[i].scores()), f"tree {i}"
    assert mb.stats()["evaluator_leaves"] == sum(j) and max(j) > visits, "the rollout count is not reset by update_roots"


# ---- 7. launches ----------------------------------------------------------------------------------------------------------------
def test_a_playout_step_takes_at_most_three_launches(az):
    visits = 12
    per_step = {}
    for n in (8, 256):
        for K in (1, 4):
            mb = az.MCTSBatch(az.Connect4GS, n, 1.25, max_simulations=visits, seeds=list(range(n)), leaves_per_step=K)
            mb.reset(_c4_mixed(az, n))
            l0 = mb.stats(); mb.search(visits, evaluator="playout"); l1 = mb.stats()
            steps = l1["steps"] - l0["steps"]
            assert steps == visits // K
            per_step[(n, K)] = (l1["launches"] - l0["launches"]) / steps
            assert l1["launches"] - l0["launches"] <= 3 * visits
            assert l1["net_calls"] == 0
            assert l1["evaluator_leaves"] + l1["terminal_leaves"] == l1["simulations"] == n * visits
    assert per_step[(8, 1)] == per_step[(256, 1)] <= 3 and per_step[(8, 4)] == per_step[(256, 4)] <= per_step[(8, 1)]


# ---- 8. enqueue-only ---------------------------------------------------------------------------------------------------------
def test_search_needs_no_synchronisation(az):
    n, visits = 16, 40
    states = _c4_mixed(az, n)
    seeds = [300 + i for i in range(n)]
    mb = az.MCTSBatch(az.Connect4GS, n, 1.25, fpu_reduction=0.25, max_simulations=visits, seeds=seeds)
    mb.reset(states)
    for _ in range(4):
        mb.search(10, evaluator="playout")
    a = _out(mb)
    mb.reset(states)
    for _ in range(4):
        mb.search(10, evaluator="playout")
        mb.synchronize()
    b = _out(mb)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
