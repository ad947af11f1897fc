"""-m gpu: moves played on an `alphazero.MCTSBatch` with tree reuse (pick_moves / update_roots / add_root_noise /
apply_root_policy_temp / play and the game read-outs).  The contract is that of tests/test_gpu_search_batch.py, carried across
moves: tree i equals the stand-alone `alphazero.MCTS(seed=seeds[i])` driven by the same calls - search, pick_move(probs(temp)),
update_root, gs.play_move - bit for bit.  Every comparison is np.array_equal."""
import numpy as np
import pytest

from test_gpu_search_batch import _c4_at, _c4_states, _drive_alone, az, c4_net  # noqa: F401
from test_gpu_search_batch_wu import _C4_ONE_COLUMN, _objects_back, _objects_find

pytestmark = pytest.mark.gpu

# one legal column and one empty cell: whatever is picked, the move fills the board and the game is over
_C4_LAST_CELL = tuple(_C4_ONE_COLUMN) + (6,) * 5
# player 0 has three stones in column 0 and is to move: a win in one
_C4_WIN_IN_ONE = (0, 1, 0, 1, 0, 1)
_C4_MIXED = [(), (3, 3, 2), _C4_WIN_IN_ONE, (1, 6, 3, 6, 4, 2, 2), _C4_LAST_CELL, (3, 3, 3, 3, 3, 3)]


def _four(mb):
    return dict(counts=mb.counts(), rv=mb.root_values(), root_n=mb.root_ns(), depth=mb.depths())


def _four_one(m):
    return dict(counts=m.counts(), rv=m.root_value(), root_n=m.root_n(), depth=m.depth())


def _assert_four(out, i, m, what):
    for k, want in _four_one(m).items():
        assert np.array_equal(np.asarray(out[k][i]), np.asarray(want)), f"{what}: tree {i}: {k} differs: {out[k][i]} vs {want}"


def _search_objects(az, ms, gss, live, visits, K=1, noise=False):
    """search(visits) with the RANDOM evaluator on the stand-alone objects of the live trees (K > 1: the batched calls)."""
    if K == 1:
        for i in live:
            _drive_alone(az, ms[i], gss[i], visits, noise)
        return
    sub, st = [ms[i] for i in live], [gss[i] for i in live]
    left = visits
    while left:
        kk = min(K, left)
        pending, _ = _objects_find(az, sub, st, kk, noise, now=lambda t, leaf: az.dumb_eval(leaf))
        assert not pending
        _objects_back(sub, st, [], None, None, noise)
        left -= kk


def _walk(az, mb, ms, gss, moves, visits, temp=1.0, K=1, what=""):
    """`moves` x (search, pick, update_roots) on the batch beside the objects, everything compared after every move.
    -> (the read-outs after every search, the picked moves)"""
    n = len(ms)
    live = [i for i in range(n) if gss[i].scores() is None]
    outs, picks = [], []
    for mv_no in range(moves):
        mb.search(visits)
        _search_objects(az, ms, gss, live, visits, K)
        out = _four(mb)
        for i in range(n):
            _assert_four(out, i, ms[i], f"{what} move {mv_no}, after the search")
        got = mb.pick_moves(temp)
        want = np.full(n, -1, np.int32)
        for i in live:
            want[i] = ms[i].pick_move(ms[i].probs(temp))
        assert got.dtype == np.int32 and np.array_equal(got, want), f"{what} move {mv_no}: picked {got}, the objects {want}"
        mb.update_roots()
        for i in live:
            ms[i].update_root(gss[i], int(want[i]))
            gss[i].play_move(int(want[i]))
        out2 = _four(mb)
        for i in range(n):
            _assert_four(out2, i, ms[i], f"{what} move {mv_no}, after update_roots")
        live = [i for i in live if gss[i].scores() is None]
        fin = mb.finished()
        assert fin.dtype == np.bool_ and fin.tolist() == [g.scores() is not None for g in gss], f"{what} move {mv_no}"
        outs.append(out); picks.append(got)
    return outs, picks


# ---- 1. moves and reuse equal stand-alone objects, Connect4 ---------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 4])
def test_connect4_moves_and_reuse_equal_stand_alone_objects(az, K):
    """6 trees from mixed positions (empty, mid-game records, a win in one, a board with one empty cell, a full column), 5 moves
    x 24 visits, RANDOM evaluator, temp 1; K = 4 against the batched object calls."""
    n, moves, visits = 6, 5, 24
    gss = [_c4_at(az, p) for p in _C4_MIXED]
    assert all(g.scores() is None for g in gss)
    seeds = [4100 + 13 * i for i in range(n)]
    mb = az.MCTSBatch(az.Connect4GS, n, 1.25, fpu_reduction=0.25, max_simulations=visits * moves, seeds=seeds, leaves_per_step=K)
    mb.reset(gss)
    ms = [az.MCTS(1.25, 2, 7, fpu_reduction=0.25, seed=seeds[i], max_simulations=visits * moves) for i in range(n)]
    _walk(az, mb, ms, gss, moves, visits, K=K, what=f"K = {K}")
    fin = mb.finished()
    assert fin[4], "the board with one empty cell is full after one move"
    logs = mb.move_logs()
    assert int(logs[4].size) == 1 and [int(l.size) for l in logs] == [len(g._moves) - len(p) for g, p in zip(gss, _C4_MIXED)]
    for i, g in enumerate(mb.states()):
        assert g == gss[i] and g._moves == gss[i]._moves, f"tree {i}: states() is not the object's game state"
    fs = mb.final_scores()
    for i in range(n):
        if fin[i]:
            assert np.array_equal(fs[i], gss[i].scores()), f"tree {i}"
    st = mb.stats()
    assert st["simulations"] < n * visits * moves, "a finished tree costs no further simulation"


# ---- 2. every wide game, with and without compaction after every move ----------------------------------------------------
@pytest.mark.parametrize("name", ["BrandubhGS", "TawlbwrddGS", "OpenTaflGS", "StarGambitUnifiedGS"])
def test_every_wide_game_equals_stand_alone_objects_and_compaction_is_transparent(az, name, monkeypatch):
    """3 trees, 3 moves x 16 visits.  max_simulations = 16: the wide games' budget counts the descents since the last
    update_roots.  Once with AZMI_COMPACT_ABOVE=0 (the arena is compacted after every move), once without."""
    Game = getattr(az, name)
    n, moves, visits = 3, 3, 16
    rng = np.random.default_rng(11)
    start = []
    gs = Game(0) if name == "StarGambitUnifiedGS" else Game()
    for _ in range(n):
        start.append(gs.copy())
        for _ in range(2):
            gs.play_move(int(rng.choice(np.flatnonzero(gs.valid_moves()))))
            assert gs.scores() is None
    seeds = [31 + i for i in range(n)]
    runs = []
    for compact_every_move in (True, False):
        if compact_every_move:
            monkeypatch.setenv("AZMI_COMPACT_ABOVE", "0")
        else:
            monkeypatch.delenv("AZMI_COMPACT_ABOVE", raising=False)
        mb = az.MCTSBatch(Game, n, 1.25, fpu_reduction=0.25, max_simulations=visits, seeds=seeds)
        ms = [az.MCTS(1.25, 2, Game.NUM_MOVES(), game=Game, fpu_reduction=0.25, seed=seeds[i], max_simulations=visits * moves,
                      relative_values=(name == "StarGambitUnifiedGS")) for i in range(n)]
        gss = [g.copy() for g in start]
        mb.reset(gss)
        players = [[g.current_player() for g in gss]]
        outs, picks = [], []
        for mv_no in range(moves):
            o, p = _walk(az, mb, ms, gss, 1, visits, what=f"{name}, compact_every_move = {compact_every_move}, move {mv_no}:")
            outs += o; picks += p
            now = [g.current_player() for g in mb.states()]
            assert now == [g.current_player() for g in gss], f"{name}: the player to move after move {mv_no}"
            players.append(now)
        with pytest.raises(RuntimeError, match="since the last update_roots"):
            mb.search(visits + 1)
        runs.append((outs, picks, players))
    (oa, pa, pla), (ob, pb, plb) = runs
    assert all(np.array_equal(x, y) for x, y in zip(pa, pb)) and pla == plb
    for a, b in zip(oa, ob):
        for k in a:
            assert np.array_equal(a[k], b[k]), f"{name}: {k} depends on compaction"
    if name == "StarGambitUnifiedGS":      # several actions per turn: some move left the same player to move
        assert any(pla[m][i] == pla[m + 1][i] for m in range(moves) for i in range(n))


# ---- 3. play() equals the step-by-step calls; launches per move ------------------------------------------------------------
def test_play_equals_the_step_by_step_calls(az, c4_net):
    n, visits, moves = 16, 20, 4
    states = _c4_states(az, n, seed=41)
    seeds = [600 + i for i in range(n)]
    kw = dict(fpu_reduction=0.25, max_simulations=visits * moves, seeds=seeds)
    a = az.MCTSBatch(az.Connect4GS, n, 1.25, **kw)
    ca = az.ShardedS3FIFOCache.for_engine(1 << 14, 7, 3)
    a.reset(states)
    a.play(visits=visits, max_moves=moves, net=c4_net, cache=ca)          # one call, nothing read back inside
    b = az.MCTSBatch(az.Connect4GS, n, 1.25, **kw)
    cb = az.ShardedS3FIFOCache.for_engine(1 << 14, 7, 3)
    b.reset(states)
    for _ in range(moves):
        b.search(visits, net=c4_net, cache=cb); b.synchronize()
        b.pick_moves(1.0); b.synchronize()
        b.update_roots(); b.synchronize()
    la, lb = a.move_logs(), b.move_logs()
    assert all(np.array_equal(x, y) for x, y in zip(la, lb)) and all(x.size > 0 for x in la)
    assert np.array_equal(a.counts(), b.counts()) and np.array_equal(a.root_values(), b.root_values())
    assert (ca.hits(), ca.misses(), ca.size()) == (cb.hits(), cb.misses(), cb.size()) and ca.misses() > 0
    sa, sb = a.stats(), b.stats()
    assert {k: sa[k] for k in sa if k != "launches"} == {k: sb[k] for k in sb if k != "launches"}


def test_a_move_adds_a_constant_number_of_launches(az, c4_net):
    """a Connect4 move adds 2 launches (pick, update-root) to the steps of its search, whatever N is; the root
    prior is one more; a wide game's compaction is one more."""
    visits, moves = 6, 3
    per_move = {}
    for n in (8, 256):
        mb = az.MCTSBatch(az.Connect4GS, n, 1.25, max_simulations=visits * (2 * moves + 1), seeds=list(range(n)))
        mb.reset(_c4_states(az, n, seed=43))
        l0 = mb.stats(); mb.search(visits, net=c4_net); l1 = mb.stats()
        mb.play(visits, net=c4_net, max_moves=moves); l2 = mb.stats()
        mb.play(visits, net=c4_net, max_moves=moves, root_noise=True); l3 = mb.stats()
        search = l1["launches"] - l0["launches"]
        per_move[n] = ((l2["launches"] - l1["launches"] - moves * search) / moves, (l3["launches"] - l2["launches"] - moves * search) / moves)
        assert l3["net_calls"] - l0["net_calls"] == visits * (2 * moves + 1)
    assert per_move[8] == per_move[256] == (2.0, 3.0)
    mb = az.MCTSBatch(az.BrandubhGS, 4, 1.25, max_simulations=2 * visits, seeds=list(range(4)))
    mb.reset([az.BrandubhGS() for _ in range(4)])
    l0 = mb.stats(); mb.search(visits); l1 = mb.stats()
    mb.play(visits, max_moves=moves); l2 = mb.stats()
    assert (l2["launches"] - l1["launches"] - moves * (l1["launches"] - l0["launches"])) / moves == 3.0


# ---- 4. whole games -------------------------------------------------------------------------------------------------------------
def test_whole_games_in_one_call(az):
    n, visits = 8, 16
    mb = az.MCTSBatch(az.Connect4GS, n, 1.25, fpu_reduction=0.25, max_simulations=visits * 42 + 64, seeds=[70 + i for i in range(n)])
    mb.reset([az.Connect4GS() for _ in range(n)])
    mb.play(visits=visits, max_moves=42)
    assert mb.finished().all()
    logs, states, fs = mb.move_logs(), mb.states(), mb.final_scores()
    assert len({tuple(l.tolist()) for l in logs}) > 1, "eight streams, eight games"
    for i in range(n):
        gs = az.Connect4GS()
        for ply, mv in enumerate(logs[i]):
            assert gs.scores() is None and gs.valid_moves()[int(mv)], f"tree {i}: ply {ply} is not legal"
            gs.play_move(int(mv))
        assert gs == states[i] and gs.scores() is not None
        assert np.array_equal(fs[i], states[i].scores()), f"tree {i}"
        assert 7 <= logs[i].size <= 42
    s0 = mb.stats()
    mb.play(visits=visits, max_moves=2)             # every tree is finished: nothing is searched, nothing moves
    s1 = mb.stats()
    assert s1["simulations"] == s0["simulations"] and s1["terminal_leaves"] == s0["terminal_leaves"]
    assert all(np.array_equal(x, y) for x, y in zip(mb.move_logs(), logs))
    assert mb.pick_moves(1.0).tolist() == [-1] * n


# ---- 5. Gumbel trees ----------------------------------------------------------------------------------------------------------------
def test_gumbel_trees_take_the_final_action_and_reset_their_state(az):
    n, moves, visits = 4, 3, 16
    gss = [_c4_at(az, p) for p in [(), (3, 3, 2), (1, 6, 3, 6, 4, 2, 2), (2, 4)]]
    seeds = [900 + 5 * i for i in range(n)]
    kw = dict(gumbel_enabled=True, gumbel_m=4)
    mb = az.MCTSBatch(az.Connect4GS, n, 2.0, max_simulations=visits * (moves + 1), seeds=seeds, **kw)
    mb.reset(gss)
    ms = [az.MCTS(2.0, 2, 7, seed=seeds[i], max_simulations=visits * (moves + 1), **kw) for i in range(n)]
    for mv_no in range(moves + 1):
        mb.search(visits)                           # (sets the Gumbel budget itself, like the objects below)
        for i in range(n):
            ms[i].set_gumbel_num_sims(visits)
            _drive_alone(az, ms[i], gss[i], visits)
        gp = mb.gumbel_improved_policies()
        for i in range(n):                          # move > 0: the state was reset by update_root and built again
            assert np.array_equal(gp[i], ms[i].gumbel_improved_policy()), f"move {mv_no}, tree {i}"
            assert np.array_equal(mb.counts()[i], ms[i].counts()), f"move {mv_no}, tree {i}"
        if mv_no == moves:
            break
        want = [ms[i].gumbel_final_action() for i in range(n)]
        assert mb.pick_moves(1.0).tolist() == want, f"move {mv_no}"
        mb.update_roots()
        for i in range(n):
            ms[i].update_root(gss[i], want[i])
            gss[i].play_move(want[i])
            assert gss[i].scores() is None


# ---- 6. root prior after reuse -------------------------------------------------------------------------------------------------
def test_root_prior_after_reuse_equals_the_objects(az):
    n, visits = 4, 16
    start = [_c4_at(az, p) for p in [(), (3, 3, 2), (1, 6, 3, 6, 4, 2, 2), (2, 4)]]
    seeds = [300 + 9 * i for i in range(n)]
    kw = dict(fpu_reduction=0.25, epsilon=0.25, root_policy_temp=1.3)
    mb = az.MCTSBatch(az.Connect4GS, n, 1.25, max_simulations=2 * visits, seeds=seeds, **kw)
    gss = [g.copy() for g in start]
    mb.reset(gss)
    ms = [az.MCTS(1.25, 2, 7, seed=seeds[i], max_simulations=2 * visits, **kw) for i in range(n)]
    mb.search(visits, root_noise=True)
    want = []
    for i in range(n):
        _drive_alone(az, ms[i], gss[i], visits, noise=True)
        want.append(ms[i].pick_move(ms[i].probs(1.0)))
    assert mb.pick_moves(1.0).tolist() == want
    mb.update_roots(); mb.apply_root_policy_temp(); mb.add_root_noise()
    mb.search(visits, root_noise=True)
    for i in range(n):
        ms[i].update_root(gss[i], want[i]); gss[i].play_move(want[i])
        ms[i].apply_root_policy_temp(); ms[i].add_root_noise()
        _drive_alone(az, ms[i], gss[i], visits, noise=True)
    out = dict(_four(mb), q=mb.root_q_values(), p1=mb.probs(1.0))
    for i in range(n):
        _assert_four(out, i, ms[i], "temp + noise on the reused root")
        assert np.array_equal(out["q"][i], ms[i].root_q_values()) and np.array_equal(out["p1"][i], ms[i].probs(1.0)), f"tree {i}"
    # play(root_noise=True) is that sequence
    pb = az.MCTSBatch(az.Connect4GS, n, 1.25, max_simulations=2 * visits, seeds=seeds, **kw)
    pb.reset(start)
    pb.play(visits, max_moves=1, root_noise=True)
    pb.search(visits, root_noise=True)
    assert [l.tolist() for l in pb.move_logs()] == [[w] for w in want]
    assert np.array_equal(pb.counts(), out["counts"]) and np.array_equal(pb.root_q_values(), out["q"])


# ---- 7. errors leave the batch usable ------------------------------------------------------------------------------------------
def _known_answer(az, mb, n):
    """test_reference_known_answer_inside_a_batch on tree 5 of this batch (seed 12345, max_simulations = 800)"""
    mb.reset([_c4_at(az, (1, 6, 3, 6)) for _ in range(n)])
    mb.search(800)
    assert mb.counts()[5].tolist() == [62, 21, 631, 21, 22, 21, 21]
    assert int(mb.depths()[5]) == 800


def test_errors_leave_the_batch_usable(az):
    n = 8
    seeds = [1000 + i for i in range(n)]
    seeds[5] = 12345
    mb = az.MCTSBatch(az.Connect4GS, n, 2.0, max_simulations=800, seeds=seeds)
    states = [_c4_at(az, (3, 3, 2)) for _ in range(n)]
    states[2] = _c4_at(az, (0, 0, 0, 0, 0, 0))                    # column 0 is full
    # a move that is not one of tree 2's root: tree 2 is named and left where it was, the other trees' moves are applied
    mb.reset(states)
    with pytest.raises(RuntimeError, match=r"tree 2\b.*what is this move"):
        mb.update_roots([0] * n)
    assert [int(l.size) for l in mb.move_logs()] == [1, 1, 0, 1, 1, 1, 1, 1]
    assert not mb.finished().any()
    mb.update_roots([-1, -1, 3] + [-1] * (n - 3))                  # tree 2 is still live
    assert [l.tolist() for l in mb.move_logs()] == [[0], [0], [3]] + [[0]] * (n - 3)
    mb.search(10)
    assert mb.depths().tolist() == [10] * n
    with pytest.raises(RuntimeError, match="out of range"):
        mb.update_roots([7] * n)
    with pytest.raises(RuntimeError, match="one move per tree"):
        mb.update_roots([0] * (n - 1))
    _known_answer(az, mb, n)
    # a root without visits has no move to pick
    mb.reset(states)
    with pytest.raises(RuntimeError, match=r"tree 0\b.*no visits"):
        mb.pick_moves(1.0)
    mb.search(10)
    assert (mb.pick_moves(1.0) >= 0).all()
    _known_answer(az, mb, n)
    # a pending find_leaves() step
    mb.reset(states)
    mb.find_leaves(numpy=True)
    l0 = mb.stats()["launches"]
    for call in (lambda: mb.update_roots(), lambda: mb.update_roots([3] * n), lambda: mb.pick_moves(1.0), lambda: mb.play(4),
                 lambda: mb.add_root_noise()):
        with pytest.raises(RuntimeError, match="find_leaves step is pending"):
            call()
    assert mb.stats()["launches"] == l0
    assert not mb.finished().any() and [int(l.size) for l in mb.move_logs()] == [0] * n      # the game read-outs stay legal
    _known_answer(az, mb, n)
    # a pick is played once: update_roots() without a pick before it (after a reset, after the pick was consumed) moves nothing
    mb.reset(states)
    mb.update_roots()
    assert [int(l.size) for l in mb.move_logs()] == [0] * n
    mb.search(10); mb.pick_moves(1.0); mb.update_roots(); mb.update_roots()
    assert [int(l.size) for l in mb.move_logs()] == [1] * n
    _known_answer(az, mb, n)
    # the Connect4 budget counts every descent since reset, moves included: refused before anything is enqueued
    mb.reset(states)
    mb.play(100, max_moves=2)
    l0 = mb.stats()
    with pytest.raises(RuntimeError, match="since reset"):
        mb.play(100, max_moves=7)
    with pytest.raises(RuntimeError, match="since reset"):
        mb.search(601)
    assert mb.stats() == l0
    mb.play(100, max_moves=6)
    assert all(int(l.size) == 8 or f for l, f in zip(mb.move_logs(), mb.finished()))
    _known_answer(az, mb, n)
